// cxl-speckv_amd/csrc/copy_records_kv.hip -- k_copy_records_kv: k_copy_records (copy_records.hip) over the two allocation pairs of a
// split-pool request, FP8_E4M3 keys and MXFP4 values, in ONE launch (Engine::copy_runs_kv, speckv_ext_copy_runs_kv: a split request
// forked from positions another one holds).  Nothing is decoded.
//
// A translation unit of its own beside copy_records.hip: that unit's six instances keep their instructions, and what the two share --
// the accesses, the scalar bookkeeping, the copy of a record's bytes and of its entry -- is copy_records_device.hpp.
//
// Execution model as there: one wave takes one record and issues all of its loads before its first store; the grid is persistent,
// kCopyWgsPerCu workgroups of 4 waves per CU walk the flat record index grid-stride; no LDS, no workgroup barrier, no atomics.
//
// Which record a wave owns: flat index i -> pair = the last one whose exclusive prefix of 2 * n_runs * n_pages is <= i (binary
// search), local = i - prefix, side = local >= n_runs * n_pages (0: the K allocations, 1: the V allocations), and inside the side run
// and page as k_copy_records has them: consecutive waves take consecutive pages of one run of one allocation.  All of this is the same
// for every lane and lives in scalar registers, so the choice between the FP8 and the MXFP4 body is a scalar branch: a wave runs one
// of the two, never both under an exec mask.  Everything written goes out through vector stores.
#include "copy_records_device.hpp"

namespace speckv {
namespace {

__global__ __launch_bounds__(64 * kCopyWaves) void k_copy_records_kv(const CopyPairKV* __restrict__ pairs, const uint64_t* __restrict__ run_firsts,
                                                                     const DevAlloc* __restrict__ tab, uint32_t n_pairs, uint32_t n_runs, uint64_t n_recs)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t step = static_cast<uint64_t>(gridDim.x) * kCopyWaves;
    for (uint64_t i = static_cast<uint64_t>(blockIdx.x) * kCopyWaves + wave; i < n_recs; i += step) {
        // the last pair whose prefix is <= i (pairs without pages share their successor's prefix and are passed over)
        uint32_t lo = 0, hi = n_pairs;
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (cp_uniform(pairs[mid].first_rec) <= i) lo = mid; else hi = mid;
        }
        const CopyPairKV* g = pairs + lo;
        const uint64_t n_pages = cp_uniform(g->n_pages), both = i - cp_uniform(g->first_rec), half = n_pages * n_runs;
        const uint32_t side = both >= half ? 1u : 0u;             // wave-uniform: allocations and record format
        const uint64_t local = both - (side ? half : 0u);
        const uint64_t run = local / n_pages;
        const uint64_t page = cp_uniform(run_firsts[run]) + (local - run * n_pages);
        PageEntry* const d_entries = reinterpret_cast<PageEntry*>(cp_uniform(reinterpret_cast<uint64_t>(g->entries[side])));
        const PageEntry* const s_entries = reinterpret_cast<const PageEntry*>(cp_uniform(reinterpret_cast<uint64_t>(tab[g->src_row[side]].entries)));
        EntryWords s{0, 0, 0x3F800000u};
        if (s_entries) s = cp_entry(s_entries + page);            // a source freed meanwhile copies as a page never written
        const EntryWords d = cp_entry(d_entries + page);
        if (side) {
            const uint32_t len = copy_record_bytes<kMxFp4>(s, d, lane);
            if (lane == 0u) copy_record_entry<kMxFp4, false>(d_entries + page, page, len, s.scale_bits, g);
        } else {
            const uint32_t len = copy_record_bytes<kFp8E4m3>(s, d, lane);
            if (lane == 0u) copy_record_entry<kFp8E4m3, true>(d_entries + page, page, len, s.scale_bits, g);
        }
    }
}

} // namespace

hipError_t launch_copy_records_kv(const CopyKVArgs& a, hipStream_t s)
{
    if (a.n_recs == 0) return hipSuccess;
    if (!a.pairs || !a.run_firsts || !a.tab || a.n_pairs == 0 || a.n_runs == 0 || a.n_cus == 0) return hipErrorInvalidValue;
    const uint64_t wgs = (a.n_recs + kCopyWaves - 1u) / kCopyWaves, cap = static_cast<uint64_t>(a.n_cus) * kCopyWgsPerCu;
    const uint32_t grid = static_cast<uint32_t>(wgs < cap ? wgs : cap);
    hipLaunchKernelGGL(k_copy_records_kv, dim3(grid), dim3(64 * kCopyWaves), 0, s, a.pairs, a.run_firsts, a.tab, a.n_pairs, a.n_runs, a.n_recs);
    return hipGetLastError();
}

} // namespace speckv
