// cxl-speckv_amd/csrc/copy_records.hip -- k_copy_records: the stored records of page runs copied from one allocation to another,
// nothing decoded (Engine::copy_runs, speckv_ext_copy_runs: a request forked from positions another request holds).
//
// A translation unit of its own: the headline kernel of kernels.hip is pinned by the hash of its instructions, and nothing here
// needs the codec.
//
// Execution model.  A byte kernel: records of 1088..4096 B, 128-byte aligned, each read once and written once.  One wave takes
// one record -- lane l moves bytes [16 l + 1024 j, 16 l + 1024 j + 16), j < 4, so every access is one coalesced 1 KiB instruction --
// and issues ALL loads of the record before its first store.  The grid is persistent: kCopyWgsPerCu workgroups of 4 waves per CU
// walk the flat record index grid-stride, so a CU has 32 waves x (1..4 KiB) = 32..128 KiB of loads in flight, at or above the
// ~32 KiB per CU that streaming from HBM takes.  No LDS, no workgroup barrier, no atomics.
//
// Which record a wave owns: flat index i -> pair = the last one whose exclusive prefix of n_runs * n_pages is <= i (binary search,
// the host computed the prefixes), then run = (i - prefix) / n_pages and page = run_firsts[run] + (i - prefix) % n_pages: consecutive
// waves take consecutive pages of one run.  The index is the same for all lanes; what it selects is read once and kept in scalar
// registers.  Everything written goes out through vector stores.
#include "copy_records_device.hpp"    // the accesses and the scalar bookkeeping, shared with copy_records_kv.hip

namespace speckv {
namespace {

template <int SCHEME>
__global__ __launch_bounds__(64 * kCopyWaves) void k_copy_records(const CopyPair* __restrict__ pairs, const uint64_t* __restrict__ run_firsts,
                                                                  const DevAlloc* __restrict__ tab, uint32_t n_pairs, uint64_t n_recs)
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
        const CopyPair* g = pairs + lo;
        const uint64_t n_pages = cp_uniform(g->n_pages), local = i - cp_uniform(g->first_rec);
        const uint64_t run = local / n_pages;
        const uint64_t page = cp_uniform(run_firsts[run]) + (local - run * n_pages);
        PageEntry* const d_entries = reinterpret_cast<PageEntry*>(cp_uniform(reinterpret_cast<uint64_t>(g->entries)));
        const PageEntry* const s_entries = reinterpret_cast<const PageEntry*>(cp_uniform(reinterpret_cast<uint64_t>(tab[g->src_row].entries)));
        EntryWords s{0, 0, 0x3F800000u};
        if (s_entries) s = cp_entry(s_entries + page);            // a source freed meanwhile copies as a page never written
        const EntryWords d = cp_entry(d_entries + page);
        const uint8_t* src = reinterpret_cast<const uint8_t*>(s.addr);
        uint8_t* dst = reinterpret_cast<uint8_t*>(d.addr);
        constexpr uint32_t kMax = max_rec_bytes<SCHEME>();
        const uint32_t len = s.len < kMax ? s.len : kMax;
        if (len) {
            if (SCHEME == kMxFp4) {
                // tile-planar: the nibble row at the record's address, the 64 code bytes a slot-dependent distance behind it -- the
                // source's distance to read, the destination's own to write (PageEntry::scale holds it; it is not copied)
                const u32x4 nib = cp_ld16(src + 16u * lane);
                u32x4 code = {0u, 0u, 0u, 0u};
                if (lane < 4u) code = cp_ld16(src + s.scale_bits + 16u * lane);
                cp_st16(dst + 16u * lane, nib);
                if (lane < 4u) cp_st16(dst + d.scale_bits + 16u * lane, code);
            } else {
                // rounded up to 16 inside the slot: the encoder zero-pads a record's last 16-byte piece, slots and packed extents are
                // 128-byte aligned
                const uint32_t bytes = (len + 15u) & ~15u;
                u32x4 v[4];
#pragma unroll
                for (uint32_t j = 0; j < 4u; ++j) {
                    const uint32_t b = 1024u * j + 16u * lane;
                    if (1024u * j < kMax && b < bytes) v[j] = cp_ld16(src + b);
                }
#pragma unroll
                for (uint32_t j = 0; j < 4u; ++j) {
                    const uint32_t b = 1024u * j + 16u * lane;
                    if (1024u * j < kMax && b < bytes) cp_st16(dst + b, v[j]);
                }
            }
        } else if (d.len) {
            // a page never written replaces a record: the slot goes back to zero bytes, which is what the attention forms that
            // compute record addresses read for a page never written
            const u32x4 zero = {0u, 0u, 0u, 0u};
            if (SCHEME == kMxFp4) {
                cp_st16(dst + 16u * lane, zero);
                if (lane < 4u) cp_st16(dst + d.scale_bits + 16u * lane, zero);
            } else {
                const uint32_t bytes = ((d.len < kMax ? d.len : kMax) + 15u) & ~15u;
#pragma unroll
                for (uint32_t j = 0; j < 4u; ++j) {
                    const uint32_t b = 1024u * j + 16u * lane;
                    if (1024u * j < kMax && b < bytes) cp_st16(dst + b, zero);
                }
            }
        }
        if (lane == 0u) {
            PageEntry* e = d_entries + page;
            cp_store<uint32_t>(&e->rec_bytes, len);
            if (SCHEME != kMxFp4) cp_store<uint32_t>(&e->scale, s.scale_bits);
            // the block scale wherever k_compress leaves it (FP8 allocations with a layout), a page never written as
            // launch_build_scale_tab has it
            float* const scale_tab = g->scale_tab;
            if (scale_tab) {
                const uint32_t region_pages = g->region_pages, scale_run = g->scale_run;
                const uint32_t sc = len >= kBlockElems ? s.scale_bits : 0u;
                const uint32_t j = static_cast<uint32_t>(page % region_pages) & 15u;
                cp_store<uint32_t>(&scale_tab[page - j + attend_tile_slot(j)], sc);
                if (scale_run) cp_store<uint32_t>(scale_tab + scale_run_index(page, scale_run), sc);
            }
        }
    }
}

template <int SCHEME>
hipError_t launch_copy(const CopyArgs& a, uint32_t grid, hipStream_t s)
{
    hipLaunchKernelGGL(k_copy_records<SCHEME>, dim3(grid), dim3(64 * kCopyWaves), 0, s, a.pairs, a.run_firsts, a.tab, a.n_pairs, a.n_recs);
    return hipGetLastError();
}

} // namespace

hipError_t launch_copy_records(const CopyArgs& a, hipStream_t s)
{
    if (a.n_recs == 0) return hipSuccess;
    if (!a.pairs || !a.run_firsts || !a.tab || a.n_pairs == 0 || a.n_cus == 0) return hipErrorInvalidValue;
    const uint64_t wgs = (a.n_recs + kCopyWaves - 1u) / kCopyWaves, cap = static_cast<uint64_t>(a.n_cus) * kCopyWgsPerCu;
    const uint32_t grid = static_cast<uint32_t>(wgs < cap ? wgs : cap);
    switch (a.scheme) {
    case kFp16: return launch_copy<kFp16>(a, grid, s);
    case kInt8: return launch_copy<kInt8>(a, grid, s);
    case kInt8DeltaRle: return launch_copy<kInt8DeltaRle>(a, grid, s);
    case kInt4G32: return launch_copy<kInt4G32>(a, grid, s);
    case kFp8E4m3: return launch_copy<kFp8E4m3>(a, grid, s);
    case kMxFp4: return launch_copy<kMxFp4>(a, grid, s);
    default: return hipErrorInvalidValue;
    }
}

} // namespace speckv
