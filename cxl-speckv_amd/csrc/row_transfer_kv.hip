// cxl-speckv_amd/csrc/row_transfer_kv.hip -- the paged-cache transfers of the split pool (Engine::read_slots_kv / write_slots_kv):
// k_read_slots_ex and k_compress_slots_ex (row_transfer.hip) with both codecs in one launch.  A span names two allocations, an
// FP8_E4M3 one with the K rows and an MXFP4 one with the V rows (SlotSpanKV, kernels.hpp); wave j = (layer, kind) of a page takes
// allocation and codec j & 1.  The cache side, the held rows, the move waves and both wave orders are the _ex kernels': the work of
// a wave is found by the same slot_work and move_work (slot_transfer_device.hpp).  Beside them k_read_pairs_kv, k_read_pairs
// (row_transfer.hip) with both codecs: the rollback and the fork of split requests (Engine::read_pairs_kv).
//
// A translation unit of its own: row_transfer.o holds the single-allocation families and nothing else (tests/test_commit_cpu.py
// reads its symbols), and those kernels' register figures must not move with what is added here.
//
// Execution model as there.  One wave owns one block; which block, and with it the KIND, depends on blockIdx and the wave number
// alone and lives in scalar registers, so the choice between the FP8 and the MXFP4 body is a scalar branch: a wave runs one of the
// two, never both under an exec mask.  Neither body has a workgroup barrier (block_codec_device.hpp: the waves of a workgroup are
// independent), which is what lets a workgroup hold waves of both kinds under kind_fast = 1.  The encoder's LDS is the larger of
// the two codecs', MXFP4's staging of its record (kWaves x 1088 bytes); the FP8 encoder uses none.  No scratch: the build checks it.
#include "kernels.hpp"
#include "block_codec_device.hpp"
#include "slot_transfer_device.hpp"

#include <type_traits>

namespace speckv {
namespace {
typedef SlotWorkT<SlotSpanKV> SlotWorkKV;

template <bool BF16>
__global__ __launch_bounds__(kThreads) void k_read_slots_kv(SlotKVArgs x)
{
    typedef typename std::conditional<BF16, RowSinkBf16, RowSink>::type Sink;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kWaves + wave;
    const uint64_t n_dec = static_cast<uint64_t>(x.a.n_pairs) * 2u * x.a.n_layers;
    if (i >= n_dec) {                                                // a held row into the slot of the span's last position
        uint8_t *held_row = nullptr, *cache_row = nullptr;
        if (move_work(x, i - n_dec, false, &held_row, &cache_row) && cache_row) move_row(held_row, cache_row, lane, BF16 ? kMoveToBf16 : kMoveCopy);
        return;
    }
    SlotWorkKV w;
    if (!slot_work(x.a, wave, &w)) return;
    uint8_t* const base = const_cast<uint8_t*>(w.base);
    const Sink dst{w.slot[0] >= 0 ? base + static_cast<uint64_t>(w.slot[0]) * 2048u : nullptr,
                   w.slot[1] >= 0 ? base + static_cast<uint64_t>(w.slot[1]) * 2048u : nullptr};
    if (!dst.even && !dst.odd) return;
    const uint32_t kind = w.j & 1u;                                  // wave-uniform: allocation and codec
    const PageEntry* entries = x.a.tab[w.g->table_row[kind]].entries;
    PageEntry e{0, 0, 1.0f};
    if (entries) e = entries[(static_cast<uint64_t>(x.a.layer_begin) + (w.j >> 1)) * x.a.page_step + w.pair];   // a row freed meanwhile decodes as a never-written page
    // pool records as in k_read_slots_ex: trusted streams, tile-planar MXFP4 codes
    const uint8_t* rec = reinterpret_cast<const uint8_t*>(e.pool_addr);
    const uint32_t len = e.rec_bytes;
    if (kind) decode_mx4<false, Sink>(rec, rec + __float_as_uint(e.scale), len, dst, lane);
    else decode_fp8<false, Sink>(rec, len > kBlockElems ? kBlockElems : len, e.scale, dst, lane);
}

// Neither FP8_E4M3 nor MXFP4 has a quantiser mode (by_scheme_mode, row_transfer.hip: kRefExact names their one instance), so the
// encoder is one kernel.
__global__ __launch_bounds__(kThreads) void k_compress_slots_kv(SlotKVArgs x)
{
    SPECKV_ENC_LDS(kMxFp4);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t uwave = __builtin_amdgcn_readfirstlane(wave);
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kWaves + uwave;
    const uint64_t n_enc = static_cast<uint64_t>(x.a.n_pairs) * 2u * x.a.n_layers;
    const bool bf16 = x.bf16 != 0u;
    if (i >= n_enc) {                                                // the span's last position into its held row (no row: zeros)
        uint8_t *held_row = nullptr, *cache_row = nullptr;
        if (move_work(x, i - n_enc, true, &held_row, &cache_row)) move_row(cache_row, held_row, lane, bf16 ? kMoveFromBf16 : kMoveCopy);
        return;
    }
    SlotWorkKV w;
    if (!slot_work(x.a, uwave, &w)) return;
    const uint32_t kind = w.j & 1u;                                  // wave-uniform: allocation and codec
    SrcPairMixed src{w.slot[0] >= 0 ? w.base + static_cast<uint64_t>(w.slot[0]) * 2048u : x.a.zeros,
                     w.slot[1] >= 0 ? w.base + static_cast<uint64_t>(w.slot[1]) * 2048u : x.a.zeros, bf16, bf16};
    if (x.held && 2u * w.pair < w.g->first_token) {                  // the pair begins one position in front of the span: its held row
        const uint64_t h = x.held[w.g - x.a.spans].in[kind];
        if (h) {
            src.lo = reinterpret_cast<const uint8_t*>(h) + static_cast<uint64_t>(w.j >> 1) * x.held_stride;
            src.lo_bf16 = false;
        }
    }
    PageEntry* entries = w.g->entries[kind];
    __builtin_assume(entries != nullptr);
    const EncTarget t{entries, w.g->scale_tab[kind], w.g->region_pages[kind], w.g->scale_run[kind], nullptr, nullptr, 0, nullptr, nullptr};
    const uint64_t page = (static_cast<uint64_t>(x.a.layer_begin) + (w.j >> 1)) * x.a.page_step + w.pair;
    if (kind) compress_block<kMxFp4, kRefExact>(t, page, src, lds, lane, wave);
    else compress_block<kFp8E4m3, kRefExact>(t, page, src, lds, lane, wave);
}

// k_read_pairs (row_transfer.hip) with both codecs: the rollback and the fork of split requests (Engine::read_pairs_kv).  Wave i is
// block j = i % (2 * n_layers) of pair i / (2 * n_layers) -- layer j >> 1, kind j & 1 -- and decodes page first + (j >> 1) *
// page_step of the pair's K allocation (kind 0, decode_fp8) or of its V allocation (kind 1, decode_mx4 with the tile-planar codes
// PageEntry::scale points to) into the pair's two rows of that kind, layer_stride bytes further on per layer.  n_layers counts REAL
// layers: a single-kind allocation has one region per layer, so there is no factor 2 and no kind term in the page.  The record is
// found through the allocation table and the page's entry (any placement, a sealed source); a row that is nullptr is not stored
// and, in the FP8 body, not read.  One block per wave, no LDS, no workgroup barrier.
__global__ __launch_bounds__(kThreads) void k_read_pairs_kv(ReadPairKVArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kWaves + wave;
    const uint32_t per = 2u * a.n_layers;
    if (i >= static_cast<uint64_t>(a.n_pairs) * per) return;        // (whole waves leave: the body has no workgroup barrier)
    const uint32_t pi = static_cast<uint32_t>(i / per), j = static_cast<uint32_t>(i - static_cast<uint64_t>(pi) * per);
    const ReadPairKV* g = a.pairs + pi;
    const uint32_t kind = j & 1u;                                    // wave-uniform: allocation and codec
    const uint64_t off = static_cast<uint64_t>(j >> 1) * a.layer_stride;
    uint8_t* const even = g->row[2u * kind];
    uint8_t* const odd = g->row[2u * kind + 1u];
    const RowSink dst{even ? even + off : nullptr, odd ? odd + off : nullptr};
    if (!dst.even && !dst.odd) return;
    const PageEntry* entries = a.tab[g->table_row[kind]].entries;
    PageEntry e{0, 0, 1.0f};
    if (entries) e = entries[g->first + static_cast<uint64_t>(j >> 1) * a.page_step];     // a row freed meanwhile decodes as a never-written page
    const uint8_t* rec = reinterpret_cast<const uint8_t*>(e.pool_addr);
    const uint32_t len = e.rec_bytes;
    if (kind) decode_mx4<false, RowSink>(rec, rec + __float_as_uint(e.scale), len, dst, lane);
    else decode_fp8<false, RowSink>(rec, len > kBlockElems ? kBlockElems : len, e.scale, dst, lane);
}

// what both launchers ask of a SlotKVArgs (slot_ex_args_ok, row_transfer.hip); *grid = one page or one moved row per wave, 0 =
// nothing to do
bool slot_kv_args_ok(const SlotKVArgs& x, uint32_t* grid)
{
    const SlotKVArgs::Pages& a = x.a;
    const uint64_t waves = static_cast<uint64_t>(a.n_pairs) * 2u * a.n_layers + x.n_moves;
    if (!a.spans || !a.caches || !a.slots || a.n_spans == 0 || a.page_step == 0 || a.kind_stride % 16u || x.held_stride % 16u) return false;
    if ((x.n_moves != 0u && (!x.held || x.n_moves != static_cast<uint64_t>(a.n_spans) * 2u * a.n_layers)) || waves > (1ull << 31)) return false;
    *grid = static_cast<uint32_t>((waves + kWaves - 1) / kWaves);
    return true;
}
} // namespace

hipError_t launch_compress_slots_kv(const SlotKVArgs& x, hipStream_t s)
{
    if (x.a.n_layers == 0) return hipSuccess;
    uint32_t grid = 0;
    if (!slot_kv_args_ok(x, &grid) || !x.a.zeros) return hipErrorInvalidValue;
    if (grid == 0) return hipSuccess;
    hipLaunchKernelGGL(k_compress_slots_kv, dim3(grid), dim3(kThreads), 0, s, x);
    return hipGetLastError();
}

hipError_t launch_read_slots_kv(const SlotKVArgs& x, hipStream_t s)
{
    if (x.a.n_layers == 0) return hipSuccess;
    uint32_t grid = 0;
    if (!slot_kv_args_ok(x, &grid) || !x.a.tab) return hipErrorInvalidValue;
    if (grid == 0) return hipSuccess;
    if (x.bf16) hipLaunchKernelGGL((k_read_slots_kv<true>), dim3(grid), dim3(kThreads), 0, s, x);
    else hipLaunchKernelGGL((k_read_slots_kv<false>), dim3(grid), dim3(kThreads), 0, s, x);
    return hipGetLastError();
}

hipError_t launch_read_pairs_kv(const ReadPairKVArgs& a, hipStream_t s)
{
    const uint64_t waves = static_cast<uint64_t>(a.n_pairs) * 2u * a.n_layers;       // one block per wave
    if (waves == 0) return hipSuccess;
    if (!a.pairs || !a.tab || a.page_step == 0 || a.layer_stride % 16u || waves > (1ull << 31)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_read_pairs_kv, dim3(static_cast<uint32_t>((waves + kWaves - 1) / kWaves)), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

} // namespace speckv
