// cxl-speckv_amd/csrc/row_transfer.hip -- the row transfers: K and V rows moved between the pool's records and caller memory,
// two positions (one page) per wave, no page image assembled on either side.  Three pairs of kernels, an encoder and its inverse:
//   k_compress_pairs / k_read_pairs            rows named by four host pointers per position pair  (Engine::write_pairs / read_pairs:
//                                              the commit of a multi-position step and its rollback)
//   k_compress_slots / k_read_slots            rows named by a slot mapping on the device and a cache base per layer
//                                              (Engine::write_slots / read_slots: paged caches)
//   k_compress_slots_ex / k_read_slots_ex      the same for caches that hold bf16 and for spans with held rows; their SlotKmulArgs
//                                              instances multiply K by a per-channel factor on the way (the connector's K pre-scale)
// (The split pool's pair, k_compress_slots_kv / k_read_slots_kv -- a K and a V allocation per span, both codecs in one launch --
// is row_transfer_kv.hip; what the slot kernels of both units share, slot_work and the move of a held row, is
// slot_transfer_device.hpp.)
//
// A translation unit of its own: the headline kernel of kernels.hip is pinned by the hash of its instructions, and these kernels
// share the block codec's device code (block_codec_device.hpp), not its launch path.  The unit contains kernels only -- every
// decoder and encoder it uses is inlined into them, and the build and tests/test_commit_cpu.py hold it to that -- so no code here
// is reached by a pc-relative call and the file may grow without moving anything else.
//
// Execution model.  Byte kernels like the codec's: one wave owns one block (the [heads][128] rows of an even and an odd position of
// one layer and kind), lane l holds elements [8l+512j, 8l+512j+8), every global access is 16 B per lane, 1 KiB per instruction.
// Which block a wave owns depends on blockIdx and the wave number alone, is worked out once per wave and lives in scalar
// registers.  No workgroup barrier anywhere: whole waves leave where they have no work.  Every instance keeps its state in
// registers (no scratch: the build checks it).
#include "kernels.hpp"
#include "block_codec_device.hpp"
#include "slot_transfer_device.hpp"

#include <type_traits>

namespace speckv {
namespace {

// One instance per (scheme, quantiser mode): the launchers hand by_scheme_mode a generic lambda that takes the pair as two
// integral constants and launches k_...<decltype(scheme)::value, decltype(mode)::value>.  INT4_G32, FP8 and MXFP4 have no
// quantiser mode (kRefExact names their one instance); FP16 has one where FP16_MODES says so -- the encoders were always
// instantiated in both, the readers (a copy or a conversion: no quantiser) in kRefExact alone.
template <int V> using int_c = std::integral_constant<int, V>;
template <int SCHEME, bool MODES, class LAUNCH>
hipError_t by_mode(int quant_mode, const LAUNCH& launch)
{
    if constexpr (MODES) { if (quant_mode == kIntent) return launch(int_c<SCHEME>{}, int_c<kIntent>{}); }
    return launch(int_c<SCHEME>{}, int_c<kRefExact>{});
}
template <bool FP16_MODES, class LAUNCH>
hipError_t by_scheme_mode(int scheme, int quant_mode, const LAUNCH& launch)
{
    switch (scheme) {
    case kFp16: return by_mode<kFp16, FP16_MODES>(quant_mode, launch);
    case kInt8: return by_mode<kInt8, true>(quant_mode, launch);
    case kInt8DeltaRle: return by_mode<kInt8DeltaRle, true>(quant_mode, launch);
    case kInt4G32: return by_mode<kInt4G32, false>(quant_mode, launch);
    case kFp8E4m3: return by_mode<kFp8E4m3, false>(quant_mode, launch);
    case kMxFp4: return by_mode<kMxFp4, false>(quant_mode, launch);
    default: return hipErrorInvalidValue;
    }
}

// The commit of a multi-position step (Engine::write_pairs): wave i encodes block j = i % (2 * n_layers) of position pair
// i / (2 * n_layers) -- layer j >> 1, kind j & 1 (K, V), page first + j * page_step -- from the pair's two rows of that kind,
// layer_stride bytes further on per layer.  No page image is ever assembled.  One block per wave; the records are those
// k_compress stores for the same 4096 bytes.
template <int SCHEME, int MODE>
__global__ __launch_bounds__(kThreads) void k_compress_pairs(PairArgs a)
{
    SPECKV_ENC_LDS(SCHEME);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kWaves + wave;
    const uint32_t per = 2u * a.n_layers;
    if (i >= static_cast<uint64_t>(a.n_pairs) * per) return;        // (whole waves leave: the body has no workgroup barrier)
    const uint32_t pi = static_cast<uint32_t>(i / per), j = static_cast<uint32_t>(i - static_cast<uint64_t>(pi) * per);
    const CommitPair* g = a.pairs + pi;
    const uint32_t kind = j & 1u;
    const uint64_t off = static_cast<uint64_t>(j >> 1) * a.layer_stride;
    const SrcPair src{g->row[2u * kind] + off, g->row[2u * kind + 1u] + off};     // (read by address: no register copy of row[])
    PageEntry* entries = g->entries;
    __builtin_assume(entries != nullptr);
    const EncTarget t{entries, g->scale_tab, g->region_pages, g->scale_run, nullptr, nullptr, 0, nullptr, nullptr};
    compress_block<SCHEME, MODE>(t, g->first + static_cast<uint64_t>(j) * a.page_step, src, lds, lane, wave);
}
} // namespace

hipError_t launch_compress_pairs(const PairArgs& a, hipStream_t s)
{
    const uint64_t waves = static_cast<uint64_t>(a.n_pairs) * 2u * a.n_layers;       // one block per wave
    if (waves == 0) return hipSuccess;
    if (!a.pairs || a.page_step == 0 || a.layer_stride % 16u || waves > (1ull << 31)) return hipErrorInvalidValue;
    const uint32_t grid = static_cast<uint32_t>((waves + kWaves - 1) / kWaves);
    return by_scheme_mode<true>(a.scheme, a.quant_mode, [&](auto scheme, auto mode) {
        hipLaunchKernelGGL((k_compress_pairs<decltype(scheme)::value, decltype(mode)::value>), dim3(grid), dim3(kThreads), 0, s, a);
        return hipGetLastError();
    });
}

// The inverse of the pair-gather encoder (Engine::read_pairs: the rollback of committed positions).  Wave i decodes block
// j = i % (2 * n_layers) of position pair i / (2 * n_layers) -- layer j >> 1, kind j & 1, page first + j * page_step of the
// allocation in table row `row` -- into the pair's two rows of that kind, layer_stride bytes further on per layer.  The record is
// found through the allocation table and the page's entry like every fetch (linear, striped, migrated, sealed: one body), and
// decoded by the fetch kernel's own decoders through a RowSink: a row that is not wanted is neither loaded (FP16,
// INT8, FP8, INT4_G32 and its group scales) nor stored (every scheme; the RLE stream and the MXFP4 nibble bytes carry both
// positions and are decoded whole).  Stores are 16 B per lane, 1 KiB per instruction.  One block per wave, no workgroup barrier.
namespace {
template <int SCHEME, int MODE>
__global__ __launch_bounds__(kThreads) void k_read_pairs(ReadPairArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds[SCHEME == kInt8DeltaRle ? kWaves * kDecLdsWords : 4];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kWaves + wave;
    const uint32_t per = 2u * a.n_layers;
    if (i >= static_cast<uint64_t>(a.n_pairs) * per) return;        // (whole waves leave: the body has no workgroup barrier)
    const uint32_t pi = static_cast<uint32_t>(i / per), j = static_cast<uint32_t>(i - static_cast<uint64_t>(pi) * per);
    const ReadPair* g = a.pairs + pi;
    const uint32_t kind = j & 1u;
    const uint64_t off = static_cast<uint64_t>(j >> 1) * a.layer_stride;
    uint8_t* const even = g->row[2u * kind];
    uint8_t* const odd = g->row[2u * kind + 1u];
    const RowSink dst{even ? even + off : nullptr, odd ? odd + off : nullptr};
    if (!dst.even && !dst.odd) return;
    const PageEntry* entries = a.tab[g->table_row].entries;
    PageEntry e{0, 0, 1.0f};
    if (entries) e = entries[g->first + static_cast<uint64_t>(j) * a.page_step];     // a row freed meanwhile decodes as a never-written page
    // the decoders of fetch_decompress_body, told where the two rows go (pool records: trusted streams, tile-planar MXFP4 codes).
    // This block stands in k_read_slots and k_read_slots_ex too, as the same text: called as one device function the compiler
    // schedules the FP16 forms of those two differently and takes 18-20 VGPRs where they have 13-15 (profiles/row_transfer_split.txt)
    const uint8_t* rec = reinterpret_cast<const uint8_t*>(e.pool_addr);
    uint32_t len = e.rec_bytes;
    if (SCHEME == kInt8DeltaRle) {
        if (len > 2u * kBlockElems) len = 2u * kBlockElems;
        uint32_t* region = lds + wave * kDecLdsWords;
        if (!decode_rle_fast<MODE, false, false, RowSink>(rec, len, e.scale, dst, reinterpret_cast<uint8_t*>(region), lane, true))
            decode_rle_general_to<MODE, false, RowSink>(rec, len, e.scale, dst, lane);
    } else if (SCHEME == kInt8) {
        decode_int8<MODE, false, RowSink>(rec, len > kBlockElems ? kBlockElems : len, e.scale, dst, lane);
    } else if (SCHEME == kInt4G32) {
        decode_int4<false, RowSink>(rec, len, dst, lane);
    } else if (SCHEME == kMxFp4) {
        decode_mx4<false, RowSink>(rec, rec + __float_as_uint(e.scale), len, dst, lane);
    } else if (SCHEME == kFp8E4m3) {
        decode_fp8<false, RowSink>(rec, len > kBlockElems ? kBlockElems : len, e.scale, dst, lane);
    } else {
        decode_fp16<false, RowSink>(rec, len > 2u * kBlockElems ? 2u * kBlockElems : len, dst, lane);
    }
}
} // namespace

hipError_t launch_read_pairs(const ReadPairArgs& a, hipStream_t s)
{
    const uint64_t waves = static_cast<uint64_t>(a.n_pairs) * 2u * a.n_layers;       // one block per wave
    if (waves == 0) return hipSuccess;
    if (!a.pairs || !a.tab || a.page_step == 0 || a.layer_stride % 16u || waves > (1ull << 31)) return hipErrorInvalidValue;
    const uint32_t grid = static_cast<uint32_t>((waves + kWaves - 1) / kWaves);
    return by_scheme_mode<false>(a.scheme, a.quant_mode, [&](auto scheme, auto mode) {
        hipLaunchKernelGGL((k_read_pairs<decltype(scheme)::value, decltype(mode)::value>), dim3(grid), dim3(kThreads), 0, s, a);
        return hipGetLastError();
    });
}

// Paged-cache transfers (Engine::read_slots / write_slots): k_read_pairs and k_compress_pairs with a row's address taken from a
// slot mapping on the device and a cache base per layer instead of four host pointers per pair.  Wave i is one page: block
// j < 2 * n_layers (layer layer_begin + (j >> 1), kind j & 1) of flat position pair pp < n_pairs -- i = j * n_pairs + pp (pair
// fastest: neighbouring waves take neighbouring pages of one (layer, kind) region) or i = pp * 2 * n_layers + j (kind_fast: as
// k_read_pairs).  The span of pp is the last one whose exclusive prefix of pair counts is <= pp (binary search as in
// copy_records.hip), the pair first_token / 2 + (pp - prefix), its two positions rows t = 2 * pair - first_token and t + 1 of the
// span.  A row outside [0, n_tokens) is not wanted and its slot is not read; a wanted row whose slot is < 0 or >= n_slots is no
// row either.  Everything up to here is the same for all lanes of a wave (it depends on blockIdx and the wave number alone) and
// is loaded once per wave.
namespace {
typedef SlotWorkT<SlotSpan> SlotWork;      // (found by slot_work, slot_transfer_device.hpp)

template <int SCHEME, int MODE>
__global__ __launch_bounds__(kThreads) void k_read_slots(SlotArgs a)
{
    __shared__ __attribute__((aligned(16))) uint32_t lds[SCHEME == kInt8DeltaRle ? kWaves * kDecLdsWords : 4];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    SlotWork w;
    if (!slot_work(a, wave, &w)) return;
    uint8_t* const base = const_cast<uint8_t*>(w.base);
    const RowSink dst{w.slot[0] >= 0 ? base + static_cast<uint64_t>(w.slot[0]) * 2048u : nullptr,
                      w.slot[1] >= 0 ? base + static_cast<uint64_t>(w.slot[1]) * 2048u : nullptr};
    if (!dst.even && !dst.odd) return;
    const PageEntry* entries = a.tab[w.g->table_row].entries;
    PageEntry e{0, 0, 1.0f};
    if (entries) e = entries[(2ull * a.layer_begin + w.j) * a.page_step + w.pair];  // a row freed meanwhile decodes as a never-written page
    const uint8_t* rec = reinterpret_cast<const uint8_t*>(e.pool_addr);
    uint32_t len = e.rec_bytes;
    if (SCHEME == kInt8DeltaRle) {
        if (len > 2u * kBlockElems) len = 2u * kBlockElems;
        uint32_t* region = lds + wave * kDecLdsWords;
        if (!decode_rle_fast<MODE, false, false, RowSink>(rec, len, e.scale, dst, reinterpret_cast<uint8_t*>(region), lane, true))
            decode_rle_general_to<MODE, false, RowSink>(rec, len, e.scale, dst, lane);
    } else if (SCHEME == kInt8) {
        decode_int8<MODE, false, RowSink>(rec, len > kBlockElems ? kBlockElems : len, e.scale, dst, lane);
    } else if (SCHEME == kInt4G32) {
        decode_int4<false, RowSink>(rec, len, dst, lane);
    } else if (SCHEME == kMxFp4) {
        decode_mx4<false, RowSink>(rec, rec + __float_as_uint(e.scale), len, dst, lane);
    } else if (SCHEME == kFp8E4m3) {
        decode_fp8<false, RowSink>(rec, len > kBlockElems ? kBlockElems : len, e.scale, dst, lane);
    } else {
        decode_fp16<false, RowSink>(rec, len > 2u * kBlockElems ? 2u * kBlockElems : len, dst, lane);
    }
}

// The encoder body with its third source form: beside the contiguous image (SrcRun) and the four row pointers of a commit, the
// two rows of a page read from the slots of a paged cache.  No row (a padding slot) reads the launch's 2048 zero bytes: the
// record of a zero row, and never memory outside the cache.
template <int SCHEME, int MODE>
__global__ __launch_bounds__(kThreads) void k_compress_slots(SlotArgs a)
{
    SPECKV_ENC_LDS(SCHEME);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    SlotWork w;
    if (!slot_work(a, __builtin_amdgcn_readfirstlane(wave), &w)) return;
    const SrcPair src{w.slot[0] >= 0 ? w.base + static_cast<uint64_t>(w.slot[0]) * 2048u : a.zeros,
                      w.slot[1] >= 0 ? w.base + static_cast<uint64_t>(w.slot[1]) * 2048u : a.zeros};
    PageEntry* entries = w.g->entries;
    __builtin_assume(entries != nullptr);
    const EncTarget t{entries, w.g->scale_tab, w.g->region_pages, w.g->scale_run, nullptr, nullptr, 0, nullptr, nullptr};
    compress_block<SCHEME, MODE>(t, (2ull * a.layer_begin + w.j) * a.page_step + w.pair, src, lds, lane, wave);
}

// what both launchers ask of a SlotArgs; *grid = one block per wave
bool slot_args_ok(const SlotArgs& a, uint32_t* grid)
{
    const uint64_t waves = static_cast<uint64_t>(a.n_pairs) * 2u * a.n_layers;
    if (!a.spans || !a.caches || !a.slots || a.n_spans == 0 || a.page_step == 0 || a.kind_stride % 16u || waves > (1ull << 31)) return false;
    *grid = static_cast<uint32_t>((waves + kWaves - 1) / kWaves);
    return true;
}
} // namespace

hipError_t launch_compress_slots(const SlotArgs& a, hipStream_t s)
{
    if (a.n_pairs == 0 || a.n_layers == 0) return hipSuccess;
    uint32_t grid = 0;
    if (!slot_args_ok(a, &grid) || !a.zeros) return hipErrorInvalidValue;
    return by_scheme_mode<true>(a.scheme, a.quant_mode, [&](auto scheme, auto mode) {
        hipLaunchKernelGGL((k_compress_slots<decltype(scheme)::value, decltype(mode)::value>), dim3(grid), dim3(kThreads), 0, s, a);
        return hipGetLastError();
    });
}

hipError_t launch_read_slots(const SlotArgs& a, hipStream_t s)
{
    if (a.n_pairs == 0 || a.n_layers == 0) return hipSuccess;
    uint32_t grid = 0;
    if (!slot_args_ok(a, &grid) || !a.tab) return hipErrorInvalidValue;
    return by_scheme_mode<false>(a.scheme, a.quant_mode, [&](auto scheme, auto mode) {
        hipLaunchKernelGGL((k_read_slots<decltype(scheme)::value, decltype(mode)::value>), dim3(grid), dim3(kThreads), 0, s, a);
        return hipGetLastError();
    });
}

// The two kernels above for caches that hold bf16 and for spans with held rows (SlotExArgs, kernels.hpp).  Waves [0, n_pairs *
// 2 * n_layers) are the pages of k_read_slots / k_compress_slots, found by the same slot_work; behind them wave m = span * 2 *
// n_layers + j moves the one position of span `span` that travels between a held row and a slot, for (layer, kind) j: 2048 bytes,
// two 16-byte loads and stores per lane, converted in registers where the cache holds bf16, no record touched.  Which way a wave
// goes depends on blockIdx and the wave number alone.
namespace {
template <int SCHEME, int MODE, bool BF16>
__global__ __launch_bounds__(kThreads) void k_read_slots_ex(SlotExArgs x)
{
    typedef typename std::conditional<BF16, RowSinkBf16, RowSink>::type Sink;
    __shared__ __attribute__((aligned(16))) uint32_t lds[SCHEME == kInt8DeltaRle ? kWaves * kDecLdsWords : 4];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kWaves + wave;
    const uint64_t n_dec = static_cast<uint64_t>(x.a.n_pairs) * 2u * x.a.n_layers;
    if (i >= n_dec) {                                                // a held row into the slot of the span's last position
        uint8_t *held_row = nullptr, *cache_row = nullptr;
        if (move_work(x, i - n_dec, false, &held_row, &cache_row) && cache_row) move_row(held_row, cache_row, lane, BF16 ? kMoveToBf16 : kMoveCopy);
        return;
    }
    SlotWork w;
    if (!slot_work(x.a, wave, &w)) return;
    uint8_t* const base = const_cast<uint8_t*>(w.base);
    const Sink dst{w.slot[0] >= 0 ? base + static_cast<uint64_t>(w.slot[0]) * 2048u : nullptr,
                   w.slot[1] >= 0 ? base + static_cast<uint64_t>(w.slot[1]) * 2048u : nullptr};
    if (!dst.even && !dst.odd) return;
    const PageEntry* entries = x.a.tab[w.g->table_row].entries;
    PageEntry e{0, 0, 1.0f};
    if (entries) e = entries[(2ull * x.a.layer_begin + w.j) * x.a.page_step + w.pair];
    const uint8_t* rec = reinterpret_cast<const uint8_t*>(e.pool_addr);
    uint32_t len = e.rec_bytes;
    if (SCHEME == kInt8DeltaRle) {
        if (len > 2u * kBlockElems) len = 2u * kBlockElems;
        uint32_t* region = lds + wave * kDecLdsWords;
        if (!decode_rle_fast<MODE, false, false, Sink>(rec, len, e.scale, dst, reinterpret_cast<uint8_t*>(region), lane, true))
            decode_rle_general_to<MODE, false, Sink>(rec, len, e.scale, dst, lane);
    } else if (SCHEME == kInt8) {
        decode_int8<MODE, false, Sink>(rec, len > kBlockElems ? kBlockElems : len, e.scale, dst, lane);
    } else if (SCHEME == kInt4G32) {
        decode_int4<false, Sink>(rec, len, dst, lane);
    } else if (SCHEME == kMxFp4) {
        decode_mx4<false, Sink>(rec, rec + __float_as_uint(e.scale), len, dst, lane);
    } else if (SCHEME == kFp8E4m3) {
        decode_fp8<false, Sink>(rec, len > kBlockElems ? kBlockElems : len, e.scale, dst, lane);
    } else {
        decode_fp16<false, Sink>(rec, len > 2u * kBlockElems ? 2u * kBlockElems : len, dst, lane);
    }
}

template <int SCHEME, int MODE>
__global__ __launch_bounds__(kThreads) void k_compress_slots_ex(SlotExArgs x)
{
    SPECKV_ENC_LDS(SCHEME);
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
    SlotWork w;
    if (!slot_work(x.a, uwave, &w)) return;
    SrcPairMixed src{w.slot[0] >= 0 ? w.base + static_cast<uint64_t>(w.slot[0]) * 2048u : x.a.zeros,
                     w.slot[1] >= 0 ? w.base + static_cast<uint64_t>(w.slot[1]) * 2048u : x.a.zeros, bf16, bf16};
    if (x.held && 2u * w.pair < w.g->first_token) {                  // the pair begins one position in front of the span: its held row
        const uint64_t h = x.held[w.g - x.a.spans].in[w.j & 1u];
        if (h) {
            src.lo = reinterpret_cast<const uint8_t*>(h) + static_cast<uint64_t>(w.j >> 1) * x.held_stride;
            src.lo_bf16 = false;
        }
    }
    PageEntry* entries = w.g->entries;
    __builtin_assume(entries != nullptr);
    const EncTarget t{entries, w.g->scale_tab, w.g->region_pages, w.g->scale_run, nullptr, nullptr, 0, nullptr, nullptr};
    compress_block<SCHEME, MODE>(t, (2ull * x.a.layer_begin + w.j) * x.a.page_step + w.pair, src, lds, lane, wave);
}

// The two _ex kernels with a per-channel K factor (SlotKmulArgs, kernels.hpp), as overloads on the argument struct: the kernels of
// this unit are the k_(read|compress)_(pairs|slots)[_ex] families and nothing else (tests/test_commit_cpu.py reads the symbols).
// The waves, their work and every address are the _ex kernels'; a K wave (j & 1 == 0: blockIdx and the wave number alone) takes the
// scaled sink or source with the factor row of its layer, a V wave the sink or source of the _ex kernels and loads no factor.
// The decoders of a page entry, told where the rows go: here one device function for the two sinks of a kernel (the text that
// stands three times above, for the reason given in k_read_pairs).
template <int SCHEME, int MODE, class SINK>
__device__ __forceinline__ void decode_entry(const PageEntry& e, const SINK& dst, uint32_t* lds, uint32_t wave, uint32_t lane)
{
    const uint8_t* rec = reinterpret_cast<const uint8_t*>(e.pool_addr);
    uint32_t len = e.rec_bytes;
    if (SCHEME == kInt8DeltaRle) {
        if (len > 2u * kBlockElems) len = 2u * kBlockElems;
        uint32_t* region = lds + wave * kDecLdsWords;
        if (!decode_rle_fast<MODE, false, false, SINK>(rec, len, e.scale, dst, reinterpret_cast<uint8_t*>(region), lane, true))
            decode_rle_general_to<MODE, false, SINK>(rec, len, e.scale, dst, lane);
    } else if (SCHEME == kInt8) {
        decode_int8<MODE, false, SINK>(rec, len > kBlockElems ? kBlockElems : len, e.scale, dst, lane);
    } else if (SCHEME == kInt4G32) {
        decode_int4<false, SINK>(rec, len, dst, lane);
    } else if (SCHEME == kMxFp4) {
        decode_mx4<false, SINK>(rec, rec + __float_as_uint(e.scale), len, dst, lane);
    } else if (SCHEME == kFp8E4m3) {
        decode_fp8<false, SINK>(rec, len > kBlockElems ? kBlockElems : len, e.scale, dst, lane);
    } else {
        decode_fp16<false, SINK>(rec, len > 2u * kBlockElems ? 2u * kBlockElems : len, dst, lane);
    }
}
// move_row for a K row: every element times the factor of its channel, rounded once to the destination's type (src == nullptr:
// zeros, as they are)
__device__ __forceinline__ void move_row_mul(const uint8_t* src, uint8_t* dst, const uint8_t* mul, uint32_t lane, int conv)
{
#pragma unroll
    for (uint32_t h = 0; h < 2u; ++h) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (src) {
            v = ld16(src + 1024u * h + 16u * lane);
            const uint4 m = ld16(mul + 1024u * h + 16u * lane);
            v = conv == kMoveToBf16 ? mul_half8_to_bf16(v, m) : conv == kMoveFromBf16 ? mul_bf16_to_half8(v, m) : mul_half8(v, m);
        }
        st16(dst + 1024u * h + 16u * lane, v);
    }
}

template <int SCHEME, int MODE, bool BF16>
__global__ __launch_bounds__(kThreads) void k_read_slots_ex(SlotKmulArgs y)
{
    typedef typename std::conditional<BF16, RowSinkBf16, RowSink>::type Sink;
    typedef typename std::conditional<BF16, RowSinkBf16Mul, RowSinkMul>::type SinkMul;
    __shared__ __attribute__((aligned(16))) uint32_t lds[SCHEME == kInt8DeltaRle ? kWaves * kDecLdsWords : 4];
    const SlotExArgs& x = y.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kWaves + wave;
    const uint64_t n_dec = static_cast<uint64_t>(x.a.n_pairs) * 2u * x.a.n_layers;
    if (i >= n_dec) {                                                // a held row into the slot of the span's last position
        const uint64_t m = i - n_dec;
        uint8_t *held_row = nullptr, *cache_row = nullptr;
        if (!move_work(x, m, false, &held_row, &cache_row) || !cache_row) return;
        const uint32_t j = static_cast<uint32_t>(m % (2u * x.a.n_layers));
        if (j & 1u) move_row(held_row, cache_row, lane, BF16 ? kMoveToBf16 : kMoveCopy);
        else move_row_mul(held_row, cache_row, y.k_mul + static_cast<uint64_t>(j >> 1) * y.k_mul_stride, lane, BF16 ? kMoveToBf16 : kMoveCopy);
        return;
    }
    SlotWork w;
    if (!slot_work(x.a, wave, &w)) return;
    uint8_t* const base = const_cast<uint8_t*>(w.base);
    uint8_t* const even = w.slot[0] >= 0 ? base + static_cast<uint64_t>(w.slot[0]) * 2048u : nullptr;
    uint8_t* const odd = w.slot[1] >= 0 ? base + static_cast<uint64_t>(w.slot[1]) * 2048u : nullptr;
    if (!even && !odd) return;
    const PageEntry* entries = x.a.tab[w.g->table_row].entries;
    PageEntry e{0, 0, 1.0f};
    if (entries) e = entries[(2ull * x.a.layer_begin + w.j) * x.a.page_step + w.pair];
    if (w.j & 1u) decode_entry<SCHEME, MODE, Sink>(e, Sink{even, odd}, lds, wave, lane);
    else decode_entry<SCHEME, MODE, SinkMul>(e, SinkMul{even, odd, y.k_mul + static_cast<uint64_t>(w.j >> 1) * y.k_mul_stride}, lds, wave, lane);
}

template <int SCHEME, int MODE>
__global__ __launch_bounds__(kThreads) void k_compress_slots_ex(SlotKmulArgs y)
{
    SPECKV_ENC_LDS(SCHEME);
    const SlotExArgs& x = y.x;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    const uint32_t uwave = __builtin_amdgcn_readfirstlane(wave);
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kWaves + uwave;
    const uint64_t n_enc = static_cast<uint64_t>(x.a.n_pairs) * 2u * x.a.n_layers;
    const bool bf16 = x.bf16 != 0u;
    if (i >= n_enc) {                                                // the span's last position into its held row (no row: zeros)
        const uint64_t m = i - n_enc;
        uint8_t *held_row = nullptr, *cache_row = nullptr;
        if (!move_work(x, m, true, &held_row, &cache_row)) return;
        const uint32_t j = static_cast<uint32_t>(m % (2u * x.a.n_layers));
        if (j & 1u) move_row(cache_row, held_row, lane, bf16 ? kMoveFromBf16 : kMoveCopy);
        else move_row_mul(cache_row, held_row, y.k_mul + static_cast<uint64_t>(j >> 1) * y.k_mul_stride, lane, bf16 ? kMoveFromBf16 : kMoveCopy);
        return;
    }
    SlotWork w;
    if (!slot_work(x.a, uwave, &w)) return;
    const uint8_t* lo = w.slot[0] >= 0 ? w.base + static_cast<uint64_t>(w.slot[0]) * 2048u : nullptr;      // nullptr: a padding slot
    const uint8_t* const hi = w.slot[1] >= 0 ? w.base + static_cast<uint64_t>(w.slot[1]) * 2048u : nullptr;
    bool lo_cache = lo != nullptr;                                   // the row is read from the cache: bf16 where the cache is, K scaled
    if (x.held && 2u * w.pair < w.g->first_token) {                  // the pair begins one position in front of the span: its held row
        const uint64_t h = x.held[w.g - x.a.spans].in[w.j & 1u];
        if (h) {
            lo = reinterpret_cast<const uint8_t*>(h) + static_cast<uint64_t>(w.j >> 1) * x.held_stride;
            lo_cache = false;
        }
    }
    PageEntry* entries = w.g->entries;
    __builtin_assume(entries != nullptr);
    const EncTarget t{entries, w.g->scale_tab, w.g->region_pages, w.g->scale_run, nullptr, nullptr, 0, nullptr, nullptr};
    const uint64_t page = (2ull * x.a.layer_begin + w.j) * x.a.page_step + w.pair;
    if (w.j & 1u) {
        const SrcPairMixed src{lo ? lo : x.a.zeros, hi ? hi : x.a.zeros, bf16 && lo_cache, bf16 && hi != nullptr};
        compress_block<SCHEME, MODE>(t, page, src, lds, lane, wave);
    } else {
        const uint8_t* mul = y.k_mul + static_cast<uint64_t>(w.j >> 1) * y.k_mul_stride;
        const SrcPairScaled src{lo ? lo : x.a.zeros, hi ? hi : x.a.zeros, bf16 && lo_cache, bf16 && hi != nullptr, lo_cache ? mul : nullptr, hi ? mul : nullptr};
        compress_block<SCHEME, MODE>(t, page, src, lds, lane, wave);
    }
}

// what both launchers ask of a SlotExArgs; *grid = one page or one moved row per wave, 0 = nothing to do
bool slot_ex_args_ok(const SlotExArgs& x, uint32_t* grid)
{
    const SlotArgs& a = x.a;
    const uint64_t waves = static_cast<uint64_t>(a.n_pairs) * 2u * a.n_layers + x.n_moves;
    if (!a.spans || !a.caches || !a.slots || a.n_spans == 0 || a.page_step == 0 || a.kind_stride % 16u || x.held_stride % 16u) return false;
    if ((x.n_moves != 0u && (!x.held || x.n_moves != static_cast<uint64_t>(a.n_spans) * 2u * a.n_layers)) || waves > (1ull << 31)) return false;
    *grid = static_cast<uint32_t>((waves + kWaves - 1) / kWaves);
    return true;
}
} // namespace

hipError_t launch_compress_slots_ex(const SlotExArgs& x, hipStream_t s)
{
    if (x.a.n_layers == 0) return hipSuccess;
    uint32_t grid = 0;
    if (!slot_ex_args_ok(x, &grid) || !x.a.zeros) return hipErrorInvalidValue;
    if (grid == 0) return hipSuccess;
    return by_scheme_mode<true>(x.a.scheme, x.a.quant_mode, [&](auto scheme, auto mode) {
        hipLaunchKernelGGL((k_compress_slots_ex<decltype(scheme)::value, decltype(mode)::value>), dim3(grid), dim3(kThreads), 0, s, x);
        return hipGetLastError();
    });
}

hipError_t launch_read_slots_ex(const SlotExArgs& x, hipStream_t s)
{
    if (x.a.n_layers == 0) return hipSuccess;
    uint32_t grid = 0;
    if (!slot_ex_args_ok(x, &grid) || !x.a.tab) return hipErrorInvalidValue;
    if (grid == 0) return hipSuccess;
    return by_scheme_mode<false>(x.a.scheme, x.a.quant_mode, [&](auto scheme, auto mode) {
        constexpr int SCHEME = decltype(scheme)::value, MODE = decltype(mode)::value;
        if (x.bf16) hipLaunchKernelGGL((k_read_slots_ex<SCHEME, MODE, true>), dim3(grid), dim3(kThreads), 0, s, x);
        else hipLaunchKernelGGL((k_read_slots_ex<SCHEME, MODE, false>), dim3(grid), dim3(kThreads), 0, s, x);
        return hipGetLastError();
    });
}

// The _ex launches with the K factor: what the _ex launchers ask, and a factor table that 16-byte loads can read
hipError_t launch_compress_slots_kmul(const SlotKmulArgs& y, hipStream_t s)
{
    if (y.x.a.n_layers == 0) return hipSuccess;
    uint32_t grid = 0;
    if (!slot_ex_args_ok(y.x, &grid) || !y.x.a.zeros) return hipErrorInvalidValue;
    if (!y.k_mul || reinterpret_cast<uintptr_t>(y.k_mul) % 16u || y.k_mul_stride % 16u) return hipErrorInvalidValue;
    if (grid == 0) return hipSuccess;
    return by_scheme_mode<true>(y.x.a.scheme, y.x.a.quant_mode, [&](auto scheme, auto mode) {
        hipLaunchKernelGGL((k_compress_slots_ex<decltype(scheme)::value, decltype(mode)::value>), dim3(grid), dim3(kThreads), 0, s, y);
        return hipGetLastError();
    });
}

hipError_t launch_read_slots_kmul(const SlotKmulArgs& y, hipStream_t s)
{
    if (y.x.a.n_layers == 0) return hipSuccess;
    uint32_t grid = 0;
    if (!slot_ex_args_ok(y.x, &grid) || !y.x.a.tab) return hipErrorInvalidValue;
    if (!y.k_mul || reinterpret_cast<uintptr_t>(y.k_mul) % 16u || y.k_mul_stride % 16u) return hipErrorInvalidValue;
    if (grid == 0) return hipSuccess;
    return by_scheme_mode<false>(y.x.a.scheme, y.x.a.quant_mode, [&](auto scheme, auto mode) {
        constexpr int SCHEME = decltype(scheme)::value, MODE = decltype(mode)::value;
        if (y.x.bf16) hipLaunchKernelGGL((k_read_slots_ex<SCHEME, MODE, true>), dim3(grid), dim3(kThreads), 0, s, y);
        else hipLaunchKernelGGL((k_read_slots_ex<SCHEME, MODE, false>), dim3(grid), dim3(kThreads), 0, s, y);
        return hipGetLastError();
    });
}

} // namespace speckv
