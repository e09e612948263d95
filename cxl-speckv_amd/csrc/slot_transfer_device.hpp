// cxl-speckv_amd/csrc/slot_transfer_device.hpp -- what the paged-cache transfer kernels of row_transfer.hip (one allocation per
// span) and of row_transfer_kv.hip (the split pool: a K and a V allocation per span) share (device code only): which page a wave
// owns, and the move of a held row.  Templates over the argument struct, because the two span descriptors differ (SlotSpan,
// SlotSpanKV: kernels.hpp); the fields they read carry the same names in both.  Everything is __forceinline__: neither unit gets
// an out-of-line function from here.
#pragma once
#include "kernels.hpp"
#include "block_codec_device.hpp"

namespace speckv {
namespace {

// Wave i is one page: block j < 2 * n_layers (layer layer_begin + (j >> 1), kind j & 1) of flat position pair pp < n_pairs -- i =
// j * n_pairs + pp (pair fastest: neighbouring waves take neighbouring pages of one (layer, kind) region) or i = pp * 2 * n_layers
// + j (kind_fast: as k_read_pairs).  The span of pp is the last one whose exclusive prefix of pair counts is <= pp (binary search as
// in copy_records.hip), the pair first_token / 2 + (pp - prefix), its two positions rows t = 2 * pair - first_token and t + 1 of the
// span.  A row outside [0, n_tokens) is not wanted and its slot is not read; a wanted row whose slot is < 0 or >= n_slots is no
// row either.  Everything here is the same for all lanes of a wave (it depends on blockIdx and the wave number alone) and is
// loaded once per wave.
template <class SPAN>
struct SlotWorkT {
    const SPAN* g;
    uint32_t j;                       // (layer, kind) of the launch: layer_begin + (j >> 1), j & 1
    uint32_t pair;                    // position pair of the allocation
    const uint8_t* base;              // caches[j >> 1] + (j & 1) * kind_stride
    int64_t  slot[2];                 // of the even and the odd position; -1 = no row
};
template <class ARGS, class SPAN>
__device__ __forceinline__ bool slot_work(const ARGS& a, uint32_t wave, SlotWorkT<SPAN>* w)
{
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * kWaves + wave;
    const uint32_t per = 2u * a.n_layers;
    if (i >= static_cast<uint64_t>(a.n_pairs) * per) return false;   // (whole waves leave: the bodies have no workgroup barrier)
    uint32_t pp, j;
    if (a.kind_fast) { pp = static_cast<uint32_t>(i / per); j = static_cast<uint32_t>(i - static_cast<uint64_t>(pp) * per); }
    else             { j = static_cast<uint32_t>(i / a.n_pairs); pp = static_cast<uint32_t>(i - static_cast<uint64_t>(j) * a.n_pairs); }
    uint32_t lo = 0, hi = a.n_spans;                                 // spans without pairs share their successor's prefix and are passed over
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.spans[mid].first_pair <= pp) lo = mid; else hi = mid;
    }
    const SPAN* g = a.spans + lo;
    const uint32_t first = g->first_token, n = g->n_tokens;
    const uint32_t pair = (first >> 1) + (pp - g->first_pair);
    const int64_t t0 = 2ll * pair - static_cast<int64_t>(first);     // -1 where the span begins on an odd position
    const int64_t n_slots = static_cast<int64_t>(a.n_slots);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int64_t t = t0 + h;
        int64_t s = -1;
        if (t >= 0 && t < static_cast<int64_t>(n)) s = a.slots[g->slot_begin + static_cast<uint64_t>(t)];
        w->slot[h] = (s >= 0 && s < n_slots) ? s : -1;
    }
    w->g = g;
    w->j = j;
    w->pair = pair;
    w->base = reinterpret_cast<const uint8_t*>(a.caches[j >> 1]) + static_cast<uint64_t>(j & 1u) * a.kind_stride;
    return true;
}

// Behind the page waves, wave m = span * 2 * n_layers + j moves the one position of span `span` that travels between a held row and
// a slot, for (layer, kind) j: 2048 bytes, two 16-byte loads and stores per lane, converted in registers where the cache holds
// bf16, no record touched.  Which way a wave goes depends on blockIdx and the wave number alone.
enum { kMoveCopy = 0, kMoveToBf16 = 1, kMoveFromBf16 = 2 };
__device__ __forceinline__ void move_row(const uint8_t* src, uint8_t* dst, uint32_t lane, int conv)     // src == nullptr: zeros
{
#pragma unroll
    for (uint32_t h = 0; h < 2u; ++h) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        if (src) v = ld16(src + 1024u * h + 16u * lane);
        if (conv == kMoveToBf16) v = half8_to_bf16(v);
        else if (conv == kMoveFromBf16) v = bf16_to_half8(v);
        st16(dst + 1024u * h + 16u * lane, v);
    }
}
// move wave m's work: false = it has none.  *held_row = the held row of its span and (layer, kind), *cache_row = the row of the
// span's last position in the cache, nullptr where its slot names no row
template <class EXARGS>
__device__ __forceinline__ bool move_work(const EXARGS& x, uint64_t m, bool out, uint8_t** held_row, uint8_t** cache_row)
{
    if (m >= x.n_moves) return false;
    const uint32_t per = 2u * x.a.n_layers;
    const uint32_t sp = static_cast<uint32_t>(m / per), j = static_cast<uint32_t>(m - static_cast<uint64_t>(sp) * per);
    const uint64_t h = out ? x.held[sp].out[j & 1u] : x.held[sp].in[j & 1u];
    if (!h) return false;
    const auto* g = x.a.spans + sp;
    if (g->n_tokens == 0) return false;
    const int64_t s = x.a.slots[g->slot_begin + g->n_tokens - 1u];
    *held_row = reinterpret_cast<uint8_t*>(h) + static_cast<uint64_t>(j >> 1) * x.held_stride;
    *cache_row = (s >= 0 && s < static_cast<int64_t>(x.a.n_slots))
        ? reinterpret_cast<uint8_t*>(x.a.caches[j >> 1]) + static_cast<uint64_t>(j & 1u) * x.a.kind_stride + static_cast<uint64_t>(s) * 2048u : nullptr;
    return true;
}

} // namespace
} // namespace speckv
