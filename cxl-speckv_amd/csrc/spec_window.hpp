// cxl-speckv_amd/csrc/spec_window.hpp -- the walk rule of the split pool's multi-position step under a sliding window
// (speckv_ext_attend_kv_spec_window, k_attend_k8v4<true, true>) as pure functions usable from host and device: where a member's launch
// begins, how many pages it walks, and how many leading positions of the walk each query row does not see.  Engine::attend_batch_kv
// (engine_attend_kv.cpp) fills the descriptors from them, the kernel (attend_kv.hip) takes its row mask from spec_window_skip,
// speckv_ext_spec_window_range (c_api.cpp) exports the same body and the connector restates it (SpeckvKVConnector.spec_window_range), so
// the engine, the kernel, the export and the CPU tests agree by construction.  Plain C++17; under hipcc the functions are host and
// device functions.
//
// A member has `length` committed positions; stored = length & ~1 of them lie in the pool, with an odd length the last one is the tail
// held outside it.  The step's new positions follow: a draft node of depth d (0 = a root of the step) sits at the absolute position
// length + d and, under a window W >= 1, sees [lo(d), length + d] with
//     lo(d) = max(0, length + d + 1 - W)
// Its pool part is [lo(d), stored).  What it sees of the held positions (the tail, its ancestors) lies in the caller's mask words alone.
// The query rows of a wave no longer share a lower bound, so the launch walks from the tile of the SHALLOWEST bound and masks per row:
//     begin   = lo(0) & ~31                         (a multiple of 32 positions: a kernel tile stays one MXFP4 storage tile and one group
//                                                    of the K scale table, as in decode_window.hpp)
//     n_pages = lo(0) < stored ? (stored - begin) / 2 : 0
//     rel     = (length + 1) - W - begin            SIGNED, per member: negative while the window has not yet left position 0
//     skip(d) = max(0, rel + min(d, 15))            the leading POSITIONS of the walk a row of depth d does not see
// so that {begin + skip(d) <= p < begin + 2 n_pages} = {lo(d) <= p < stored} for every depth.  Depths above 15 are clamped to 15: a step
// carries SPECKV_HELD_MAX - 1 = 16 new positions at most, so no node is deeper.  rel <= 31, hence skip <= 46: only tiles 0 and 1 of the
// walk can carry a mask, and a deep row may see nothing of tile 0 (or of a short walk) at all.  The tiles walked stay within
// decode_window_tiles_bound(W): stored - begin <= length - (length + 1 - W) + 31.
// THE HOST WALKS FROM DEPTH 0 WHATEVER DEPTHS A CALL CARRIES: a later group of a step (deeper nodes only) starts at the same tile as the
// first and pays one extra, partly masked tile at most; descriptors, pieces and the rel array are the same for every group of a step.
// lo(0) >= stored (W = 1, or W = 2 on an odd length, or nothing stored): no row sees a pool position, n_pages = 0 -- the member is one with
// nothing stored, its rows are the held positions alone.
#pragma once
#include <cstdint>

#include "decode_window.hpp"

namespace speckv {

constexpr uint32_t kSpecWindowMaxDepth = 15u;          // SPECKV_HELD_MAX - 2

struct SpecWindowRange { uint32_t begin; int32_t rel; uint32_t n_pages; };

// lo(d): the first absolute position a node of depth d sees behind `length` committed positions
SPECKV_HD inline uint32_t spec_window_lo(uint32_t length, uint32_t depth, uint32_t window)
{
    const uint64_t end = static_cast<uint64_t>(length) + depth + 1u;
    return end > window ? static_cast<uint32_t>(end - window) : 0u;
}

SPECKV_HD inline SpecWindowRange spec_window_range(uint32_t length, uint32_t window)
{
    const uint32_t stored = length & ~1u, lo = spec_window_lo(length, 0u, window);
    const uint32_t begin = lo & ~31u;
    const int64_t rel = static_cast<int64_t>(length) + 1 - static_cast<int64_t>(window) - static_cast<int64_t>(begin);
    return SpecWindowRange{begin, static_cast<int32_t>(rel < INT32_MIN ? INT32_MIN : rel), lo < stored ? (stored - begin) / 2u : 0u};
}

// skip(d): the leading positions of the member's walk that a row of depth d does not see
SPECKV_HD inline uint32_t spec_window_skip(int32_t rel, uint32_t depth)
{
    const int32_t s = rel + static_cast<int32_t>(depth < kSpecWindowMaxDepth ? depth : kSpecWindowMaxDepth);
    return s > 0 ? static_cast<uint32_t>(s) : 0u;
}

} // namespace speckv
