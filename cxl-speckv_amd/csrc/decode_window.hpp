// cxl-speckv_amd/csrc/decode_window.hpp -- the walk rule of the windowed decode attention (speckv_ext_attend_batch_window,
// speckv_ext_attend_batch_plan_window) as pure functions usable from host and device: where a member's launch begins, how many leading
// positions of its first tile are masked and how many pages it walks.  Engine::gather_members (engine_attend.cpp) fills the descriptors
// from them, speckv_ext_decode_window_range (c_api.cpp) exports the same body and the connector restates it
// (SpeckvKVConnector.decode_window_range), so the engine, the export and the CPU tests agree by construction.  Plain C++17; under hipcc
// the functions are host and device functions.
//
// A member has `length` positions, the step's own included (the connector's state when attend() runs, after append).  stored =
// length & ~1 of them lie in the pool; with an odd length the last one is the tail held outside the pool.  The query sits at
// P = length - 1 and, under a window W >= 1, sees the absolute positions [lo, P], lo = max(0, length - W).  W = 0: no window (lo = 0).
// The pool part is [lo, stored); the launch walks from the tile of lo, for all three formats:
//     begin = lo & ~31      skip = lo - begin (0..31, may be odd)      n_pages = (stored - begin) / 2
// lo == stored (W = 1 with an odd length, or a length below 2): no pool position, n_pages = 0 (the member has its tail at most).
// Aligning begin to the tile costs one extra tile at most and keeps FP8 on its scale table, MXFP4 on its tile-planar records and the
// tiles of the launch inside the region exactly where they were without a window.  The tiles walked never exceed
// decode_window_tiles_bound(W) = ceil((W + 31) / 32), whatever the length.
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SPECKV_HD __host__ __device__
#else
#define SPECKV_HD
#endif

namespace speckv {

struct DecodeWindowRange { uint32_t begin, skip, n_pages; };

// lo: the first absolute position the query of a member of `length` positions sees
SPECKV_HD inline uint32_t decode_window_lo(uint32_t length, uint32_t window)
{
    return window && length > window ? length - window : 0u;
}

SPECKV_HD inline DecodeWindowRange decode_window_range(uint32_t length, uint32_t window)
{
    const uint32_t stored = length & ~1u, lo = decode_window_lo(length, window);
    const uint32_t begin = lo & ~31u;
    return DecodeWindowRange{begin, lo - begin, lo < stored ? (stored - begin) / 2u : 0u};
}

// the tiles (of 32 positions) a member walks at most under window W >= 1
SPECKV_HD inline uint32_t decode_window_tiles_bound(uint32_t window)
{
    return static_cast<uint32_t>((static_cast<uint64_t>(window) + 31u + 31u) / 32u);
}

} // namespace speckv
