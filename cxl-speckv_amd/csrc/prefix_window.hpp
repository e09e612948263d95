// cxl-speckv_amd/csrc/prefix_window.hpp -- the walk rule of the shared-prefix fold under a sliding window
// (speckv_ext_attend_prefix_fold_window) as pure functions usable from host and device: the lower bound of a query row over its
// group's prefix and the tiles a group's blocks walk.  k_attend_prefix<.., WINDOW> (attend_prefix.hip) masks by the first,
// Engine::attend_prefix (engine_prefix.cpp) plans by the second and speckv_ext_prefix_window_walk (c_api.cpp) exports the same
// bodies, so the kernel, the engine, the export and the CPU tests agree by construction.  Plain C++17; under hipcc the functions are
// host and device functions.
//
// Member m sees the stored positions [0, prefix_len[m]) of its group's prefix IN FRONT OF its own positions.  own_seen[m] = how many
// of its OWN positions the member's query position of depth 0 sees without a window, itself included (a decode step after append:
// the member's length; a chunk or tree step: pos_end + base + 1; 0: the member holds nothing and the query is judged as sitting
// directly behind the prefix).  The row of depth d (a chain: its index j; a tree: the node's depth) sees own_seen + d own keys, so
// without a window it sees prefix_len + own_seen + d positions in all and under a window W >= 1 the last W of them: of the prefix
// [lo, prefix_len), lo = max(0, prefix_len + own_seen + d - W).  lo >= prefix_len (own_seen + d >= W): the row sees nothing of the
// prefix and is DEAD for the fold.  W = 0: no window (lo = 0).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SPECKV_HD __host__ __device__
#else
#define SPECKV_HD
#endif

namespace speckv {

// lo: the first position of the prefix the row of depth `depth` sees (>= prefix_len: none; the sum is taken in 64 bits and the
// result saturates, so no argument wraps)
SPECKV_HD inline uint32_t prefix_window_lo(uint32_t prefix_len, uint32_t own_seen, uint32_t depth, uint32_t window)
{
    if (!window) return 0u;
    const uint64_t seen = static_cast<uint64_t>(prefix_len) + own_seen + depth;          // what the row sees without a window
    if (seen <= window) return 0u;
    const uint64_t lo = seen - window;
    return lo > 0xFFFFFFFFull ? 0xFFFFFFFFu : static_cast<uint32_t>(lo);
}

// The walk of one group over its n members that are live for the fold: a member counts when n_q > 0, prefix_len > 0 and its
// depth-0 bound is below prefix_len (depths live on the device and are unordered; depth 0 gives a member's lowest bound, so it is a
// safe start for every row).  first_tile = the minimum of those bounds >> 5, max_len = the largest prefix_len of those members; the
// group's blocks walk the tiles [first_tile, ceil(max_len / 32)).  max_len == 0: no such member, the group has no blocks.
// own_seen == null: every member holds nothing of its own (zeros).
struct PrefixWalk { uint32_t first_tile, max_len; };
inline PrefixWalk prefix_window_group(uint32_t n, const uint32_t* prefix_len, const uint32_t* own_seen, const uint32_t* n_q, uint32_t window)
{
    PrefixWalk w{0u, 0u};
    uint32_t lo_min = 0xFFFFFFFFu;
    for (uint32_t m = 0; m < n; ++m) {
        if (!n_q[m] || !prefix_len[m]) continue;
        const uint32_t lo = prefix_window_lo(prefix_len[m], own_seen ? own_seen[m] : 0u, 0u, window);
        if (lo >= prefix_len[m]) continue;
        if (lo < lo_min) lo_min = lo;
        if (prefix_len[m] > w.max_len) w.max_len = prefix_len[m];
    }
    if (w.max_len) w.first_tile = lo_min >> 5;
    return w;
}
inline uint32_t prefix_window_tiles(const PrefixWalk& w) { return w.max_len ? ((w.max_len + 31u) >> 5) - w.first_tile : 0u; }

// Per group g = the members [first_member[g], first_member[g + 1]): first_tile[g] and n_tiles[g] = ceil(max_len / 32) - first_tile
// (0 / 0: a group without a member that is live for the fold).  false: first_member does not ascend from 0 or a prefix_len is odd
// (what was written up to there stays).
inline bool prefix_window_walk(uint32_t n_groups, const uint32_t* first_member, const uint32_t* prefix_len, const uint32_t* own_seen,
                               const uint32_t* n_q, uint32_t window, uint32_t* first_tile, uint32_t* n_tiles)
{
    if (n_groups && first_member[0] != 0u) return false;
    for (uint32_t g = 0; g < n_groups; ++g) {
        const uint32_t m0 = first_member[g], m1 = first_member[g + 1];
        if (m1 < m0) return false;
        for (uint32_t m = m0; m < m1; ++m)
            if (prefix_len[m] % 2u) return false;
        const PrefixWalk w = prefix_window_group(m1 - m0, prefix_len + m0, own_seen ? own_seen + m0 : nullptr, n_q + m0, window);
        first_tile[g] = w.first_tile;
        n_tiles[g] = prefix_window_tiles(w);
    }
    return true;
}

} // namespace speckv
