// cxl-speckv_amd/csrc/chunk_window.hpp -- the walk rule of the windowed chunk attention (speckv_ext_attend_chunk_window) as pure
// functions usable from host and device: the lower bound of a query row, the first tile a query block walks and the first pool tile
// any block of a sequence walks.  k_attend_chunk<.., WINDOW> (attend_chunk.hip) walks by them, Engine::attend_chunk (engine_chunk.cpp)
// plans the pieces of the split form from them and speckv_ext_chunk_window_walk (c_api.cpp) exports the same bodies, so the kernel,
// the export and the CPU tests agree by construction.  Plain C++17; under hipcc the functions are host and device functions.
//
// Sequence i holds pos_end (even) stored positions, base in {0, 1} held tail positions and n_q new positions; query position j sits
// at the absolute position P = pos_end + base + j and, under a window W >= 1, sees the absolute positions [lo(j), P],
// lo(j) = max(0, P + 1 - W).  W = 0: no window (lo = 0).  The kernel's tile index counts the pool tiles first (n_pool =
// ceil(pos_end / 32)), then the held tiles (held position t = the absolute position pos_end + t).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SPECKV_HD __host__ __device__
#else
#define SPECKV_HD
#endif

namespace speckv {

// lo(j): the first absolute position query position j sees
SPECKV_HD inline uint32_t chunk_window_lo(uint32_t pos_end, uint32_t base, uint32_t j, uint32_t window)
{
    const uint32_t seen = pos_end + base + j + 1u;            // P + 1: what the row sees without a window
    return window && seen > window ? seen - window : 0u;
}

// The first tile the query block whose first position is j_first walks: the tile of lo(j_first) -- a pool tile while that position
// is stored, otherwise the held tile of lo - pos_end.  Every later row of the block has a higher bound, every tile behind this one
// up to the block's last (n_pool + ((base + j_last) >> 5)) holds a position a live row of the block sees.
SPECKV_HD inline uint32_t chunk_window_first_tile(uint32_t pos_end, uint32_t base, uint32_t j_first, uint32_t window)
{
    const uint32_t lo = chunk_window_lo(pos_end, base, j_first, window);
    return lo < pos_end ? lo >> 5 : ((pos_end + 31u) >> 5) + ((lo - pos_end) >> 5);
}

// The first POOL tile any block of the sequence walks (ChunkSeq::first_tile; its pieces are planned over the pool tiles from here):
// block 0's first tile, or n_pool where position 0 already sees no stored position.
SPECKV_HD inline uint32_t chunk_window_first_pool_tile(uint32_t pos_end, uint32_t base, uint32_t window)
{
    const uint32_t lo = chunk_window_lo(pos_end, base, 0u, window);
    return lo < pos_end ? lo >> 5 : (pos_end + 31u) >> 5;
}

// Per (sequence, query block), sequences in order and a sequence's blocks in order (ceil(n_q / (64 / rows_per_pos)) each): the first
// tile of the walk and its tile count, n_tiles - t_first with n_tiles = n_pool + ((base + j_last) >> 5) + 1.  base may be null (no
// tails).  false: rows_per_pos is none of 1, 2, 4, 8, 16, an odd pos_end or a base above 1 (what was written up to there stays).
inline bool chunk_window_walk(uint32_t n_seq, const uint32_t* pos_end, const uint32_t* base, const uint32_t* n_q, uint32_t rows_per_pos,
                              uint32_t window, uint32_t* first_tile, uint32_t* n_walked)
{
    if (rows_per_pos == 0 || rows_per_pos > 16u || (rows_per_pos & (rows_per_pos - 1u))) return false;
    const uint32_t per_blk = 64u / rows_per_pos;
    uint64_t at = 0;
    for (uint32_t i = 0; i < n_seq; ++i) {
        const uint32_t b = base ? base[i] : 0u;
        if (pos_end[i] % 2u || b > 1u) return false;
        const uint32_t n_pool = (pos_end[i] + 31u) >> 5;
        for (uint32_t j_first = 0; j_first < n_q[i]; j_first += per_blk, ++at) {
            const uint32_t j_last = (n_q[i] - j_first > per_blk ? j_first + per_blk : n_q[i]) - 1u;
            const uint32_t t_first = chunk_window_first_tile(pos_end[i], b, j_first, window);
            first_tile[at] = t_first;
            n_walked[at] = n_pool + ((b + j_last) >> 5) + 1u - t_first;
        }
    }
    return true;
}

} // namespace speckv
