// cxl-speckv_amd/csrc/chunk_split.hpp -- the piece rule of the split chunk attention (speckv_ext_attend_chunk_split) as ONE pure host
// function: into how many pieces the stored positions of every sequence of a call are cut, and how many 32-position pool tiles a piece
// walks.  Engine::attend_chunk (engine_chunk.cpp) decides with it and speckv_ext_chunk_split_plan (c_api.cpp) exports the same body,
// so the engine, the export and the CPU tests agree by construction.  Plain C++17, no HIP.
#pragma once
#include <cstdint>

namespace speckv {

constexpr uint32_t kChunkSplitsMax = 64;                  // SPECKV_CHUNK_SPLITS_MAX (include/speckv_ext.h)
// Resident workgroups of k_attend_chunk per CU at its occupancy (3 waves per SIMD, 4-wave workgroups, two 17.5 KiB LDS buffers each).
constexpr uint32_t kChunkResidentPerCu = 3;
// The library's rule never makes a piece shorter than this many pool tiles.  A piece's partial costs about 65 KiB of write + read per
// (query block, kv head) -- 32.5 KiB written by the piece, read once by the merge -- while a tile is about 8 KiB of FP8 records per
// head (32 positions x 128 bytes x K and V): below about 32 tiles a piece the merge traffic stops being small against the records.
// A first value from that argument.  Measured (profiles/chunk_split.txt): nothing the rule splits loses with it, but it is
// conservative for the shortest contexts -- at 2k stored positions 8 pieces of 8 tiles ran 1.3-1.5 x faster than the 2 pieces of
// 32 it allows; lowering it wants figures for more than 16 pieces first.
constexpr uint32_t kChunkPieceFloorTiles = 32;

inline uint32_t chunk_pool_tiles(uint32_t pos_end) { return static_cast<uint32_t>((static_cast<uint64_t>(pos_end) + 31u) >> 5); }

// n_splits 1: one piece each.  n_splits N > 1 (forced): min(N, the sequence's pool tiles) pieces, from the sequence alone.
// n_splits 0 (the library's rule): from the whole call -- with G0 = 8 kv heads x the call's query blocks and target =
// kChunkResidentPerCu x n_cus, as many pieces as still fit ONE round of resident workgroups, floor(target / G0), never under
// kChunkPieceFloorTiles tiles a piece; none while G0 > target / 2.  (Measured: rounding UP to the target -- 2 pieces for a
// 512-position chunk of one request, 5 for four 40-node trees -- starts a second round and lost 4-11 % against no pieces, resp. 25 %
// against 4 pieces: profiles/archive/chunk_split_before.txt against profiles/chunk_split.txt.)
// Then tiles_per_piece = ceil(pool tiles / pieces) and pieces = ceil(pool tiles / tiles_per_piece): no piece is empty.  A sequence
// without pool tiles has one piece of 0 pool tiles (its held positions).  false: rows_per_pos is none of 1, 2, 4, 8, 16 or
// n_splits > kChunkSplitsMax (nothing is written).
inline bool chunk_split_plan(uint32_t n_seq, const uint32_t* pos_end, const uint32_t* n_q, uint32_t rows_per_pos, uint32_t n_splits,
                             uint32_t n_cus, uint32_t* pieces, uint32_t* tiles_per_piece)
{
    if (rows_per_pos == 0 || rows_per_pos > 16u || (rows_per_pos & (rows_per_pos - 1u)) || n_splits > kChunkSplitsMax) return false;
    uint32_t most = n_splits;
    if (n_splits == 0) {
        const uint32_t per_block = 64u / rows_per_pos;
        uint64_t blocks = 0;
        for (uint32_t i = 0; i < n_seq; ++i) blocks += (static_cast<uint64_t>(n_q[i]) + per_block - 1u) / per_block;
        const uint64_t g0 = 8u * blocks, target = static_cast<uint64_t>(kChunkResidentPerCu) * (n_cus ? n_cus : 256u);
        const uint64_t want = g0 == 0 || g0 >= target ? 1u : target / g0;
        most = static_cast<uint32_t>(want < kChunkSplitsMax ? want : kChunkSplitsMax);
    }
    for (uint32_t i = 0; i < n_seq; ++i) {
        const uint32_t n_pool = chunk_pool_tiles(pos_end[i]);
        uint32_t p = n_splits == 0 ? n_pool / kChunkPieceFloorTiles : n_pool;
        p = p < 1u ? 1u : p > most ? most : p;
        const uint32_t tpp = (n_pool + p - 1u) / p;
        pieces[i] = tpp ? (n_pool + tpp - 1u) / tpp : 1u;
        tiles_per_piece[i] = tpp;
    }
    return true;
}

} // namespace speckv
