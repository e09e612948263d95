// cxl-speckv_amd/csrc/engine_chunk.cpp -- speckv_ext_attend_chunk / speckv_ext_attend_chunk_masked / speckv_ext_attend_chunk_split /
// speckv_ext_attend_chunk_window / speckv_ext_attend_chunk_tree_window: causal attention of a chunk of new positions per sequence over stored and held positions, one launch -- or, where the stored
// positions are split across the chip, a piece launch and its merge (Engine member; the kernels are in attend_chunk.hip)
#include "engine_internal.hpp"
#include "chunk_split.hpp"
#include "chunk_window.hpp"

namespace speckv {

// Sequence i = allocation handles[i] with pos_end[i] stored positions, its tail (tail_idx[i] >= 0: row tail_idx[i] of d_k_tail /
// d_v_tail) and n_q[i] <= C new positions in d_k_new / d_v_new; ONE launch on the caller's stream.  Ordering as read_pairs: behind
// what the caller queued on `s`, and behind the asynchronous pool writes on every other caller stream the engine knows.  Nothing is
// written to the pool and no residency changes.  The per-sequence descriptors travel through a slot of the pinned descriptor ring
// to its device twin, so the call cannot be captured into a HIP graph; nothing is allocated once the slots are large enough.
// `mask` (the masked entry; the causal one passes none): per query position mask->words words of visible HELD positions, a device
// array the kernel reads in place -- nothing about it is staged.
// `n_splits` (the split entry; the other two pass none = every sequence whole): 1 every sequence whole, N > 1 that many pieces per
// sequence, 0 the library's rule (chunk_split.hpp).  A plan of one piece everywhere issues the launch of the other two entries; any
// other plan issues the piece launch and the merge behind it on `s`, the partials in a scratch buffer of their own (s_chunk_: a
// chunk call does not order itself behind the decode entries' s_attn_ on another stream).
// `window` (the window entry; the other three pass none): query position j sees the absolute positions [max(0, P + 1 - *window), P],
// P = pos_end + base + j (chunk_window.hpp); never with a mask.  0, or a window under which no row of the call loses a position, issues
// the unwindowed launch -- the other entries' bits by construction.  Otherwise the whole call runs on the WINDOW instances: a query
// block walks from its first row's bound, and the pieces are planned by the unchanged chunk_split_plan over the pool tiles that are
// left from the sequence's first_tile (the first pool tile its position 0 sees) on.
// `mask->by_depth` (the tree-window entry; the only one that passes a mask AND a window): mask->d_depth = device depths [n_seq][C],
// read by the kernel in place like the mask.  The engine cannot read either array, so whether the window cuts anything is judged by
// the same rule as above -- a depth is below n_q -- and a window that cuts nothing issues the unwindowed masked launch.  Otherwise
// the call runs on the MASKED + WINDOW instances: every block of a sequence walks from first_tile, the pieces are planned as above.
int Engine::attend_chunk(uint32_t n_seq, const uint64_t* handles, uint32_t layer, const void* d_q_f16, uint32_t C, uint32_t rows_per_pos,
                         const uint32_t* pos_end, const uint32_t* n_q, const void* d_k_new, const void* d_v_new, uint64_t seq_stride,
                         uint64_t pos_stride, const int32_t* tail_idx, const void* d_k_tail, const void* d_v_tail, uint64_t tail_stride,
                         float sm_scale, float* d_out, float* d_lse, hipStream_t s, const ChunkMask* mask, const uint32_t* n_splits,
                         const uint32_t* window)
{
    const bool by_depth = mask && mask->by_depth;
    const char* entry = by_depth ? "speckv_ext_attend_chunk_tree_window" : window ? "speckv_ext_attend_chunk_window" : n_splits ? "speckv_ext_attend_chunk_split" : mask ? "speckv_ext_attend_chunk_masked" : "speckv_ext_attend_chunk";
    if (null_) return no_data_path(entry);
    if (!s || !handles || !pos_end || !n_q || !d_q_f16 || !d_k_new || !d_v_new || !d_out) return SPECKV_ERR_INVAL;
    if (rows_per_pos == 0 || rows_per_pos > 16u || (rows_per_pos & (rows_per_pos - 1u)) || C == 0) return SPECKV_ERR_INVAL;
    if (n_splits && *n_splits > kChunkSplitsMax) return SPECKV_ERR_INVAL;
    if (window && mask && !by_depth) return SPECKV_ERR_INVAL;
    if (by_depth && (!window || !mask->d_depth || reinterpret_cast<uintptr_t>(mask->d_depth) % 4u)) return SPECKV_ERR_INVAL;
    // a row's words cover held positions 0 .. C (a tail and C new positions)
    if (mask && (!mask->d_mask || reinterpret_cast<uintptr_t>(mask->d_mask) % 4u || mask->words < (static_cast<uint64_t>(C) + 32u) / 32u))
        return SPECKV_ERR_INVAL;
    const auto aligned16 = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16u == 0; };
    if (!aligned16(d_q_f16) || !aligned16(d_k_new) || !aligned16(d_v_new) || !aligned16(d_k_tail) || !aligned16(d_v_tail) || !aligned16(d_out))
        return SPECKV_ERR_INVAL;
    // a row is one position of one layer: 8 heads x 128 elements, 16-byte aligned pieces
    if (seq_stride % 8u || pos_stride % 8u || pos_stride < 1024u || (n_seq > 1 && seq_stride < 1024u)) return SPECKV_ERR_INVAL;
    bool any_tail = false, any_q = false;
    for (uint32_t i = 0; i < n_seq; ++i) {
        if (n_q[i] > C || pos_end[i] % 2u) return SPECKV_ERR_INVAL;
        any_q = any_q || n_q[i];
        any_tail = any_tail || (tail_idx && tail_idx[i] >= 0);
    }
    if (any_tail && (!d_k_tail || !d_v_tail || tail_stride % 8u || tail_stride < 1024u)) return SPECKV_ERR_INVAL;
    if (is_capturing(s)) {
        SPECKV_ERR("%s cannot be captured into a HIP graph (its descriptors are staged per call)", entry);
        return SPECKV_ERR_INVAL;
    }
    const uint32_t per_block = 64u / rows_per_pos;
    std::vector<Allocation*> as(n_seq);
    int scheme = -1;
    const auto check = [&]() -> int {
        for (uint32_t i = 0; i < n_seq; ++i) {
            Allocation* a = find(handles[i]);
            if (!a) return SPECKV_ERR_GENERAL;
            if (scheme < 0) scheme = a->scheme;
            if (!a->has_layout || a->scheme != scheme ||
                (scheme != SPECKV_COMP_FP8_E4M3 && scheme != SPECKV_COMP_INT4_G32 && scheme != SPECKV_COMP_MXFP4))
                return SPECKV_ERR_INVAL;
            const Layout& L = a->layout;
            if (L.head_dim != 128 || L.bytes_per_element != 2 || L.num_heads != 8 || L.num_tokens % 2) return SPECKV_ERR_INVAL;
            if (layer >= L.num_layers || pos_end[i] > L.num_tokens) return SPECKV_ERR_INVAL;
            if ((static_cast<uint64_t>(layer) + 1u) * L.num_tokens > a->n_pages) return SPECKV_ERR_INVAL;     // K + V pages of the layer
            as[i] = a;
        }
        return SPECKV_OK;
    };
    RC_TRY(check());
    if (n_seq == 0 || !any_q) return SPECKV_OK;
    uint64_t n_blocks = 0;
    for (uint32_t i = 0; i < n_seq; ++i) n_blocks += (n_q[i] + per_block - 1u) / per_block;
    if (n_blocks * 8u > 0x7FFFFFFFull) return SPECKV_ERR_INVAL;
    // the pieces of every sequence (all 1: today's launch) -- from the arguments alone, so the plan holds across descriptor_slot
    std::vector<uint32_t> pieces(n_seq, 1u), tpp(n_seq, 0u), first_tile(n_seq, 0u);
    uint64_t n_items = n_blocks;
    bool split = false;
    // the window the kernel gets: 0 while no row of the call loses a position (the unwindowed launch)
    uint32_t win = 0;
    if (window && *window)
        for (uint32_t i = 0; i < n_seq; ++i)
            if (n_q[i] && static_cast<uint64_t>(pos_end[i]) + (tail_idx && tail_idx[i] >= 0 ? 1u : 0u) + n_q[i] > *window) win = *window;
    if (n_splits && *n_splits != 1u) {
        const uint32_t* plan_end = pos_end;
        std::vector<uint32_t> rest;                                // window: the stored positions from first_tile on, as whole tiles
        if (win) {
            rest.resize(n_seq);
            for (uint32_t i = 0; i < n_seq; ++i) {
                first_tile[i] = chunk_window_first_pool_tile(pos_end[i], tail_idx && tail_idx[i] >= 0 ? 1u : 0u, win);
                rest[i] = 32u * (chunk_pool_tiles(pos_end[i]) - first_tile[i]);
            }
            plan_end = rest.data();
        }
        if (!chunk_split_plan(n_seq, plan_end, n_q, rows_per_pos, *n_splits, cus(), pieces.data(), tpp.data())) return SPECKV_ERR_INVAL;
        n_items = 0;
        for (uint32_t i = 0; i < n_seq; ++i) {
            n_items += static_cast<uint64_t>((n_q[i] + per_block - 1u) / per_block) * pieces[i];
            split = split || (n_q[i] && pieces[i] > 1u);
        }
        if (n_items * 8u > 0x7FFFFFFFull) return SPECKV_ERR_INVAL;
    }
    DeviceScope device_scope(device_);
    const size_t bytes = static_cast<size_t>(n_seq) * sizeof(ChunkSeq);
    int slot = 0;
    void *staged = nullptr, *d_slot = nullptr;
    RC_TRY(descriptor_slot(bytes, &slot, &staged, &d_slot));      // may release the ABI lock: every sequence is judged again
    RC_TRY(check());
    uint8_t* part = nullptr;
    if (split) {                                                   // items x 8 heads x (32 KiB + 512 B); nothing is launched without it
        part = static_cast<uint8_t*>(scratch(s_chunk_, static_cast<size_t>(n_items) * 8u * kChunkPartBytes, s));
        if (!part) return SPECKV_ERR_NOMEM;
    }
    uint32_t first_block = 0, first_item = 0;
    for (uint32_t i = 0; i < n_seq; ++i) {
        const Layout& L = as[i]->layout;
        const uint64_t k_first = static_cast<uint64_t>(layer) * L.num_tokens;
        const int32_t tail = tail_idx && tail_idx[i] >= 0 ? tail_idx[i] : -1;
        const uint32_t blocks = (n_q[i] + per_block - 1u) / per_block;
        if (!split) { pieces[i] = 1u; tpp[i] = chunk_pool_tiles(pos_end[i]); first_tile[i] = 0u; }
        static_cast<ChunkSeq*>(staged)[i] = ChunkSeq{as[i]->row, pos_end[i], n_q[i], first_block, k_first, k_first + L.num_tokens / 2u,
                                                     tail, tail >= 0 ? 1u : 0u, pieces[i], tpp[i], first_item, first_tile[i]};
        first_block += blocks;
        first_item += blocks * pieces[i];
    }
    for (auto& w : write_evs_)
        if (w.s != s) HIP_TRY(hipStreamWaitEvent(s, w.ev, 0));
    HIP_TRY(hipMemcpyAsync(d_slot, staged, bytes, hipMemcpyHostToDevice, s));
    ChunkArgs ca{};
    ca.seqs = static_cast<const ChunkSeq*>(d_slot);
    ca.tab = d_tab_;
    ca.q = static_cast<const _Float16*>(d_q_f16);
    ca.k_new = static_cast<const _Float16*>(d_k_new);
    ca.v_new = static_cast<const _Float16*>(d_v_new);
    ca.k_tail = static_cast<const _Float16*>(d_k_tail);
    ca.v_tail = static_cast<const _Float16*>(d_v_tail);
    ca.out = d_out;
    ca.lse = d_lse;
    ca.seq_stride = seq_stride;
    ca.pos_stride = pos_stride;
    ca.tail_stride = tail_stride;
    ca.n_seq = n_seq;
    ca.n_blocks = first_block;
    ca.C = C;
    ca.rows_per_pos = rows_per_pos;
    ca.heads = 8;
    ca.sm_scale = sm_scale;
    ca.scheme = scheme;
    ca.mask = mask ? mask->d_mask : nullptr;
    ca.mask_words = mask ? mask->words : 0u;
    ca.part = part;
    ca.n_items = first_item;
    ca.window = win;
    ca.depth = win && by_depth ? mask->d_depth : nullptr;
    HIP_TRY(launch_attend_chunk(ca, s));
    for (uint32_t i = 0; i < n_seq; ++i) note_use(as[i], s);     // speckv_free waits for this stream
    if (hipEventRecord(grp_ring_.ev[slot], s) != hipSuccess) {      // the staging slot must not be reused under the kernel
        (void)hipGetLastError();
        HIP_TRY(hipStreamSynchronize(s));
    }
    return SPECKV_OK;
}

} // namespace speckv
