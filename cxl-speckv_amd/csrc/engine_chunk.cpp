// cxl-speckv_amd/csrc/engine_chunk.cpp -- Engine::attend_chunk, the one body behind speckv_ext_attend_chunk, _masked, _split, _window,
// _tree_window and _kv (the split pool: K and V pages in an allocation each): causal attention of a chunk of new positions per sequence over stored and held positions, one launch -- or, where the
// stored positions are split across the chip, a piece launch and its merge (the kernels are in attend_chunk.hip)
#include "engine_internal.hpp"
#include "chunk_split.hpp"
#include "chunk_window.hpp"

namespace speckv {

namespace {

// How a call is cut into launches, from its arguments alone (so the plan holds across descriptor_slot).
struct ChunkPlan {
    uint32_t win = 0;                                  // the window the kernel gets: 0 while no row of the call loses a position
    bool split = false;                                // some sequence has pieces: the piece launch and the merge, partials in scratch
    uint64_t n_items = 0;                              // query blocks x pieces over the call
    std::vector<uint32_t> pieces, tpp, first_tile;     // per sequence, as ChunkSeq takes them
};

// false: more work than a launch can index, or a piece count chunk_split_plan refuses.  Under a window that cuts, chunk_split_plan
// (unchanged) cuts the pool tiles that are left from first_tile on.  One piece everywhere is the plan of whole sequences.
bool plan_chunk(const Engine::ChunkCall& c, uint32_t n_cus, ChunkPlan& p)
{
    const uint32_t per_block = 64u / c.rows_per_pos;
    const auto blocks = [&](uint32_t i) { return static_cast<uint64_t>((c.n_q[i] + per_block - 1u) / per_block); };
    const auto base = [&](uint32_t i) { return c.tail_idx && c.tail_idx[i] >= 0 ? 1u : 0u; };
    for (uint32_t i = 0; i < c.n_seq; ++i) {
        p.n_items += blocks(i);
        if (c.window && c.n_q[i] && static_cast<uint64_t>(c.pos_end[i]) + base(i) + c.n_q[i] > c.window) p.win = c.window;
    }
    if (p.n_items * 8u > 0x7FFFFFFFull) return false;
    p.pieces.assign(c.n_seq, 1u); p.tpp.assign(c.n_seq, 0u); p.first_tile.assign(c.n_seq, 0u);
    if (c.n_splits != 1u) {
        const uint32_t* plan_end = c.pos_end;
        std::vector<uint32_t> rest;                    // window: the stored positions from first_tile on, as whole tiles
        if (p.win) {
            rest.resize(c.n_seq);
            for (uint32_t i = 0; i < c.n_seq; ++i) {
                p.first_tile[i] = chunk_window_first_pool_tile(c.pos_end[i], base(i), p.win);
                rest[i] = 32u * (chunk_pool_tiles(c.pos_end[i]) - p.first_tile[i]);
            }
            plan_end = rest.data();
        }
        if (!chunk_split_plan(c.n_seq, plan_end, c.n_q, c.rows_per_pos, c.n_splits, n_cus, p.pieces.data(), p.tpp.data())) return false;
        p.n_items = 0;
        for (uint32_t i = 0; i < c.n_seq; ++i) {
            p.n_items += blocks(i) * p.pieces[i];
            p.split = p.split || (c.n_q[i] && p.pieces[i] > 1u);
        }
        if (p.n_items * 8u > 0x7FFFFFFFull) return false;
    }
    if (!p.split)
        for (uint32_t i = 0; i < c.n_seq; ++i) { p.pieces[i] = 1u; p.tpp[i] = chunk_pool_tiles(c.pos_end[i]); p.first_tile[i] = 0u; }
    return true;
}

} // namespace

// Sequence i = allocation handles[i] with pos_end[i] stored positions, its tail (tail_idx[i] >= 0: row tail_idx[i] of d_k_tail /
// d_v_tail) and n_q[i] <= C new positions in d_k_new / d_v_new; ONE launch on the caller's stream.  Ordering as read_pairs: behind
// what the caller queued on `s`, and behind the asynchronous pool writes on every other caller stream the engine knows.  Nothing is
// written to the pool and no residency changes.  The per-sequence descriptors travel through a slot of the pinned descriptor ring
// to its device twin, so the call cannot be captured into a HIP graph; nothing is allocated once the slots are large enough.
// The forms, by field of the call (ChunkCall, engine.hpp):
// `masked`: per query position mask_words words of visible HELD positions at d_mask, a device array the kernel reads in place --
// nothing about it is staged.
// `n_splits`: 1 every sequence whole, N > 1 that many pieces per sequence, 0 the library's rule (chunk_split.hpp).  A plan of one
// piece everywhere issues the launch of a call with n_splits 1; any other plan issues the piece launch and the merge behind it on
// `s`, the partials in a scratch buffer of their own (s_chunk_: a chunk call does not order itself behind the decode entries'
// s_attn_ on another stream).
// `window`: query position j sees the absolute positions [max(0, P + 1 - window), P], P = pos_end + base + j (chunk_window.hpp).  0,
// or a window under which no row of the call loses a position, issues the unwindowed launch -- the other calls' bits by
// construction.  Otherwise the whole call runs on the WINDOW instances: a query block walks from its first row's bound.
// `by_depth` (a mask AND a window): d_depth = device depths [n_seq][C], read by the kernel in place like the mask.  The engine cannot
// read either array, so whether the window cuts anything is judged by the same rule as above -- a depth is below n_q -- and a window
// that cuts nothing issues the unwindowed masked launch.  Otherwise the call runs on the MASKED + WINDOW instances: every block of a
// sequence walks from first_tile (the first pool tile its position 0 sees).  A window with a mask that does not go by depth is refused.
// `split_kv` (speckv_ext_attend_chunk_kv, the K8V4 split pool): handles[i] is an FP8_E4M3 allocation and v_handles[i] an MXFP4 one, both
// laid out as regions of num_tokens / 2 pages: K of the layer = region `layer` of the first, V = region `layer` of the second.  The
// one mixed pair of schemes the kernel has instances of; everything else -- plan, forms, ordering -- is the call of one allocation.
int Engine::attend_chunk(const ChunkCall& c, hipStream_t s)
{
    if (null_) return no_data_path(c.entry);
    if (c.split_kv && !c.v_handles) return SPECKV_ERR_INVAL;
    if (!s || !c.handles || !c.pos_end || !c.n_q || !c.d_q_f16 || !c.d_k_new || !c.d_v_new || !c.d_out) return SPECKV_ERR_INVAL;
    if (c.rows_per_pos == 0 || c.rows_per_pos > 16u || (c.rows_per_pos & (c.rows_per_pos - 1u)) || c.C == 0) return SPECKV_ERR_INVAL;
    if (c.n_splits > kChunkSplitsMax) return SPECKV_ERR_INVAL;
    if (c.window && c.masked && !c.by_depth) return SPECKV_ERR_INVAL;
    if (c.by_depth && (!c.d_depth || reinterpret_cast<uintptr_t>(c.d_depth) % 4u)) return SPECKV_ERR_INVAL;
    // a row's words cover held positions 0 .. C (a tail and C new positions)
    if (c.masked && (!c.d_mask || reinterpret_cast<uintptr_t>(c.d_mask) % 4u || c.mask_words < (static_cast<uint64_t>(c.C) + 32u) / 32u))
        return SPECKV_ERR_INVAL;
    const auto aligned16 = [](const void* p) { return reinterpret_cast<uintptr_t>(p) % 16u == 0; };
    if (!aligned16(c.d_q_f16) || !aligned16(c.d_k_new) || !aligned16(c.d_v_new) || !aligned16(c.d_k_tail) || !aligned16(c.d_v_tail) || !aligned16(c.d_out))
        return SPECKV_ERR_INVAL;
    // a row is one position of one layer: 8 heads x 128 elements, 16-byte aligned pieces
    if (c.seq_stride % 8u || c.pos_stride % 8u || c.pos_stride < 1024u || (c.n_seq > 1 && c.seq_stride < 1024u)) return SPECKV_ERR_INVAL;
    bool any_tail = false, any_q = false;
    for (uint32_t i = 0; i < c.n_seq; ++i) {
        if (c.n_q[i] > c.C || c.pos_end[i] % 2u) return SPECKV_ERR_INVAL;
        any_q = any_q || c.n_q[i];
        any_tail = any_tail || (c.tail_idx && c.tail_idx[i] >= 0);
    }
    if (any_tail && (!c.d_k_tail || !c.d_v_tail || c.tail_stride % 8u || c.tail_stride < 1024u)) return SPECKV_ERR_INVAL;
    if (is_capturing(s)) {
        SPECKV_ERR("%s cannot be captured into a HIP graph (its descriptors are staged per call)", c.entry);
        return SPECKV_ERR_INVAL;
    }
    const uint32_t per_block = 64u / c.rows_per_pos;
    std::vector<Allocation*> as(c.n_seq), vs(c.split_kv ? c.n_seq : 0u);
    int scheme = -1;
    const auto check = [&]() -> int {
        for (uint32_t i = 0; c.split_kv && i < c.n_seq; ++i) {
            Allocation *k = find(c.handles[i]), *v = find(c.v_handles[i]);
            if (!k || !v) return SPECKV_ERR_GENERAL;
            if (!split_region_ok(k, SPECKV_COMP_FP8_E4M3, c.layer, c.pos_end[i], 2u) || !split_region_ok(v, SPECKV_COMP_MXFP4, c.layer, c.pos_end[i], 2u) ||
                k->layout.num_tokens != v->layout.num_tokens)
                return SPECKV_ERR_INVAL;
            as[i] = k; vs[i] = v;
        }
        if (c.split_kv) { scheme = SPECKV_COMP_FP8_E4M3; return SPECKV_OK; }
        for (uint32_t i = 0; i < c.n_seq; ++i) {
            Allocation* a = find(c.handles[i]);
            if (!a) return SPECKV_ERR_GENERAL;
            if (scheme < 0) scheme = a->scheme;
            if (!a->has_layout || a->scheme != scheme ||
                (scheme != SPECKV_COMP_FP8_E4M3 && scheme != SPECKV_COMP_INT4_G32 && scheme != SPECKV_COMP_MXFP4))
                return SPECKV_ERR_INVAL;
            const Layout& L = a->layout;
            if (L.head_dim != 128 || L.bytes_per_element != 2 || L.num_heads != 8 || L.num_tokens % 2) return SPECKV_ERR_INVAL;
            if (c.layer >= L.num_layers || c.pos_end[i] > L.num_tokens) return SPECKV_ERR_INVAL;
            if ((static_cast<uint64_t>(c.layer) + 1u) * L.num_tokens > a->n_pages) return SPECKV_ERR_INVAL;     // K + V pages of the layer
            as[i] = a;
        }
        return SPECKV_OK;
    };
    RC_TRY(check());
    if (c.n_seq == 0 || !any_q) return SPECKV_OK;
    ChunkPlan plan;
    if (!plan_chunk(c, cus(), plan)) return SPECKV_ERR_INVAL;
    DeviceScope device_scope(device_);
    const size_t bytes = static_cast<size_t>(c.n_seq) * sizeof(ChunkSeq);
    int slot = 0;
    void *staged = nullptr, *d_slot = nullptr;
    RC_TRY(descriptor_slot(bytes, &slot, &staged, &d_slot));      // may release the ABI lock: every sequence is judged again
    RC_TRY(check());
    uint8_t* part = nullptr;
    if (plan.split) {                                              // items x 8 heads x (32 KiB + 512 B); nothing is launched without it
        part = static_cast<uint8_t*>(scratch(s_chunk_, static_cast<size_t>(plan.n_items) * 8u * kChunkPartBytes, s));
        if (!part) return SPECKV_ERR_NOMEM;
    }
    uint32_t first_block = 0, first_item = 0;
    for (uint32_t i = 0; i < c.n_seq; ++i) {
        const Layout& L = as[i]->layout;
        // split pool: region `layer` of either allocation; otherwise the layer's K region and the V region behind it
        const uint64_t k_first = static_cast<uint64_t>(c.layer) * (c.split_kv ? L.num_tokens / 2u : L.num_tokens);
        const uint64_t v_first = c.split_kv ? k_first : k_first + L.num_tokens / 2u;
        const int32_t tail = c.tail_idx && c.tail_idx[i] >= 0 ? c.tail_idx[i] : -1;
        const uint32_t blocks = (c.n_q[i] + per_block - 1u) / per_block;
        static_cast<ChunkSeq*>(staged)[i] = ChunkSeq{as[i]->row, c.pos_end[i], c.n_q[i], first_block, k_first, v_first,
                                                     tail, tail >= 0 ? 1u : 0u, plan.pieces[i], plan.tpp[i], first_item, plan.first_tile[i],
                                                     c.split_kv ? vs[i]->row : as[i]->row};
        first_block += blocks;
        first_item += blocks * plan.pieces[i];
    }
    for (auto& w : write_evs_)
        if (w.s != s) HIP_TRY(hipStreamWaitEvent(s, w.ev, 0));
    HIP_TRY(hipMemcpyAsync(d_slot, staged, bytes, hipMemcpyHostToDevice, s));
    ChunkArgs ca{};
    ca.seqs = static_cast<const ChunkSeq*>(d_slot);
    ca.tab = d_tab_;
    ca.q = static_cast<const _Float16*>(c.d_q_f16);
    ca.k_new = static_cast<const _Float16*>(c.d_k_new);
    ca.v_new = static_cast<const _Float16*>(c.d_v_new);
    ca.k_tail = static_cast<const _Float16*>(c.d_k_tail);
    ca.v_tail = static_cast<const _Float16*>(c.d_v_tail);
    ca.out = c.d_out;
    ca.lse = c.d_lse;
    ca.seq_stride = c.seq_stride;
    ca.pos_stride = c.pos_stride;
    ca.tail_stride = c.tail_stride;
    ca.n_seq = c.n_seq;
    ca.n_blocks = first_block;
    ca.C = c.C;
    ca.rows_per_pos = c.rows_per_pos;
    ca.heads = 8;
    ca.sm_scale = c.sm_scale;
    ca.scheme = scheme;
    ca.v_scheme = c.split_kv ? SPECKV_COMP_MXFP4 : scheme;
    ca.mask = c.masked ? c.d_mask : nullptr;
    ca.mask_words = c.masked ? c.mask_words : 0u;
    ca.part = part;
    ca.n_items = first_item;
    ca.window = plan.win;
    ca.depth = plan.win && c.by_depth ? c.d_depth : nullptr;
    HIP_TRY(launch_attend_chunk(ca, s));
    for (uint32_t i = 0; i < c.n_seq; ++i) note_use(as[i], s);   // speckv_free waits for this stream
    for (Allocation* v : vs) note_use(v, s);
    if (hipEventRecord(grp_ring_.ev[slot], s) != hipSuccess) {      // the staging slot must not be reused under the kernel
        (void)hipGetLastError();
        HIP_TRY(hipStreamSynchronize(s));
    }
    return SPECKV_OK;
}

} // namespace speckv
