// cxl-speckv_amd/csrc/engine_prefix.cpp -- Engine::attend_prefix, the body of speckv_ext_attend_prefix_fold: the query rows of several
// requests (the members of a group) attend the stored positions of ONE other allocation (the group's prefix) and fold the result
// into the (out, lse) each member attended on its own -- one launch, or a piece launch and its merge (kernels: attend_prefix.hip)
#include "engine_internal.hpp"
#include "chunk_split.hpp"
#include "prefix_window.hpp"

namespace speckv {

// Group g = allocation prefix_handles[g] and the members [first_member[g], first_member[g + 1]) of the call; member m brings
// n_q[m] <= C positions (rows [m][j] of d_q_f16 / d_out / d_lse) that see the stored positions [0, prefix_len[m]) of the prefix.
// The launch goes onto the caller's stream, behind what the caller queued there -- the launches that wrote the members' own
// (out, lse) -- and behind the asynchronous pool writes on every other caller stream the engine knows.  out and lse are read and
// written in place; nothing is written to the pool and no residency changes.  Every refusal comes before any launch.  The
// descriptors (groups, prefix_len, n_q) travel through a slot of the pinned descriptor ring, so the call cannot be captured into a
// HIP graph.  n_splits as Engine::attend_chunk: the piece rule is chunk_split_plan, unchanged, over one "sequence" per group with
// pos_end = the group's largest live prefix_len and n_q = members x C; the partials live in s_chunk_.
// The window entry (c.windowed: speckv_ext_attend_prefix_fold_window) adds own_seen (host, per member), d_depth (device, may be null)
// and window.  window == 0, or a window under which no live row can lose a prefix position -- prefix_len[m] + own_seen[m] + n_q[m]
// - 1 <= W for every member with n_q[m] > 0 and a prefix (a depth is below n_q[m]; d_depth is on the device and is not read here)
// -- issues exactly the launches above.  Otherwise the WINDOW instances: a group's walk and its live members are
// prefix_window_group's, chunk_split_plan cuts the tiles that are LEFT from first_tile on, and own_seen travels in the same
// descriptor slot behind n_q.
// `split_kv` (speckv_ext_attend_prefix_fold_kv, the K8V4 split pool): handles[g] is the prefix's FP8_E4M3 allocation and v_handles[g] its
// MXFP4 one, both laid out as regions of num_tokens / 2 pages and judged by the region rule of Engine::attend_chunk: K of the layer =
// region `layer` of the first, V = region `layer` of the second.  The one mixed pair of schemes the kernel has instances of;
// everything else -- plan, window rule, descriptor slot, ordering -- is the call of one allocation per group.
int Engine::attend_prefix(const PrefixCall& c, hipStream_t s)
{
    const char* entry = c.split_kv ? "speckv_ext_attend_prefix_fold_kv" : c.windowed ? "speckv_ext_attend_prefix_fold_window" : "speckv_ext_attend_prefix_fold";
    if (null_) return no_data_path(entry);
    if (c.split_kv && (!c.handles || !c.v_handles)) return SPECKV_ERR_INVAL;
    if (!s || !c.d_q_f16 || !c.d_out || !c.d_lse) return SPECKV_ERR_INVAL;
    if (c.n_groups && (!c.handles || !c.first_member)) return SPECKV_ERR_INVAL;
    if (c.rows_per_pos == 0 || c.rows_per_pos > 16u || (c.rows_per_pos & (c.rows_per_pos - 1u)) || c.C == 0) return SPECKV_ERR_INVAL;
    if (c.n_splits > kChunkSplitsMax) return SPECKV_ERR_INVAL;
    if (reinterpret_cast<uintptr_t>(c.d_q_f16) % 16u || reinterpret_cast<uintptr_t>(c.d_out) % 16u || reinterpret_cast<uintptr_t>(c.d_lse) % 4u)
        return SPECKV_ERR_INVAL;
    if (c.n_groups && c.first_member[0] != 0) return SPECKV_ERR_INVAL;
    for (uint32_t g = 0; g < c.n_groups; ++g)
        if (c.first_member[g + 1] < c.first_member[g]) return SPECKV_ERR_INVAL;
    const uint32_t n_members = c.n_groups ? c.first_member[c.n_groups] : 0u;
    if (n_members && (!c.prefix_len || !c.n_q || (c.windowed && !c.own_seen))) return SPECKV_ERR_INVAL;
    if (reinterpret_cast<uintptr_t>(c.d_depth) % 4u) return SPECKV_ERR_INVAL;
    for (uint32_t m = 0; m < n_members; ++m)
        if (c.n_q[m] > c.C || c.prefix_len[m] % 2u) return SPECKV_ERR_INVAL;
    if (is_capturing(s)) {
        SPECKV_ERR("%s cannot be captured into a HIP graph (its descriptors are staged per call)", entry);
        return SPECKV_ERR_INVAL;
    }
    const uint32_t per_block = 64u / c.rows_per_pos;
    // per group, as chunk_split_plan takes a sequence: the largest prefix_len of a live member (0: no live pair) and members x C
    uint32_t win = 0;                                             // the window, where it cuts something
    if (c.windowed && c.window)
        for (uint32_t m = 0; m < n_members && !win; ++m)
            if (c.n_q[m] && c.prefix_len[m] && static_cast<uint64_t>(c.prefix_len[m]) + c.own_seen[m] + c.n_q[m] - 1u > c.window) win = c.window;
    std::vector<uint32_t> max_len(c.n_groups, 0u), pairs(c.n_groups, 0u), first_tile(c.n_groups, 0u);
    uint64_t n_blocks = 0;
    for (uint32_t g = 0; g < c.n_groups; ++g) {
        const uint32_t m0 = c.first_member[g];
        if (win) {                                                 // the members that are live for the fold, and where they start
            const PrefixWalk w = prefix_window_group(c.first_member[g + 1] - m0, c.prefix_len + m0, c.own_seen + m0, c.n_q + m0, win);
            max_len[g] = w.max_len;
            first_tile[g] = w.first_tile;
        } else {
            for (uint32_t m = m0; m < c.first_member[g + 1]; ++m)
                if (c.n_q[m] && c.prefix_len[m] > max_len[g]) max_len[g] = c.prefix_len[m];
        }
        const uint64_t p = static_cast<uint64_t>(c.first_member[g + 1] - c.first_member[g]) * c.C;
        if (p > 0x7FFFFFFFull) return SPECKV_ERR_INVAL;
        pairs[g] = max_len[g] ? static_cast<uint32_t>(p) : 0u;
        n_blocks += (pairs[g] + per_block - 1u) / per_block;
    }
    if (n_blocks * 8u > 0x7FFFFFFFull) return SPECKV_ERR_INVAL;
    std::vector<Allocation*> as(c.n_groups), vs(c.split_kv ? c.n_groups : 0u);
    int scheme = -1;
    const auto check = [&]() -> int {
        for (uint32_t g = 0; c.split_kv && g < c.n_groups; ++g) {
            Allocation *k = find(c.handles[g]), *v = find(c.v_handles[g]);
            if (!k || !v) return SPECKV_ERR_GENERAL;
            if (!split_region_ok(k, SPECKV_COMP_FP8_E4M3, c.layer, 0u, 2u) || !split_region_ok(v, SPECKV_COMP_MXFP4, c.layer, 0u, 2u) ||
                k->layout.num_tokens != v->layout.num_tokens)
                return SPECKV_ERR_INVAL;
            for (uint32_t m = c.first_member[g]; m < c.first_member[g + 1]; ++m)
                if (c.prefix_len[m] > k->layout.num_tokens) return SPECKV_ERR_INVAL;
            as[g] = k; vs[g] = v;
        }
        if (c.split_kv) { scheme = SPECKV_COMP_FP8_E4M3; return SPECKV_OK; }
        for (uint32_t g = 0; g < c.n_groups; ++g) {
            Allocation* a = find(c.handles[g]);
            if (!a) return SPECKV_ERR_GENERAL;
            if (scheme < 0) scheme = a->scheme;
            if (!a->has_layout || a->scheme != scheme ||
                (scheme != SPECKV_COMP_FP8_E4M3 && scheme != SPECKV_COMP_INT4_G32 && scheme != SPECKV_COMP_MXFP4))
                return SPECKV_ERR_INVAL;
            const Layout& L = a->layout;
            if (L.head_dim != 128 || L.bytes_per_element != 2 || L.num_heads != 8 || L.num_tokens % 2) return SPECKV_ERR_INVAL;
            if (c.layer >= L.num_layers) return SPECKV_ERR_INVAL;
            for (uint32_t m = c.first_member[g]; m < c.first_member[g + 1]; ++m)
                if (c.prefix_len[m] > L.num_tokens) return SPECKV_ERR_INVAL;
            if ((static_cast<uint64_t>(c.layer) + 1u) * L.num_tokens > a->n_pages) return SPECKV_ERR_INVAL;     // K + V pages of the layer
            as[g] = a;
        }
        return SPECKV_OK;
    };
    RC_TRY(check());
    if (n_blocks == 0) return SPECKV_OK;                          // no groups, no members or no live pair
    std::vector<uint32_t> pieces(c.n_groups, 1u), tpp(c.n_groups, 0u);
    bool split = false;
    uint64_t n_items = n_blocks;
    if (c.n_splits != 1u) {
        const uint32_t* plan_end = max_len.data();
        std::vector<uint32_t> rest;                                // window: the positions from first_tile on, as whole tiles
        if (win) {
            rest.resize(c.n_groups);
            for (uint32_t g = 0; g < c.n_groups; ++g) rest[g] = 32u * (chunk_pool_tiles(max_len[g]) - first_tile[g]);
            plan_end = rest.data();
        }
        if (!chunk_split_plan(c.n_groups, plan_end, pairs.data(), c.rows_per_pos, c.n_splits, cus(), pieces.data(), tpp.data()))
            return SPECKV_ERR_INVAL;
        n_items = 0;
        for (uint32_t g = 0; g < c.n_groups; ++g) {
            n_items += static_cast<uint64_t>((pairs[g] + per_block - 1u) / per_block) * pieces[g];
            split = split || (pairs[g] && pieces[g] > 1u);
        }
        if (n_items * 8u > 0x7FFFFFFFull) return SPECKV_ERR_INVAL;
    }
    if (!split) {
        n_items = n_blocks;
        for (uint32_t g = 0; g < c.n_groups; ++g) { pieces[g] = 1u; tpp[g] = chunk_pool_tiles(max_len[g]) - first_tile[g]; }
    }
    DeviceScope device_scope(device_);
    const size_t group_bytes = static_cast<size_t>(c.n_groups) * sizeof(PrefixGroup), member_bytes = static_cast<size_t>(n_members) * sizeof(uint32_t);
    const size_t bytes = group_bytes + (win ? 3u : 2u) * member_bytes;
    int slot = 0;
    void *staged = nullptr, *d_slot = nullptr;
    RC_TRY(descriptor_slot(bytes, &slot, &staged, &d_slot));      // may release the ABI lock: every prefix is judged again
    RC_TRY(check());
    uint8_t* part = nullptr;
    if (split) {                                                   // items x 8 heads x (32 KiB + 512 B); nothing is launched without it
        part = static_cast<uint8_t*>(scratch(s_chunk_, static_cast<size_t>(n_items) * 8u * kChunkPartBytes, s));
        if (!part) return SPECKV_ERR_NOMEM;
    }
    uint32_t first_block = 0, first_item = 0;
    for (uint32_t g = 0; g < c.n_groups; ++g) {
        const Layout& L = as[g]->layout;
        // split pool: region `layer` of either allocation; otherwise the layer's K region and the V region behind it
        const uint64_t k_first = static_cast<uint64_t>(c.layer) * (c.split_kv ? L.num_tokens / 2u : L.num_tokens);
        const uint64_t v_first = c.split_kv ? k_first : k_first + L.num_tokens / 2u;
        const uint32_t blocks = (pairs[g] + per_block - 1u) / per_block;
        static_cast<PrefixGroup*>(staged)[g] = PrefixGroup{as[g]->row, max_len[g], c.first_member[g], pairs[g], k_first, v_first,
                                                           first_block, first_item, pieces[g], tpp[g], first_tile[g],
                                                           c.split_kv ? vs[g]->row : as[g]->row};
        first_block += blocks;
        first_item += blocks * pieces[g];
    }
    memcpy(static_cast<uint8_t*>(staged) + group_bytes, c.prefix_len, member_bytes);
    memcpy(static_cast<uint8_t*>(staged) + group_bytes + member_bytes, c.n_q, member_bytes);
    if (win) memcpy(static_cast<uint8_t*>(staged) + group_bytes + 2u * member_bytes, c.own_seen, member_bytes);
    for (auto& w : write_evs_)
        if (w.s != s) HIP_TRY(hipStreamWaitEvent(s, w.ev, 0));
    HIP_TRY(hipMemcpyAsync(d_slot, staged, bytes, hipMemcpyHostToDevice, s));
    PrefixArgs pa{};
    pa.groups = static_cast<const PrefixGroup*>(d_slot);
    pa.prefix_len = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(d_slot) + group_bytes);
    pa.n_q = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(d_slot) + group_bytes + member_bytes);
    pa.tab = d_tab_;
    pa.q = static_cast<const _Float16*>(c.d_q_f16);
    pa.out = c.d_out;
    pa.lse = c.d_lse;
    pa.part = part;
    pa.n_groups = c.n_groups;
    pa.n_blocks = first_block;
    pa.n_items = first_item;
    pa.C = c.C;
    pa.rows_per_pos = c.rows_per_pos;
    pa.heads = 8;
    pa.sm_scale = c.sm_scale;
    pa.scheme = scheme;
    pa.v_scheme = c.split_kv ? SPECKV_COMP_MXFP4 : scheme;
    if (win) {
        pa.own_seen = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(d_slot) + group_bytes + 2u * member_bytes);
        pa.depth = c.d_depth;
        pa.window = win;
    }
    HIP_TRY(launch_attend_prefix(pa, s));
    for (uint32_t g = 0; g < c.n_groups; ++g) note_use(as[g], s);  // speckv_free of a prefix waits for this stream
    for (Allocation* v : vs) note_use(v, s);                       // (of either allocation in the split pool)
    if (hipEventRecord(grp_ring_.ev[slot], s) != hipSuccess) {      // the staging slot must not be reused under the kernel
        (void)hipGetLastError();
        HIP_TRY(hipStreamSynchronize(s));
    }
    return SPECKV_OK;
}

} // namespace speckv
