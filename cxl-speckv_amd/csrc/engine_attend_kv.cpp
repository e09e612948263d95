// cxl-speckv_amd/csrc/engine_attend_kv.cpp -- Engine::attend_batch_kv, the body behind speckv_ext_attend_kv_batch and
// speckv_ext_attend_kv_batch_window: one decode step of a batch over the SPLIT POOL ("K8V4": a sequence's K rows in an FP8_E4M3
// allocation, its V rows in an MXFP4 allocation), one attention launch (k_attend_k8v4, attend_kv.hip) and, where members have several
// pieces, the merge behind it; Engine::attend_layers_kv, the same step for several layers in one launch; Engine::split_member, the member
// of the split pool as these two and the draft step (Engine::attend_spec_kv, engine_attend_spec.cpp) fill it.  What all of them do once
// their members stand is Engine::staged_launch (engine_internal.hpp).
#include "engine_internal.hpp"
#include "decode_window.hpp"
#include "tuning.hpp"

namespace speckv {

// Member i = the allocations k_handle / v_handle with pos_end stored positions; both are read as arrays of regions of num_tokens / 2 pages,
// region `layer` of either (the addressing of Engine::attend_chunk's split_kv form, judged by the same rule for `layer` and `layer_last`).
// ONE form: both allocations in a single run (Allocation::linear_base) and a scale table on K; any other placement (striped over several
// pools, pages migrated) is refused with SPECKV_ERR_INVAL before anything is launched.  The descriptor walks n_pages pages from position
// `begin` of the region in BOTH allocations (begin % 32 == 0: a multiple of 16 records, a kernel tile stays one storage tile and one group
// of the scale table).
int Engine::split_member(StagedStep& m, uint32_t i, uint64_t k_handle, uint64_t v_handle, uint32_t layer, uint64_t layer_last, uint32_t pos_end, uint32_t begin,
                         uint32_t n_pages)
{
    Allocation *k = find(k_handle), *v = find(v_handle);
    if (!k || !v) return SPECKV_ERR_GENERAL;
    const auto regions_ok = [&](uint32_t l) { return split_region_ok(k, SPECKV_COMP_FP8_E4M3, l, pos_end, 32u) && split_region_ok(v, SPECKV_COMP_MXFP4, l, pos_end, 32u); };
    if (pos_end % 2u || layer_last >= 0xFFFFFFFFull || !regions_ok(layer) || (layer_last != layer && !regions_ok(static_cast<uint32_t>(layer_last))) ||
        k->layout.num_tokens != v->layout.num_tokens) {
        SPECKV_ERR("%s: sequence %u: an allocation of the wrong scheme or layout, an odd pos_end or one beyond the layout, or a layer past its regions", m.entry, i);
        return SPECKV_ERR_INVAL;
    }
    if (!k->linear_base || !k->d_scale_tab || !v->linear_base) {
        SPECKV_ERR("%s: sequence %u: the %s allocation's records do not lie in one run (striped over several pools, "
                   "or pages migrated); this entry has the single-run form only -- speckv_ext_attend_chunk_kv serves any placement",
                   m.entry, i, (!k->linear_base || !k->d_scale_tab) ? "K" : "V");
        return SPECKV_ERR_INVAL;
    }
    m.allocs.push_back(k);
    m.allocs.push_back(v);
    const uint32_t region = k->layout.num_tokens / 2u;
    AttendSeq& q = m.seqs[i];
    q = AttendSeq{};
    q.lin_base = k->linear_base;
    q.scale_tab = k->d_scale_tab;
    q.k_first = q.v_first = static_cast<uint64_t>(layer) * region + begin / 2u;
    q.n_pages = m.pages[i] = n_pages;
    q.layer_pages = region;
    q.stripe_n = 1u;
    q.n_splits = m.tiles[i] = (n_pages + 15u) / 16u;                     // tiles for now, pieces in staged_launch
    m.total_tiles += m.tiles[i];
    m.vside[i] = AttendKvSide{v->linear_base, q.v_first};               // (region % 16 == 0, begin % 32 == 0: a kernel tile is one storage tile)
    return SPECKV_OK;
}

// Sequence i = the allocations k_handles[i] / v_handles[i] with pos_end[i] stored positions (split_member).
// The workgroup shape is the FP8 batch kernel's, so the launch decision is attend_geometry.hpp's for BatchShape{fp8 = true}: form,
// dispatch order, one split length, the members' pieces -- with the tuning keys attend_tiles_per_split and attend_order_as_given.
// The descriptors travel through a slot of the pinned descriptor ring, read in place: not capturable into a HIP graph.
// Under a window (q_pos, window >= 1: a local layer; decode_window.hpp) member i's query sits at q_pos[i] -- its last stored position or the
// tail behind it -- and sees [lo, q_pos[i]]: the descriptor starts at the tile of lo in BOTH allocations, the tiles, the dispatch order and
// the pieces are those of the pages actually walked, and the leading positions of tile 0 in front of lo travel as the skip array
// (AttendArgs::seq_skip: k_attend_k8v4<true>).  window = 0, or a window that cuts no member: the descriptors, the instance and the launches
// of the entry without one.
int Engine::attend_batch_kv(uint32_t n_seq, const uint64_t* k_handles, const uint64_t* v_handles, uint32_t layer, const void* d_q_f16, uint32_t g,
                            const uint32_t* pos_end, float sm_scale, float* d_out, float* d_lse, hipStream_t s, const uint32_t* q_pos, uint32_t window)
{
    const char* entry = window ? "speckv_ext_attend_kv_batch_window" : "speckv_ext_attend_kv_batch";
    if (null_) return no_data_path(entry);
    if (window && !q_pos) return SPECKV_ERR_INVAL;
    if (!window) q_pos = nullptr;                                        // (no window: the launches of the entry without one)
    if (n_seq == 0) return SPECKV_OK;
    if (is_capturing(s)) {
        SPECKV_ERR("%s cannot be captured into a HIP graph (its descriptors are staged per call)", entry);
        return SPECKV_ERR_INVAL;
    }
    if (!k_handles || !v_handles || !pos_end || !d_q_f16 || !d_out || g == 0 || g > 16u) return SPECKV_ERR_INVAL;
    if (reinterpret_cast<uintptr_t>(d_q_f16) % 16u || reinterpret_cast<uintptr_t>(d_out) % 16u) return SPECKV_ERR_INVAL;
    StagedStep m(entry, n_seq, n_seq, true, d_q_f16, g, sm_scale, d_out, d_lse);
    m.skip.resize(q_pos ? n_seq : 0u);
    bool cut = false;                                                    // the window cuts some member's pool positions
    for (uint32_t i = 0; i < n_seq; ++i) {
        // the member's walk: everything stored, or under a window the tiles from lo's on (they end where they ended without one: inside the region)
        DecodeWindowRange w{0u, 0u, pos_end[i] / 2u};
        if (q_pos) w = decode_window_range(q_pos[i] + 1u, window);
        if (w.n_pages == 0u) w = DecodeWindowRange{0u, 0u, 0u};          // no pool position in the window: the member of pos_end = 0 (zeros, lse -inf)
        RC_TRY(split_member(m, i, k_handles[i], v_handles[i], layer, layer, pos_end[i], w.begin, w.n_pages));
        if (!q_pos) continue;
        if (q_pos[i] > pos_end[i] || q_pos[i] + 1u < pos_end[i]) return SPECKV_ERR_INVAL;       // the query: the last stored position or the tail behind it
        m.skip[i] = w.skip;
        cut = cut || w.begin != 0u || w.skip != 0u || w.n_pages != pos_end[i] / 2u;
    }
    if (!cut) m.skip.clear();                                            // (the plain instance)
    return staged_launch(m, s, [&](AttendArgs& k, const AttendKvSide* d_vside, uint32_t, bool merge, hipStream_t st) {
        HIP_TRY(launch_attend_k8v4(k, d_vside, n_seq, merge, d_out, d_lse, st));
        return SPECKV_OK;
    });
}

// speckv_ext_attend_kv_layers: the decode step of n_layers consecutive layers whose query rows exist at once, in one attention launch (and one
// merge).  The handle look-ups, the region rule for every layer of the range, note_use, the waits on the write events, the ring slot and its
// guard happen once per call; the descriptors are staged once per SEQUENCE (for region 0: k_attend_k8v4<false, false, AttendKvLayers> moves to
// its layer itself), so the staged bytes do not grow with n_layers apart from the dispatch order, which lists members.  No new launch
// rule: the FP8 batch rule of attend_geometry.hpp is asked once for n_seq x n_layers members, every sequence's tiles repeated per layer --
// 256 x 8 layers are 2048 members of one piece each and no merge, 8 x 32k x 8 layers are cut less finely than 8 members alone.  A member's
// pieces depend on the geometry and its own tiles alone (member_pieces), so they are the same on every layer: assign_pieces runs over the
// sequences, layer i's partials lie i x (partials of one layer) further on.  n_layers = 1: the decision of attend_batch_kv.
// The tail of an odd length (tail_idx[i] >= 0: fp16 rows [tail][layers][heads][128], `tail_stride` elements apart, layers counted from 0)
// is folded inside the launch by split 0 of every member, so d_lse is optional here too.
int Engine::attend_layers_kv(uint32_t n_seq, const uint64_t* k_handles, const uint64_t* v_handles, uint32_t layer_begin, uint32_t n_layers, const void* d_q_f16,
                             uint32_t g, const uint32_t* pos_end, uint32_t n_tail, const int32_t* d_tail_idx, const void* d_k_tail, const void* d_v_tail,
                             uint64_t tail_stride, float sm_scale, float* d_out, float* d_lse, hipStream_t s)
{
    const char* entry = "speckv_ext_attend_kv_layers";
    const auto refuse = [&](const char* why) { SPECKV_ERR("%s: %s", entry, why); return SPECKV_ERR_INVAL; };
    // what the arguments alone decide is judged first, so it is SPECKV_ERR_INVAL on every engine (attend_spec_kv's rule)
    if (g == 0 || g > 16) return refuse("g outside 1..16");
    if (n_layers == 0) return refuse("n_layers is 0");
    if (reinterpret_cast<uintptr_t>(d_q_f16) % 16u || reinterpret_cast<uintptr_t>(d_out) % 16u) return refuse("the query or the output is not 16-byte aligned");
    for (uint32_t i = 0; pos_end && i < n_seq; ++i)
        if (pos_end[i] % 2u) return refuse("an odd pos_end");
    const uint64_t layer_end = static_cast<uint64_t>(layer_begin) + n_layers;
    if (n_tail) {
        if (!d_tail_idx || !d_k_tail || !d_v_tail) return refuse("n_tail != 0 without the tail rows or the tail index");
        if (reinterpret_cast<uintptr_t>(d_k_tail) % 16u || reinterpret_cast<uintptr_t>(d_v_tail) % 16u || tail_stride % 8u)
            return refuse("the tail rows are not 16-byte aligned (pointers, or a stride that is no multiple of 8 elements)");
        if (tail_stride < layer_end * 8u * 128u) return refuse("tail_stride_elems does not hold the layers of the range ([tail][layers][8][128])");
    }
    if (null_) return no_data_path(entry);
    if (n_seq == 0) return SPECKV_OK;
    if (is_capturing(s)) return refuse("cannot be captured into a HIP graph (its descriptors are staged per call)");
    if (!k_handles || !v_handles || !pos_end || !d_q_f16 || !d_out) return refuse("a NULL handle array, pos_end, query or output");
    const size_t n_mem = static_cast<size_t>(n_seq) * n_layers;          // the members [layer][sequence] of the launch decision
    if (n_mem > 0x7FFFFFFFull / 2u) return refuse("a grid beyond the launch limits (n_seq x n_layers)");
    StagedStep m(entry, n_seq, n_mem, true, d_q_f16, g, sm_scale, d_out, d_lse);
    m.copies = n_layers;
    m.grid_rows = n_mem * 2u;                                            // (n_seq x n_layers x 2 workgroup rows)
    for (uint32_t i = 0; i < n_seq; ++i) {
        RC_TRY(split_member(m, i, k_handles[i], v_handles[i], layer_begin, layer_end - 1u, pos_end[i], 0u, pos_end[i] / 2u));
        m.seqs[i].k_first = m.seqs[i].v_first = m.vside[i].v_first = 0u;                       // region 0: the kernel adds layer * layer_pages
        for (uint32_t l = 1; l < n_layers; ++l) { m.tiles[static_cast<size_t>(l) * n_seq + i] = m.tiles[i]; m.pages[static_cast<size_t>(l) * n_seq + i] = m.pages[i]; }
    }
    return staged_launch(m, s, [&](AttendArgs& k, const AttendKvSide* d_vside, uint32_t layer_parts, bool merge, hipStream_t st) {
        k.batch_n_seq = n_seq;
        k.batch_layer = layer_begin;
        if (n_tail) {
            k.tail_k = static_cast<const uint16_t*>(d_k_tail);
            k.tail_v = static_cast<const uint16_t*>(d_v_tail);
            k.tail_idx = d_tail_idx;
            k.tail_stride = tail_stride;
        }
        HIP_TRY(launch_attend_k8v4_layers(k, d_vside, n_seq, n_layers, layer_parts, merge, d_out, d_lse, st));
        return SPECKV_OK;
    });
}

} // namespace speckv
