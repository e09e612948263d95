// cxl-speckv_amd/csrc/engine_attend_kv.cpp -- Engine::attend_batch_kv, the body behind speckv_ext_attend_kv_batch,
// speckv_ext_attend_kv_batch_window, speckv_ext_attend_kv_spec and speckv_ext_attend_kv_spec_window: one decode step of a batch over the SPLIT POOL ("K8V4": a sequence's K rows in an FP8_E4M3
// allocation, its V rows in an MXFP4 allocation), one attention launch (k_attend_k8v4, attend_kv.hip) and, where members have several
// pieces, the merge behind it
#include "engine_internal.hpp"
#include "decode_window.hpp"
#include "spec_window.hpp"
#include "tuning.hpp"

namespace speckv {

// Sequence i = the allocations k_handles[i] / v_handles[i] with pos_end[i] stored positions; both are read as arrays of regions of
// num_tokens / 2 pages, region `layer` of either (the addressing of Engine::attend_chunk's split_kv form, judged by the same rule).
// The workgroup shape is the FP8 batch kernel's, so the launch decision is attend_geometry.hpp's for BatchShape{fp8 = true}: form,
// dispatch order, one split length, the members' pieces -- with the tuning keys attend_tiles_per_split and attend_order_as_given.
// ONE form: both allocations of every member in a single run (Allocation::linear_base) and a scale table on K; any other placement
// (striped over several pools, pages migrated) is refused with SPECKV_ERR_INVAL before anything is launched.
// The descriptors travel through a slot of the pinned descriptor ring, read in place: not capturable into a HIP graph.
// Under a window (q_pos, window >= 1: a local layer; decode_window.hpp) member i's query sits at q_pos[i] -- its last stored position or the
// tail behind it -- and sees [lo, q_pos[i]]: the descriptor starts at the tile of lo in BOTH allocations (begin / 2 pages in: a multiple
// of 16 records, a kernel tile stays one storage tile and one group of the scale table), the tiles, the dispatch order and the pieces are
// those of the pages actually walked, and the leading positions of tile 0 in front of lo travel as the skip array (AttendArgs::seq_skip:
// k_attend_k8v4<true>).  window = 0, or a window that cuts no member: the descriptors, the instance and the launches of the entry without one.
// held (attend_spec_kv): the step of several positions -- g = n_q x rows_per_pos query rows that all see every stored
// position, so descriptors, geometry, pieces and slot are those of a decode step of g rows; the launch is k_attend_k8v4<false, true>, whose
// split 0 folds the held rows of every member into its final rows or its partial (launch_attend_k8v4_held).
// held under a window (speckv_ext_attend_kv_spec_window; spec_window.hpp): q_pos carries the members' committed LENGTHS (judged by
// attend_spec_kv).  The rows of a member no longer share a lower bound, so its descriptor starts at the tile of depth 0's bound in both
// allocations whatever depths the call carries, the tiles, the dispatch order and the pieces are those of the pages walked, and the skip
// slot of the descriptor ring carries the member's SIGNED rel (k_attend_k8v4<true, true> adds the row's depth).  A member no row of
// which sees a pool position is one with nothing stored: its held positions alone.  A window that can cut no member (length + 16 <=
// window for all): the descriptors, the instance and the launches of the entry without one.
int Engine::attend_batch_kv(uint32_t n_seq, const uint64_t* k_handles, const uint64_t* v_handles, uint32_t layer, const void* d_q_f16, uint32_t g,
                            const uint32_t* pos_end, float sm_scale, float* d_out, float* d_lse, hipStream_t s, const uint32_t* q_pos, uint32_t window,
                            const AttendHeldArgs* held)
{
    const char* entry = held ? (window ? "speckv_ext_attend_kv_spec_window" : "speckv_ext_attend_kv_spec")
                             : window ? "speckv_ext_attend_kv_batch_window" : "speckv_ext_attend_kv_batch";
    if (null_) return no_data_path(entry);
    if (window && !q_pos) return SPECKV_ERR_INVAL;
    if (!window) q_pos = nullptr;                                        // (no window: the launches of the entry without one)
    if (n_seq == 0) return SPECKV_OK;
    if (is_capturing(s)) {
        SPECKV_ERR("%s cannot be captured into a HIP graph (its descriptors are staged per call)", entry);
        return SPECKV_ERR_INVAL;
    }
    if (!k_handles || !v_handles || !pos_end || !d_q_f16 || !d_out || g == 0 || g > 16) return SPECKV_ERR_INVAL;
    if (reinterpret_cast<uintptr_t>(d_q_f16) % 16u || reinterpret_cast<uintptr_t>(d_out) % 16u) return SPECKV_ERR_INVAL;
    std::vector<AttendSeq> seqs(n_seq);
    std::vector<AttendKvSide> vside(n_seq);
    std::vector<uint32_t> tiles(n_seq), pages(n_seq), skips(q_pos ? n_seq : 0u);      // (skips: AttendArgs::seq_skip of a windowed launch)
    bool cut = false;                                                    // the window cuts some member's pool positions
    std::vector<Allocation*> ks(n_seq), vs(n_seq);
    uint64_t total_tiles = 0;
    for (uint32_t i = 0; i < n_seq; ++i) {
        Allocation *k = find(k_handles[i]), *v = find(v_handles[i]);
        if (!k || !v) return SPECKV_ERR_GENERAL;
        if (pos_end[i] % 2u || !split_region_ok(k, SPECKV_COMP_FP8_E4M3, layer, pos_end[i], 32u) || !split_region_ok(v, SPECKV_COMP_MXFP4, layer, pos_end[i], 32u) ||
            k->layout.num_tokens != v->layout.num_tokens)
            return SPECKV_ERR_INVAL;
        if (!k->linear_base || !k->d_scale_tab || !v->linear_base) {
            SPECKV_ERR("%s: sequence %u: the %s allocation's records do not lie in one run (striped over several pools, "
                       "or pages migrated); this entry has the single-run form only -- speckv_ext_attend_chunk_kv serves any placement",
                       entry, i, (!k->linear_base || !k->d_scale_tab) ? "K" : "V");
            return SPECKV_ERR_INVAL;
        }
        ks[i] = k; vs[i] = v;
        const uint32_t region = k->layout.num_tokens / 2u;
        // the member's walk: everything stored, or under a window the tiles from lo's on (they end where they ended without one: inside the region)
        DecodeWindowRange w{0u, 0u, pos_end[i] / 2u};
        if (q_pos && held) {
            if (q_pos[i] != pos_end[i] && q_pos[i] != pos_end[i] + 1u) return SPECKV_ERR_INVAL;     // the committed length: what is stored, or the tail behind it
            const SpecWindowRange r = spec_window_range(q_pos[i], window);
            w = DecodeWindowRange{r.n_pages ? r.begin : 0u, 0u, r.n_pages};                           // (no pool position in any row's window: nothing stored)
            skips[i] = r.n_pages ? static_cast<uint32_t>(r.rel) : 0u;
            cut = cut || static_cast<uint64_t>(q_pos[i]) + (SPECKV_HELD_MAX - 1u) > window;
        } else if (q_pos) {
            if (q_pos[i] > pos_end[i] || q_pos[i] + 1u < pos_end[i]) return SPECKV_ERR_INVAL;       // the query: the last stored position or the tail behind it
            w = decode_window_range(q_pos[i] + 1u, window);
            if (w.n_pages == 0u) w = DecodeWindowRange{0u, 0u, 0u};      // no pool position in the window: the member of pos_end = 0 (zeros, lse -inf)
            skips[i] = w.skip;
            cut = cut || w.begin != 0u || w.skip != 0u || w.n_pages != pos_end[i] / 2u;
        }
        AttendSeq& q = seqs[i];
        q = AttendSeq{};
        q.lin_base = k->linear_base;
        q.scale_tab = k->d_scale_tab;
        q.k_first = q.v_first = static_cast<uint64_t>(layer) * region + w.begin / 2u;
        q.n_pages = pages[i] = w.n_pages;
        q.layer_pages = region;
        q.stripe_n = 1u;
        q.n_splits = tiles[i] = (q.n_pages + 15u) / 16u;                 // tiles for now, pieces below
        total_tiles += tiles[i];
        vside[i] = AttendKvSide{v->linear_base, q.v_first};              // (region % 16 == 0, begin % 32 == 0: a kernel tile is one storage tile)
    }
    DeviceScope device_scope(device_);
    // NULL = the engine's stream and a synchronous call: the query may have been produced on any stream of the caller
    if (!s) HIP_TRY(hipDeviceSynchronize());
    hipStream_t st = s ? s : stream_;
    // the launch decision of the FP8 batch kernel (attend_geometry.hpp), members in one run each
    const BatchTuning tun = batch_tuning();
    const BatchShape shape{true, false, n_seq, 8u, cus(), false, false};
    const BatchForm form = batch_form(shape, tun);
    std::vector<uint32_t> order(n_seq);
    const bool ordered = batch_dispatch_order(form, tun, pages.data(), n_seq, order.data());
    const BatchGeometry geo = batch_geometry(kEntryBatch, shape, form, tun, tiles.data(), 0, ordered, nullptr);
    if (!geo.fits) return SPECKV_ERR_INVAL;
    const uint64_t parts = assign_pieces(geo, 8u, seqs.data(), n_seq);
    bool merge = false;
    for (uint32_t i = 0; i < n_seq; ++i) merge = merge || seqs[i].n_splits > 1u;
    AttendArgs k{};
    if (!attend_scratch(k, merge ? parts : 1u, 0, s)) return SPECKV_ERR_NOMEM;
    // descriptors, then the V sides, then the dispatch order, then the skip array of a launch that a window cuts: one slot, read in place by
    // the kernels (Engine::attend_batch)
    const size_t desc_bytes = n_seq * sizeof(AttendSeq), side_bytes = n_seq * sizeof(AttendKvSide), idx_bytes = n_seq * sizeof(uint32_t);
    int slot = 0;
    void* staged = nullptr;
    RC_TRY(take_seq_slot(desc_bytes + side_bytes + idx_bytes + (cut ? idx_bytes : 0u), &slot, &staged));
    memcpy(staged, seqs.data(), desc_bytes);
    memcpy(static_cast<uint8_t*>(staged) + desc_bytes, vside.data(), side_bytes);
    if (ordered) memcpy(static_cast<uint8_t*>(staged) + desc_bytes + side_bytes, order.data(), idx_bytes);
    if (cut) memcpy(static_cast<uint8_t*>(staged) + desc_bytes + side_bytes + idx_bytes, skips.data(), idx_bytes);
    uint8_t* d_slot = nullptr;
    HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_slot), staged, 0));
    k.heads = 8u;
    k.g = g;
    k.n_splits = total_tiles ? geo.max_splits : 0u;
    k.tiles_per_split = geo.tps;
    k.q16 = static_cast<const uint16_t*>(d_q_f16);
    k.scale_log2e = sm_scale * 1.4426950408889634f;
    k.lin_base = seqs[0].lin_base;                                       // (overridden per sequence)
    k.seqs = reinterpret_cast<const AttendSeq*>(d_slot);
    if (ordered) k.order = reinterpret_cast<const uint32_t*>(d_slot + desc_bytes + side_bytes);
    if (cut) k.seq_skip = reinterpret_cast<const uint32_t*>(d_slot + desc_bytes + side_bytes + idx_bytes);
    if (geo.rows_first) k.rows_first = 1u;
    k.direct_out = d_out;
    k.direct_lse = d_lse;
    k.direct_per_seq = 1u;                                               // members with one piece are final, the merge passes them over
    // behind the asynchronous pool writes on every other caller stream the engine knows (a commit on another stream)
    for (auto& w : write_evs_)
        if (w.s != st) HIP_TRY(hipStreamWaitEvent(st, w.ev, 0));
    for (uint32_t i = 0; i < n_seq; ++i) { note_use(ks[i], s); note_use(vs[i], s); }      // speckv_free waits for this stream
    // The guard event is recorded on every way out from here on: the slot must not be written again under a kernel still reading it.
    SlotGuard slot_guard{seq_ring_.ev[slot], st};
    if (held) HIP_TRY(launch_attend_k8v4_held(k, reinterpret_cast<const AttendKvSide*>(d_slot + desc_bytes), *held, n_seq, merge, d_out, d_lse, st));
    else HIP_TRY(launch_attend_k8v4(k, reinterpret_cast<const AttendKvSide*>(d_slot + desc_bytes), n_seq, merge, d_out, d_lse, st));
    if (!s) HIP_TRY(hipStreamSynchronize(stream_));
    return SPECKV_OK;
}

// speckv_ext_attend_kv_spec.  What concerns the held rows and the mask is judged first, so a bad set is SPECKV_ERR_INVAL on every engine
// (the folds' rule: Engine::fold_held_args_ok); the rest is attend_batch_kv's.  window != 0 (speckv_ext_attend_kv_spec_window): length and
// d_depth are judged here as well; window == 0: neither is looked at.
int Engine::attend_spec_kv(uint32_t n_seq, const uint64_t* k_handles, const uint64_t* v_handles, uint32_t layer, const void* d_q_f16, uint32_t g,
                           uint32_t rows_per_pos, const uint32_t* pos_end, const void* d_k_held, const void* d_v_held, uint64_t seq_stride_elems,
                           uint64_t pos_stride_elems, const uint32_t* d_mask, uint32_t mask_stride, float sm_scale, float* d_out, float* d_lse, hipStream_t s,
                           const uint32_t* length, const uint32_t* d_depth, uint32_t window)
{
    if (rows_per_pos == 0 || g % rows_per_pos || g / rows_per_pos > SPECKV_HELD_MAX - 1u) return SPECKV_ERR_INVAL;
    if (!d_k_held || !d_v_held || !d_mask || mask_stride < g / rows_per_pos) return SPECKV_ERR_INVAL;
    if (seq_stride_elems % 8u || pos_stride_elems % 8u || pos_stride_elems < 8u * 128u) return SPECKV_ERR_INVAL;
    if (reinterpret_cast<uintptr_t>(d_k_held) % 16u || reinterpret_cast<uintptr_t>(d_v_held) % 16u) return SPECKV_ERR_INVAL;
    if (window) {
        if (!length || !d_depth) return SPECKV_ERR_INVAL;
        for (uint32_t i = 0; pos_end && i < n_seq; ++i)
            if (length[i] != pos_end[i] && length[i] != pos_end[i] + 1u) return SPECKV_ERR_INVAL;
    }
    const AttendHeldArgs held{static_cast<const uint16_t*>(d_k_held), static_cast<const uint16_t*>(d_v_held), seq_stride_elems, pos_stride_elems,
                              d_mask, mask_stride, rows_per_pos, window ? d_depth : nullptr};
    return attend_batch_kv(n_seq, k_handles, v_handles, layer, d_q_f16, g, pos_end, sm_scale, d_out, d_lse, s, window ? length : nullptr, window, &held);
}

} // namespace speckv
