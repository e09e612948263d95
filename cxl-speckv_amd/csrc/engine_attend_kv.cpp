// cxl-speckv_amd/csrc/engine_attend_kv.cpp -- Engine::attend_batch_kv, the body behind speckv_ext_attend_kv_batch,
// speckv_ext_attend_kv_batch_window, speckv_ext_attend_kv_spec, speckv_ext_attend_kv_spec_window and speckv_ext_attend_kv_spec_wide: one decode step of a batch over the SPLIT POOL ("K8V4": a sequence's K rows in an FP8_E4M3
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
// wide (speckv_ext_attend_kv_spec_wide, with held): 17 <= g <= 32 rows in one pass -- k_attend_k8v4_wide (attend_kv_wide.hip), a wave per kv
// head, sequence and piece as ever, so look-ups, the region rule, the window range, the launch decision (the FP8 batch rule with the same
// members and tiles: no split rule of its own), the slot and the refusals are the ones above.  What differs: the bound on g, twice the
// partials (a piece leaves one of 16 rows per block) and the launcher.
int Engine::attend_batch_kv(uint32_t n_seq, const uint64_t* k_handles, const uint64_t* v_handles, uint32_t layer, const void* d_q_f16, uint32_t g,
                            const uint32_t* pos_end, float sm_scale, float* d_out, float* d_lse, hipStream_t s, const uint32_t* q_pos, uint32_t window,
                            const AttendHeldArgs* held, bool wide)
{
    const char* entry = wide ? "speckv_ext_attend_kv_spec_wide"
                        : held ? (window ? "speckv_ext_attend_kv_spec_window" : "speckv_ext_attend_kv_spec")
                               : window ? "speckv_ext_attend_kv_batch_window" : "speckv_ext_attend_kv_batch";
    if (null_) return no_data_path(entry);
    if (window && !q_pos) return SPECKV_ERR_INVAL;
    if (!window) q_pos = nullptr;                                        // (no window: the launches of the entry without one)
    if (n_seq == 0) return SPECKV_OK;
    if (is_capturing(s)) {
        SPECKV_ERR("%s cannot be captured into a HIP graph (its descriptors are staged per call)", entry);
        return SPECKV_ERR_INVAL;
    }
    if (!k_handles || !v_handles || !pos_end || !d_q_f16 || !d_out || g == 0 || g > (wide ? 32u : 16u) || (wide && (!held || g <= 16))) return SPECKV_ERR_INVAL;
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
    if (wide && parts > 0xFFFFFFFFull) return SPECKV_ERR_INVAL;
    if (!attend_scratch(k, merge ? parts * (wide ? 2u : 1u) : 1u, 0, s)) return SPECKV_ERR_NOMEM;
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
    if (wide) HIP_TRY(launch_attend_k8v4_wide(k, reinterpret_cast<const AttendKvSide*>(d_slot + desc_bytes), *held, n_seq, static_cast<uint32_t>(parts), merge, d_out, d_lse, st));
    else if (held) HIP_TRY(launch_attend_k8v4_held(k, reinterpret_cast<const AttendKvSide*>(d_slot + desc_bytes), *held, n_seq, merge, d_out, d_lse, st));
    else HIP_TRY(launch_attend_k8v4(k, reinterpret_cast<const AttendKvSide*>(d_slot + desc_bytes), n_seq, merge, d_out, d_lse, st));
    if (!s) HIP_TRY(hipStreamSynchronize(stream_));
    return SPECKV_OK;
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
    std::vector<AttendSeq> seqs(n_seq);
    std::vector<AttendKvSide> vside(n_seq);
    std::vector<Allocation*> ks(n_seq), vs(n_seq);
    const size_t n_mem = static_cast<size_t>(n_seq) * n_layers;
    if (n_mem > 0x7FFFFFFFull / 2u) return refuse("a grid beyond the launch limits (n_seq x n_layers)");
    std::vector<uint32_t> tiles(n_mem), pages(n_mem);                    // the members [layer][sequence] of the launch decision
    uint64_t total_tiles = 0;
    for (uint32_t i = 0; i < n_seq; ++i) {
        Allocation *k = find(k_handles[i]), *v = find(v_handles[i]);
        if (!k || !v) return SPECKV_ERR_GENERAL;
        if (layer_end > 0xFFFFFFFFull || !split_region_ok(k, SPECKV_COMP_FP8_E4M3, layer_begin, pos_end[i], 32u) ||
            !split_region_ok(v, SPECKV_COMP_MXFP4, layer_begin, pos_end[i], 32u) || k->layout.num_tokens != v->layout.num_tokens ||
            !split_region_ok(k, SPECKV_COMP_FP8_E4M3, static_cast<uint32_t>(layer_end - 1u), pos_end[i], 32u) ||
            !split_region_ok(v, SPECKV_COMP_MXFP4, static_cast<uint32_t>(layer_end - 1u), pos_end[i], 32u))
            return refuse("an allocation of the wrong scheme or layout, a pos_end beyond it, or a layer range past its regions");
        if (!k->linear_base || !k->d_scale_tab || !v->linear_base) {
            SPECKV_ERR("%s: sequence %u: the %s allocation's records do not lie in one run (striped over several pools, "
                       "or pages migrated); this entry has the single-run form only -- speckv_ext_attend_chunk_kv serves any placement",
                       entry, i, (!k->linear_base || !k->d_scale_tab) ? "K" : "V");
            return SPECKV_ERR_INVAL;
        }
        ks[i] = k; vs[i] = v;
        AttendSeq& q = seqs[i];
        q = AttendSeq{};
        q.lin_base = k->linear_base;
        q.scale_tab = k->d_scale_tab;
        q.k_first = q.v_first = 0u;                                      // region 0: the kernel adds layer * layer_pages
        q.n_pages = pos_end[i] / 2u;
        q.layer_pages = k->layout.num_tokens / 2u;
        q.stripe_n = 1u;
        q.n_splits = (q.n_pages + 15u) / 16u;                            // tiles for now, pieces below
        total_tiles += q.n_splits;
        vside[i] = AttendKvSide{v->linear_base, 0u};
        for (uint32_t l = 0; l < n_layers; ++l) { tiles[static_cast<size_t>(l) * n_seq + i] = q.n_splits; pages[static_cast<size_t>(l) * n_seq + i] = q.n_pages; }
    }
    DeviceScope device_scope(device_);
    // NULL = the engine's stream and a synchronous call: the query may have been produced on any stream of the caller
    if (!s) HIP_TRY(hipDeviceSynchronize());
    hipStream_t st = s ? s : stream_;
    // the launch decision of the FP8 batch kernel (attend_geometry.hpp) for n_seq x n_layers members, each in one run
    const uint32_t members = static_cast<uint32_t>(n_mem);
    const BatchTuning tun = batch_tuning();
    const BatchShape shape{true, false, members, 8u, cus(), false, false};
    const BatchForm form = batch_form(shape, tun);
    std::vector<uint32_t> order(members);
    const bool ordered = batch_dispatch_order(form, tun, pages.data(), members, order.data());
    const BatchGeometry geo = batch_geometry(kEntryBatch, shape, form, tun, tiles.data(), 0, ordered, nullptr);
    if (!geo.fits) return refuse("a member in more than 2048 pieces");
    const uint64_t layer_parts = assign_pieces(geo, 8u, seqs.data(), n_seq), parts = layer_parts * n_layers;
    const uint64_t rows = static_cast<uint64_t>(members) * 2u;
    if (parts > 0xFFFFFFFFull || (!geo.rows_first && rows > 65535u)) return refuse("a grid beyond the launch limits (n_seq x n_layers x 2 workgroup rows, or the partials)");
    bool merge = false;
    for (uint32_t i = 0; i < n_seq; ++i) merge = merge || seqs[i].n_splits > 1u;
    AttendArgs k{};
    if (!attend_scratch(k, merge ? parts : 1u, 0, s)) return SPECKV_ERR_NOMEM;
    // descriptors, then the V sides (one each per sequence), then the dispatch order of the members: one slot, read in place by the kernels
    const size_t desc_bytes = n_seq * sizeof(AttendSeq), side_bytes = n_seq * sizeof(AttendKvSide), idx_bytes = ordered ? members * sizeof(uint32_t) : 0u;
    int slot = 0;
    void* staged = nullptr;
    RC_TRY(take_seq_slot(desc_bytes + side_bytes + idx_bytes, &slot, &staged));
    memcpy(staged, seqs.data(), desc_bytes);
    memcpy(static_cast<uint8_t*>(staged) + desc_bytes, vside.data(), side_bytes);
    if (ordered) memcpy(static_cast<uint8_t*>(staged) + desc_bytes + side_bytes, order.data(), idx_bytes);
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
    if (geo.rows_first) k.rows_first = 1u;
    k.direct_out = d_out;
    k.direct_lse = d_lse;
    k.direct_per_seq = 1u;
    k.batch_n_seq = n_seq;
    k.batch_layer = layer_begin;
    if (n_tail) {
        k.tail_k = static_cast<const uint16_t*>(d_k_tail);
        k.tail_v = static_cast<const uint16_t*>(d_v_tail);
        k.tail_idx = d_tail_idx;
        k.tail_stride = tail_stride;
    }
    // behind the asynchronous pool writes on every other caller stream the engine knows (a commit on another stream)
    for (auto& w : write_evs_)
        if (w.s != st) HIP_TRY(hipStreamWaitEvent(st, w.ev, 0));
    for (uint32_t i = 0; i < n_seq; ++i) { note_use(ks[i], s); note_use(vs[i], s); }      // speckv_free waits for this stream
    SlotGuard slot_guard{seq_ring_.ev[slot], st};
    HIP_TRY(launch_attend_k8v4_layers(k, reinterpret_cast<const AttendKvSide*>(d_slot + desc_bytes), n_seq, n_layers, static_cast<uint32_t>(layer_parts), merge,
                                      d_out, d_lse, st));
    if (!s) HIP_TRY(hipStreamSynchronize(stream_));
    return SPECKV_OK;
}

// speckv_ext_attend_kv_spec.  What concerns the held rows and the mask is judged first, so a bad set is SPECKV_ERR_INVAL on every engine
// (the folds' rule: Engine::fold_held_args_ok); the rest is attend_batch_kv's.  window != 0 (speckv_ext_attend_kv_spec_window): length and
// d_depth are judged here as well; window == 0: neither is looked at.  wide (speckv_ext_attend_kv_spec_wide): the same judgement for
// 17 <= g <= 32 with rows_per_pos >= 2.
int Engine::attend_spec_kv(uint32_t n_seq, const uint64_t* k_handles, const uint64_t* v_handles, uint32_t layer, const void* d_q_f16, uint32_t g,
                           uint32_t rows_per_pos, const uint32_t* pos_end, const void* d_k_held, const void* d_v_held, uint64_t seq_stride_elems,
                           uint64_t pos_stride_elems, const uint32_t* d_mask, uint32_t mask_stride, float sm_scale, float* d_out, float* d_lse, hipStream_t s,
                           const uint32_t* length, const uint32_t* d_depth, uint32_t window, bool wide)
{
    // speckv_ext_attend_kv_spec_wide: 17..32 rows; fewer belong to the entries above, and one row per position would be 17+ positions
    if (wide && (g <= 16 || g > 32 || rows_per_pos == 1)) return SPECKV_ERR_INVAL;
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
    return attend_batch_kv(n_seq, k_handles, v_handles, layer, d_q_f16, g, pos_end, sm_scale, d_out, d_lse, s, window ? length : nullptr, window, &held, wide);
}

} // namespace speckv
