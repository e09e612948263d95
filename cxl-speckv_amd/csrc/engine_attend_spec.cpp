// cxl-speckv_amd/csrc/engine_attend_spec.cpp -- Engine::attend_spec_window, the body behind speckv_ext_attend_spec_window: the draft step
// of a batch over an FP8_E4M3 pool on a SLIDING-WINDOW layer, one attention launch (k_attend_fp8_spec, attend_fp8_spec.hip) with the rows
// held outside the pool folded inside it and, where members have several pieces, the merge behind it.  The FP8 counterpart of
// Engine::attend_batch_kv's held-and-window path (engine_attend_kv.cpp), with one allocation per sequence in the place of two.
// wide: the body behind speckv_ext_attend_spec_wide as well -- 17 <= g <= 32 rows in one pass (k_attend_fp8_wide, attend_fp8_wide.hip),
// on a sliding-window layer or, window == 0, on a global one; the same descriptor staging, a.part_acc / part_ml for 2 x parts partials.
// Engine::attend_spec_mx4, the body behind speckv_ext_attend_spec_mx4: the same step over an MXFP4 pool on a global layer (k_attend_mx4_spec,
// attend_mx4_spec.hip).  What both judge alike is spec_rows_refusal; what both do once the descriptors stand is Engine::spec_step_launch.
#include "engine_internal.hpp"
#include "spec_window.hpp"
#include "tuning.hpp"

namespace speckv {

// What the draft-step entries over one allocation per sequence judge alike, from the arguments alone, behind the held rows' own rule
// (Engine::fold_held_args_ok): the mask table, the alignment of the rows a lane reads 16 bytes at a time, whole pages.  NULL: nothing to refuse.
static const char* spec_rows_refusal(uint32_t n_seq, const void* d_q_f16, uint32_t g, uint32_t rows_per_pos, const uint32_t* pos_end, const void* d_k_held,
                                     const void* d_v_held, const uint32_t* d_mask, uint32_t mask_stride, const float* d_out)
{
    if (!d_mask || mask_stride < g / rows_per_pos) return "no mask table, or mask_stride below g / rows_per_pos";
    if (reinterpret_cast<uintptr_t>(d_q_f16) % 16u || reinterpret_cast<uintptr_t>(d_out) % 16u || reinterpret_cast<uintptr_t>(d_k_held) % 16u ||
        reinterpret_cast<uintptr_t>(d_v_held) % 16u)
        return "the query, the output or the held rows are not 16-byte aligned";
    for (uint32_t i = 0; pos_end && i < n_seq; ++i)
        if (pos_end[i] % 2u) return "an odd pos_end";
    return nullptr;
}

// The members of such a step once their descriptors stand (n_splits = the member's tiles until assign_pieces), and what the launch needs of the call.
struct Engine::SpecStep {
    const char* entry;
    bool mx4, wide;                   // the pool's format (else FP8_E4M3); 17..32 rows in one pass (FP8 only)
    std::vector<AttendSeq> seqs;
    std::vector<uint32_t> tiles, pages, rels;      // rels: staged only under a window
    std::vector<Allocation*> allocs;
    uint64_t total_tiles = 0;
    bool window = false;
    const void* d_q_f16; uint32_t g; float sm_scale;
    AttendHeldArgs held;
    float* d_out; float* d_lse;
};

// Sequence i = the allocation handles[i] with pos_end[i] stored positions and length[i] committed ones; layer `layer` of its layout is
// read as the FP8 batch form reads it: the K region at page layer x num_tokens, the V region num_tokens / 2 pages behind it.
// What the arguments alone decide is judged first, so it is SPECKV_ERR_INVAL on every engine: the held rows (Engine::fold_held_args_ok,
// the folds' rule -- d_lse is optional here, the rule's pointer check is given d_out in its place), the mask table, the window, the lengths.
// ONE form: every member in a single run with a scale table (Allocation::linear_base, d_scale_tab); a striped or migrated placement is
// refused with SPECKV_ERR_INVAL -- speckv_ext_attend_chunk_window serves any placement.  An allocation of another scheme (INT4_G32, MXFP4)
// is refused likewise: this entry serves the FP8 pool alone.
// wide with window == 0: every member is walked over all pos_end / 2 pages from page 0, no rel array is staged (a.seq_skip stays NULL: the
// kernel's plain instance), and neither length nor d_depth is looked at.
// The walk is spec_window_range's: the descriptor starts at the tile of depth 0's bound in both regions (begin / 2 pages in: a multiple of
// 16 records, a kernel tile stays one group of the scale table) whatever depths the call carries; a member no row of which sees a pool
// position is one with nothing stored.  The launch decision is attend_geometry.hpp's for BatchShape{fp8 = true} over the pages actually
// walked -- form, dispatch order, one split length, the members' pieces, with the tuning keys attend_tiles_per_split and
// attend_order_as_given.  Descriptors, dispatch order and the rel array (always staged: the kernel has one instance, and a window that cuts
// no row passes none of its gates) travel through ONE slot of the pinned descriptor ring, read in place: not capturable into a HIP graph.
int Engine::attend_spec_window(uint32_t n_seq, const uint64_t* handles, uint32_t layer, const void* d_q_f16, uint32_t g, uint32_t rows_per_pos,
                               const uint32_t* pos_end, const uint32_t* length, const uint32_t* d_depth, uint32_t window, const void* d_k_held,
                               const void* d_v_held, uint64_t seq_stride_elems, uint64_t pos_stride_elems, const uint32_t* d_mask, uint32_t mask_stride,
                               float sm_scale, float* d_out, float* d_lse, hipStream_t s, bool wide)
{
    const char* entry = wide ? "speckv_ext_attend_spec_wide" : "speckv_ext_attend_spec_window";
    const auto refuse = [&](const char* why) { SPECKV_ERR("%s: %s", entry, why); return SPECKV_ERR_INVAL; };
    // speckv_ext_attend_spec_wide: 17..32 rows; fewer belong to the 16-row routes, and one row per position would be 17+ positions.  The
    // rest of the held rows' rule is the folds', judged on the rows of one block
    if (wide && (g <= 16 || g > 32 || rows_per_pos < 2u || g % rows_per_pos))
        return refuse("g outside 17..32 or no multiple of rows_per_pos, or rows_per_pos below 2 (16 rows or fewer: speckv_ext_attend_spec_window, or the planned step and the fold launch)");
    const uint32_t n_pos = rows_per_pos ? g / rows_per_pos : 0u;
    if (!fold_held_args_ok(8u, wide ? n_pos : g, wide ? 1u : rows_per_pos, d_q_f16, d_k_held, d_v_held, seq_stride_elems, pos_stride_elems, d_out, d_lse ? d_lse : d_out))
        return refuse(wide ? "more than SPECKV_HELD_MAX - 1 positions, overlapping held rows, or a NULL query, held row or output" :
                      "g outside 1..16 or no multiple of rows_per_pos, more than SPECKV_HELD_MAX - 1 positions, overlapping held rows, or a NULL query, held row or output");
    if (const char* why = spec_rows_refusal(n_seq, d_q_f16, g, rows_per_pos, pos_end, d_k_held, d_v_held, d_mask, mask_stride, d_out)) return refuse(why);
    if (window == 0 && !wide) return refuse("window is 0 (a global layer: the planned step and the fold launch)");
    if (window && (!length || !d_depth)) return refuse("a NULL length or d_depth");
    for (uint32_t i = 0; pos_end && i < n_seq; ++i)
        if (window && length[i] != pos_end[i] && length[i] != pos_end[i] + 1u) return refuse("a length outside {pos_end, pos_end + 1}");
    if (null_) return no_data_path(entry);
    if (n_seq == 0) return SPECKV_OK;
    if (is_capturing(s)) return refuse("cannot be captured into a HIP graph (its descriptors are staged per call)");
    if (!handles || !pos_end) return refuse("a NULL handle array or pos_end");
    SpecStep m{entry, false, wide};
    m.seqs.resize(n_seq); m.tiles.resize(n_seq); m.pages.resize(n_seq); m.rels.resize(n_seq); m.allocs.resize(n_seq);
    std::vector<AttendSeq>& seqs = m.seqs;
    std::vector<uint32_t>&tiles = m.tiles, &pages = m.pages, &rels = m.rels;
    std::vector<Allocation*>& allocs = m.allocs;
    uint64_t& total_tiles = m.total_tiles;
    for (uint32_t i = 0; i < n_seq; ++i) {
        Allocation* a = find(handles[i]);
        if (!a) return SPECKV_ERR_GENERAL;
        if (!a->has_layout || a->scheme != SPECKV_COMP_FP8_E4M3) return refuse("an allocation that is no FP8_E4M3 pool with a layout (INT4_G32 and MXFP4 pools: speckv_ext_attend_chunk_window; on a global layer the planned step and the fold launch)");
        const Layout& L = a->layout;
        // the region rule of the FP8 batch form: 8 x 128 fp16 per position, regions that start on a tile, the layer and pos_end inside the layout
        if (L.head_dim != 128 || L.bytes_per_element != 2 || L.num_heads != 8 || L.num_tokens % 32u || layer >= L.num_layers || pos_end[i] > L.num_tokens ||
            (static_cast<uint64_t>(layer) + 1u) * L.num_tokens > a->n_pages)
            return refuse("a layout that is not 8 heads x 128 fp16 with num_tokens % 32 == 0, or a layer or pos_end outside it");
        if (!a->linear_base || !a->d_scale_tab) {
            SPECKV_ERR("%s: sequence %u: the allocation's records do not lie in one run (striped over several pools, or pages migrated); "
                       "this entry has the single-run form only -- speckv_ext_attend_chunk_window serves any placement", entry, i);
            return SPECKV_ERR_INVAL;
        }
        allocs[i] = a;
        const SpecWindowRange r = window ? spec_window_range(length[i], window) : SpecWindowRange{0u, 0, pos_end[i] / 2u};
        const uint32_t begin = r.n_pages ? r.begin : 0u;                // (no pool position in any row's window: nothing stored)
        rels[i] = r.n_pages ? static_cast<uint32_t>(r.rel) : 0u;
        AttendSeq& q = seqs[i];
        q = AttendSeq{};
        q.lin_base = a->linear_base;
        q.scale_tab = a->d_scale_tab;
        q.k_first = static_cast<uint64_t>(layer) * L.num_tokens + begin / 2u;         // both regions from the tile of depth 0's bound on
        q.v_first = q.k_first + L.num_tokens / 2u;
        q.n_pages = pages[i] = r.n_pages;
        q.layer_pages = L.num_tokens;
        q.stripe_n = 1u;
        q.n_splits = tiles[i] = (q.n_pages + 15u) / 16u;                 // tiles for now, pieces below
        total_tiles += tiles[i];
    }
    m.window = window != 0;
    m.d_q_f16 = d_q_f16; m.g = g; m.sm_scale = sm_scale;
    m.held = AttendHeldArgs{static_cast<const uint16_t*>(d_k_held), static_cast<const uint16_t*>(d_v_held), seq_stride_elems, pos_stride_elems,
                            d_mask, mask_stride, rows_per_pos, window ? d_depth : nullptr};
    m.d_out = d_out; m.d_lse = d_lse;
    return spec_step_launch(m, s);
}

// The step once the members' descriptors stand, for both entries above and below: the launch decision, the scratch, ONE slot of the pinned
// descriptor ring (descriptors, then the dispatch order, then -- under a window -- the rel array), the waits, the launch and its merge.
int Engine::spec_step_launch(SpecStep& m, hipStream_t s)
{
    const auto refuse = [](const char* entry, const char* why) { SPECKV_ERR("%s: %s", entry, why); return SPECKV_ERR_INVAL; };
    DeviceScope device_scope(device_);
    // NULL = the engine's stream and a synchronous call: the query may have been produced on any stream of the caller
    if (!s) HIP_TRY(hipDeviceSynchronize());
    hipStream_t st = s ? s : stream_;
    // the launch decision of the format's batch kernel (attend_geometry.hpp) over the pages walked, members in one run each
    const BatchTuning tun = batch_tuning();
    const uint32_t n_seq = static_cast<uint32_t>(m.seqs.size());
    const BatchShape shape{!m.mx4, m.mx4, n_seq, 8u, cus(), false, false};
    const BatchForm form = batch_form(shape, tun);
    std::vector<uint32_t> order(n_seq);
    const bool ordered = batch_dispatch_order(form, tun, m.pages.data(), n_seq, order.data());
    const BatchGeometry geo = batch_geometry(kEntryBatch, shape, form, tun, m.tiles.data(), 0, ordered, nullptr);
    if (!geo.fits) return refuse(m.entry, "a member in more than 2048 pieces");
    const uint64_t parts = assign_pieces(geo, 8u, m.seqs.data(), n_seq);
    bool merge = false;
    for (uint32_t i = 0; i < n_seq; ++i) merge = merge || m.seqs[i].n_splits > 1u;
    AttendArgs k{};
    if (m.wide && parts > 0xFFFFFFFFull) return refuse(m.entry, "more than 2^32 partials per row block");
    if (!attend_scratch(k, merge ? parts * (m.wide ? 2u : 1u) : 1u, 0, s)) return SPECKV_ERR_NOMEM;
    // descriptors, then the dispatch order, then the rel array: one slot, read in place by the kernel (Engine::attend_batch)
    const size_t desc_bytes = n_seq * sizeof(AttendSeq), idx_bytes = n_seq * sizeof(uint32_t);
    int slot = 0;
    void* staged = nullptr;
    RC_TRY(take_seq_slot(desc_bytes + 2u * idx_bytes, &slot, &staged));
    memcpy(staged, m.seqs.data(), desc_bytes);
    if (ordered) memcpy(static_cast<uint8_t*>(staged) + desc_bytes, order.data(), idx_bytes);
    if (m.window) memcpy(static_cast<uint8_t*>(staged) + desc_bytes + idx_bytes, m.rels.data(), idx_bytes);
    uint8_t* d_slot = nullptr;
    HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_slot), staged, 0));
    k.heads = 8u;
    k.g = m.g;
    k.n_splits = m.total_tiles ? geo.max_splits : 0u;
    k.tiles_per_split = geo.tps;
    k.q16 = static_cast<const uint16_t*>(m.d_q_f16);
    k.scale_log2e = m.sm_scale * 1.4426950408889634f;
    k.lin_base = m.seqs[0].lin_base;                                       // (overridden per sequence)
    k.seqs = reinterpret_cast<const AttendSeq*>(d_slot);
    if (ordered) k.order = reinterpret_cast<const uint32_t*>(d_slot + desc_bytes);
    if (m.window) k.seq_skip = reinterpret_cast<const uint32_t*>(d_slot + desc_bytes + idx_bytes);
    if (geo.rows_first) k.rows_first = 1u;
    k.direct_out = m.d_out;
    k.direct_lse = m.d_lse;
    k.direct_per_seq = 1u;                                               // members with one piece or none are final, the merge passes them over
    // behind the asynchronous pool writes on every other caller stream the engine knows (a commit on another stream)
    for (auto& w : write_evs_)
        if (w.s != st) HIP_TRY(hipStreamWaitEvent(st, w.ev, 0));
    for (uint32_t i = 0; i < n_seq; ++i) note_use(m.allocs[i], s);         // speckv_free waits for this stream
    // The guard event is recorded on every way out from here on: the slot must not be written again under a kernel still reading it.
    SlotGuard slot_guard{seq_ring_.ev[slot], st};
    if (m.mx4) HIP_TRY(launch_attend_mx4_spec(k, m.held, n_seq, merge, m.d_out, m.d_lse, st));
    else if (m.wide) HIP_TRY(launch_attend_fp8_wide(k, m.held, n_seq, static_cast<uint32_t>(parts), merge, m.d_out, m.d_lse, st));
    else HIP_TRY(launch_attend_fp8_spec(k, m.held, n_seq, merge, m.d_out, m.d_lse, st));
    if (!s) HIP_TRY(hipStreamSynchronize(stream_));
    return SPECKV_OK;
}

// The same step over an MXFP4 pool on a global layer: sequence i = the MXFP4 allocation handles[i] with pos_end[i] stored positions, every row
// of the step sees them all; layer `layer` is read as the MXFP4 batch form reads it (Engine::gather_members for scheme 5): the K region at
// record layer x num_tokens, the V region num_tokens / 2 records behind it -- with num_tokens % 32 == 0 both start on a storage tile of the
// tile-planar run, which is what k_attend_mx4_spec's ten requests per tile assume.  Judged as attend_spec_window judges: the arguments first
// (SPECKV_ERR_INVAL on every engine), then the capture, then the allocations.  ONE form: every member in a single run
// (Allocation::linear_base); a striped or migrated placement, and an allocation of another scheme, is refused with SPECKV_ERR_INVAL --
// speckv_ext_attend_chunk serves every placement and scheme.  The launch decision is attend_geometry.hpp's for BatchShape{mx4 = true}.
int Engine::attend_spec_mx4(uint32_t n_seq, const uint64_t* handles, uint32_t layer, const void* d_q_f16, uint32_t g, uint32_t rows_per_pos,
                            const uint32_t* pos_end, const void* d_k_held, const void* d_v_held, uint64_t seq_stride_elems, uint64_t pos_stride_elems,
                            const uint32_t* d_mask, uint32_t mask_stride, float sm_scale, float* d_out, float* d_lse, hipStream_t s)
{
    const char* entry = "speckv_ext_attend_spec_mx4";
    const auto refuse = [&](const char* why) { SPECKV_ERR("%s: %s", entry, why); return SPECKV_ERR_INVAL; };
    if (!fold_held_args_ok(8u, g, rows_per_pos, d_q_f16, d_k_held, d_v_held, seq_stride_elems, pos_stride_elems, d_out, d_lse ? d_lse : d_out))
        return refuse("g outside 1..16 or no multiple of rows_per_pos, more than SPECKV_HELD_MAX - 1 positions, overlapping held rows, or a NULL query, held row or output");
    if (const char* why = spec_rows_refusal(n_seq, d_q_f16, g, rows_per_pos, pos_end, d_k_held, d_v_held, d_mask, mask_stride, d_out)) return refuse(why);
    if (null_) return no_data_path(entry);
    if (n_seq == 0) return SPECKV_OK;
    if (is_capturing(s)) return refuse("cannot be captured into a HIP graph (its descriptors are staged per call)");
    if (!handles || !pos_end) return refuse("a NULL handle array or pos_end");
    SpecStep m{entry, true, false};
    m.seqs.resize(n_seq); m.tiles.resize(n_seq); m.pages.resize(n_seq); m.allocs.resize(n_seq);
    for (uint32_t i = 0; i < n_seq; ++i) {
        Allocation* a = find(handles[i]);
        if (!a) return SPECKV_ERR_GENERAL;
        if (!a->has_layout || a->scheme != SPECKV_COMP_MXFP4)
            return refuse("an allocation that is no MXFP4 pool with a layout (FP8_E4M3 pools: the planned step and the fold launch, speckv_ext_attend_spec_wide; any scheme: speckv_ext_attend_chunk)");
        const Layout& L = a->layout;
        if (L.head_dim != 128 || L.bytes_per_element != 2 || L.num_heads != 8 || L.num_tokens % 32u || layer >= L.num_layers || pos_end[i] > L.num_tokens ||
            (static_cast<uint64_t>(layer) + 1u) * L.num_tokens > a->n_pages)
            return refuse("a layout that is not 8 heads x 128 fp16 with num_tokens % 32 == 0, or a layer or pos_end outside it");
        if (!a->linear_base) {
            SPECKV_ERR("%s: sequence %u: the allocation's records do not lie in one run (striped over several pools, or pages migrated); "
                       "this entry has the single-run form only -- speckv_ext_attend_chunk serves any placement", entry, i);
            return SPECKV_ERR_INVAL;
        }
        m.allocs[i] = a;
        AttendSeq& q = m.seqs[i];
        q = AttendSeq{};
        q.lin_base = a->linear_base;
        q.k_first = static_cast<uint64_t>(layer) * L.num_tokens;
        q.v_first = q.k_first + L.num_tokens / 2u;
        q.n_pages = m.pages[i] = pos_end[i] / 2u;
        q.layer_pages = L.num_tokens;
        q.stripe_n = 1u;
        q.n_splits = m.tiles[i] = (q.n_pages + 15u) / 16u;               // tiles for now, pieces in spec_step_launch
        m.total_tiles += m.tiles[i];
    }
    m.d_q_f16 = d_q_f16; m.g = g; m.sm_scale = sm_scale;
    m.held = AttendHeldArgs{static_cast<const uint16_t*>(d_k_held), static_cast<const uint16_t*>(d_v_held), seq_stride_elems, pos_stride_elems,
                            d_mask, mask_stride, rows_per_pos, nullptr};
    m.d_out = d_out; m.d_lse = d_lse;
    return spec_step_launch(m, s);
}

} // namespace speckv
