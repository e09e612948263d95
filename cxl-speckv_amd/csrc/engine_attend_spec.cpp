// cxl-speckv_amd/csrc/engine_attend_spec.cpp -- the DRAFT STEP of a batch, one attention launch with the rows held outside the pool folded
// inside it and, where members have several pieces, the merge behind it:
//   Engine::attend_spec_window  speckv_ext_attend_spec_window: an FP8_E4M3 pool on a SLIDING-WINDOW layer (k_attend_fp8_spec, attend_fp8_spec.hip),
//                               and speckv_ext_attend_spec_wide: 17 <= g <= 32 rows in one pass (k_attend_fp8_wide, attend_fp8_wide.hip), on a
//                               sliding-window layer or, window == 0, on a global one
//   Engine::attend_spec_mx4     speckv_ext_attend_spec_mx4: an MXFP4 pool on a global layer (k_attend_mx4_spec, attend_mx4_spec.hip)
//   Engine::attend_spec_kv      speckv_ext_attend_kv_spec, _window and _wide: the split pool (k_attend_k8v4<.., true>, k_attend_k8v4_wide)
// What the first two judge alike is spec_rows_refusal, their members are Engine::spec_members'; the split pool's are Engine::split_member's
// (engine_attend_kv.cpp).  What all do once the descriptors stand is Engine::staged_launch (engine_internal.hpp).
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

// The members of a draft step over ONE allocation per sequence of `scheme` (FP8_E4M3, MXFP4): sequence i = the allocation handles[i] with
// pos_end[i] stored positions and, under a window, length[i] committed ones; layer `layer` of its layout is read as the format's batch form
// reads it: the K region at page layer x num_tokens, the V region num_tokens / 2 pages behind it (num_tokens % 32 == 0: both start on a tile).
// ONE form: every member in a single run (Allocation::linear_base; FP8: with a scale table); a striped or migrated placement and an
// allocation of another scheme are refused with SPECKV_ERR_INVAL -- the chunk entries serve any placement.
// The walk: everything stored, or under a window spec_window_range's -- the descriptor starts at the tile of depth 0's bound in both regions
// (begin / 2 pages in: a multiple of 16 records, a kernel tile stays one group of the scale table) whatever depths the call carries, a member
// no row of which sees a pool position is one with nothing stored, and m.skip carries the members' signed rel.
int Engine::spec_members(StagedStep& m, int scheme, uint32_t n_seq, const uint64_t* handles, uint32_t layer, const uint32_t* pos_end, const uint32_t* length,
                         uint32_t window)
{
    const bool fp8 = scheme == SPECKV_COMP_FP8_E4M3;
    const auto refuse = [&](const char* why) { SPECKV_ERR("%s: %s", m.entry, why); return SPECKV_ERR_INVAL; };
    m.fp8 = fp8;
    m.mx4 = !fp8;
    m.skip.resize(window ? n_seq : 0u);
    for (uint32_t i = 0; i < n_seq; ++i) {
        Allocation* a = find(handles[i]);
        if (!a) return SPECKV_ERR_GENERAL;
        if (!a->has_layout || a->scheme != scheme)
            return refuse(fp8 ? "an allocation that is no FP8_E4M3 pool with a layout (INT4_G32 and MXFP4 pools: speckv_ext_attend_chunk_window; on a global layer the planned step and the fold launch)"
                              : "an allocation that is no MXFP4 pool with a layout (FP8_E4M3 pools: the planned step and the fold launch, speckv_ext_attend_spec_wide; any scheme: speckv_ext_attend_chunk)");
        const Layout& L = a->layout;
        // the region rule of the batch form: 8 x 128 fp16 per position, regions that start on a tile, the layer and pos_end inside the layout
        if (L.head_dim != 128 || L.bytes_per_element != 2 || L.num_heads != 8 || L.num_tokens % 32u || layer >= L.num_layers || pos_end[i] > L.num_tokens ||
            (static_cast<uint64_t>(layer) + 1u) * L.num_tokens > a->n_pages)
            return refuse("a layout that is not 8 heads x 128 fp16 with num_tokens % 32 == 0, or a layer or pos_end outside it");
        if (!a->linear_base || (fp8 && !a->d_scale_tab)) {
            SPECKV_ERR("%s: sequence %u: the allocation's records do not lie in one run (striped over several pools, or pages migrated); "
                       "this entry has the single-run form only -- %s serves any placement", m.entry, i, fp8 ? "speckv_ext_attend_chunk_window" : "speckv_ext_attend_chunk");
            return SPECKV_ERR_INVAL;
        }
        m.allocs.push_back(a);
        const SpecWindowRange r = window ? spec_window_range(length[i], window) : SpecWindowRange{0u, 0, pos_end[i] / 2u};
        if (window) m.skip[i] = r.n_pages ? static_cast<uint32_t>(r.rel) : 0u;
        AttendSeq& q = m.seqs[i];
        q = AttendSeq{};
        q.lin_base = a->linear_base;
        if (fp8) q.scale_tab = a->d_scale_tab;
        q.k_first = static_cast<uint64_t>(layer) * L.num_tokens + (r.n_pages ? r.begin : 0u) / 2u;      // (no pool position in any row's window: nothing stored)
        q.v_first = q.k_first + L.num_tokens / 2u;
        q.n_pages = m.pages[i] = r.n_pages;
        q.layer_pages = L.num_tokens;
        q.stripe_n = 1u;
        q.n_splits = m.tiles[i] = (q.n_pages + 15u) / 16u;               // tiles for now, pieces in staged_launch
        m.total_tiles += m.tiles[i];
    }
    return SPECKV_OK;
}

// speckv_ext_attend_spec_window, and with `wide` speckv_ext_attend_spec_wide.  What the arguments alone decide is judged first, so it is
// SPECKV_ERR_INVAL on every engine: the held rows (Engine::fold_held_args_ok, the folds' rule -- d_lse is optional here, the rule's pointer
// check is given d_out in its place), the mask table, the window, the lengths.  The members are spec_members' for FP8_E4M3; the launch
// decision is attend_geometry.hpp's for BatchShape{fp8 = true} over the pages actually walked.  Under a window the rel array is always
// staged: k_attend_fp8_spec has one instance, and a window that cuts no row passes none of its gates.
// wide with window == 0: every member is walked over all pos_end / 2 pages from page 0, no rel array is staged (a.seq_skip stays NULL: the
// kernel's plain instance), and neither length nor d_depth is looked at; the partials are 2 x those of the pieces.
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
    StagedStep m(entry, n_seq, n_seq, false, d_q_f16, g, sm_scale, d_out, d_lse);
    RC_TRY(spec_members(m, SPECKV_COMP_FP8_E4M3, n_seq, handles, layer, pos_end, length, window));
    m.copies = wide ? 2u : 1u;
    const AttendHeldArgs held{static_cast<const uint16_t*>(d_k_held), static_cast<const uint16_t*>(d_v_held), seq_stride_elems, pos_stride_elems,
                              d_mask, mask_stride, rows_per_pos, window ? d_depth : nullptr};
    return staged_launch(m, s, [&](AttendArgs& k, const AttendKvSide*, uint32_t parts, bool merge, hipStream_t st) {
        if (wide) HIP_TRY(launch_attend_fp8_wide(k, held, n_seq, parts, merge, d_out, d_lse, st));
        else HIP_TRY(launch_attend_fp8_spec(k, held, n_seq, merge, d_out, d_lse, st));
        return SPECKV_OK;
    });
}

// speckv_ext_attend_spec_mx4: the same step over an MXFP4 pool on a global layer -- every row of the step sees all pos_end[i] stored
// positions; the members are spec_members' for MXFP4 (both regions start on a storage tile of the tile-planar run, which is what
// k_attend_mx4_spec's ten requests per tile assume).  Judged as attend_spec_window judges: the arguments first (SPECKV_ERR_INVAL on every
// engine), then the capture, then the allocations.  The launch decision is attend_geometry.hpp's for BatchShape{mx4 = true}.
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
    StagedStep m(entry, n_seq, n_seq, false, d_q_f16, g, sm_scale, d_out, d_lse);
    RC_TRY(spec_members(m, SPECKV_COMP_MXFP4, n_seq, handles, layer, pos_end, nullptr, 0u));
    const AttendHeldArgs held{static_cast<const uint16_t*>(d_k_held), static_cast<const uint16_t*>(d_v_held), seq_stride_elems, pos_stride_elems,
                              d_mask, mask_stride, rows_per_pos, nullptr};
    return staged_launch(m, s, [&](AttendArgs& k, const AttendKvSide*, uint32_t, bool merge, hipStream_t st) {
        HIP_TRY(launch_attend_mx4_spec(k, held, n_seq, merge, d_out, d_lse, st));
        return SPECKV_OK;
    });
}

// speckv_ext_attend_kv_spec: the step over the SPLIT POOL -- g = n_q x rows_per_pos query rows that all see every stored position, so
// members (Engine::split_member), geometry, pieces and slot are those of a decode step of g rows (Engine::attend_batch_kv); the launch is
// k_attend_k8v4<false, true>, whose split 0 folds the held rows of every member into its final rows or its partial.  What concerns the held
// rows and the mask is judged first, so a bad set is SPECKV_ERR_INVAL on every engine (the folds' rule restated: Engine::fold_held_args_ok,
// with pos_stride_elems bounded from below as well).
// window != 0 (speckv_ext_attend_kv_spec_window; spec_window.hpp): length and d_depth are judged as well; window == 0: neither is looked at.
// The rows of a member no longer share a lower bound, so its descriptor starts at the tile of depth 0's bound in both allocations whatever
// depths the call carries, the tiles, the dispatch order and the pieces are those of the pages walked, and the skip array carries the
// member's SIGNED rel (k_attend_k8v4<true, true> adds the row's depth).  A member no row of which sees a pool position is one with nothing
// stored: its held positions alone.  A window that can cut no member (length + 16 <= window for all): the descriptors, the instance and
// the launches of the entry without one.
// wide (speckv_ext_attend_kv_spec_wide): 17 <= g <= 32 rows with rows_per_pos >= 2 in one pass -- k_attend_k8v4_wide (attend_kv_wide.hip), a
// wave per kv head, sequence and piece as ever, so everything above holds; what differs is the bound on g, twice the partials (a piece
// leaves one of 16 rows per block) and the launcher.
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
            if (length[i] != pos_end[i] && length[i] != pos_end[i] + 1u) return SPECKV_ERR_INVAL;      // the committed length: what is stored, or the tail behind it
    }
    const char* entry = wide ? "speckv_ext_attend_kv_spec_wide" : window ? "speckv_ext_attend_kv_spec_window" : "speckv_ext_attend_kv_spec";
    if (null_) return no_data_path(entry);
    if (n_seq == 0) return SPECKV_OK;
    if (is_capturing(s)) {
        SPECKV_ERR("%s cannot be captured into a HIP graph (its descriptors are staged per call)", entry);
        return SPECKV_ERR_INVAL;
    }
    if (!k_handles || !v_handles || !pos_end || !d_q_f16 || !d_out || g == 0 || g > (wide ? 32u : 16u)) return SPECKV_ERR_INVAL;
    if (reinterpret_cast<uintptr_t>(d_q_f16) % 16u || reinterpret_cast<uintptr_t>(d_out) % 16u) return SPECKV_ERR_INVAL;
    StagedStep m(entry, n_seq, n_seq, true, d_q_f16, g, sm_scale, d_out, d_lse);
    m.copies = wide ? 2u : 1u;
    m.skip.resize(window ? n_seq : 0u);
    bool cut = false;                                                    // the window cuts some member's pool positions
    for (uint32_t i = 0; i < n_seq; ++i) {
        const SpecWindowRange r = window ? spec_window_range(length[i], window) : SpecWindowRange{0u, 0, pos_end[i] / 2u};
        RC_TRY(split_member(m, i, k_handles[i], v_handles[i], layer, layer, pos_end[i], r.n_pages ? r.begin : 0u, r.n_pages));      // (no pool position in any row's window: nothing stored)
        if (!window) continue;
        m.skip[i] = r.n_pages ? static_cast<uint32_t>(r.rel) : 0u;
        cut = cut || static_cast<uint64_t>(length[i]) + (SPECKV_HELD_MAX - 1u) > window;
    }
    if (!cut) m.skip.clear();                                            // (the plain instance)
    const AttendHeldArgs held{static_cast<const uint16_t*>(d_k_held), static_cast<const uint16_t*>(d_v_held), seq_stride_elems, pos_stride_elems,
                              d_mask, mask_stride, rows_per_pos, window ? d_depth : nullptr};
    return staged_launch(m, s, [&](AttendArgs& k, const AttendKvSide* d_vside, uint32_t parts, bool merge, hipStream_t st) {
        if (wide) HIP_TRY(launch_attend_k8v4_wide(k, d_vside, held, n_seq, parts, merge, d_out, d_lse, st));
        else HIP_TRY(launch_attend_k8v4_held(k, d_vside, held, n_seq, merge, d_out, d_lse, st));
        return SPECKV_OK;
    });
}

} // namespace speckv
