// cxl-speckv_amd/csrc/engine_attend.cpp -- fused decode attention over FP8 / INT4_G32 / MXFP4 records, single sequences and batches (Engine members):
// checks, scratch, arguments and launches around the launch decisions of attend_geometry.hpp
#include "engine_internal.hpp"
#include "decode_window.hpp"
#include "tuning.hpp"

#include <optional>

namespace speckv {

// ---- what the entries share ---------------------------------------------------------------------------------------------------
// One single-sequence call (qk_scores_fp8, attend_fp8 / _int4 / _mx4) between attend_begin and attend_end.
struct Engine::SeqCall {
    Allocation* a = nullptr;
    std::optional<DeviceScope> device_scope;
    hipStream_t st = nullptr;                 // the caller's stream, or the engine's (NULL: a synchronous call)
    bool done = false;                        // an empty range: answered by attend_begin
    uint32_t pos_begin = 0, n_pages = 0, skip_pages = 0;
    uint64_t k_first = 0, v_first = 0, layer_stride = 0;
    int scheme = -1;
    bool scores = false;
    uint32_t n_layers = 0, g = 0;
    // the call as the launch decision sees it (attend_geometry.hpp)
    SeqShape shape(uint32_t cus) const
    {
        return SeqShape{scheme == SPECKV_COMP_FP8_E4M3, scheme == SPECKV_COMP_MXFP4, scores, n_layers, a->layout.num_heads, g, cus, a->layout.num_tokens,
                        pos_begin, n_pages, skip_pages, a->d_scale_tab != nullptr, a->linear_base != nullptr, a->stripe_n};
    }
    // the fields an attention launch takes from the call and its decision (zero_page: after ensure_zero_page, where the form needs it); the query
    // pointers and the FP8 tables are the entry's
    void args(AttendArgs& k, const SeqDecision& d, float sm_scale, const uint8_t* zero_page, float* d_out, float* d_lse) const
    {
        k.entries = a->d_entries;
        k.k_first = k_first;
        k.v_first = v_first;
        k.layer_stride = layer_stride;
        k.n_pages = n_pages;
        k.skip_pages = skip_pages;
        k.heads = a->layout.num_heads;
        k.g = g;
        k.scale_log2e = sm_scale * 1.4426950408889634f;
        k.zero_page = zero_page;
        k.n_splits = d.slots;
        k.tiles_per_split = d.tiles_per_split;
        k.stream = d.stream;
        k.wg8 = d.wg8;
        if (d.place == kSeqLinear) k.lin_base = a->linear_base;
        if (d.place == kSeqStriped) {
            k.stripe_bases = a->d_stripe;
            k.stripe_n = a->stripe_n;
            k.stripe_magic = static_cast<uint32_t>((1ull << 32) / a->stripe_n + 1u);
        }
        if (d.place == kSeqTable) k.table_form = 1u;
        if (d.direct_out) { k.direct_out = d_out; k.direct_lse = d_lse; }
    }
};

// Checks the allocation's layout and the range, applies the NULL stream rule, answers an empty range (zeros; qk_scores_fp8, scores: nothing to
// write) and gives the pages of the range in the shim layout.
int Engine::attend_begin(int scheme, bool scores, uint64_t handle, uint32_t layer, uint32_t n_layers, const void* d_q_f16, uint32_t g, uint32_t pos_begin,
                         uint32_t pos_end, float* d_out, hipStream_t s, SeqCall& c)
{
    Allocation* a = find(handle);
    if (!a) return SPECKV_ERR_GENERAL;
    if (!a->has_layout || a->scheme != scheme) return SPECKV_ERR_INVAL;
    const Layout& L = a->layout;
    // one K row (all heads of a position) must be 2048 B: two positions per page
    if (L.head_dim != 128 || L.bytes_per_element != 2 || L.num_heads * L.head_dim != 1024 || (!scores && L.num_tokens % 2)) return SPECKV_ERR_INVAL;
    if (n_layers == 0 || layer >= L.num_layers || n_layers > L.num_layers - layer || pos_begin % 2 || pos_begin > pos_end ||
        pos_end > L.num_tokens || pos_end % 2)
        return SPECKV_ERR_INVAL;
    if (g == 0 || g > 16 || !d_q_f16 || !d_out) return SPECKV_ERR_INVAL;
    c.a = a;
    c.scheme = scheme; c.scores = scores; c.n_layers = n_layers; c.g = g;
    const bool empty = pos_end == pos_begin;
    if (scores && empty) { c.done = true; return SPECKV_OK; }
    if (!empty) {
        // The scale table is laid out in tiles of 32 positions from the start of a region: a range that starts inside a tile is
        // attended from the tile's start with its leading positions masked (AttendArgs::skip_pages), so every range of a layout
        // with a scale table takes the tile forms (linear / striped / table) -- the per-wave page-table kernel is left with the
        // layouts that have none (num_tokens not a multiple of 32).
        // (INT4 / MXFP4: tiles of 32 positions count from pos_begin -- the scales travel inside the records: no table to stay aligned with)
        const bool align = !scores && scheme == SPECKV_COMP_FP8_E4M3 && a->d_scale_tab != nullptr;
        c.pos_begin = align ? (pos_begin & ~31u) : pos_begin;
        c.skip_pages = (pos_begin - c.pos_begin) / 2;
        c.n_pages = (pos_end - c.pos_begin) / 2;
        // shim layout [req 0][layer][kind][pos][head]: K pages of a layer, then its V pages
        c.k_first = (static_cast<uint64_t>(layer) * 2 * L.num_tokens + c.pos_begin) / 2;
        c.v_first = c.k_first + L.num_tokens / 2;
        c.layer_stride = static_cast<uint64_t>(L.num_tokens);      // pages per layer: K + V = 2*T/2
        if ((scores ? c.k_first : c.v_first) + (n_layers - 1) * c.layer_stride + c.n_pages > a->n_pages) return SPECKV_ERR_GENERAL;
    }
    c.device_scope.emplace(device_);
    // NULL = the engine's stream and a synchronous call: the query may have been produced on any stream of the caller
    if (!s) HIP_TRY(hipDeviceSynchronize());
    c.st = s ? s : stream_;
    if (empty) {  // empty range: softmax over nothing -> zeros (and -inf lse is left to the caller)
        const size_t out_elems = static_cast<size_t>(n_layers) * L.num_heads * g * 128;
        HIP_TRY(hipMemsetAsync(d_out, 0, out_elems * sizeof(float), c.st));
        if (!s) HIP_TRY(hipStreamSynchronize(stream_));
        c.done = true;
    }
    return SPECKV_OK;
}

int Engine::attend_end(const SeqCall& c, hipStream_t s)
{
    note_use(c.a, s);
    if (!s) RC_TRY(wait_stream());
    return SPECKV_OK;
}

// the page that stands in for never-written pages (table forms)
int Engine::ensure_zero_page(hipStream_t s)
{
    if (d_zero_page_) return SPECKV_OK;
    if (is_capturing(s)) return SPECKV_ERR_INVAL;        // first call must run outside a capture (see scratch())
    DeviceScope zero_scope(device_);
    HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_zero_page_), kPageSize));
    HIP_TRY(hipMemset(d_zero_page_, 0, kPageSize));
    return SPECKV_OK;
}

// the launch's scratch: head_bytes of the caller's (the FP8 kernels' quantised query), then the partials -- accumulators and (m, l) pairs
uint8_t* Engine::attend_scratch(AttendArgs& k, uint64_t parts, size_t head_bytes, hipStream_t s)
{
    const size_t acc_bytes = static_cast<size_t>(parts) * 16 * 128 * sizeof(float), ml_bytes = static_cast<size_t>(parts) * 32 * sizeof(float);
    uint8_t* buf = static_cast<uint8_t*>(scratch(s_attn_, head_bytes + acc_bytes + ml_bytes, s));
    if (!buf) return nullptr;
    k.part_acc = reinterpret_cast<float*>(buf + head_bytes);
    k.part_ml = reinterpret_cast<float*>(buf + head_bytes + acc_bytes);
    return buf;
}

// A launch under a window runs the bodies that mask the leading positions of a member's first tile (AttendArgs::seq_skip): the linear, striped and
// table forms.  The forms by residue class (k_attend_mx4<1>, k_attend_int4_wg8<.., true>, k_attend_fp8_linear<.., CLS>) count their tiles class by class and
// have no such mask: their launches go through the page tables, which take any range (FP8: the register-staged table kernel -- k_attend_fp8_dma<1> has
// no leading mask either; launch_attend_fp8_batch).  Everything else of the decision is batch_form's.
static BatchForm window_form(BatchForm f)
{
    if (f.by_class) { f.table = true; f.striped = f.fp8_cls = f.int4_cls = f.by_class = false; f.wg8 = 0u; }
    return f;
}
// the tiles a member of a plan has at most: the context's bound, under a window the smaller of that and the window's
static uint32_t plan_bound(uint32_t max_pos_end, uint32_t stripe_n_max, uint32_t window)
{
    const uint32_t ctx = plan_tiles_bound(max_pos_end, stripe_n_max);
    return window ? std::min(ctx, decode_window_tiles_bound(window)) : ctx;
}

// ---- one sequence ------------------------------------------------------------------------------------------------------------
// Every entry: attend_begin, the launch decision on the call's shape (attend_geometry.hpp seq_decide: the rules and the measurements behind them),
// the zero page and the scratch it asks for, the arguments from call and decision, the launch, attend_end.
int Engine::qk_scores_fp8(uint64_t handle, uint32_t layer, uint32_t n_layers, const void* d_q_f16, uint32_t g,
                          uint32_t pos_begin, uint32_t pos_end, float* d_out, hipStream_t s)
{
    if (null_) return no_data_path("speckv_ext_qk_scores_fp8");
    SeqCall c;
    const int rc = attend_begin(SPECKV_COMP_FP8_E4M3, true, handle, layer, n_layers, d_q_f16, g, pos_begin, pos_end, d_out, s, c);
    if (rc != SPECKV_OK || c.done) return rc;
    Allocation* a = c.a;
    const Layout& L = a->layout;
    const SeqDecision d = seq_decide(c.shape(cus()), seq_tuning());
    // shim layout [req 0][layer][kind 0 = K][pos][head]: page of (layer, pos) = c.k_first + layer * c.layer_stride
    if (!d.quantize_q) {
        AttendArgs k{};
        k.k_first = c.k_first;
        k.layer_stride = c.layer_stride;
        k.n_pages = c.n_pages;
        k.heads = L.num_heads;
        k.g = g;
        k.tiles_per_split = 16;
        k.lin_base = a->linear_base;
        k.scale_tab = a->d_scale_tab;
        k.q16 = static_cast<const uint16_t*>(d_q_f16);
        HIP_TRY(launch_qk_scores_fp8_linear(k, n_layers, d_out, c.st));
        return attend_end(c, s);
    }
    const size_t rows = static_cast<size_t>(n_layers) * L.num_heads * 16;
    uint8_t* q8 = static_cast<uint8_t*>(scratch(s_req_, rows * 128 + rows * sizeof(float), s));
    if (!q8) return SPECKV_ERR_NOMEM;
    float* qs = reinterpret_cast<float*>(q8 + rows * 128);
    HIP_TRY(launch_quantize_q_e4m3(d_q_f16, n_layers * L.num_heads, g, L.head_dim, q8, qs, c.st));
    HIP_TRY(launch_qk_scores_fp8(a->d_entries, c.k_first, c.layer_stride, n_layers, c.n_pages, L.num_heads, g, q8, qs, d_out, c.st));
    return attend_end(c, s);
}

// Fused decode attention over the FP8 K and V regions of [layer, layer+n_layers) (attend.hip).
int Engine::attend_fp8(uint64_t handle, uint32_t layer, uint32_t n_layers, const void* d_q_f16, uint32_t g,
                       uint32_t pos_begin, uint32_t pos_end, float sm_scale, float* d_out, float* d_lse, hipStream_t s)
{
    if (null_) return no_data_path("speckv_ext_attend_fp8");
    SeqCall c;
    const int rc = attend_begin(SPECKV_COMP_FP8_E4M3, false, handle, layer, n_layers, d_q_f16, g, pos_begin, pos_end, d_out, s, c);
    if (rc != SPECKV_OK || c.done) return rc;
    const Allocation* a = c.a;
    const SeqDecision d = seq_decide(c.shape(cus()), seq_tuning());
    if (d.zero_page) RC_TRY(ensure_zero_page(s));
    // in front of the partials: the quantised query [rows][16][128] e4m3 and its scales [rows][16]
    const uint32_t rows = n_layers * a->layout.num_heads;
    const size_t q_bytes = static_cast<size_t>(rows) * 16 * 128, qs_bytes = static_cast<size_t>(rows) * 16 * sizeof(float);
    AttendArgs k{};
    uint8_t* buf = attend_scratch(k, d.parts, q_bytes + qs_bytes, s);
    if (!buf) return SPECKV_ERR_NOMEM;
    c.args(k, d, sm_scale, d_zero_page_, d_out, d_lse);
    k.q8 = buf;
    k.qs = reinterpret_cast<float*>(buf + q_bytes);
    k.scale_tab = a->d_scale_tab;
    k.q16 = static_cast<const uint16_t*>(d_q_f16);
    if (d.cls) { k.fp8_cls = 1u; k.scale_run = a->scale_run; }
    if (d.quantize_q) HIP_TRY(launch_quantize_q_e4m3(d_q_f16, rows, g, a->layout.head_dim, buf, reinterpret_cast<float*>(buf + q_bytes), c.st));
    HIP_TRY(launch_attend_fp8(k, d.kernel, n_layers, d_out, d_lse, c.st));
    return attend_end(c, s);
}

// Fused decode attention over INT4_G32 K and V records (attend_int4.hip): any placement.
int Engine::attend_int4(uint64_t handle, uint32_t layer, uint32_t n_layers, const void* d_q_f16, uint32_t g,
                        uint32_t pos_begin, uint32_t pos_end, float sm_scale, float* d_out, float* d_lse, hipStream_t s)
{
    if (null_) return no_data_path("speckv_ext_attend_int4");
    SeqCall c;
    const int rc = attend_begin(SPECKV_COMP_INT4_G32, false, handle, layer, n_layers, d_q_f16, g, pos_begin, pos_end, d_out, s, c);
    if (rc != SPECKV_OK || c.done) return rc;
    const SeqDecision d = seq_decide(c.shape(cus()), seq_tuning());
    if (d.zero_page) RC_TRY(ensure_zero_page(s));
    AttendArgs k{};
    if (!attend_scratch(k, d.parts, 0, s)) return SPECKV_ERR_NOMEM;
    c.args(k, d, sm_scale, d_zero_page_, d_out, d_lse);
    k.q8 = static_cast<const uint8_t*>(d_q_f16);
    HIP_TRY(launch_attend_int4(k, n_layers, c.st));
    if (!d.rows_final) HIP_TRY(launch_attend_combine(k, n_layers, d_out, d_lse, c.st));
    return attend_end(c, s);
}

// Fused decode attention over MXFP4 K and V records (attend_mx4.hip): any placement.
int Engine::attend_mx4(uint64_t handle, uint32_t layer, uint32_t n_layers, const void* d_q_f16, uint32_t g,
                       uint32_t pos_begin, uint32_t pos_end, float sm_scale, float* d_out, float* d_lse, hipStream_t s)
{
    if (null_) return no_data_path("speckv_ext_attend_mx4");
    SeqCall c;
    const int rc = attend_begin(SPECKV_COMP_MXFP4, false, handle, layer, n_layers, d_q_f16, g, pos_begin, pos_end, d_out, s, c);
    if (rc != SPECKV_OK || c.done) return rc;
    const SeqDecision d = seq_decide(c.shape(cus()), seq_tuning());
    if (d.zero_page) RC_TRY(ensure_zero_page(s));
    AttendArgs k{};
    if (!attend_scratch(k, d.parts, 0, s)) return SPECKV_ERR_NOMEM;
    c.args(k, d, sm_scale, d_zero_page_, d_out, d_lse);
    k.q16 = static_cast<const uint16_t*>(d_q_f16);
    HIP_TRY(launch_attend_mx4(k, n_layers, d_out, d_lse, c.st));
    return attend_end(c, s);
}

// ---- batches ------------------------------------------------------------------------------------------------------------------
// The members of a batch or a plan: descriptors (n_splits = the member's tiles until assign_pieces), page tables, tiles and pages per member,
// the shape the launch decision is taken on (attend_geometry.hpp).
struct Engine::BatchMembers {
    std::vector<AttendSeq> seqs;
    std::vector<const PageEntry*> ents;
    std::vector<uint32_t> tiles, pages;
    BatchShape shape{};
    int scheme = -1;
    uint32_t min_layers = UINT32_MAX, stripe_n_max = 0;      // (stripe_n_max: the largest run count, where the tiles are counted by residue class)
    uint64_t total_tiles = 0;
    std::vector<uint32_t> skips;      // the window entries: leading positions of member i's first tile in front of its window (AttendArgs::seq_skip)
    bool cut = false;                 // ... and whether the window cuts any member's pool positions at all
    // what the form asks of the descriptors: the page tables in table launches, the tiles counted by residue class
    void apply(const BatchForm& f)
    {
        const uint32_t n_seq = static_cast<uint32_t>(seqs.size());
        if (f.table)                                             // (AttendSeq::lin_base carries the page table in table launches)
            for (uint32_t i = 0; i < n_seq; ++i) seqs[i].lin_base = reinterpret_cast<const uint8_t*>(ents[i]);
        if (f.by_class)     // the striped forms of k_attend_mx4 / k_attend_int4_wg8 / k_attend_fp8_linear count their tiles by residue class
            for (uint32_t i = 0; i < n_seq; ++i) {
                seqs[i].n_splits = tiles[i] = mx4_striped_tiles(seqs[i].n_pages, seqs[i].stripe_n);
                stripe_n_max = std::max(stripe_n_max, seqs[i].stripe_n);
            }
    }
};

// Looks the members up and fills their descriptors for `layer` (a plan: layer 0, the launch adds layer * layer_pages; the format from the first member).
int Engine::gather_members(bool batch_entry, int scheme, uint32_t n_seq, const uint64_t* handles, const uint32_t* pos_end, uint32_t layer, uint32_t max_pos_end,
                           hipStream_t s, BatchMembers& m, const uint32_t* q_pos, uint32_t window)
{
    m.seqs.resize(n_seq); m.ents.resize(n_seq); m.tiles.resize(n_seq); m.pages.resize(n_seq);
    m.skips.assign(q_pos ? n_seq : 0u, 0u);
    bool any_striped = false;                 // then the whole launch takes the striped kernels (a single run is "striped over 1")
    bool any_table = false;                   // ... or, with a member that has no regular placement, the table forms
    uint32_t heads = 0;
    for (uint32_t i = 0; i < n_seq; ++i) {
        Allocation* a = find(handles[i]);
        if (!a) return SPECKV_ERR_GENERAL;
        if (scheme < 0) scheme = a->scheme;
        if (!a->has_layout || a->scheme != scheme || (scheme != SPECKV_COMP_FP8_E4M3 && scheme != SPECKV_COMP_INT4_G32 && scheme != SPECKV_COMP_MXFP4)) return SPECKV_ERR_INVAL;
        const Layout& L = a->layout;
        if (L.head_dim != 128 || L.bytes_per_element != 2 || L.num_heads * L.head_dim != 1024 || L.num_tokens % 2) return SPECKV_ERR_INVAL;
        if (layer >= L.num_layers || pos_end[i] % 2 || pos_end[i] > L.num_tokens || pos_end[i] > max_pos_end) return SPECKV_ERR_INVAL;
        // under a window the member is walked from the tile of its lower bound (decode_window.hpp): the descriptor's region starts `begin` positions in,
        // the tiles are those that are left -- they end where the member's tiles end without a window, so the same condition keeps them inside the region
        DecodeWindowRange w{0u, 0u, pos_end[i] / 2};
        if (q_pos) {
            if (q_pos[i] > pos_end[i] || q_pos[i] + 1u < pos_end[i]) return SPECKV_ERR_INVAL;       // the query: the last stored position or the tail behind it
            w = decode_window_range(q_pos[i] + 1u, window);
            m.skips[i] = w.skip;
            m.cut = m.cut || w.n_pages != pos_end[i] / 2 || w.skip != 0u;
        }
        const uint32_t n_pages = w.n_pages, n_tiles = (n_pages + 15u) / 16u;
        const bool fp8 = scheme == SPECKV_COMP_FP8_E4M3;
        if ((fp8 && !a->d_scale_tab) || static_cast<uint64_t>(w.begin) + static_cast<uint64_t>(n_tiles) * 32u > L.num_tokens) {
            if (batch_entry)
                SPECKV_ERR("speckv_ext_attend_*_batch: sequence %u does not qualify for the tile-aligned forms (pos_end rounded up "
                           "to 32 inside the layer%s)", i, fp8 ? ", layout with num_tokens %% 32 == 0" : "");
            return SPECKV_ERR_INVAL;
        }
        m.min_layers = std::min(m.min_layers, L.num_layers);
        heads = L.num_heads;
        note_use(a, s);
        any_table = any_table || !a->stripe_n;                 // no regular placement (migrated pages): the launch reads addresses from the page tables
        m.ents[i] = a->d_entries;
        any_striped = any_striped || !a->linear_base;
        AttendSeq& q = m.seqs[i];
        q.stripe_bases = a->d_stripe;
        q.stripe_n = a->stripe_n;
        q.lin_base = a->linear_base;
        q.scale_tab = a->d_scale_tab;
        q.k_first = static_cast<uint64_t>(layer) * L.num_tokens + w.begin / 2u;       // (layer*2*T)/2, from the window's first tile on
        q.v_first = q.k_first + L.num_tokens / 2;
        q.n_pages = m.pages[i] = n_pages;
        q.layer_pages = L.num_tokens;                                   // K + V pages of one layer
        q.n_splits = m.tiles[i] = n_tiles;                              // tiles for now, splits below
        m.total_tiles += n_tiles;
    }
    m.scheme = scheme;
    m.shape = BatchShape{scheme == SPECKV_COMP_FP8_E4M3, scheme == SPECKV_COMP_MXFP4, n_seq, heads, cus(), any_striped, any_table};
    return SPECKV_OK;
}

// A slot of the pinned descriptor ring of at least `bytes` (the ring grows to fit), free for writing: whatever last used it (a launch that read
// it in place, a plan's copy) has finished.  The caller records seq_ring_.ev[slot] behind what reads the slot.
int Engine::take_seq_slot(size_t bytes, int* slot, void** staged)
{
    if (seq_ring_.slot_bytes < bytes) {
        if (seq_ring_.base) { HIP_TRY(hipDeviceSynchronize()); (void)hipHostFree(seq_ring_.base); seq_ring_.base = nullptr; }
        seq_ring_.slot_bytes = std::max<size_t>(bytes * 2, 16384);
        HIP_TRY(hipHostMalloc(&seq_ring_.base, seq_ring_.slot_bytes * kSeqRingSlots, hipHostMallocDefault));
        for (auto& ev : seq_ring_.ev)
            if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    *slot = seq_ring_.next;
    seq_ring_.next = (*slot + 1) % kSeqRingSlots;
    HIP_TRY(hipEventSynchronize(seq_ring_.ev[*slot]));
    *staged = static_cast<uint8_t*>(seq_ring_.base) + static_cast<size_t>(*slot) * seq_ring_.slot_bytes;
    return SPECKV_OK;
}

// One decode step of a batch: the fused attention of ONE layer for many sequences (allocations) in one launch
// (BASELINE configs[3] shape: 256 sequences).  Every allocation must qualify for the linear form.
// Not capturable into a HIP graph: the per-call descriptors travel through a pinned slot that later calls reuse, so a
// replay would read other calls' descriptors -- the call refuses to run on a capturing stream (the per-sequence
// entry points speckv_ext_attend_fp8 / _int4 are capturable).
int Engine::attend_batch(int scheme, uint32_t n_seq, const uint64_t* handles, uint32_t layer, const void* d_q_f16, uint32_t g,
                         const uint32_t* pos_end, float sm_scale, float* d_out, float* d_lse, hipStream_t s, const uint32_t* q_pos, uint32_t window)
{
    const bool fp8 = scheme == SPECKV_COMP_FP8_E4M3, mx4 = scheme == SPECKV_COMP_MXFP4;
    if (null_) return no_data_path("speckv_ext_attend_*_batch");
    if (window && !q_pos) return SPECKV_ERR_INVAL;
    if (!window) q_pos = nullptr;                              // (no window: the launches of the entries without one)
    if (n_seq == 0) return SPECKV_OK;
    if (is_capturing(s)) {
        SPECKV_ERR("speckv_ext_attend_*_batch cannot be captured into a HIP graph (its descriptors are staged per call); "
                   "capture the per-sequence speckv_ext_attend_fp8 / _int4 calls instead");
        return SPECKV_ERR_INVAL;
    }
    if (!handles || !pos_end || !d_q_f16 || !d_out || g == 0 || g > 16) return SPECKV_ERR_INVAL;
    BatchMembers m;
    RC_TRY(gather_members(true, scheme, n_seq, handles, pos_end, layer, UINT32_MAX, s, m, q_pos, window));
    const uint32_t heads = m.shape.heads;
    DeviceScope device_scope(device_);
    // NULL = the engine's stream and a synchronous call: the query may have been produced on any stream of the caller
    if (!s) HIP_TRY(hipDeviceSynchronize());
    hipStream_t st = s ? s : stream_;
    const size_t out_elems = static_cast<size_t>(n_seq) * heads * g * 128;
    if (m.total_tiles == 0) {
        HIP_TRY(hipMemsetAsync(d_out, 0, out_elems * sizeof(float), st));
        if (!s) HIP_TRY(hipStreamSynchronize(stream_));
        return SPECKV_OK;
    }
    // the launch decision (attend_geometry.hpp): the form, the dispatch order, one split length for the whole batch, the pieces of every member
    // (a window that cuts no member's pool positions: the descriptors, the form and the launches of the entry without a window, no skip array)
    const BatchTuning tun = batch_tuning();
    const BatchForm form = m.cut ? window_form(batch_form(m.shape, tun)) : batch_form(m.shape, tun);
    m.apply(form);
    std::vector<uint32_t> order(n_seq);
    const bool ordered = batch_dispatch_order(form, tun, m.pages.data(), n_seq, order.data());
    const BatchGeometry geo = batch_geometry(kEntryBatch, m.shape, form, tun, m.tiles.data(), 0, ordered, nullptr);
    if (!geo.fits) return SPECKV_ERR_INVAL;
    const uint64_t parts = assign_pieces(geo, heads, m.seqs.data(), n_seq);
    AttendArgs k{};
    if (!attend_scratch(k, parts, 0, s)) return SPECKV_ERR_NOMEM;
    // The kernels read the descriptors IN PLACE from a pinned slot: each workgroup fetches its own 64 bytes over the host link when
    // it starts (one round trip, all workgroups at once).  Copying the slot to the device first was a copy-engine operation in
    // front of every launch, 7-8 us that the kernels waited for: 256 x 1k MXFP4 59.5 -> 53 us per call, FP8 96 -> 88
    // (profiles/r05_mx4.txt; the planned form never had it).  A slot is reused once the launches that read it have finished.
    const size_t desc_bytes = m.seqs.size() * sizeof(AttendSeq), idx_bytes = m.seqs.size() * sizeof(uint32_t);
    const size_t seq_bytes = desc_bytes + idx_bytes + (m.cut ? idx_bytes : 0u);      // descriptors, then the dispatch order, then the skip array of a windowed launch
    int slot = 0;
    void* staged = nullptr;
    RC_TRY(take_seq_slot(seq_bytes, &slot, &staged));
    memcpy(staged, m.seqs.data(), desc_bytes);
    if (ordered) memcpy(static_cast<uint8_t*>(staged) + desc_bytes, order.data(), idx_bytes);
    if (m.cut) memcpy(static_cast<uint8_t*>(staged) + desc_bytes + idx_bytes, m.skips.data(), idx_bytes);
    AttendSeq* d_seqs = nullptr;
    HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&d_seqs), staged, 0));
    // sequences without positions have no splits: their rows are written as zeros by the merge (L == 0)
    k.heads = heads;
    k.g = g;
    k.n_splits = geo.max_splits;
    k.tiles_per_split = geo.tps;
    k.layer_stride = 0;
    k.q16 = static_cast<const uint16_t*>(d_q_f16);
    k.q8 = static_cast<const uint8_t*>(d_q_f16);          // the INT4 kernel reads the fp16 query through q8
    k.scale_log2e = sm_scale * 1.4426950408889634f;
    if (form.table) {
        k.table_form = 1u;
        RC_TRY(ensure_zero_page(s));
        k.zero_page = d_zero_page_;
    }
    else if (form.striped) k.stripe_bases = m.seqs[0].stripe_bases;          // marks a striped launch (each sequence brings its own table)
    else k.lin_base = m.seqs[0].lin_base;                                    // (overridden per sequence)
    if (form.fp8_cls) k.fp8_cls = 1u;
    k.seqs = d_seqs;
    if (ordered) k.order = reinterpret_cast<const uint32_t*>(d_seqs + n_seq);
    if (m.cut) k.seq_skip = reinterpret_cast<const uint32_t*>(d_seqs + n_seq) + n_seq;
    if (geo.rows_first) k.rows_first = 1u;
    bool one_split_each = true;                           // then the attention kernel writes the final rows itself
    for (uint32_t i = 0; i < n_seq; ++i) one_split_each = one_split_each && m.seqs[i].n_splits == 1u;
    if (one_split_each) { k.direct_out = d_out; k.direct_lse = d_lse; }
    // MXFP4, whole sequences in single runs and a CU to each: 8-wave workgroups, the run cut in two (k_attend_mx4<0, 2>)
    if (mx4 && one_split_each && !form.striped && !form.table && static_cast<uint64_t>(n_seq) * ((g + 7u) / 8u) <= cus() && tuning().attend_mx4_one_half == 0) k.mx4_halves = 1u;
    k.wg8 = form.wg8;
    // The kernels read the slot's descriptors in place: the guard event is recorded on every way out from here on (SlotGuard).
    SlotGuard slot_guard{seq_ring_.ev[slot], st};
    if (fp8) {
        HIP_TRY(launch_attend_fp8_batch(k, n_seq, d_out, d_lse, st));
    } else if (mx4) {
        HIP_TRY(launch_attend_mx4(k, n_seq, d_out, d_lse, st));
    } else {
        HIP_TRY(launch_attend_int4(k, n_seq, st));        // grid y = sequences x head groups, as for layers
        if (!k.direct_out) HIP_TRY(launch_attend_combine(k, n_seq, d_out, d_lse, st));
    }
    if (!s) HIP_TRY(hipStreamSynchronize(stream_));
    return SPECKV_OK;
}

// ---- planned batches: descriptors resident on the device, the launches capturable ---------------------------------------
// A decode step under a HIP graph replays the same launches with new sequence lengths.  speckv_ext_attend_batch_plan
// (outside the graph, once per step) writes one descriptor per sequence -- valid for every layer -- into a device buffer
// of the caller; speckv_ext_attend_*_planned is kernel launches only: no handle look-ups, no staging, grid and scratch
// sized from max_pos_end alone, so a captured launch stays valid for as long as the lengths stay within that bound.
int Engine::attend_batch_plan(uint32_t n_seq, const uint64_t* handles, const uint32_t* pos_end, uint32_t max_pos_end,
                              void* d_plan, size_t plan_bytes, hipStream_t s, const uint32_t* q_pos, uint32_t window)
{
    if (null_) return no_data_path("speckv_ext_attend_batch_plan");
    if (n_seq == 0) return SPECKV_OK;
    if (!handles || !pos_end || !d_plan || !s || max_pos_end % 2 || plan_bytes < n_seq * sizeof(AttendSeq)) return SPECKV_ERR_INVAL;
    // a plan under a window holds descriptors, dispatch order and skip array (speckv_ext_attend_plan_window_bytes), whatever the lengths of this step
    if (window && (!q_pos || plan_bytes < n_seq * (sizeof(AttendSeq) + 2u * sizeof(uint32_t)))) return SPECKV_ERR_INVAL;
    if (!window) q_pos = nullptr;
    if (is_capturing(s)) return SPECKV_ERR_INVAL;            // the plan is what changes between replays: it stays outside the graph
    BatchMembers m;
    RC_TRY(gather_members(false, -1, n_seq, handles, pos_end, 0, max_pos_end, s, m, q_pos, window));
    const int scheme = m.scheme;
    const BatchTuning tun = batch_tuning();
    // (the launch decision: attend_geometry.hpp.  Under a window the form, the bound and the skip array follow from the window alone, not from what
    //  it cuts in this step: a graph captured over the plan's launches stays valid while the lengths move)
    const BatchForm form = window ? window_form(batch_form(m.shape, tun)) : batch_form(m.shape, tun);
    m.apply(form);
    const uint32_t bound_tiles = plan_bound(max_pos_end, m.stripe_n_max, window);
    const BatchGeometry rule = batch_geometry(kEntryPlan, m.shape, form, tun, nullptr, bound_tiles, false, nullptr);      // the rule for equal lengths under the bound
    if (!rule.fits) return SPECKV_ERR_INVAL;
    // the dispatch order behind the descriptors, where the caller's buffer has the room (speckv_ext_attend_plan_bytes says so since round 6)
    std::vector<uint32_t> order(n_seq);
    // (always written when there is room -- the order as given for sequences of one length: a graph captured over this plan keeps reading it as the lengths change)
    const bool ordered = plan_bytes >= n_seq * (sizeof(AttendSeq) + sizeof(uint32_t));
    const bool by_length = ordered && batch_dispatch_order(form, tun, m.pages.data(), n_seq, order.data());
    if (ordered && !by_length)
        for (uint32_t i = 0; i < n_seq; ++i) order[i] = i;
    // The room of this shape in this buffer: what its first plan fixed, kept by every later one (batch_geometry says why)
    // (... the rule for equal lengths is part of the shape: the tuning keys move it)
    const std::array<uint64_t, 5> room_key{reinterpret_cast<uintptr_t>(d_plan), n_seq | (static_cast<uint64_t>(scheme) << 32), max_pos_end | (static_cast<uint64_t>(rule.rule_tps) << 32), rule.rule_splits, window};
    const auto old = plan_rooms_.find(room_key);
    const bool plan_sticky = old != plan_rooms_.end();
    const BatchGeometry geo = batch_geometry(kEntryPlan, m.shape, form, tun, m.tiles.data(), bound_tiles, by_length, plan_sticky ? &old->second : nullptr);
    if (plans_.size() >= 64 && !plans_.count(d_plan)) plans_.clear();        // (buffers of long-gone steps)
    if (form.table) RC_TRY(ensure_zero_page(s));
    // (under a window: a member without pool positions.  W = 1 is the one window under which a member that has a split in this step has none in the
    //  next -- an odd length -- so its plans always send the tails through the fold launch: a captured launch must not fold into a split that is gone)
    bool any_empty = window == 1u;
    for (uint32_t i = 0; i < n_seq; ++i) any_empty = any_empty || m.pages[i] == 0u;
    if (!plan_sticky) {
        // (a graph captured over a buffer replays the room of its shape without calling in: a room is dropped only once its buffer has left plans_ --
        //  rooms of live buffers are kept however many shapes pass through them)
        if (plan_rooms_.size() >= 4096)
            for (auto it = plan_rooms_.begin(); it != plan_rooms_.end();) {
                const void* buf = reinterpret_cast<const void*>(static_cast<uintptr_t>((*it).first[0]));
                it = buf != d_plan && !plans_.count(buf) ? plan_rooms_.erase(it) : std::next(it);
            }
        plan_rooms_[room_key] = BatchRoom{geo.max_splits, geo.rows_first};
    }
    plans_[d_plan] = PlanInfo{scheme, m.min_layers, max_pos_end, m.shape, form, m.stripe_n_max, any_empty, ordered, BatchRoom{geo.max_splits, geo.rows_first}, window};
    assign_pieces(geo, m.shape.heads, m.seqs.data(), n_seq);
    DeviceScope device_scope(device_);
    const size_t desc_bytes = m.seqs.size() * sizeof(AttendSeq), idx_bytes = m.seqs.size() * sizeof(uint32_t);
    const size_t seq_bytes = desc_bytes + (ordered ? idx_bytes : 0u) + (window ? idx_bytes : 0u);      // (a windowed plan is always ordered: its buffer has the room)
    int slot = 0;
    void* staged = nullptr;
    RC_TRY(take_seq_slot(seq_bytes, &slot, &staged));
    memcpy(staged, m.seqs.data(), desc_bytes);
    if (ordered) memcpy(static_cast<uint8_t*>(staged) + desc_bytes, order.data(), idx_bytes);
    if (window) memcpy(static_cast<uint8_t*>(staged) + desc_bytes + idx_bytes, m.skips.data(), idx_bytes);
    HIP_TRY(hipMemcpyAsync(d_plan, staged, seq_bytes, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(seq_ring_.ev[slot], s));
    return SPECKV_OK;
}

// Several layers of a planned batch in one call (speckv_ext_attend_planned_layers): d_q_f16 [n_layers][n_seq][heads][g][128], d_out /
// d_lse likewise.  MXFP4 with a geometry of one split per sequence: ONE launch over layers x sequences (the workgroups of the next
// layer start while the last of this one drain: a batch of 256 x 2k is eight launches of 92 us, each a third fill and drain --
// or one of 0.68 ms); anything else: the per-layer launches, from one call.
int Engine::attend_planned_layers(int scheme, const void* d_plan, uint32_t n_seq, uint32_t layer_begin, uint32_t n_layers, const void* d_q_f16, uint32_t g,
                                  uint32_t max_pos_end, float sm_scale, float* d_out, float* d_lse, hipStream_t s, const TailArgs* tail)
{
    if (n_layers == 0 || n_seq == 0) return SPECKV_OK;
    if (n_layers == 1) return attend_planned(scheme, d_plan, n_seq, layer_begin, d_q_f16, g, max_pos_end, sm_scale, d_out, d_lse, s, tail);
    if (g == 0 || g > 16) return SPECKV_ERR_INVAL;
    const auto plan = plans_.find(d_plan);
    const bool one_launch = scheme == SPECKV_COMP_MXFP4 && plan != plans_.end() && layer_begin + n_layers <= plan->second.n_layers &&
                            static_cast<uint64_t>(n_seq) * n_layers <= 65535u && tuning().attend_layers_loop == 0 &&
                            plan->second.room.max_splits == 1u;
    if (one_launch) return attend_planned(scheme, d_plan, n_seq, layer_begin, d_q_f16, g, max_pos_end, sm_scale, d_out, d_lse, s, tail, n_layers);
    // layer by layer; the position the caller still holds outside the pool is folded into ALL layers by one launch at the end (the
    // attention launches of the step then stand back to back: 8 layers of FP8, 256 x 2k, 7 fold launches and their gaps less)
    const size_t rows = static_cast<size_t>(n_seq) * 8u * g;
    const bool have_tail = tail && tail->n_tail != 0u;
    const bool fold_once = have_tail && scheme != SPECKV_COMP_MXFP4 && d_lse && tail->d_k_tail && tail->d_v_tail && tuning().attend_fold_launch == 0;     // (MXFP4 folds inside its kernel)
    if (have_tail && fold_once && (tail->stride_elems % 8u || tail->stride_elems < static_cast<uint64_t>(layer_begin + n_layers) * 8u * 128u)) return SPECKV_ERR_INVAL;
    for (uint32_t l = 0; l < n_layers; ++l)
        RC_TRY(attend_planned(scheme, d_plan, n_seq, layer_begin + l, static_cast<const uint16_t*>(d_q_f16) + l * rows * 128u, g, max_pos_end, sm_scale,
                              d_out + l * rows * 128u, d_lse ? d_lse + l * rows : nullptr, s, fold_once ? nullptr : tail));
    if (fold_once) {
        DeviceScope device_scope(device_);
        const uint64_t off = static_cast<uint64_t>(layer_begin) * 8u * 128u;
        HIP_TRY(launch_attend_fold_tail(tail->n_tail, tail->n_tail == n_seq ? nullptr : tail->d_tail_rows, 8u, g, d_q_f16,
                                        static_cast<const uint16_t*>(tail->d_k_tail) + off, static_cast<const uint16_t*>(tail->d_v_tail) + off, tail->stride_elems,
                                        sm_scale, d_out, d_lse, s, n_layers, n_seq));
    }
    return SPECKV_OK;
}

int Engine::attend_planned(int scheme, const void* d_plan, uint32_t n_seq, uint32_t layer, const void* d_q_f16, uint32_t g,
                           uint32_t max_pos_end, float sm_scale, float* d_out, float* d_lse, hipStream_t s, const TailArgs* tail, uint32_t n_layers)
{
    const bool fp8 = scheme == SPECKV_COMP_FP8_E4M3, mx4 = scheme == SPECKV_COMP_MXFP4;
    if (null_) return no_data_path("speckv_ext_attend_*_planned");
    if (n_seq == 0) return SPECKV_OK;
    if (!d_plan || !d_q_f16 || !d_out || !s || g == 0 || g > 16 || max_pos_end % 2 || max_pos_end == 0) return SPECKV_ERR_INVAL;
    const uint32_t heads = 8;                                  // the page-wise layout: 8 kv heads x 128
    const auto plan = plans_.find(d_plan);                     // what speckv_ext_attend_batch_plan last wrote there
    if (plan == plans_.end() || plan->second.shape.n_seq != n_seq || plan->second.scheme != scheme || plan->second.max_pos_end != max_pos_end ||
        layer >= plan->second.n_layers || n_layers == 0 || n_layers > plan->second.n_layers - layer) {
        SPECKV_ERR("speckv_ext_attend_*_planned: no plan of this shape at %p (n_seq, format and max_pos_end as planned, layer inside every layout)", d_plan);
        return SPECKV_ERR_INVAL;
    }
    const PlanInfo& p = plan->second;
    // (tps by the rule for equal lengths under the bound; max_splits and rows_first as the first plan of this shape in this buffer fixed them: attend_batch_plan)
    const BatchGeometry pg = batch_geometry(kEntryPlan, p.shape, p.form, batch_tuning(), nullptr, plan_bound(max_pos_end, p.stripe_n_max, p.window), false, &p.room);
    DeviceScope device_scope(device_);
    AttendArgs k{};
    if (!attend_scratch(k, static_cast<uint64_t>(n_seq) * heads * pg.max_splits, 0, s))      // (growth during a capture is refused: warm up once)
        return is_capturing(s) ? SPECKV_ERR_INVAL : SPECKV_ERR_NOMEM;
    k.heads = heads;
    k.g = g;
    k.n_splits = pg.max_splits;
    k.tiles_per_split = pg.tps;
    k.layer_stride = 0;
    k.q16 = static_cast<const uint16_t*>(d_q_f16);
    k.q8 = static_cast<const uint8_t*>(d_q_f16);
    k.scale_log2e = sm_scale * 1.4426950408889634f;
    if (p.form.table) { k.table_form = 1u; k.zero_page = d_zero_page_; }           // a member without a regular placement: addresses from the page tables
    else if (p.form.striped) k.stripe_bases = reinterpret_cast<const uint64_t*>(1);      // striped launch: every descriptor brings its table
    else k.lin_base = reinterpret_cast<const uint8_t*>(1);     // non-null: linear form (the real base comes from the descriptor)
    k.wg8 = p.form.wg8;                                        // (INT4 in single runs, or planned by residue classes: the whole-record kernel)
    if (p.form.fp8_cls) k.fp8_cls = 1u;                        // (... the register-staged kernel by residue classes)
    k.seqs = static_cast<const AttendSeq*>(d_plan);
    if (plan->second.ordered) k.order = reinterpret_cast<const uint32_t*>(static_cast<const AttendSeq*>(d_plan) + n_seq);
    if (p.window) k.seq_skip = reinterpret_cast<const uint32_t*>(static_cast<const AttendSeq*>(d_plan) + n_seq) + n_seq;       // (behind the order: attend_batch_plan)
    k.batch_layer = layer;
    k.direct_out = d_out;                                      // sequences with a single split are written directly ...
    k.direct_lse = d_lse;
    // ... decided per sequence on the device, the merge skips those; a geometry of one split at most needs no merge at all
    k.direct_per_seq = pg.max_splits == 1u ? 2u : 1u;
    if (mx4 && pg.max_splits == 1u && !p.form.striped && !p.form.table && static_cast<uint64_t>(n_seq) * ((g + 7u) / 8u) <= cus() &&
        tuning().attend_mx4_one_half == 0)
        k.mx4_halves = 1u;                                     // (see attend_batch)
    if (pg.rows_first) k.rows_first = 1u;
    // The position the caller still holds outside the pool (TailArgs: a connector's odd last position).  MXFP4: folded in by the
    // attention kernel's own epilogue (split 0 of every sequence) -- needs a lse to be of use to nobody else, a batch without an
    // empty member (an empty sequence has no split to fold into) and the tail index by sequence; otherwise, and for the other
    // formats, one k_attend_fold_tail launch behind the attention, as the connector used to issue itself.
    const bool have_tail = tail && tail->n_tail != 0u;
    if (have_tail && (!tail->d_k_tail || !tail->d_v_tail || !d_lse || tail->stride_elems % 8u || tail->stride_elems < static_cast<uint64_t>(layer + n_layers) * heads * 128u))
        return SPECKV_ERR_INVAL;
    const bool fold_in_kernel = have_tail && mx4 && !p.any_empty && !p.form.table && (tail->d_tail_idx || tail->n_tail == n_seq) && tuning().attend_fold_launch == 0;
    if (n_layers > 1u) {                                       // (attend_planned_layers checked the geometry: MXFP4, one split per sequence)
        if (!mx4 || pg.max_splits != 1u) return SPECKV_ERR_INVAL;
        k.batch_n_seq = n_seq;
    }
    if (fold_in_kernel) {
        k.tail_k = static_cast<const uint16_t*>(tail->d_k_tail);
        k.tail_v = static_cast<const uint16_t*>(tail->d_v_tail);
        k.tail_idx = tail->n_tail == n_seq && !tail->d_tail_idx ? nullptr : tail->d_tail_idx;
        k.tail_stride = tail->stride_elems;
    }
    if (fp8) {
        HIP_TRY(launch_attend_fp8_batch(k, n_seq, d_out, d_lse, s));
    } else if (mx4) {
        HIP_TRY(launch_attend_mx4(k, n_seq * n_layers, d_out, d_lse, s));
    } else {
        HIP_TRY(launch_attend_int4(k, n_seq, s));
        if (k.direct_per_seq != 2u) HIP_TRY(launch_attend_combine(k, n_seq, d_out, d_lse, s));
    }
    if (have_tail && !fold_in_kernel) {
        const size_t rows = static_cast<size_t>(n_seq) * heads * g;
        for (uint32_t l = 0; l < n_layers; ++l) {
            const uint64_t off = static_cast<uint64_t>(layer + l) * heads * 128u;
            HIP_TRY(launch_attend_fold_tail(tail->n_tail, tail->n_tail == n_seq ? nullptr : tail->d_tail_rows, heads, g, static_cast<const uint16_t*>(d_q_f16) + l * rows * 128u,
                                            static_cast<const uint16_t*>(tail->d_k_tail) + off, static_cast<const uint16_t*>(tail->d_v_tail) + off, tail->stride_elems,
                                            sm_scale, d_out + l * rows * 128u, d_lse + l * rows, s));
        }
    }
    return SPECKV_OK;
}

// A launch on the caller's stream; NULL: the engine's stream, synchronous (include/speckv_ext.h)
template <class Launch>
int Engine::launch_on(hipStream_t s, Launch launch)
{
    DeviceScope device_scope(device_);
    if (!s) HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(launch(s ? s : stream_));
    if (!s) HIP_TRY(hipStreamSynchronize(stream_));
    return SPECKV_OK;
}

int Engine::attend_fold_tail(uint32_t n_rows, const uint32_t* d_rows, uint32_t heads, uint32_t g, const void* d_q_f16, const void* d_k_tail,
                             const void* d_v_tail, uint64_t tail_stride_elems, float sm_scale, float* d_out, float* d_lse, hipStream_t s)
{
    if (null_) return no_data_path("speckv_ext_attend_fold_tail");
    if (n_rows == 0) return SPECKV_OK;
    if (!d_q_f16 || !d_k_tail || !d_v_tail || !d_out || !d_lse || heads == 0 || g == 0 || g > 16 || tail_stride_elems % 2 ||
        tail_stride_elems < static_cast<uint64_t>(heads) * 128u)
        return SPECKV_ERR_INVAL;
    return launch_on(s, [&](hipStream_t st) { return launch_attend_fold_tail(n_rows, d_rows, heads, g, d_q_f16, d_k_tail, d_v_tail, tail_stride_elems, sm_scale, d_out, d_lse, st); });
}

// What speckv_ext_attend_fold_held and speckv_ext_attend_fold_masked judge alike.  Both judge their arguments before anything else, so a
// bad set is SPECKV_ERR_INVAL on every device.
bool Engine::fold_held_args_ok(uint32_t heads, uint32_t g, uint32_t rows_per_pos, const void* d_q_f16, const void* d_k_held, const void* d_v_held,
                               uint64_t seq_stride_elems, uint64_t pos_stride_elems, const float* d_out, const float* d_lse)
{
    if (heads == 0 || g == 0 || g > 16 || rows_per_pos == 0 || g % rows_per_pos || g / rows_per_pos > SPECKV_HELD_MAX - 1u) return false;
    const uint64_t n_q = g / rows_per_pos, row = static_cast<uint64_t>(heads) * 128u;
    if (pos_stride_elems % 8u || seq_stride_elems % 8u || pos_stride_elems < row || seq_stride_elems < (n_q - 1u) * pos_stride_elems + row)
        return false;                                           // (positions or sequences that overlap)
    return d_q_f16 && d_k_held && d_v_held && d_out && d_lse;
}

int Engine::attend_fold_held(uint32_t n_rows, const uint32_t* d_rows, uint32_t heads, uint32_t g, uint32_t rows_per_pos, const void* d_q_f16,
                             const void* d_k_held, const void* d_v_held, uint64_t seq_stride_elems, uint64_t pos_stride_elems, const uint32_t* d_base,
                             const uint32_t* d_n_q, float sm_scale, float* d_out, float* d_lse, hipStream_t s)
{
    if (!fold_held_args_ok(heads, g, rows_per_pos, d_q_f16, d_k_held, d_v_held, seq_stride_elems, pos_stride_elems, d_out, d_lse) || !d_base)
        return SPECKV_ERR_INVAL;
    if (null_) return no_data_path("speckv_ext_attend_fold_held");
    if (n_rows == 0) return SPECKV_OK;
    return launch_on(s, [&](hipStream_t st) { return launch_attend_fold_held(n_rows, d_rows, heads, g, rows_per_pos, d_q_f16, d_k_held, d_v_held, seq_stride_elems,
                                                                             pos_stride_elems, d_base, d_n_q, sm_scale, d_out, d_lse, st); });
}

// the mask table in the place of d_base / d_n_q
int Engine::attend_fold_masked(uint32_t n_rows, const uint32_t* d_rows, uint32_t heads, uint32_t g, uint32_t rows_per_pos, const void* d_q_f16,
                               const void* d_k_held, const void* d_v_held, uint64_t seq_stride_elems, uint64_t pos_stride_elems, const uint32_t* d_mask,
                               uint32_t mask_stride, float sm_scale, float* d_out, float* d_lse, hipStream_t s)
{
    if (!fold_held_args_ok(heads, g, rows_per_pos, d_q_f16, d_k_held, d_v_held, seq_stride_elems, pos_stride_elems, d_out, d_lse) || !d_mask ||
        mask_stride < g / rows_per_pos)
        return SPECKV_ERR_INVAL;
    if (null_) return no_data_path("speckv_ext_attend_fold_masked");
    if (n_rows == 0) return SPECKV_OK;
    return launch_on(s, [&](hipStream_t st) { return launch_attend_fold_masked(n_rows, d_rows, heads, g, rows_per_pos, d_q_f16, d_k_held, d_v_held, seq_stride_elems,
                                                                               pos_stride_elems, d_mask, mask_stride, sm_scale, d_out, d_lse, st); });
}

} // namespace speckv
