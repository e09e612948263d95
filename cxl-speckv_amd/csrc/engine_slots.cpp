// cxl-speckv_amd/csrc/engine_slots.cpp -- Engine::read_slots / write_slots, the bodies of speckv_ext_read_slots / _write_slots: spans
// of positions moved between the pool and the slots of a caller's paged cache (one cache tensor per layer, rows addressed by a slot
// mapping on the device) by ONE launch each way (kernels: k_read_slots / k_compress_slots, row_transfer.hip)
#include "engine_internal.hpp"
#include "tuning.hpp"

namespace speckv {

// Span i = positions [first_tokens[i], first_tokens[i] + n_tokens[i]) of allocation handles[i], row t of it in slot
// d_slots[slot_begins[i] + t]; page of (layer, kind, position) = (2 * layer + kind) * page_step + position / 2 for the layers
// [layer_begin, layer_begin + n_layers), whose cache bases are d_caches[0 .. n_layers).  What travels to the device is one
// SlotSpan per span and the n_layers bases, through a slot of the pinned descriptor ring (so the call cannot be captured): nothing
// grows with the token count.
// Reading is read_pairs' bracket: record addresses from the device allocation table (any placement, a sealed allocation stays
// sealed), behind what the caller queued on `s` and behind the asynchronous pool writes on every other caller stream the engine
// knows; nothing is written to the pool.  Writing is write_groups': whole pairs only, sealed destinations are unpacked, cached
// destination pages invalidated, the host mirror and note_async_write_or_wait follow the launch; two spans of one allocation that
// share a page are refused.  Every refusal comes before any launch.
// The _ex entries (c.ex) add the caches' element type and held rows -- one position per span and kind that lives outside pool and
// caches as fp16 (SlotExArgs, kernels.hpp).  A span's pages are then [first / 2, p1): p1 = (first + n) / 2 on the write side (a
// held-in row completes the first pair, a held-out row takes the odd last position), (first + n - 1) / 2 on the read side where
// the last position comes from a held row, (first + n + 1) / 2 otherwise; a held row adds one SlotHeld per span to the staged
// slot and the move waves to the launch.  With fp16 caches and no held rows the call is the plain one, launch for launch.
// The _kmul entries (c.k_mul) add the K factor rows: the same call and the same waves, through the kernel instances that multiply
// every K element between a cache row and the pool side (SlotKmulArgs, kernels.hpp); without a factor the call is the _ex one.
// The _kv entries (c.kv: the split pool) name TWO allocations per span, an FP8_E4M3 one with the K rows (c.handles) and an MXFP4 one
// with the V rows (c.v_handles), each laid out as one region per layer: the page of (layer, position) is layer * page_step +
// position / 2 in either.  Everything above is done for both allocations of a span -- find, the region and last-page checks, the
// shared-page test, unpack, the cached-page test, the host mirror, note_use -- and the ONE launch is k_read_slots_kv /
// k_compress_slots_kv (row_transfer_kv.hip), whose waves pick allocation and codec by their kind.  A single-allocation call takes
// exactly the path it took before.
int Engine::slots_call(const SlotCall& c, bool write, hipStream_t s)
{
    const char* entry = c.kv ? (write ? "speckv_ext_write_slots_kv" : "speckv_ext_read_slots_kv") : c.k_mul ? (write ? "speckv_ext_write_slots_kmul" : "speckv_ext_read_slots_kmul")
                        : write ? (c.ex ? "speckv_ext_write_slots_ex" : "speckv_ext_write_slots") : (c.ex ? "speckv_ext_read_slots_ex" : "speckv_ext_read_slots");
    if (null_) return no_data_path(entry);
    if (!s || !c.handles || !c.first_tokens || !c.n_tokens || !c.slot_begins || !c.d_slots || !c.d_caches) return SPECKV_ERR_INVAL;
    if (c.kind_stride % 16u || c.page_step == 0 || (c.kv && (!c.v_handles || c.k_mul))) return SPECKV_ERR_INVAL;
    if (c.elem > SPECKV_SLOT_ELEM_BF16 || c.reserved != 0 || c.held_stride % 16u || (!write && c.held_out)) return SPECKV_ERR_INVAL;
    if (c.k_mul && (reinterpret_cast<uintptr_t>(c.k_mul) % 16u || c.k_mul_stride % 16u)) return SPECKV_ERR_INVAL;      // (16-byte loads)
    if (c.n_spans == 0 || c.n_layers == 0) return SPECKV_OK;
    for (uint32_t l = 0; l < c.n_layers; ++l)
        if (!c.d_caches[l] || reinterpret_cast<uintptr_t>(c.d_caches[l]) % 16u) return SPECKV_ERR_INVAL;
    uint64_t n_pairs = 0, n_held = 0, n_in = 0;              // n_held: spans with a position that only moves
    std::vector<uint64_t> p1(c.n_spans);                                         // span i's pages: [first / 2, p1[i]) of every region
    for (uint32_t i = 0; i < c.n_spans; ++i) {
        const uint64_t first = c.first_tokens[i], n = c.n_tokens[i];
        bool in = false, out = false;                                           // held rows of this span: K and V, or neither
        for (int dir = 0; dir < 2; ++dir) {
            const void* k = dir ? (c.held_out ? c.held_out[2 * i] : nullptr) : (c.held_in ? c.held_in[2 * i] : nullptr);
            const void* v = dir ? (c.held_out ? c.held_out[2 * i + 1] : nullptr) : (c.held_in ? c.held_in[2 * i + 1] : nullptr);
            if (!k != !v || reinterpret_cast<uintptr_t>(k) % 16u || reinterpret_cast<uintptr_t>(v) % 16u) return SPECKV_ERR_INVAL;
            (dir ? out : in) = k != nullptr;
        }
        if (write && ((first & 1u) != (in ? 1u : 0u) || ((first + n) & 1u) != (out ? 1u : 0u))) return SPECKV_ERR_INVAL;   // whole pairs only
        if ((in || out) && n == 0) return SPECKV_ERR_INVAL;
        if (!write && in && ((first + n - 1) & 1u)) return SPECKV_ERR_INVAL;      // the held position of a span is an even one
        if (first > UINT32_MAX || n > UINT32_MAX || first + n > UINT32_MAX) return SPECKV_ERR_GENERAL;
        p1[i] = n == 0 ? first / 2 : write ? (first + n) / 2 : in ? (first + n - 1) / 2 : (first + n + 1) / 2;
        n_pairs += p1[i] - first / 2;
        n_held += (write ? out : in) ? 1u : 0u;
        n_in += in ? 1u : 0u;
    }
    if (n_pairs == 0 && n_held == 0) return SPECKV_OK;
    const bool held = n_held != 0 || n_in != 0;                                 // (a held-in row of a write rides on its pair's wave)
    const bool ex = held || c.elem != SPECKV_SLOT_ELEM_FP16 || c.k_mul;
    if (is_capturing(s)) {
        SPECKV_ERR("%s cannot be captured into a HIP graph (its descriptors are staged per call)", entry);
        return SPECKV_ERR_INVAL;
    }
    const uint64_t n_each = 2ull * c.n_layers;                                   // waves per pair: its (layer, kind) blocks
    // the regions of ONE allocation that the call names: (layer, kind) ones, or with c.kv one per layer in each of the two
    const uint64_t n_regions = c.kv ? c.n_layers : n_each, first_region = c.kv ? c.layer_begin : 2ull * c.layer_begin;
    if ((n_pairs + (held ? c.n_spans : 0u)) * n_each > (1ull << 31)) return SPECKV_ERR_INVAL;
    std::vector<Allocation*> as(c.n_spans), vs(c.kv ? c.n_spans : 0u);         // vs: the V allocations of a split call
    const int n_allocs = c.kv ? 2 : 1;                                          // allocations per span
    const auto alloc_of = [&](uint32_t i, int k) { return k ? vs[i] : as[i]; };
    const auto check = [&]() -> int {
        for (uint32_t i = 0; i < c.n_spans; ++i) {
            if (c.kv && c.handles[i] == c.v_handles[i]) return SPECKV_ERR_INVAL;
            Allocation* a = find(c.handles[i]);
            Allocation* v = c.kv ? find(c.v_handles[i]) : nullptr;
            if (!a || (c.kv && !v)) return SPECKV_ERR_GENERAL;
            if (c.kv ? (a->scheme != SPECKV_COMP_FP8_E4M3 || v->scheme != SPECKV_COMP_MXFP4) : a->scheme != find(c.handles[0])->scheme)
                return SPECKV_ERR_INVAL;
            const uint64_t end = c.first_tokens[i] + c.n_tokens[i];
            if (end > 2 * c.page_step) return SPECKV_ERR_GENERAL;                // the span leaves its (layer, kind) region
            if (p1[i] > c.first_tokens[i] / 2) {
                const uint64_t last = (first_region + n_regions - 1) * c.page_step + p1[i] - 1;         // the last page named
                for (const Allocation* x : {static_cast<const Allocation*>(a), static_cast<const Allocation*>(v)}) {
                    if (!x) continue;
                    if (c.page_step > x->n_pages || last >= x->n_pages) return SPECKV_ERR_GENERAL;
                    if (write && x->size_bytes % kPageSize && last == x->n_pages - 1) return SPECKV_ERR_INVAL;
                }
            }
            as[i] = a;
            if (c.kv) vs[i] = v;
        }
        return SPECKV_OK;
    };
    RC_TRY(check());
    // the pages of span i: (first_region + j) * page_step + p for j < n_regions, p in [first / 2, p1[i]), in each of its allocations
    const auto each_page = [&](auto&& f) {
        for (uint32_t i = 0; i < c.n_spans; ++i) {
            const uint64_t p0 = c.first_tokens[i] / 2;
            for (int k = 0; k < n_allocs; ++k)
                for (uint64_t j = 0; j < n_regions; ++j)
                    for (uint64_t p = p0; p < p1[i]; ++p) f(alloc_of(i, k), (first_region + j) * c.page_step + p);
        }
    };
    if (write) {
        std::vector<uint32_t> order;                                             // the spans of one allocation must not share a page
        for (uint32_t i = 0; i < c.n_spans; ++i) if (p1[i] > c.first_tokens[i] / 2) order.push_back(i);    // (the pair through a held-in row is one)
        for (int k = 0; k < n_allocs; ++k) {                                     // (a split call: in either allocation)
            const uint64_t* hs = k ? c.v_handles : c.handles;
            std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
                return hs[x] != hs[y] ? hs[x] < hs[y] : c.first_tokens[x] < c.first_tokens[y]; });
            for (size_t m = 1; m < order.size(); ++m) {
                const uint32_t x = order[m - 1], y = order[m];
                if (hs[x] == hs[y] && c.first_tokens[y] / 2 < p1[x]) return SPECKV_ERR_INVAL;
            }
        }
        for (uint32_t i = 0; i < c.n_spans; ++i)
            for (int k = 0; k < n_allocs; ++k)
                if (p1[i] > c.first_tokens[i] / 2 && alloc_of(i, k)->packed) {   // sealed destinations go back into slots first
                    DeviceScope scope(device_);
                    RC_TRY(unpack(alloc_of(i, k)));
                    RC_TRY(check());
                }
    }
    DeviceScope device_scope(device_);
    if (write) {
        bool cached = false;
        each_page([&](Allocation* a, uint64_t p) { cached = cached || (res_flags(a, p) & 3u) != 0; });
        if (cached || !flights_.empty() || ring_busy_ > 0) {
            RC_TRY(quiesce());
            RC_TRY(check());
            each_page([&](Allocation* a, uint64_t p) { drop_page(a, static_cast<uint32_t>(p)); });
            RC_TRY(flush_mirror());
            RC_TRY(wait_stream());
        }
        if (!d_zero_page_) {                                                   // the row a padding slot reads; once, and complete
            RC_TRY(ensure_zero_page(s));                                        // before a kernel on `s` (not ordered behind the
            HIP_TRY(hipDeviceSynchronize());                                    // null stream's memset) can read it
        }
    }
    const size_t span_bytes = static_cast<size_t>(c.n_spans) * (c.kv ? sizeof(SlotSpanKV) : sizeof(SlotSpan));    // (a multiple of 8: the cache bases follow)
    const size_t base_bytes = static_cast<size_t>(c.n_layers) * sizeof(uint64_t);
    const size_t bytes = span_bytes + base_bytes + (held ? static_cast<size_t>(c.n_spans) * sizeof(SlotHeld) : 0);   // (the held rows last)
    int slot = 0;
    void *staged = nullptr, *d_slot = nullptr;
    RC_TRY(descriptor_slot(bytes, &slot, &staged, &d_slot));     // may release the ABI lock: every span is judged again
    RC_TRY(check());
    uint32_t prefix = 0;
    for (uint32_t i = 0; i < c.n_spans; ++i) {
        const Allocation* a = as[i];
        const Allocation* v = c.kv ? vs[i] : nullptr;
        if (write && p1[i] > c.first_tokens[i] / 2 && (a->packed || (v && v->packed))) return SPECKV_ERR_GENERAL;      // sealed again by another caller meanwhile
        const uint32_t first = static_cast<uint32_t>(c.first_tokens[i]), n = static_cast<uint32_t>(c.n_tokens[i]);
        if (c.kv)
            static_cast<SlotSpanKV*>(staged)[i] = SlotSpanKV{{write ? a->d_entries : nullptr, write ? v->d_entries : nullptr},
                                                             {write ? a->d_scale_tab : nullptr, write ? v->d_scale_tab : nullptr},
                                                             {a->region_pages, v->region_pages}, {a->scale_run, v->scale_run}, {a->row, v->row},
                                                             first, n, prefix, 0u, c.slot_begins[i]};
        else
            static_cast<SlotSpan*>(staged)[i] = SlotSpan{write ? a->d_entries : nullptr, write ? a->d_scale_tab : nullptr, a->region_pages,
                                                         a->scale_run, a->row, first, n, prefix, c.slot_begins[i]};
        prefix += static_cast<uint32_t>(p1[i]) - first / 2u;
    }
    uint64_t* bases = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(staged) + span_bytes);
    for (uint32_t l = 0; l < c.n_layers; ++l) bases[l] = reinterpret_cast<uint64_t>(c.d_caches[l]);
    if (held) {
        SlotHeld* h = reinterpret_cast<SlotHeld*>(static_cast<uint8_t*>(staged) + span_bytes + base_bytes);
        for (uint32_t i = 0; i < c.n_spans; ++i)
            for (int k = 0; k < 2; ++k) {
                h[i].in[k] = c.held_in ? reinterpret_cast<uint64_t>(c.held_in[2 * i + k]) : 0;
                h[i].out[k] = c.held_out ? reinterpret_cast<uint64_t>(c.held_out[2 * i + k]) : 0;
            }
    }
    if (!write)
        for (auto& w : write_evs_)
            if (w.s != s) HIP_TRY(hipStreamWaitEvent(s, w.ev, 0));
    HIP_TRY(hipMemcpyAsync(d_slot, staged, bytes, hipMemcpyHostToDevice, s));
    SlotArgs sa{};
    sa.spans = static_cast<const SlotSpan*>(d_slot);
    sa.caches = reinterpret_cast<const uint64_t*>(static_cast<const uint8_t*>(d_slot) + span_bytes);
    sa.slots = c.d_slots;
    sa.tab = d_tab_;
    sa.zeros = d_zero_page_;
    sa.n_slots = c.n_slots;
    sa.kind_stride = c.kind_stride;
    sa.page_step = c.page_step;
    sa.n_spans = c.n_spans;
    sa.n_pairs = static_cast<uint32_t>(n_pairs);
    sa.n_layers = c.n_layers;
    sa.layer_begin = c.layer_begin;
    sa.kind_fast = tuning().slots_kind_fast != 0;
    sa.scheme = as[0]->scheme;
    sa.quant_mode = quant_mode_;
    if (c.kv) {                                                                 // the same pages, slots and held rows; a codec per kind
        SlotKVArgs x{};
        x.a = SlotKVArgs::Pages{static_cast<const SlotSpanKV*>(d_slot), sa.caches, sa.slots, sa.tab, sa.zeros, sa.n_slots, sa.kind_stride,
                                sa.page_step, sa.n_spans, sa.n_pairs, sa.n_layers, sa.layer_begin, sa.kind_fast};
        x.held = held ? reinterpret_cast<const SlotHeld*>(static_cast<const uint8_t*>(d_slot) + span_bytes + base_bytes) : nullptr;
        x.held_stride = c.held_stride;
        x.n_moves = n_held ? c.n_spans * 2u * c.n_layers : 0u;
        x.bf16 = c.elem == SPECKV_SLOT_ELEM_BF16;
        HIP_TRY(write ? launch_compress_slots_kv(x, s) : launch_read_slots_kv(x, s));
    } else if (ex) {
        SlotExArgs x{};
        x.a = sa;
        x.held = held ? reinterpret_cast<const SlotHeld*>(static_cast<const uint8_t*>(d_slot) + span_bytes + base_bytes) : nullptr;
        x.held_stride = c.held_stride;
        x.n_moves = n_held ? c.n_spans * 2u * c.n_layers : 0u;
        x.bf16 = c.elem == SPECKV_SLOT_ELEM_BF16;
        if (c.k_mul) {
            const SlotKmulArgs y{x, static_cast<const uint8_t*>(c.k_mul), c.k_mul_stride};
            HIP_TRY(write ? launch_compress_slots_kmul(y, s) : launch_read_slots_kmul(y, s));
        } else {
            HIP_TRY(write ? launch_compress_slots_ex(x, s) : launch_read_slots_ex(x, s));
        }
    } else {
        HIP_TRY(write ? launch_compress_slots(sa, s) : launch_read_slots(sa, s));
    }
    for (uint32_t i = 0; i < c.n_spans; ++i)                                    // the kernel is queued: speckv_free waits for this stream
        for (int k = 0; k < n_allocs; ++k) note_use(alloc_of(i, k), s);
    const uint64_t n = n_pairs * n_each;
    if (write) {                                                                // host mirror first, then the orderings
        each_page([&](Allocation* a, uint64_t p) {
            if (a->scheme != SPECKV_COMP_FP16) a->flags[p] |= 4u; else a->flags[p] &= ~4u;
        });
        st_.total_compressions += n;
        st_.original_bytes += n * kPageSize;
    } else {
        st_.total_decompressions += n;
        st_.dma_submitted += n;
        st_.dma_completed += n;                                   // completion belongs to the caller's stream
    }
    if (hipEventRecord(grp_ring_.ev[slot], s) != hipSuccess) {      // the staging slot must not be reused under the kernel
        (void)hipGetLastError();
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (write) RC_TRY(note_async_write_or_wait(s));
    return SPECKV_OK;
}

int Engine::read_slots(const SlotCall& c, hipStream_t s) { return slots_call(c, false, s); }
int Engine::write_slots(const SlotCall& c, hipStream_t s) { return slots_call(c, true, s); }
int Engine::read_slots_kv(const SlotCall& c, hipStream_t s) { return c.kv ? slots_call(c, false, s) : SPECKV_ERR_INVAL; }
int Engine::write_slots_kv(const SlotCall& c, hipStream_t s) { return c.kv ? slots_call(c, true, s) : SPECKV_ERR_INVAL; }

} // namespace speckv
