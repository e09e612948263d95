// cxl-speckv_amd/csrc/engine_io.cpp -- the data path: writes (compress into the pool), reads, bulk fetch + decompress (Engine members)
#include "engine_internal.hpp"
#include "tuning.hpp"

namespace speckv {

// device-visible address of an allocation's record-length samples (null where there are none: other schemes, the fake device)
static uint32_t* len_samples_dev(const Allocation* a)
{
    if (!a->len_samples || a->scheme != SPECKV_COMP_INT8_DELTA_RLE) return nullptr;
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, a->len_samples, 0) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    return static_cast<uint32_t*>(dp);
}
// "this allocation holds data that compresses": the mean of the record lengths the compress kernel left behind (every 1024th
// page) is under 512 B.  Read without any ordering -- samples of writes still in flight may be missing -- because it only picks
// between two decoders that produce the same bytes.
static bool looks_structured(const Allocation* a)
{
    if (!a->len_samples || a->scheme != SPECKV_COMP_INT8_DELTA_RLE) return false;
    uint64_t sum = 0, cnt = 0;
    for (uint32_t i = 0; i < kLenSamples; ++i) {
        const uint32_t v = *const_cast<volatile uint32_t*>(a->len_samples + i);
        if (v) { sum += v; ++cnt; }
    }
    return cnt && sum / cnt < 512u;
}


// -------------------------------------------------------------- data path
int Engine::write(uint64_t handle, uint64_t off, const void* src, size_t len, bool on_device)
{
    if (null_) return no_data_path("speckv_ext_write");
    Allocation* a = find(handle);
    if (!a) return SPECKV_ERR_GENERAL;
    if (off % kPageSize || !src) return SPECKV_ERR_INVAL;
    if (off > a->size_bytes || len > a->size_bytes - off) return SPECKV_ERR_GENERAL;
    const bool to_end = (off + len == a->size_bytes);
    if (len % kPageSize && !to_end) return SPECKV_ERR_INVAL;
    if (len == 0) return SPECKV_OK;
    const uint64_t p0 = off / kPageSize;
    const uint64_t full = len / kPageSize, tail = len % kPageSize;
    DeviceScope device_scope(device_);
    if (a->packed) { RC_TRY(unpack(a)); if ((a = find(handle)) == nullptr) return SPECKV_ERR_GENERAL; }   // a sealed allocation goes back into slots first
    RC_TRY(quiesce());
    if ((a = find(handle)) == nullptr) return SPECKV_ERR_GENERAL;
    reap(false);
    // the source may have been produced on any stream of the caller: this call is
    // synchronous anyway, so order it after everything queued on the device
    if (on_device) HIP_TRY(hipDeviceSynchronize());
    CodecArgs c{};
    c.entries = a->d_entries;
    c.scale_tab = a->d_scale_tab;        // fused-attention scale table follows every write
    c.scale_run = a->scale_run;
    c.len_samples = len_samples_dev(a);
    c.region_pages = a->region_pages;
    c.data_stride = kPageSize;
    c.scheme = a->scheme;
    c.quant_mode = quant_mode_;
    const uint8_t* s8 = static_cast<const uint8_t*>(src);
    if (on_device) {
        if (full) {
            c.first = p0; c.n = full; c.data = const_cast<uint8_t*>(s8);
            HIP_TRY(launch_compress(c, stream_));
        }
        if (tail) {
            uint8_t* st = static_cast<uint8_t*>(scratch(s_stage_, kPageSize));
            if (!st) return SPECKV_ERR_NOMEM;
            HIP_TRY(hipMemsetAsync(st, 0, kPageSize, stream_));
            HIP_TRY(hipMemcpyAsync(st, s8 + full * kPageSize, tail, hipMemcpyDeviceToDevice, stream_));
            c.first = p0 + full; c.n = 1; c.data = st;
            HIP_TRY(launch_compress(c, stream_));
        }
    } else {
        const uint64_t total = full + (tail ? 1 : 0);
        const uint64_t chunk_pages = std::min<uint64_t>(total, 16384);      // 64 MiB staging
        uint8_t* st = static_cast<uint8_t*>(scratch(s_stage_, chunk_pages * kPageSize));
        if (!st) return SPECKV_ERR_NOMEM;
        for (uint64_t done = 0; done < total; done += chunk_pages) {
            const uint64_t np = std::min(chunk_pages, total - done);
            const size_t bytes = static_cast<size_t>(std::min<uint64_t>(np * kPageSize, len - done * kPageSize));
            if (bytes < np * kPageSize) HIP_TRY(hipMemsetAsync(st + (np - 1) * kPageSize, 0, kPageSize, stream_));
            HIP_TRY(hipMemcpyAsync(st, s8 + done * kPageSize, bytes, hipMemcpyHostToDevice, stream_));
            c.first = p0 + done; c.n = np; c.data = st;
            HIP_TRY(launch_compress(c, stream_));
            HIP_TRY(hipStreamSynchronize(stream_));       // the staging buffer is shared: keep the ABI lock
        }
    }
    HIP_TRY(hipStreamSynchronize(stream_));
    const uint64_t np = full + (tail ? 1 : 0);
    for (uint64_t p = p0; p < p0 + np; ++p) {
        drop_page(a, static_cast<uint32_t>(p));             // a cached copy is stale now
        if (a->scheme != SPECKV_COMP_FP16) a->flags[p] |= 4u; else a->flags[p] &= ~4u;
    }
    st_.total_compressions += np;
    st_.original_bytes += np * kPageSize;
    return SPECKV_OK;
}

// Asynchronous page writes for a decode loop: n pages first, first+step, first+2*step, ... (the pages of one position
// pair in every (layer, kind) region of the shim layout are `num_tokens/2` pages apart) compressed from a contiguous
// device buffer on the caller's stream.  Pages that are cached right now would go stale: that case takes the
// synchronous path (a decode loop appends positions nobody has fetched yet).
int Engine::write_strided(uint64_t handle, uint64_t first, uint64_t step, uint64_t n, const void* d_src, hipStream_t s)
{
    if (null_) return no_data_path("speckv_ext_write_strided");
    Allocation* a = find(handle);
    if (!a) return SPECKV_ERR_GENERAL;
    if (!d_src || step == 0) return SPECKV_ERR_INVAL;
    if (n == 0) return SPECKV_OK;
    if (first >= a->n_pages || (n - 1) > (a->n_pages - 1 - first) / step) return SPECKV_ERR_GENERAL;
    // a last page that is only partly inside the allocation would need zero padding of the source: not here
    if (a->size_bytes % kPageSize && first + (n - 1) * step == a->n_pages - 1) return SPECKV_ERR_INVAL;
    DeviceScope device_scope(device_);
    if (a->packed) { RC_TRY(unpack(a)); if ((a = find(handle)) == nullptr) return SPECKV_ERR_GENERAL; }
    // NULL = the engine's stream: the source may have been produced on any stream of the caller, order after all of them
    if (!s) HIP_TRY(hipDeviceSynchronize());
    bool cached = false;
    for (uint64_t i = 0; i < n && !cached; ++i) cached = (res_flags(a, first + i * step) & 3u) != 0;
    if (cached || !flights_.empty() || ring_busy_ > 0) {
        RC_TRY(quiesce());
        if ((a = find(handle)) == nullptr) return SPECKV_ERR_GENERAL;
        for (uint64_t i = 0; i < n; ++i) drop_page(a, static_cast<uint32_t>(first + i * step));
        RC_TRY(flush_mirror());
        if (s) RC_TRY(wait_stream());
    }
    CodecArgs c{};
    c.entries = a->d_entries;
    c.scale_tab = a->d_scale_tab;
    c.scale_run = a->scale_run;
    c.len_samples = len_samples_dev(a);
    c.region_pages = a->region_pages;
    c.data_stride = kPageSize;
    c.scheme = a->scheme;
    c.quant_mode = quant_mode_;
    c.first = first;
    c.page_step = step;
    c.n = n;
    c.data = static_cast<uint8_t*>(const_cast<void*>(d_src));
    hipStream_t st = s ? s : stream_;
    HIP_TRY(launch_compress(c, st));
    // The kernel is queued: from here on the host mirror follows it whatever else fails (an early return between
    // the launch and these lines left the device table and the host flags disagreeing).
    note_use(a, s);
    for (uint64_t i = 0; i < n; ++i) {
        uint32_t& f = a->flags[first + i * step];
        if (a->scheme != SPECKV_COMP_FP16) f |= 4u; else f &= ~4u;
    }
    st_.total_compressions += n;
    st_.original_bytes += n * kPageSize;
    RC_TRY(note_async_write_or_wait(s));
    if (!s) RC_TRY(wait_stream());
    return SPECKV_OK;
}

// speckv_ext_write_async: a contiguous page range from a device buffer, on the caller's stream, no device-wide wait.
int Engine::write_async(uint64_t handle, uint64_t off, const void* d_src, size_t len, hipStream_t s)
{
    if (null_) return no_data_path("speckv_ext_write_async");
    if (off % kPageSize || len % kPageSize) return SPECKV_ERR_INVAL;
    if (len == 0) return find(handle) ? SPECKV_OK : SPECKV_ERR_GENERAL;
    return write_strided(handle, off / kPageSize, 1, len / kPageSize, d_src, s);
}

// The descriptors of a grouped launch (write_groups, read_pairs) travel pinned slot -> device slot: 4 of each in rotation, a
// slot guarded by an event the caller records on its stream behind the kernel (grp_ring_.ev[slot]).  Hands out the next
// slot, `bytes` long at least, once the launch that last used it is over -- that wait may release the ABI lock: allocations
// looked up before it have to be looked up again.
int Engine::descriptor_slot(size_t bytes, int* slot_out, void** staged, void** d_slot)
{
    if (grp_ring_.slot_bytes < bytes) {
        HIP_TRY(hipDeviceSynchronize());
        if (grp_ring_.base) { (void)hipHostFree(grp_ring_.base); grp_ring_.base = nullptr; }
        if (d_groups_) { (void)hipFree(d_groups_); d_groups_ = nullptr; }
        grp_ring_.slot_bytes = std::max<size_t>(bytes * 2, 16384);
        HIP_TRY(hipHostMalloc(&grp_ring_.base, grp_ring_.slot_bytes * 4, hipHostMallocDefault));
        HIP_TRY(hipMalloc(reinterpret_cast<void**>(&d_groups_), grp_ring_.slot_bytes * 4));
        for (auto& ev : grp_ring_.ev)
            if (!ev) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    }
    const int slot = grp_ring_.next;
    grp_ring_.next = (slot + 1) & 3;
    RC_TRY(wait_event(grp_ring_.ev[slot]));
    *slot_out = slot;
    *staged = static_cast<uint8_t*>(grp_ring_.base) + static_cast<size_t>(slot) * grp_ring_.slot_bytes;
    *d_slot = reinterpret_cast<uint8_t*>(d_groups_) + static_cast<size_t>(slot) * grp_ring_.slot_bytes;
    return SPECKV_OK;
}

// write_strided for a batch of allocations in one launch (the append of a decode step: SURVEY 8f row N2), and several
// page runs of ONE allocation in one launch (a prompt's K / V regions: speckv_ext_write_runs).  Host side as in
// write_strided per group (cached pages are invalidated first); the kernel takes one descriptor per group.
// `rows` set: the pair-gather form (speckv_ext_write_pairs) -- a group is a position pair of 2 * n_layers pages read from four
// rows (d_srcs holds four pointers per group), and an allocation may have several groups as long as they share no page.
int Engine::write_groups(const uint64_t* handles, const uint64_t* firsts, const void* const* d_srcs, uint32_t n_groups,
                         uint64_t step, uint64_t n_each, hipStream_t s, bool same_allocation, const PairRows* rows)
{
    if (!handles || !firsts || !d_srcs || step == 0 || !s) return SPECKV_ERR_INVAL;
    if (rows && rows->layer_stride % 16u) return SPECKV_ERR_INVAL;
    if (n_groups == 0 || n_each == 0) return SPECKV_OK;
    std::vector<Allocation*> as(n_groups);
    bool cached = false;
    for (uint32_t i = 0; i < n_groups; ++i) {
        Allocation* a = find(handles[same_allocation ? 0 : i]);
        if (!a) return SPECKV_ERR_GENERAL;
        if (rows) {
            for (uint32_t k = 0; k < 4; ++k)
                if (!d_srcs[4u * i + k] || reinterpret_cast<uintptr_t>(d_srcs[4u * i + k]) % 16u) return SPECKV_ERR_INVAL;
        } else if (!d_srcs[i]) return SPECKV_ERR_INVAL;
        if (a->scheme != find(handles[0])->scheme) return SPECKV_ERR_INVAL;
        if (firsts[i] >= a->n_pages || (n_each - 1) > (a->n_pages - 1 - firsts[i]) / step) return SPECKV_ERR_GENERAL;
        if (a->size_bytes % kPageSize && firsts[i] + (n_each - 1) * step == a->n_pages - 1) return SPECKV_ERR_INVAL;
        if (!same_allocation && !rows)
            for (uint32_t k = 0; k < i; ++k) if (as[k] == a) return SPECKV_ERR_INVAL;   // one descriptor per allocation
        as[i] = a;
        for (uint64_t j = 0; j < n_each && !cached; ++j) cached = (res_flags(a, firsts[i] + j * step) & 3u) != 0;
    }
    for (uint32_t i = 0; i < n_groups; ++i)
        if (as[i]->packed) {                                    // sealed allocations go back into slots first
            DeviceScope scope(device_);
            RC_TRY(unpack(as[i]));
            for (uint32_t j = 0; j < n_groups; ++j)
                if ((as[j] = find(handles[same_allocation ? 0 : j])) == nullptr) return SPECKV_ERR_GENERAL;
        }
    if (same_allocation && n_groups > 1) {                      // the runs of one allocation must not overlap (racing writers)
        std::vector<uint64_t> order(firsts, firsts + n_groups);
        std::sort(order.begin(), order.end());
        const uint64_t span = (n_each - 1) * step;
        for (uint32_t i = 1; i < n_groups; ++i)
            if (step == 1 ? order[i] <= order[i - 1] + span : order[i] == order[i - 1]) return SPECKV_ERR_INVAL;
        // (strided groups that start on different pages interleave without touching: page = first + j * step)
        if (step != 1)
            for (uint32_t i = 1; i < n_groups; ++i)
                if ((order[i] - order[0]) % step == 0 && order[i] - order[0] <= span) return SPECKV_ERR_INVAL;
    }
    if (rows && n_groups > 1) {                                 // the pairs of one allocation must not share a page
        std::vector<uint32_t> order(n_groups);
        for (uint32_t i = 0; i < n_groups; ++i) order[i] = i;
        std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
            return handles[x] != handles[y] ? handles[x] < handles[y] : firsts[x] < firsts[y]; });
        for (uint32_t i = 1; i < n_groups; ++i)
            for (uint32_t k = i; k-- > 0 && handles[order[k]] == handles[order[i]];) {
                const uint64_t d = firsts[order[i]] - firsts[order[k]];
                if (d % step == 0 && d / step < n_each) return SPECKV_ERR_INVAL;
            }
    }
    DeviceScope device_scope(device_);
    if (cached || !flights_.empty() || ring_busy_ > 0) {
        RC_TRY(quiesce());
        for (uint32_t i = 0; i < n_groups; ++i) {
            if ((as[i] = find(handles[same_allocation ? 0 : i])) == nullptr) return SPECKV_ERR_GENERAL;
            for (uint64_t j = 0; j < n_each; ++j) drop_page(as[i], static_cast<uint32_t>(firsts[i] + j * step));
        }
        RC_TRY(flush_mirror());
        RC_TRY(wait_stream());
    }
    const size_t bytes = static_cast<size_t>(n_groups) * (rows ? sizeof(CommitPair) : sizeof(CompressGroup));
    int slot = 0;
    void *staged = nullptr, *d_slot = nullptr;
    RC_TRY(descriptor_slot(bytes, &slot, &staged, &d_slot));  // may release the ABI lock
    for (uint32_t i = 0; i < n_groups; ++i)
        if ((as[i] = find(handles[same_allocation ? 0 : i])) == nullptr) return SPECKV_ERR_GENERAL;
    for (uint32_t i = 0; i < n_groups; ++i) {
        const Allocation* a = as[i];
        if (rows) {
            const void* const* r = d_srcs + 4u * i;
            static_cast<CommitPair*>(staged)[i] = CommitPair{a->d_entries, a->d_scale_tab, a->region_pages, a->scale_run, firsts[i],
                {static_cast<const uint8_t*>(r[0]), static_cast<const uint8_t*>(r[1]), static_cast<const uint8_t*>(r[2]), static_cast<const uint8_t*>(r[3])}};
        } else {
            static_cast<CompressGroup*>(staged)[i] = CompressGroup{a->d_entries, a->d_scale_tab, a->region_pages, a->scale_run, firsts[i],
                                                                   static_cast<const uint8_t*>(d_srcs[i])};
        }
    }
    HIP_TRY(hipMemcpyAsync(d_slot, staged, bytes, hipMemcpyHostToDevice, s));
    CodecArgs c{};
    c.n = static_cast<uint64_t>(n_groups) * n_each;
    if (rows) {
        PairArgs pa{};
        pa.pairs = static_cast<const CommitPair*>(d_slot);
        pa.n_pairs = n_groups;
        pa.n_layers = rows->n_layers;
        pa.page_step = step;
        pa.layer_stride = rows->layer_stride;
        pa.scheme = as[0]->scheme;
        pa.quant_mode = quant_mode_;
        HIP_TRY(launch_compress_pairs(pa, s));
    } else {
        c.groups = static_cast<const CompressGroup*>(d_slot);
        c.group_n = n_each;
        c.page_step = step;
        c.data_stride = kPageSize;
        c.scheme = as[0]->scheme;
        c.quant_mode = quant_mode_;
        HIP_TRY(launch_compress(c, s));
    }
    for (uint32_t i = 0; i < n_groups; ++i) {           // the kernel is queued: host mirror first, then the orderings
        Allocation* a = as[i];
        note_use(a, s);
        for (uint64_t j = 0; j < n_each; ++j) {
            uint32_t& f = a->flags[firsts[i] + j * step];
            if (a->scheme != SPECKV_COMP_FP16) f |= 4u; else f &= ~4u;
        }
    }
    st_.total_compressions += c.n;
    st_.original_bytes += c.n * kPageSize;
    if (hipEventRecord(grp_ring_.ev[slot], s) != hipSuccess) {      // the staging slot must not be reused under the kernel
        (void)hipGetLastError();
        HIP_TRY(hipStreamSynchronize(s));
    }
    RC_TRY(note_async_write_or_wait(s));
    return SPECKV_OK;
}

int Engine::write_strided_batch(const uint64_t* handles, const uint64_t* firsts, const void* const* d_srcs, uint32_t n_alloc,
                                uint64_t step, uint64_t n_each, hipStream_t s)
{
    if (null_) return no_data_path("speckv_ext_write_strided_batch");
    return write_groups(handles, firsts, d_srcs, n_alloc, step, n_each, s, false);
}

// speckv_ext_write_pairs: the commit of a multi-position step.  Pair i is pages first + j * step, j < 2 * n_layers, of
// handles[i], encoded from d_rows[4 i .. 4 i + 3] (K even, K odd, V even, V odd), layer_stride bytes apart per layer.
int Engine::write_pairs(const uint64_t* handles, const uint64_t* firsts, const void* const* d_rows, uint32_t n_pairs, uint64_t step,
                        uint32_t n_layers, uint64_t layer_stride, hipStream_t s)
{
    if (null_) return no_data_path("speckv_ext_write_pairs");
    const PairRows rows{n_layers, layer_stride};
    return write_groups(handles, firsts, d_rows, n_pairs, step, 2ull * n_layers, s, false, &rows);
}

// speckv_ext_read_pairs: write_pairs read backwards (the rollback of committed positions).  Pair i is pages first + j * step,
// j < 2 * n_layers, of handles[i], decoded into d_rows[4 i .. 4 i + 3] (K even, K odd, V even, V odd; NULL = not wanted),
// layer_stride bytes apart per layer, by ONE launch on the caller's stream.  Ordering: the kernel follows what the caller queued
// on `s` before it (a commit on the same stream), as any stream call does; beyond that -- fetch_range leaves this to the caller --
// `s` is made to wait for the event of the last asynchronous pool write on every OTHER caller stream the engine knows
// (write_evs_; not while `s` is capturing), and the engine's own writes are synchronous.  Nothing is written to the pool,
// so a sealed allocation stays sealed and cached copies stay valid.
int Engine::read_pairs(const uint64_t* handles, const uint64_t* firsts, void* const* d_rows, uint32_t n_pairs, uint64_t step,
                       uint32_t n_layers, uint64_t layer_stride, hipStream_t s)
{
    return pairs_read(handles, nullptr, false, firsts, d_rows, n_pairs, step, n_layers, layer_stride, s);
}

// speckv_ext_read_pairs_kv: read_pairs for the split pool.  Pair i names TWO allocations, handles[i] (FP8_E4M3, the K rows) and
// v_handles[i] (MXFP4, the V rows), each laid out as one region per layer: layer l of the pair is page firsts[i] + l * step of
// either, for l < n_layers REAL layers.  One descriptor slot and ONE launch (k_read_pairs_kv) for both allocations of every pair.
int Engine::read_pairs_kv(const uint64_t* k_handles, const uint64_t* v_handles, const uint64_t* firsts, void* const* d_rows, uint32_t n_pairs,
                          uint64_t step, uint32_t n_layers, uint64_t layer_stride, hipStream_t s)
{
    return pairs_read(k_handles, v_handles, true, firsts, d_rows, n_pairs, step, n_layers, layer_stride, s);
}

// The body of both.  Everything it does per allocation -- find and the judgement repeated after descriptor_slot, the page-range
// check, note_use -- it does for every side of a pair: one side (`handles`), or with kv two (`handles` = K, `v_handles` = V).  A
// single-allocation call takes exactly the path it took before.
int Engine::pairs_read(const uint64_t* handles, const uint64_t* v_handles, bool kv, const uint64_t* firsts, void* const* d_rows, uint32_t n_pairs,
                       uint64_t step, uint32_t n_layers, uint64_t layer_stride, hipStream_t s)
{
    if (null_) return no_data_path(kv ? "speckv_ext_read_pairs_kv" : "speckv_ext_read_pairs");
    if (!handles || (kv && !v_handles) || !firsts || !d_rows || step == 0 || !s || layer_stride % 16u) return SPECKV_ERR_INVAL;
    if (n_pairs == 0 || n_layers == 0) return SPECKV_OK;
    const int n_sides = kv ? 2 : 1;
    const uint64_t n_each = 2ull * n_layers;                  // pages per pair
    const uint64_t n_side = kv ? n_layers : n_each;           // ... of which one allocation holds: firsts[i] + j * step, j < n_side
    std::vector<Allocation*> as(n_pairs), vs(kv ? n_pairs : 0u);
    const auto check = [&](uint32_t i) -> int {
        for (int side = 0; side < n_sides; ++side) {
            Allocation* a = find((side ? v_handles : handles)[i]);
            if (!a) return SPECKV_ERR_GENERAL;
            for (uint32_t k = 0; side == 0 && k < 4; ++k)
                if (reinterpret_cast<uintptr_t>(d_rows[4u * i + k]) % 16u) return SPECKV_ERR_INVAL;
            if (kv ? a->scheme != (side ? SPECKV_COMP_MXFP4 : SPECKV_COMP_FP8_E4M3) : a->scheme != find(handles[0])->scheme) return SPECKV_ERR_INVAL;
            if (firsts[i] >= a->n_pages || (n_side - 1) > (a->n_pages - 1 - firsts[i]) / step) return SPECKV_ERR_GENERAL;
            (side ? vs : as)[i] = a;
        }
        if (kv && as[i]->layout.num_tokens != vs[i]->layout.num_tokens) return SPECKV_ERR_INVAL;
        return SPECKV_OK;
    };
    for (uint32_t i = 0; i < n_pairs; ++i) RC_TRY(check(i));
    DeviceScope device_scope(device_);
    const size_t bytes = static_cast<size_t>(n_pairs) * (kv ? sizeof(ReadPairKV) : sizeof(ReadPair));
    int slot = 0;
    void *staged = nullptr, *d_slot = nullptr;
    RC_TRY(descriptor_slot(bytes, &slot, &staged, &d_slot));  // may release the ABI lock: every pair is judged again
    for (uint32_t i = 0; i < n_pairs; ++i) RC_TRY(check(i));
    for (uint32_t i = 0; i < n_pairs; ++i) {
        void* const* r = d_rows + 4u * i;
        if (kv)
            static_cast<ReadPairKV*>(staged)[i] = ReadPairKV{{as[i]->row, vs[i]->row}, firsts[i],
                {static_cast<uint8_t*>(r[0]), static_cast<uint8_t*>(r[1]), static_cast<uint8_t*>(r[2]), static_cast<uint8_t*>(r[3])}};
        else
            static_cast<ReadPair*>(staged)[i] = ReadPair{as[i]->row, 0u, firsts[i],
                {static_cast<uint8_t*>(r[0]), static_cast<uint8_t*>(r[1]), static_cast<uint8_t*>(r[2]), static_cast<uint8_t*>(r[3])}};
    }
    if (!is_capturing(s))
        for (auto& w : write_evs_)
            if (w.s != s) HIP_TRY(hipStreamWaitEvent(s, w.ev, 0));      // (`dirty` is about the engine's stream, not this one)
    HIP_TRY(hipMemcpyAsync(d_slot, staged, bytes, hipMemcpyHostToDevice, s));
    if (kv) {
        ReadPairKVArgs ra{};
        ra.pairs = static_cast<const ReadPairKV*>(d_slot);
        ra.tab = d_tab_;
        ra.n_pairs = n_pairs;
        ra.n_layers = n_layers;
        ra.page_step = step;
        ra.layer_stride = layer_stride;
        HIP_TRY(launch_read_pairs_kv(ra, s));
    } else {
        ReadPairArgs ra{};
        ra.pairs = static_cast<const ReadPair*>(d_slot);
        ra.tab = d_tab_;
        ra.n_pairs = n_pairs;
        ra.n_layers = n_layers;
        ra.page_step = step;
        ra.layer_stride = layer_stride;
        ra.scheme = as[0]->scheme;
        ra.quant_mode = quant_mode_;
        HIP_TRY(launch_read_pairs(ra, s));
    }
    for (uint32_t i = 0; i < n_pairs; ++i) {                   // speckv_free waits for this stream
        note_use(as[i], s);
        if (kv) note_use(vs[i], s);
    }
    const uint64_t n = static_cast<uint64_t>(n_pairs) * n_each;
    st_.total_decompressions += n;
    st_.dma_submitted += n;
    st_.dma_completed += n;                                    // completion belongs to the caller's stream
    if (hipEventRecord(grp_ring_.ev[slot], s) != hipSuccess) {      // the staging slot must not be reused under the kernel
        (void)hipGetLastError();
        HIP_TRY(hipStreamSynchronize(s));
    }
    return SPECKV_OK;
}

// speckv_ext_copy_runs: the stored records of pages [run_firsts[r], run_firsts[r] + n_pages[i]), every run r, copied from src[i] to
// the same pages of dst[i] by ONE launch on the caller's stream; nothing is decoded (a request forked from positions another one
// holds).  The source side is read_pairs': record addresses from the device allocation table (any placement, a sealed source stays
// sealed), behind what the caller queued on `s` and behind the asynchronous pool writes on other caller streams.  The destination
// side is write_groups': sealed destinations are unpacked, cached destination pages invalidated, the host mirror follows the launch.
int Engine::copy_runs(const uint64_t* src, const uint64_t* dst, const uint64_t* n_pages, uint32_t n_pairs, const uint64_t* run_firsts,
                      uint32_t n_runs, hipStream_t s)
{
    const uint64_t* const from[2] = {src, nullptr};
    const uint64_t* const to[2] = {dst, nullptr};
    return runs_copy(from, to, false, n_pages, n_pairs, run_firsts, n_runs, s);
}

// speckv_ext_copy_runs_kv: copy_runs for the split pool.  Pair i copies the same pages in TWO allocation pairs, k_src[i] -> k_dst[i]
// (FP8_E4M3, the K rows) and v_src[i] -> v_dst[i] (MXFP4, the V rows), with one descriptor slot and ONE launch (k_copy_records_kv).
int Engine::copy_runs_kv(const uint64_t* k_src, const uint64_t* v_src, const uint64_t* k_dst, const uint64_t* v_dst, const uint64_t* n_pages,
                         uint32_t n_pairs, const uint64_t* run_firsts, uint32_t n_runs, hipStream_t s)
{
    const uint64_t* const from[2] = {k_src, v_src};
    const uint64_t* const to[2] = {k_dst, v_dst};
    return runs_copy(from, to, true, n_pages, n_pairs, run_firsts, n_runs, s);
}

// The body of both.  Everything it does per allocation -- find and the judgement repeated after every wait, the page-range check,
// unpacking a sealed destination, dropping cached destination pages, the host mirror, note_use -- it does for every side of a pair:
// one (src[0] -> dst[0]), or with kv two (index 0 = K, 1 = V).  An allocation that is written is named once across both sides and
// is not read.  A single-allocation call takes exactly the path it took before.
int Engine::runs_copy(const uint64_t* const src[2], const uint64_t* const dst[2], bool kv, const uint64_t* n_pages, uint32_t n_pairs,
                      const uint64_t* run_firsts, uint32_t n_runs, hipStream_t s)
{
    if (null_) return no_data_path(kv ? "speckv_ext_copy_runs_kv" : "speckv_ext_copy_runs");
    const int n_sides = kv ? 2 : 1;
    for (int side = 0; side < n_sides; ++side)
        if (!src[side] || !dst[side]) return SPECKV_ERR_INVAL;
    if (!n_pages || !run_firsts || !s) return SPECKV_ERR_INVAL;
    uint64_t most = 0;
    for (uint32_t i = 0; i < n_pairs; ++i) most = std::max(most, n_pages[i]);
    if (n_pairs == 0 || n_runs == 0 || most == 0) return SPECKV_OK;
    // what depends on the arguments alone: the runs must not overlap (they do for some pair exactly if they do for the longest)
    // and must not wrap; an allocation that is written is named once, and not read
    std::vector<uint64_t> order(run_firsts, run_firsts + n_runs);
    std::sort(order.begin(), order.end());
    if (order.back() > UINT64_MAX - most) return SPECKV_ERR_GENERAL;
    for (uint32_t r = 1; r < n_runs; ++r)
        if (order[r] - order[r - 1] < most) return SPECKV_ERR_INVAL;
    {
        std::vector<uint64_t> written, read;
        for (int side = 0; side < n_sides; ++side)
            for (uint32_t i = 0; i < n_pairs; ++i) {
                if (src[side][i] == dst[side][i]) return SPECKV_ERR_INVAL;
                if (n_pages[i]) { written.push_back(dst[side][i]); read.push_back(src[side][i]); }
            }
        std::sort(written.begin(), written.end());
        std::sort(read.begin(), read.end());
        if (std::adjacent_find(written.begin(), written.end()) != written.end()) return SPECKV_ERR_INVAL;
        for (uint64_t h : written)
            if (std::binary_search(read.begin(), read.end(), h)) return SPECKV_ERR_INVAL;
    }
    std::vector<Allocation*> from[2], to[2];
    for (int side = 0; side < n_sides; ++side) { from[side].resize(n_pairs); to[side].resize(n_pairs); }
    const auto check = [&]() -> int {
        int scheme = -1;
        for (uint32_t i = 0; i < n_pairs; ++i) {
            for (int side = 0; side < n_sides; ++side) {
                Allocation *a = find(src[side][i]), *b = find(dst[side][i]);
                if (!a || !b) return SPECKV_ERR_GENERAL;
                if (kv) scheme = side ? SPECKV_COMP_MXFP4 : SPECKV_COMP_FP8_E4M3;
                else if (scheme < 0) scheme = a->scheme;
                if (a->scheme != scheme || b->scheme != scheme) return SPECKV_ERR_INVAL;
                if (n_pages[i] && (order.back() + n_pages[i] > a->n_pages || order.back() + n_pages[i] > b->n_pages)) return SPECKV_ERR_GENERAL;
                from[side][i] = a;
                to[side][i] = b;
            }
            if (kv && (from[0][i]->layout.num_tokens != from[1][i]->layout.num_tokens || to[0][i]->layout.num_tokens != to[1][i]->layout.num_tokens))
                return SPECKV_ERR_INVAL;
        }
        return SPECKV_OK;
    };
    RC_TRY(check());
    for (int side = 0; side < n_sides; ++side)
        for (uint32_t i = 0; i < n_pairs; ++i)
            if (n_pages[i] && to[side][i]->packed) {            // sealed destinations go back into slots first
                DeviceScope scope(device_);
                RC_TRY(unpack(to[side][i]));
                RC_TRY(check());
            }
    const auto each_dst_page = [&](auto&& f) {
        for (int side = 0; side < n_sides; ++side)
            for (uint32_t i = 0; i < n_pairs; ++i)
                for (uint32_t r = 0; r < n_runs; ++r)
                    for (uint64_t p = run_firsts[r]; p < run_firsts[r] + n_pages[i]; ++p) f(to[side][i], p);
    };
    bool cached = false;
    each_dst_page([&](Allocation* a, uint64_t p) { cached = cached || (res_flags(a, p) & 3u) != 0; });
    DeviceScope device_scope(device_);
    if (cached || !flights_.empty() || ring_busy_ > 0) {
        RC_TRY(quiesce());
        RC_TRY(check());
        each_dst_page([&](Allocation* a, uint64_t p) { drop_page(a, static_cast<uint32_t>(p)); });
        RC_TRY(flush_mirror());
        RC_TRY(wait_stream());
    }
    const size_t pair_bytes = static_cast<size_t>(n_pairs) * (kv ? sizeof(CopyPairKV) : sizeof(CopyPair));     // (a multiple of 8: the run firsts follow)
    const size_t bytes = pair_bytes + static_cast<size_t>(n_runs) * sizeof(uint64_t);
    int slot = 0;
    void *staged = nullptr, *d_slot = nullptr;
    RC_TRY(descriptor_slot(bytes, &slot, &staged, &d_slot));  // may release the ABI lock: every pair is judged again
    RC_TRY(check());
    uint64_t n_recs = 0;
    for (uint32_t i = 0; i < n_pairs; ++i) {
        for (int side = 0; side < n_sides; ++side)
            if (n_pages[i] && to[side][i]->packed) return SPECKV_ERR_GENERAL;          // sealed again by another caller meanwhile
        const Allocation* t = to[0][i];
        if (kv)
            static_cast<CopyPairKV*>(staged)[i] = CopyPairKV{{t->d_entries, to[1][i]->d_entries}, t->d_scale_tab, t->region_pages, t->scale_run,
                                                             {from[0][i]->row, from[1][i]->row}, n_pages[i], n_recs};
        else
            static_cast<CopyPair*>(staged)[i] = CopyPair{t->d_entries, t->d_scale_tab, t->region_pages, t->scale_run, from[0][i]->row, 0u, n_pages[i], n_recs};
        n_recs += n_pages[i] * n_runs * static_cast<uint64_t>(n_sides);
    }
    memcpy(static_cast<uint8_t*>(staged) + pair_bytes, run_firsts, static_cast<size_t>(n_runs) * sizeof(uint64_t));
    if (!is_capturing(s))
        for (auto& w : write_evs_)
            if (w.s != s) HIP_TRY(hipStreamWaitEvent(s, w.ev, 0));
    HIP_TRY(hipMemcpyAsync(d_slot, staged, bytes, hipMemcpyHostToDevice, s));
    const uint64_t* d_firsts = reinterpret_cast<const uint64_t*>(static_cast<const uint8_t*>(d_slot) + pair_bytes);
    if (kv) {
        CopyKVArgs ca{};
        ca.pairs = static_cast<const CopyPairKV*>(d_slot);
        ca.run_firsts = d_firsts;
        ca.tab = d_tab_;
        ca.n_pairs = n_pairs;
        ca.n_runs = n_runs;
        ca.n_recs = n_recs;
        ca.n_cus = cus();
        HIP_TRY(launch_copy_records_kv(ca, s));
    } else {
        CopyArgs ca{};
        ca.pairs = static_cast<const CopyPair*>(d_slot);
        ca.run_firsts = d_firsts;
        ca.tab = d_tab_;
        ca.n_pairs = n_pairs;
        ca.n_runs = n_runs;
        ca.n_recs = n_recs;
        ca.n_cus = cus();
        ca.scheme = from[0][0]->scheme;
        HIP_TRY(launch_copy_records(ca, s));
    }
    for (int side = 0; side < n_sides; ++side)
        for (uint32_t i = 0; i < n_pairs; ++i) {              // the kernel is queued: host mirror first, then the orderings
            note_use(from[side][i], s);                       // speckv_free of either side waits for this stream
            note_use(to[side][i], s);
        }
    each_dst_page([&](Allocation* a, uint64_t p) {
        if (a->scheme != SPECKV_COMP_FP16) a->flags[p] |= 4u; else a->flags[p] &= ~4u;
    });
    st_.copied_pages += n_recs;
    st_.dma_submitted += n_recs;
    st_.dma_completed += n_recs;                              // completion belongs to the caller's stream
    if (hipEventRecord(grp_ring_.ev[slot], s) != hipSuccess) {      // the staging slot must not be reused under the kernel
        (void)hipGetLastError();
        HIP_TRY(hipStreamSynchronize(s));
    }
    RC_TRY(note_async_write_or_wait(s));
    return SPECKV_OK;
}

int Engine::write_runs(uint64_t handle, const uint64_t* firsts, const void* const* d_srcs, uint32_t n_runs, uint64_t n_each, hipStream_t s)
{
    if (null_) return no_data_path("speckv_ext_write_runs");
    return write_groups(&handle, firsts, d_srcs, n_runs, 1, n_each, s, true);
}

int Engine::read(uint64_t handle, uint64_t off, void* dst, size_t len, bool on_device)
{
    if (null_) return no_data_path("speckv_ext_read");
    Allocation* a = find(handle);
    if (!a) return SPECKV_ERR_GENERAL;
    if (off % kPageSize || !dst) return SPECKV_ERR_INVAL;
    if (off > a->size_bytes || len > a->size_bytes - off) return SPECKV_ERR_GENERAL;
    if (len % kPageSize && off + len != a->size_bytes) return SPECKV_ERR_INVAL;
    if (len == 0) return SPECKV_OK;
    const uint64_t p0 = off / kPageSize, full = len / kPageSize, tail = len % kPageSize;
    DeviceScope device_scope(device_);
    if (on_device) HIP_TRY(hipDeviceSynchronize());    // dst may still be in use on a caller stream
    else RC_TRY(order_after_writes());                 // records being written asynchronously on a caller stream
    CodecArgs c{};
    c.entries = a->d_entries;
    c.trusted = 1;                       // pool records only ever come from k_compress
    c.data_stride = kPageSize;
    c.scheme = a->scheme;
    c.quant_mode = quant_mode_;
    uint8_t* d8 = static_cast<uint8_t*>(dst);
    if (on_device && !tail) {
        c.first = p0; c.n = full; c.data = d8;
        HIP_TRY(launch_decompress(c, stream_));
    } else {
        const uint64_t total = full + (tail ? 1 : 0);
        const uint64_t chunk_pages = std::min<uint64_t>(total, 16384);
        uint8_t* st = static_cast<uint8_t*>(scratch(s_stage_, chunk_pages * kPageSize));
        if (!st) return SPECKV_ERR_NOMEM;
        for (uint64_t done = 0; done < total; done += chunk_pages) {
            const uint64_t np = std::min(chunk_pages, total - done);
            const size_t bytes = static_cast<size_t>(std::min<uint64_t>(np * kPageSize, len - done * kPageSize));
            c.first = p0 + done; c.n = np; c.data = st;
            HIP_TRY(launch_decompress(c, stream_));
            HIP_TRY(hipMemcpyAsync(d8 + done * kPageSize, st, bytes,
                                   on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, stream_));
            HIP_TRY(hipStreamSynchronize(stream_));
        }
    }
    HIP_TRY(hipStreamSynchronize(stream_));
    const uint64_t np = full + (tail ? 1 : 0);
    st_.total_decompressions += np;
    st_.dma_submitted += np; st_.dma_completed += np; completed_unpolled_ += np;
    return SPECKV_OK;
}

// Copy-engine fetch of a logical page range (the reference's DMA path: one descriptor per 4 KiB page through the
// DMA engine, speckv_allocator.cpp:115-138, dma_engine.v:150-217 -- here one hipMemcpyPeerAsync per POOL GPU and
// chunk, because striping makes the range one contiguous record run on every pool): the runs are copied over xGMI
// into local staging on per-peer side streams, then decompressed locally from there.  Two staging buffers in
// rotation: the copies of chunk c+1 overlap the decompression of chunk c.
int Engine::fetch_range_copy_engine(Allocation* a, uint64_t first, uint64_t n, void* d_dst, bool f32, hipStream_t st)
{
    // data that compresses takes the flat-run decoder here too: a sealed allocation by its packed size, another by its length samples
    int hint = 0;
    if (a->scheme == SPECKV_COMP_INT8_DELTA_RLE && a->n_pages) {
        if (a->packed) { uint64_t pk = 0; for (uint64_t b : a->packed_bytes) pk += b; hint = pk / a->n_pages < 512u ? 1 : 0; }
        else hint = looks_structured(a) ? 1 : 0;
    }
    if (hint) st_.flat_decoder_fetches++;
    const uint32_t D = static_cast<uint32_t>(a->pool_of_residue.size());
    const bool packed = a->packed && a->packed_regular;
    if (D == 0 || D > 8 || !(a->regular || packed)) return SPECKV_ERR_INVAL;
    const size_t stride = a->rec_stride;
    if (!stage_[0]) {
        stage_bytes_ = env_mb("SPECKV_STAGE_MB", 64) << 20;
        for (int b = 0; b < 2; ++b) {
            HIP_TRY(hipMalloc(reinterpret_cast<void**>(&stage_[b]), stage_bytes_));
            HIP_TRY(hipEventCreateWithFlags(&stage_free_[b], hipEventDisableTiming));
        }
    }
    if (lanes_.size() < pools_.size()) {
        const size_t old = lanes_.size();
        lanes_.resize(pools_.size());
        for (size_t i = old; i < lanes_.size(); ++i) {
            HIP_TRY(hipStreamCreateWithFlags(&lanes_[i].s, hipStreamNonBlocking));
            for (auto& ev : lanes_[i].copied) HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        }
    }
    // records per pool and chunk: the staging buffer is cut into D equal regions.  Tile-planar MXFP4 runs move as whole tiles
    // (the staged copy keeps every record's place inside its tile, so "pool address + delta" still finds nibbles and codes):
    // a chunk's records may begin and end inside a tile -- one tile of the region is kept for that
    const bool planar = planar_mx4(a->scheme);
    const uint64_t region = planar ? (stage_bytes_ / D) / kMx4TileBytes * kMx4TileBytes : (stage_bytes_ / D) / stride * stride;
    const uint64_t recs_per_region = planar ? (region / kMx4TileBytes >= 2 ? (region / kMx4TileBytes - 1) * kMx4TileRecs : 0) : region / stride;
    if (recs_per_region == 0) return SPECKV_ERR_NOMEM;
    const uint64_t chunk_pages = recs_per_region * D;     // logical pages per chunk (each pool gets <= recs_per_region of them)
    // the source records must be in place: everything queued on the engine stream (writes are synchronous) and on
    // the caller's stream so far is ordered before the first copy
    hipEvent_t start = get_event();
    if (!start) return SPECKV_ERR_DRIVER;
    HIP_TRY(hipEventRecord(start, st));
    uint64_t done = 0;
    int chunk = 0;
    while (done < n) {
        const uint64_t f0 = first + done, nc = std::min(chunk_pages, n - done);
        const int b = chunk & 1;
        CodecArgs c{};
        c.entries = a->d_entries;
        c.trusted = 1;
        c.first = f0;
        c.n = nc;
        c.data = static_cast<uint8_t*>(d_dst) + done * (f32 ? 2ull * kPageSize : kPageSize);
        c.data_stride = f32 ? 2ull * kPageSize : kPageSize;
        c.scheme = a->scheme;
        c.quant_mode = quant_mode_;
        c.out_f32 = f32 ? 1 : 0;
        c.structured_hint = hint;                            // (the flat-run decoder also reads staged records: k_fetch_decompress_flat_staged)
        c.stripe_n = D;
        c.stripe_magic = (1ull << 35) / D + 1;
        for (uint32_t k = 0; k < D; ++k) {
            uint64_t rb = 0, cnt = 0;
            shard_range(f0, nc, D, k, &rb, &cnt);
            c.stripe_delta[k] = 0;
            if (cnt == 0) continue;
            const int pool = a->pool_of_residue[k];
            // the byte run of this pool's records of the chunk: fixed slots, or -- sealed allocation -- the packed records
            // themselves (record rb of residue k is page rb * D + k; the run ends where the next record of the pool starts)
            const uint8_t* src;
            size_t run_bytes;
            if (packed) {
                const uint64_t p_first = rb * D + k, p_next = (rb + cnt) * D + k;
                const uint64_t lo = static_cast<uint64_t>(a->packed_off128[p_first]) << 7;
                const uint64_t hi = p_next < a->n_pages ? static_cast<uint64_t>(a->packed_off128[p_next]) << 7 : a->packed_bytes[k];
                src = static_cast<const uint8_t*>(a->extents[k].base) + lo;
                run_bytes = static_cast<size_t>(hi - lo);
            } else if (planar) {
                const uint64_t t0 = rb / kMx4TileRecs, t1 = (rb + cnt + kMx4TileRecs - 1) / kMx4TileRecs;
                src = static_cast<const uint8_t*>(a->extents[k].base) + t0 * kMx4TileBytes;
                run_bytes = static_cast<size_t>(t1 - t0) * kMx4TileBytes;
            } else {
                src = static_cast<const uint8_t*>(a->extents[k].base) + rb * stride;
                run_bytes = cnt * stride;
            }
            uint8_t* dstk = stage_[b] + k * region;
            c.stripe_delta[k] = static_cast<int64_t>(reinterpret_cast<intptr_t>(dstk) - reinterpret_cast<intptr_t>(src));
            if (run_bytes == 0) continue;                                   // (records of zero length: nothing to move)
            PeerLane& lane = lanes_[pool];
            if (chunk == 0) HIP_TRY(hipStreamWaitEvent(lane.s, start, 0));
            HIP_TRY(hipStreamWaitEvent(lane.s, stage_free_[b], 0));        // the decompression that last read this buffer
            HIP_TRY(hipMemcpyPeerAsync(dstk, device_, src, pools_[pool]->device(), run_bytes, lane.s));
            HIP_TRY(hipEventRecord(lane.copied[b], lane.s));
            HIP_TRY(hipStreamWaitEvent(st, lane.copied[b], 0));
            st_.copy_engine_bytes += run_bytes;
        }
        HIP_TRY(launch_decompress(c, st));
        HIP_TRY(hipEventRecord(stage_free_[b], st));
        done += nc;
        ++chunk;
    }
    put_event(start);
    st_.copy_engine_runs += static_cast<uint64_t>(chunk) * D;
    return SPECKV_OK;
}

int Engine::fetch_range(uint64_t handle, uint64_t first, uint64_t n, void* d_dst, bool f32, hipStream_t s, int engine_choice)
{
    if (null_) return no_data_path("speckv_ext_fetch_range");
    Allocation* a = find(handle);
    if (!a) return SPECKV_ERR_GENERAL;
    if (first > a->n_pages || n > a->n_pages - first) return SPECKV_ERR_GENERAL;
    if (!d_dst) return SPECKV_ERR_INVAL;
    if (engine_choice < 0 || engine_choice > 2) return SPECKV_ERR_INVAL;
    if (n == 0) return SPECKV_OK;
    DeviceScope device_scope(device_);
    if (!s) HIP_TRY(hipDeviceSynchronize());      // NULL = synchronous call on the engine's stream: d_dst may be in use on any stream
    hipStream_t st = s ? s : stream_;
    // which engine moves the records: the fused peer-load kernel (the wave loads the record over xGMI and
    // decompresses in registers) or the copy engines (SDMA runs into local staging, then a local decompress).
    // Per batch: long runs on remote pools go to the copy engines, short ones to the kernel; 1 / 2 force a choice
    // (SPECKV_REMOTE_ENGINE=kernel|copy overrides "auto").
    int choice = engine_choice ? engine_choice : tuning().remote_engine;
    const uint32_t D = static_cast<uint32_t>(a->pool_of_residue.size());
    const bool capturing = is_capturing(st);
    const bool can_copy = (a->regular || (a->packed && a->packed_regular)) && D >= 1 && D <= 8 && a->n_pages < (1ull << 28) && !capturing;
    if (choice == 0) {
        bool remote = false;
        for (int p : a->pool_of_residue) remote = remote || pools_[p]->device() != device_;
        const uint64_t min_run = static_cast<uint64_t>(tuning().copy_min_run_kb > 0 ? tuning().copy_min_run_kb : 1024) << 10;
        choice = (remote && can_copy && (n / D) * a->rec_stride >= min_run) ? 2 : 1;
    }
    if (choice == 2 && !can_copy) {
        if (engine_choice == 2) return SPECKV_ERR_INVAL;     // asked for explicitly on a placement that has no runs
        choice = 1;
    }
    if (choice == 2) {
        RC_TRY(fetch_range_copy_engine(a, first, n, d_dst, f32, st));
    } else {
        CodecArgs c{};
        c.entries = a->d_entries;
        c.trusted = 1;                       // pool records only ever come from k_compress
        c.first = first;
        c.n = n;
        c.data = static_cast<uint8_t*>(d_dst);
        c.data_stride = f32 ? 2ull * kPageSize : kPageSize;
        c.scheme = a->scheme;
        c.quant_mode = quant_mode_;
        c.out_f32 = f32 ? 1 : 0;
        if (a->packed && a->n_pages) {                       // sealed: the packed size is known -- short records take the flat-run decoder
            uint64_t packed = 0;
            for (uint64_t b : a->packed_bytes) packed += b;
            c.structured_hint = packed / a->n_pages < 512u ? 1 : 0;
        } else {                                             // never sealed: the compress kernel's own length samples
            c.structured_hint = looks_structured(a) ? 1 : 0;
        }
        if (c.structured_hint) st_.flat_decoder_fetches++;
        // the same range as this allocation's previous fetch is walked the other way, with stores that stay in the Infinity Cache
        // (fetch_sweep.hpp: what the last sweep wrote last is what the cache still holds); the state is kept once the launch is out
        const FetchSweepNext sweep = fetch_sweep_next(a->sweep, first, n, capturing, tuning().fetch_sweep);
        c.descending = sweep.descending;
        c.keep_stores = sweep.keep_stores;
        HIP_TRY(launch_decompress(c, st));
        a->sweep = sweep.state;
    }
    note_use(a, s);
    st_.dma_submitted += n;
    st_.total_decompressions += n;
    if (!s) {
        hipEvent_t ev = get_event();
        if (ev) { HIP_TRY(hipEventRecord(ev, stream_)); inflight_.push_back({ev, static_cast<uint32_t>(n)}); }
    } else {
        st_.dma_completed += n;            // completion belongs to the caller's stream
    }
    return SPECKV_OK;
}

int Engine::fetch_list(uint64_t handle, const uint32_t* d_pages, uint32_t n, void* d_dst, bool f32, hipStream_t s)
{
    if (null_) return no_data_path("speckv_ext_fetch_list");
    Allocation* a = find(handle);
    if (!a) return SPECKV_ERR_GENERAL;
    if (!d_dst || (!d_pages && n)) return SPECKV_ERR_INVAL;
    if (n == 0) return SPECKV_OK;
    DeviceScope device_scope(device_);
    if (!s) HIP_TRY(hipDeviceSynchronize());      // as in fetch_range
    CodecArgs c{};
    c.entries = a->d_entries;
    c.trusted = 1;                       // pool records only ever come from k_compress
    c.page_list = d_pages;
    c.n = n;
    c.data = static_cast<uint8_t*>(d_dst);
    c.data_stride = f32 ? 2ull * kPageSize : kPageSize;
    c.scheme = a->scheme;
    c.quant_mode = quant_mode_;
    c.out_f32 = f32 ? 1 : 0;
    hipStream_t st = s ? s : stream_;
    HIP_TRY(launch_decompress(c, st));
    note_use(a, s);
    st_.dma_submitted += n;
    st_.total_decompressions += n;
    if (!s) {
        hipEvent_t ev = get_event();
        if (ev) { HIP_TRY(hipEventRecord(ev, stream_)); inflight_.push_back({ev, n}); }
    } else {
        st_.dma_completed += n;
    }
    return SPECKV_OK;
}

} // namespace speckv
