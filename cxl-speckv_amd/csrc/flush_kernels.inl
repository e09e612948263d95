// cxl-speckv_amd/csrc/flush_kernels.inl -- prefetch lookup, the device-side prefetch flush and verify: k_prefetch_lookup,
// k_scan_totals, k_flush_candidates, k_flush_mark, k_flush_assign, k_flush_small, k_verify.
//
// A section of the translation unit kernels.hip, which includes it inside namespace speckv at the place where the text stood (why
// it is not a translation unit of its own yet: see there).  As one it would need
//   kernels.hpp        Layout, FlushArgs, FlushResult, kNoSlot and the launch declarations
//   codec_device.hpp   wave_incl_add
// and nothing of kernels.hip itself.  The launchers (launch_prefetch_lookup, launch_flush_pipeline, launch_verify) are still in
// kernels.hip, behind launch_compress: see the note there.

namespace {

// ===================================================================
// prefetch lookup  (prefetch_core.v:150-241 ; speckv_allocator.cpp:105-113)
// ===================================================================
// 32 lanes per request: lane c -> kind = c>>4, position cur_pos + (c&15) + 1.
// Pages of a position = pages covering its [head 0 .. head H-1] row in the
// shim layout; a lane emits only pages its predecessor lane did not cover.
struct Cand { uint32_t lo, hi; };   // half-open range of NEW pages of this lane (before residency filter)

__device__ __forceinline__ Cand candidate(const Layout& lay, uint32_t req, uint32_t layer,
                                          uint32_t pos, uint32_t depth, uint32_t c)
{
    Cand r{0u, 0u};
    const uint32_t kind = c >> 4, i = (c & 15u) + 1u;
    const uint64_t p = static_cast<uint64_t>(pos) + i;
    if (i > depth || p >= lay.num_tokens) return r;
    const uint64_t entry = static_cast<uint64_t>(lay.head_dim) * lay.bytes_per_element;
    const uint64_t row = entry * lay.num_heads;
    if (row == 0) return r;
    // vllm_speckv_backend.py:95-100 with head = 0
    const uint64_t off = ((((static_cast<uint64_t>(req) * lay.num_layers + layer) * 2 + kind)
                           * lay.num_tokens + p) * lay.num_heads) * entry;
    uint64_t pg0 = off / kPageSize;
    const uint64_t pg1 = (off + row - 1) / kPageSize;
    if (i > 1) {                       // predecessor position p-1 covered up to:
        const uint64_t prev_pg1 = (off - 1) / kPageSize;   // (off - row + row - 1)
        if (pg0 <= prev_pg1) pg0 = prev_pg1 + 1;
    }
    uint64_t hi = pg1 + 1;
    if (hi > lay.alloc_pages) hi = lay.alloc_pages;
    if (pg0 >= hi) return r;
    r.lo = static_cast<uint32_t>(pg0);
    r.hi = static_cast<uint32_t>(hi);
    return r;
}

template <bool WRITE>
__global__ __launch_bounds__(256) void k_prefetch_lookup(Layout lay, uint32_t n,
        const uint32_t* __restrict__ req, const uint32_t* __restrict__ layer,
        const uint32_t* __restrict__ pos, const uint32_t* __restrict__ depth,
        const uint32_t* __restrict__ flags, uint32_t* __restrict__ wave_tot,
        const uint32_t* __restrict__ wave_base, uint32_t* __restrict__ out, uint32_t cap)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t gw = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;   // global wave = 2 requests
    const uint32_t r = 2u * gw + (lane >> 5);
    uint32_t cnt = 0;
    Cand cd{0u, 0u};
    const bool live_wave = 2u * gw < n;
    if (r < n) {
        uint32_t dk = depth[r];
        if (dk > 16u) dk = 16u;
        cd = candidate(lay, req[r], layer[r], pos[r], dk, lane & 31u);
        for (uint32_t pg = cd.lo; pg < cd.hi; ++pg)
            cnt += (flags && (flags[pg] & 3u)) ? 0u : 1u;
    }
    const uint32_t incl = wave_incl_add(cnt);
    if (!WRITE) {
        if (lane == 63u && live_wave) wave_tot[gw] = incl;
    } else {
        uint32_t w = (live_wave ? wave_base[gw] : 0u) + incl - cnt;
        for (uint32_t pg = cd.lo; pg < cd.hi; ++pg)
            if (!(flags && (flags[pg] & 3u))) {
                if (w < cap) out[w] = pg;
                ++w;
            }
    }
}

// single-workgroup exclusive scan of the per-wave totals (n_w is small:
// requests/2); total is clamped to cap.
__global__ __launch_bounds__(1024) void k_scan_totals(const uint32_t* __restrict__ tot,
        uint32_t* __restrict__ base, uint32_t n_w, uint32_t* __restrict__ count, uint32_t cap)
{
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t running;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) running = 0;
    __syncthreads();
    for (uint32_t i0 = 0; i0 < n_w; i0 += 1024u) {
        const uint32_t i = i0 + threadIdx.x;
        const uint32_t v = (i < n_w) ? tot[i] : 0u;
        const uint32_t incl = wave_incl_add(v);
        if (lane == 63u) wsum[wave] = incl;
        __syncthreads();
        uint32_t wbase = 0;
        for (uint32_t w = 0; w < wave; ++w) wbase += wsum[w];
        const uint32_t run = running;
        if (i < n_w) base[i] = run + wbase + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023u) running = run + wbase + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = running < cap ? running : cap;
}

// ===================================================================
// device-side prefetch flush  (prefetch_core.v:150-241: the whole loop without the host)
// ===================================================================
// Candidate words live at a fixed stride: request r, lane c (kind, look-ahead step), word t -> index
// (r*32 + c)*W + t, kNoSlot when unused.  Request order = index order, so "first occurrence" of a page is the
// smallest index naming it: every valid candidate does atomicMax(stamp[page], key(index)) with
// key = epoch<<24 | (0xFFFFFF - index); the candidate whose key survives is the one kept.  Stamps of older
// flushes carry an older epoch and lose against any key of this one (the host clears them when the 8-bit epoch wraps).
__device__ __forceinline__ uint32_t flush_key(uint32_t epoch, uint32_t index) { return (epoch << 24) | (0xFFFFFFu - index); }

__device__ __forceinline__ void flush_candidates_of(const FlushArgs& a, uint32_t gt)      // gt: one thread per (request, lane)
{
    const uint32_t r = gt >> 5, c = gt & 31u;
    if (r >= a.n) return;
    const uint32_t row = a.row[r];
    Cand cd{0u, 0u};
    DevAlloc t{};
    if (row != kNoSlot) {
        t = a.tab[row];
        if (t.entries) {
            uint32_t dk = a.depth[r];
            if (dk > 16u) dk = 16u;
            cd = candidate(t.layout, a.req[r], a.layer[r], a.pos[r], dk, c);
        }
    }
    const uint32_t base = gt * a.W;
    for (uint32_t w = 0; w < a.W; ++w) {
        uint32_t pg = kNoSlot;
        if (cd.lo + w < cd.hi && !(t.d_flags[cd.lo + w] & 3u)) {
            pg = cd.lo + w;
            atomicMax(&t.stamp[pg], flush_key(a.epoch, base + w));
        }
        a.cand[base + w] = pg;
    }
}
__global__ __launch_bounds__(256) void k_flush_candidates(FlushArgs a) { flush_candidates_of(a, blockIdx.x * blockDim.x + threadIdx.x); }

// candidate word i names page `pg` of allocation row `row` and is the first occurrence of that page in the flush
__device__ __forceinline__ bool flush_keeps(const FlushArgs& a, uint32_t i, uint32_t total, uint32_t& pg, uint32_t& row)
{
    pg = kNoSlot; row = kNoSlot;
    if (i >= total) return false;
    pg = a.cand[i];
    if (pg == kNoSlot) return false;
    row = a.row[i / (32u * a.W)];
    return a.tab[row].stamp[pg] == flush_key(a.epoch, i);
}
// Entry `rank` of the flush lands in ring slot base + rank.  Everything about it that is pointer chasing --
// its record descriptor, the slot's previous owner and that owner's residency words, the new owner, the
// page's slot words on both sides -- is done here, one THREAD per page, so that the fetch launch is the plain
// list form (descriptor + destination per block) at the bulk kernel's occupancy.  Done by the fetch kernel
// itself, one WAVE per page with a chain of ~8 dependent loads each, the 122 880-page flush of a 256-sequence
// decode step spent 210 us in the fetch; the chain now runs 64 pages per wave.
// (The words are final before the data has landed: the host waits for the flight's `done` event before it
// trusts a page whose slot lies in the flight's run, Engine::wait_landed.)
__device__ __forceinline__ void flush_place(const FlushArgs& a, const FlushResult& res, uint32_t rank, uint32_t row, uint32_t pg)
{
    const uint32_t slot = res.base + rank;
    const DevAlloc t = a.tab[row];
    a.final_entry[rank] = t.entries[pg];
    a.final_dst[rank] = reinterpret_cast<uint64_t>(a.ring_base + static_cast<uint64_t>(slot) * kPageSize);
    const uint64_t prev = a.ring_owner[slot];
    const uint64_t me = (static_cast<uint64_t>(row) << 32) | pg;
    if (prev != kNoOwner && prev != me) {
        const DevAlloc tp = a.tab[prev >> 32];
        const uint32_t pp = static_cast<uint32_t>(prev);
        // the row may have been recycled for a smaller allocation since the slot was filled
        if (tp.entries && pp < tp.layout.alloc_pages && tp.d_slot[pp] == slot)    // still pointing here: the page leaves L2
            atomicAnd(&tp.d_flags[pp], ~2u);
    }
    a.ring_owner[slot] = me;
    t.d_slot[pg] = slot;
    if (a.final_host) a.final_host[rank] = &t.h_slot[pg];     // stored by the fetch launch (CodecArgs::host_words)
    else t.h_slot[pg] = res.seq + rank;                       // the page's only host-visible word (Engine::l2_live)
    atomicOr(&t.d_flags[pg], 2u);
}
// the ring run of a flush that keeps `total` candidates: [base, base+m), a run never wraps (as Engine::take_l2_run on the
// host: same rule, so host and device agree on the hand).  *a.hand is the ring's sequence number: slot = seq % n_l2; the
// slots a run skips at the end of a lap count.
__device__ __forceinline__ FlushResult flush_take(const FlushArgs& a, uint32_t total)
{
    const uint32_t m = total < a.max_take ? total : a.max_take;
    const RingRun run = ring_take(*a.hand, m, a.n_l2);
    if (m) *a.hand = run.next;
    const FlushResult r{m, run.slot, total, run.seq};
    *a.result_dev = r;
    *a.result_host = r;
    return r;
}

// keep[i] = candidate i is the first occurrence of its page; WRITE = false: totals per workgroup (256 candidates: the
// single-workgroup scan of k_flush_assign is 4x shorter than over per-wave totals), true: ordered scatter (rank = the
// workgroup's base from k_flush_assign + the kept candidates before this one in it)
template <bool WRITE>
__global__ __launch_bounds__(256) void k_flush_mark(FlushArgs a, const FlushResult* __restrict__ res)
{
    __shared__ uint32_t wcount[4];
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t total = a.n * 32u * a.W;
    uint32_t pg, row;
    const bool keep = flush_keeps(a, i, total, pg, row);
    const unsigned long long mask = __ballot(keep);
    if (lane == 0u) wcount[wave] = static_cast<uint32_t>(__popcll(mask));
    __syncthreads();
    if (!WRITE) {
        if (threadIdx.x == 0u) a.wave_tot[blockIdx.x] = wcount[0] + wcount[1] + wcount[2] + wcount[3];
    } else if (keep) {
        uint32_t before = 0;
        for (uint32_t w = 0; w < wave; ++w) before += wcount[w];
        const uint32_t n_b = (total + 255u) >> 8;
        const uint32_t rank = a.wave_tot[n_b + blockIdx.x] + before + static_cast<uint32_t>(__popcll(mask & ((1ull << lane) - 1ull)));
        if (rank < res->m) flush_place(a, *res, rank, row, pg);
    }
}

// one workgroup: exclusive scan of the wave totals, then the ring run [base, base+m) (a run never wraps, as
// Engine::take_l2_run on the host: same rule, so host and device agree on the hand)
__global__ __launch_bounds__(1024) void k_flush_assign(FlushArgs a)
{
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t running;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t n_w = (a.n * 32u * a.W + 255u) >> 8;       // totals per workgroup of k_flush_mark
    if (threadIdx.x == 0) running = 0;
    __syncthreads();
    for (uint32_t i0 = 0; i0 < n_w; i0 += 1024u) {
        const uint32_t i = i0 + threadIdx.x;
        const uint32_t v = (i < n_w) ? a.wave_tot[i] : 0u;
        const uint32_t incl = wave_incl_add(v);
        if (lane == 63u) wsum[wave] = incl;
        __syncthreads();
        uint32_t wbase = 0;
        for (uint32_t w = 0; w < wave; ++w) wbase += wsum[w];
        const uint32_t run = running;
        if (i < n_w) a.wave_tot[n_w + i] = run + wbase + incl - v;
        __syncthreads();
        if (threadIdx.x == 1023u) running = run + wbase + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) (void)flush_take(a, running);
}

// The whole pipeline in ONE workgroup for small flushes (the reference's own call pattern: speckv_prefetch per request and
// layer, flushed every num_layers requests -- 32 requests x 32 lanes x 2 words for an 8B-shaped model):
// four launches and their three hand-overs become phases between barriers; the kept flags stay in a register (one bit per
// pass of 1024 words), the counts per (pass, wave) in LDS.  Same arithmetic, same order of entries.
constexpr uint32_t kFlushSmallPasses = 16, kFlushSmallWords = kFlushSmallPasses * 1024u;
// measured on the MI355X (time until the pages have landed, W = 2): 4 .. 64 requests 38-42 us against 42-43 us for the four
// launches, 80 requests 54 against 45 (one workgroup then chases the pointers of ~500 pages alone); the host's submit time is
// 11-14 us against 19-23.  SPECKV_FLUSH_SMALL_WORDS moves the limit, SPECKV_FLUSH_NO_SMALL=1 removes the path.
// (Letting this kernel pull the request columns from the host's pinned slot itself, instead of the upload launch in front of
// it, saved the host another 2.5 us per flush and cost 4-5 us until landed, same box: 41.5-47 against 37.2-41.9.  Not kept.)
constexpr uint64_t kFlushSmallDefault = 4096;
__global__ __launch_bounds__(1024) void k_flush_small(FlushArgs a)
{
    __shared__ uint32_t wcnt[kFlushSmallPasses * 16u];      // kept candidates of (pass, wave) -> kept candidates before it
    __shared__ uint32_t s_part[4];
    __shared__ FlushResult s_res;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t total = a.n * 32u * a.W, passes = (total + 1023u) >> 10;
    for (uint32_t gt = tid; gt < a.n * 32u; gt += 1024u) flush_candidates_of(a, gt);
    __threadfence();                                        // the stamps' atomicMax and the candidate words are out
    __syncthreads();
    uint32_t keepbits = 0;
    for (uint32_t j = 0; j < passes; ++j) {
        uint32_t pg, row;
        const bool keep = flush_keeps(a, j * 1024u + tid, total, pg, row);
        const unsigned long long mask = __ballot(keep);
        if (lane == 0u) wcnt[j * 16u + wave] = static_cast<uint32_t>(__popcll(mask));
        keepbits |= (keep ? 1u : 0u) << j;
    }
    for (uint32_t e = passes * 16u + tid; e < kFlushSmallPasses * 16u; e += 1024u) wcnt[e] = 0u;
    __syncthreads();
    {   // exclusive scan of the 256 counts (entry order = candidate order) by the first four waves
        uint32_t v = 0, incl = 0;
        if (tid < 256u) { v = wcnt[tid]; incl = wave_incl_add(v); if (lane == 63u) s_part[wave] = incl; }
        __syncthreads();
        if (tid < 256u) {
            uint32_t before = 0;
            for (uint32_t w = 0; w < wave; ++w) before += s_part[w];
            wcnt[tid] = before + incl - v;
        }
        if (tid == 0u) s_res = flush_take(a, s_part[0] + s_part[1] + s_part[2] + s_part[3]);
        __syncthreads();
    }
    const FlushResult res = s_res;
    for (uint32_t j = 0; j < passes; ++j) {
        const bool keep = (keepbits >> j) & 1u;
        const unsigned long long mask = __ballot(keep);
        if (keep) {
            const uint32_t i = j * 1024u + tid;
            const uint32_t rank = wcnt[j * 16u + wave] + static_cast<uint32_t>(__popcll(mask & ((1ull << lane) - 1ull)));
            if (rank < res.m) flush_place(a, res, rank, a.row[i / (32u * a.W)], a.cand[i]);
        }
    }
}

// ===================================================================
// verify  (speculative_prefetcher.cpp:84-96): hit[r] = actual[r] in predicted[r][0..k)
// ===================================================================
// One request per lane; the 64-bit __ballot of the per-lane result is the
// wave's verify mask (its popcount feeds the hit counter).  A wave owns 64
// consecutive bytes of hit[] and a workgroup 256, so no two workgroups ever
// write into the same 128-byte line: the earlier layout (16 lanes per request,
// 4 result bytes per wave) let eight workgroups on eight XCDs share one line and
// showed rare wrong bytes on MI355X (tests/test_gpu_engine.py::test_verify_batch_kernel).
__global__ __launch_bounds__(256) void k_verify(uint32_t n, uint32_t k,
        const int32_t* __restrict__ actual, const int32_t* __restrict__ predicted,
        uint8_t* __restrict__ hit, uint32_t* __restrict__ hit_count)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    bool h = false;
    if (r < n) {
        const int32_t a = actual[r];
        const int32_t* p = predicted + static_cast<uint64_t>(r) * k;
        for (uint32_t j = 0; j < k; ++j) h = h || (p[j] == a);
        hit[r] = h ? 1 : 0;
    }
    const unsigned long long mask = __ballot(h);              // 64-bit verify mask of this wave
    if (lane == 0u && mask) atomicAdd(hit_count, static_cast<uint32_t>(__popcll(mask)));
}

} // namespace
