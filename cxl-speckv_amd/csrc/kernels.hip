// cxl-speckv_amd/csrc/kernels.hip -- hand-written CDNA4 (gfx950) kernels of the
// KV hot path.  This file: the block codec (k_fetch_decompress*, k_compress), its launch shape (num_cus, shape_launch) and
// launchers (launch_decompress, launch_compress).  The codec's device code -- decoders, encoders, compress_block -- is
// block_codec_device.hpp, which row_transfer.hip (the pair and slot kernels, a translation unit of their own) includes too.  The
// other subjects of this translation unit are included below the codec:
//   flush_kernels.inl        prefetch lookup, device-side prefetch flush, verify
//   page_table_kernels.inl   page-table upkeep
//   qk_scores_kernels.inl    query quantisation and q.K^T over FP8 records (stand-alone forms)
//   predictor_kernels.inl    the token predictor
//
// What they replace in the reference (paths under /root/reference):
//   FPGACacheEngine::compress / ::decompress   src/fpga_engine/cache_engine.cpp:40-116,172-284
//   (RTL twins hardware/rtl/kv_compress.v, kv_decompress.v)
//   prefetch_core lookup loop                  hardware/rtl/prefetch_core.v:150-241
//   SpeculativePrefetcher::handle_misprediction src/prefetcher/speculative_prefetcher.cpp:84-96
//
// Execution model.  These are HBM-bound byte kernels, not GEMMs: no MFMA.
// One wavefront (64 lanes) owns one 2048-element block; lane l holds elements
// [8l+512j, 8l+512j+8), j=0..3, so each global access is a coalesced 1 KiB
// instruction (16 B per lane).  The serial recurrences of the reference
// (run-length expand, int8 delta chain) become wave-level scans:
//   * run start positions   = exclusive add-scan of the run counts
//   * delta prefix at a run = exclusive add-scan (mod 256) of value*count,
//     carried in the top byte of the same 32-bit scan word
//   * "which run covers output p" = max-scan over a 2048-entry head table in
//     LDS into which every run scatters one word at its start position
// Scans are DPP (row_shr / row_bcast) inside the wave; there is no workgroup
// barrier anywhere, so wavefronts never wait for each other.
#include "kernels.hpp"
#include "tuning.hpp"
#include "ring_rule.hpp"
#include "block_codec_device.hpp"
#include "attend_device.hpp"         // f32x4 and pack64 of qk_scores_kernels.inl

#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace speckv {
namespace {

// One block's source/destination, all wave-uniform (lives in SGPRs: the block
// index is made provably uniform, so these are scalar loads through the K$).
struct BlockDesc {
    const uint8_t* rec;
    uint8_t* dst;
    uint64_t page;
    uint32_t len;
    float scale;
    uint32_t row;       // table row of the block's allocation (EXT 2: ring bookkeeping / multi-allocation launches)
};
// EXT selects what a launch needs beyond the plain forms, so that the bulk path keeps its register budget
// (62 VGPRs, no SGPR spills, 8 waves per SIMD):
//   0  page table / raw records, range or list            (speckv_ext_fetch_range / _list, codec operators)
//   1  + records staged by the copy engines               (stripe_delta)
//   2  + blocks of several allocations, L2-ring bookkeeping (synchronous misses, device-side flush)
//   3  form 0 + one host-visible word per block (the fetch launch of a device-side flush)
template <int EXT>
__device__ __forceinline__ BlockDesc load_desc(const CodecArgs& a, uint64_t i, uint32_t slot0)
{
    BlockDesc d;
    d.page = a.page_list ? a.page_list[i] : a.first + i;
    d.row = 0;
    const PageEntry* entries = a.entries;
    if (EXT == 2) {
        d.row = a.alloc_list ? a.alloc_list[i] : a.alloc_idx;
        if (a.alloc_list) entries = a.tab[d.row].entries;
    }
    if (EXT == 2 || entries) {
        PageEntry e{0, 0, 1.0f};
        if (entries) e = entries[d.page];                  // a row freed meanwhile decodes as a never-written page
        d.rec = reinterpret_cast<const uint8_t*>(e.pool_addr);
        d.len = e.rec_bytes;
        d.scale = e.scale;
        if (EXT == 1) {                                    // staged copy of the record (copy-engine fetch)
            const uint64_t q = (d.page * a.stripe_magic) >> 35;        // page / stripe_n without a divide (page < 2^28)
            d.rec += a.stripe_delta[d.page - q * a.stripe_n];
        }
    } else {
        d.rec = a.recs + d.page * a.rec_stride;
        d.len = a.rec_bytes[d.page];
        d.scale = a.scales ? a.scales[d.page] : 1.0f;
    }
    if (EXT == 2 && a.ring_owner) d.dst = a.ring_base + (static_cast<uint64_t>(slot0) + i) * kPageSize;
    else d.dst = a.data_list ? reinterpret_cast<uint8_t*>(a.data_list[i]) : a.data + i * a.data_stride;
    return d;
}

// Ring bookkeeping of one fetched block (one lane): see CodecArgs::ring_owner.  Device side: the slot's previous owner
// loses its L2 bit, the new owner is recorded.  Host side: ONE store, the page's ring sequence number -- the host derives
// "still in the ring" from it (Engine::l2_live), so evictions need no host-visible store.  (Every 4-byte store to pinned
// memory is a PCIe transaction of its own: with slot, flags and the evicted page's flags stored per block, a flush of
// 19 000 blocks ran at the link's transaction rate -- 70 us against 42 us without the stores, 47 us with one.)
//
// In two halves, because a miss of one page is nothing but dependent round trips (profiles/r05_access_miss.txt: the kernel
// was 6.3 us of a 12.5 us miss -- page entry, record, then owner word, owner's table row, owner's slot word, own table row,
// one after another behind the decode).  ring_look reads what the bookkeeping needs BEFORE the block is decoded, in three
// steps of wave-uniform loads: {page entry, the slot's previous owner}, {that owner's table row, this block's row}, {the
// owner's slot word}; the last one is an ordinary load that the record's own loads follow without a wait in between.
// ring_note (one lane, after the decode) only stores.  The first two steps are scalar loads written out by hand, each
// statement ending in its own s_waitcnt: left to the compiler the chain becomes vector loads behind branches, every one
// waited for before the next and before the record (the words are written by kernels, so it will not pick scalar loads
// itself; the scalar cache is invalidated when a kernel starts, and within a launch a wave only reads words that no
// other wave of the launch writes, the previous owner's slot word aside -- which is read by a coherent vector load).
struct RingLook {
    uint32_t* evict_flags;      // previous owner's flag word, or nullptr: nothing to evict
    uint32_t  their_slot;       // previous owner's slot word (compared in ring_note: the load stays in flight over the decode)
    uint32_t* d_flags;          // this block's allocation (nullptr: row freed meanwhile)
    uint32_t* d_slot;
    uint32_t* h_slot;
};
typedef uint32_t sgpr4 __attribute__((ext_vector_type(4)));
typedef uint64_t sgpr8 __attribute__((ext_vector_type(4)));     // four pointers: entries, d_flags, d_slot, h_slot (DevAlloc)
// load_desc_ring reads these structs with hand-written scalar loads: one s_load_dwordx4 = a PageEntry {address, bytes, scale}, one
// s_load_dwordx8 = the first four pointers of a DevAlloc row, one s_load_dwordx2 = Layout::alloc_pages.  A reordered or resized
// field would silently defeat the `pp < their_pages` bound and send the atomicAnd on d_flags out of bounds: the layout
// the assembly assumes is pinned here.  (-DSPECKV_RING_VECTOR_LOADS builds the same function from plain loads, for debugging.)
static_assert(sizeof(PageEntry) == 16 && offsetof(PageEntry, pool_addr) == 0 && offsetof(PageEntry, rec_bytes) == 8 && offsetof(PageEntry, scale) == 12,
              "load_desc_ring: s_load_dwordx4 of a PageEntry");
static_assert(offsetof(DevAlloc, entries) == 0 && offsetof(DevAlloc, d_flags) == 8 && offsetof(DevAlloc, d_slot) == 16 && offsetof(DevAlloc, h_slot) == 24,
              "load_desc_ring: s_load_dwordx8 of a DevAlloc row = {entries, d_flags, d_slot, h_slot}");
static_assert(sizeof(Layout::alloc_pages) == 8 && (offsetof(DevAlloc, layout) + offsetof(Layout, alloc_pages)) % 8 == 0,
              "load_desc_ring: s_load_dwordx2 of Layout::alloc_pages");
__device__ __forceinline__ BlockDesc load_desc_ring(const CodecArgs& a, uint64_t i, uint32_t slot0, RingLook& r)
{
    BlockDesc d;
    d.page = a.page_list ? a.page_list[i] : a.first + i;
    d.row = a.alloc_idx;
    const uint32_t slot = slot0 + static_cast<uint32_t>(i);
    d.dst = a.ring_base + static_cast<uint64_t>(slot) * kPageSize;
    const uint64_t me = (static_cast<uint64_t>(d.row) << 32) | d.page;
    const uint64_t* owner_word = a.ring_owner + slot;
    const DevAlloc* mine = a.tab + d.row;
    uint64_t prev;
    sgpr4 e = {0u, 0u, 0u, 0x3f800000u};
#ifdef SPECKV_RING_VECTOR_LOADS
    if (a.entries) { const PageEntry pe = a.entries[d.page]; e = sgpr4{static_cast<uint32_t>(pe.pool_addr), static_cast<uint32_t>(pe.pool_addr >> 32), pe.rec_bytes, __float_as_uint(pe.scale)}; }
    prev = __hip_atomic_load(owner_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#else
    if (a.entries) {
        const PageEntry* ep = a.entries + d.page;
        asm volatile("s_load_dwordx4 %0, %2, 0x0\n\ts_load_dwordx2 %1, %3, 0x0\n\ts_waitcnt lgkmcnt(0)"
                     : "=&s"(e), "=&s"(prev) : "s"(ep), "s"(owner_word) : "memory");
    } else {                                                 // a row freed meanwhile decodes as a never-written page
        asm volatile("s_load_dwordx2 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=&s"(prev) : "s"(owner_word) : "memory");
    }
#endif
    d.rec = reinterpret_cast<const uint8_t*>((static_cast<uint64_t>(e.y) << 32) | e.x);
    d.len = e.z;
    d.scale = __uint_as_float(e.w);
    const bool other = prev != kNoOwner && prev != me;
    const DevAlloc* theirs = other ? a.tab + (prev >> 32) : mine;
    sgpr8 tp, mp;
    uint64_t their_pages;
#ifdef SPECKV_RING_VECTOR_LOADS
    tp = sgpr8{reinterpret_cast<uint64_t>(theirs->entries), reinterpret_cast<uint64_t>(theirs->d_flags), reinterpret_cast<uint64_t>(theirs->d_slot), reinterpret_cast<uint64_t>(theirs->h_slot)};
    mp = sgpr8{reinterpret_cast<uint64_t>(mine->entries), reinterpret_cast<uint64_t>(mine->d_flags), reinterpret_cast<uint64_t>(mine->d_slot), reinterpret_cast<uint64_t>(mine->h_slot)};
    their_pages = theirs->layout.alloc_pages;
#else
    asm volatile("s_load_dwordx8 %0, %3, 0x0\n\ts_load_dwordx2 %1, %3, %5\n\ts_load_dwordx8 %2, %4, 0x0\n\ts_waitcnt lgkmcnt(0)"
                 : "=&s"(tp), "=&s"(their_pages), "=&s"(mp) : "s"(theirs), "s"(mine),
                   "i"(offsetof(DevAlloc, layout) + offsetof(Layout, alloc_pages)) : "memory");
#endif
    const uint32_t pp = static_cast<uint32_t>(prev);
    // the row may have been recycled for a smaller allocation since the slot was filled
    const bool in_row = other && tp.x != 0 && pp < their_pages;
    const uint32_t* word = in_row ? reinterpret_cast<const uint32_t*>(tp.z) + pp : reinterpret_cast<const uint32_t*>(owner_word);
    r.their_slot = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    r.evict_flags = in_row ? reinterpret_cast<uint32_t*>(tp.y) + pp : nullptr;
    r.d_flags = mp.x != 0 ? reinterpret_cast<uint32_t*>(mp.y) : nullptr;
    r.d_slot = reinterpret_cast<uint32_t*>(mp.z);
    r.h_slot = reinterpret_cast<uint32_t*>(mp.w);
    return d;
}
__device__ __forceinline__ void ring_note(const CodecArgs& a, const BlockDesc& d, const RingLook& r, uint32_t slot, uint32_t seq)
{
    if (r.evict_flags && r.their_slot == slot) atomicAnd(r.evict_flags, ~2u);      // still pointing here: the page leaves L2
    a.ring_owner[slot] = (static_cast<uint64_t>(d.row) << 32) | d.page;
    if (!r.d_flags) return;
    r.d_slot[d.page] = slot;
    r.h_slot[d.page] = seq;
    atomicOr(&r.d_flags[d.page], 2u);
}

// where a block's image goes: the plain forms choose their store policy per launch (ImageSink), the others keep the bare pointer
template <int EXT> struct FetchDst { typedef uint8_t* type; };
template <> struct FetchDst<0> { typedef ImageSink type; };
template <int EXT> __device__ __forceinline__ typename FetchDst<EXT>::type fetch_dst(uint8_t* p, uint32_t) { return p; }
template <> __device__ __forceinline__ ImageSink fetch_dst<0>(uint8_t* p, uint32_t keep) { return ImageSink{p, keep}; }

template <int SCHEME, int MODE, bool F32, int EXT, bool FLAT>
__device__ __forceinline__ void fetch_decompress_body(const CodecArgs& a)
{
    typedef typename FetchDst<EXT>::type Dst;
    __shared__ __attribute__((aligned(16))) uint32_t lds[SCHEME == kInt8DeltaRle ? kWaves * kDecLdsWords : 4];
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    uint64_t n = a.n;
    if (a.n_dev) { const uint64_t nd = *a.n_dev; n = nd < n ? nd : n; }
    uint32_t slot0 = 0, seq0 = 0;
    if (EXT == 2) {
        slot0 = a.slot0_dev ? *a.slot0_dev : a.slot0;
        seq0 = a.seq0_dev ? *a.seq0_dev : a.seq0;
        if (a.hand_ptr && blockIdx.x == 0 && threadIdx.x == 0) *a.hand_ptr = a.new_hand;
    }
    if (EXT == 3) seq0 = *a.seq0_dev;
    // a wave's blocks: one, or (launches beyond the grid cap) `per_wave` of them, one grid apart (wave_step) or
    // consecutive (SPECKV_ROUNDS=consecutive); see codec_launch_shape
    const uint64_t per_wave = a.per_wave ? a.per_wave : 1;
    const uint64_t gw = static_cast<uint64_t>(blockIdx.x) * kWaves + wave;
    const uint64_t step = a.wave_step ? a.wave_step : 1;                  // 1: consecutive blocks, else one per round
    uint64_t i = a.wave_step ? gw : gw * per_wave;
    uint64_t end = a.wave_step ? n : ((i + per_wave < n) ? i + per_wave : n);
    if (i >= n) return;
    const bool ring = EXT == 2 && a.ring_owner;                          // (launch-uniform)
    RingLook look{};
    BlockDesc cur{};
    // EXT 0 only (launch_dec2 refuses the others): a descending launch decodes block n - 1 - i where an ascending one decodes i --
    // the same waves, rounds and strides, the range walked from its top (fetch_sweep.hpp: why)
    const bool down = EXT == 0 && a.descending;                          // (launch-uniform)
    if (!ring) cur = load_desc<EXT>(a, down ? n - 1 - i : i, slot0);
    for (;;) {
        // the next block's descriptor is fetched while this block is decoded (ring form: in front of its own decode,
        // these launches are short and wait on one block's chain of loads, not on throughput -- and inside the loop:
        // a load issued in front of it is waited for there, whatever uses it)
        if (ring) cur = load_desc_ring(a, i, slot0, look);
        const uint64_t nx = i + step;
        BlockDesc nxt = cur;
        if (nx < end && !ring) nxt = load_desc<EXT>(a, down ? n - 1 - nx : nx, slot0);
        uint32_t len = cur.len;
        const Dst dst = fetch_dst<EXT>(cur.dst, a.keep_stores);
        if (SCHEME == kInt8DeltaRle) {
            if (len > 2u * kBlockElems) len = 2u * kBlockElems;
            uint32_t* region = lds + wave * kDecLdsWords;
            if (!decode_rle_fast<MODE, F32, FLAT, Dst>(cur.rec, len, cur.scale, dst, reinterpret_cast<uint8_t*>(region), lane,
                                                       a.trusted != 0))
                decode_rle_general<MODE, F32>(cur.rec, len, cur.scale, cur.dst, lane);
        } else if (SCHEME == kInt8) {
            if (len > kBlockElems) len = kBlockElems;
            decode_int8<MODE, F32, Dst>(cur.rec, len, cur.scale, dst, lane);
        } else if (SCHEME == kInt4G32) {
            decode_int4<F32, Dst>(cur.rec, len, dst, lane);
        } else if (SCHEME == kMxFp4) {
            // pool records are tile-planar: the codes lie mx4_code_delta behind the nibbles (the entry's scale word); raw records: 1024
            decode_mx4<F32, Dst>(cur.rec, cur.rec + (a.recs ? 1024u : __float_as_uint(cur.scale)), len, dst, lane);
        } else if (SCHEME == kFp8E4m3) {
            if (len > kBlockElems) len = kBlockElems;
            decode_fp8<F32, Dst>(cur.rec, len, cur.scale, dst, lane);
        } else {
            if (len > 2u * kBlockElems) len = 2u * kBlockElems;
            decode_fp16<F32, Dst>(cur.rec, len, dst, lane);
        }
        if (lane == 0u) {
            if (ring) ring_note(a, cur, look, slot0 + static_cast<uint32_t>(i), seq0 + static_cast<uint32_t>(i));
            else if (EXT == 3) *a.host_words[i] = seq0 + static_cast<uint32_t>(i);
            else if (a.flags) atomicOr(&a.flags[cur.page], a.set_flags);   // neighbours belong to other waves / XCDs
        }
        if (nx >= end) break;
        cur = nxt;
        i = nx;
    }
    if (EXT == 2 && a.done_flag) {                                      // (launch-uniform; one block per wave: n waves had work)
        __threadfence_system();                                          // the page, its residency words and the host-visible word are out
        if (n == 1u) {                                                   // the lone wave has nobody to count
            if (lane == 0u) __hip_atomic_store(a.done_flag, a.done_token, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        } else if (lane == 0u && atomicAdd(a.done_count, 1u) + 1u == static_cast<uint32_t>(n)) {
            *a.done_count = 0u;
            __hip_atomic_store(a.done_flag, a.done_token, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}
template <int SCHEME, int MODE, bool F32, int EXT>
__global__ __launch_bounds__(kThreads) void k_fetch_decompress(CodecArgs a) { fetch_decompress_body<SCHEME, MODE, F32, EXT, false>(a); }
// the FLAT instantiation (data known to compress) as a kernel of its own: these launches are store-bound with short waves, and
// a wave slot more or less per SIMD shows (all-zero blocks 86 us at 8 waves per SIMD, 93 us at 7: the compiler is told to stay at 8)
template <int MODE>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_fetch_decompress_flat(CodecArgs a)
{
    fetch_decompress_body<kInt8DeltaRle, MODE, false, 0, true>(a);
}
template <int MODE>
__global__ __launch_bounds__(kThreads) void k_fetch_decompress_flat_f32(CodecArgs a) { fetch_decompress_body<kInt8DeltaRle, MODE, true, 0, true>(a); }
// ... and for records the copy engines staged (EXT 1: a remote pool's allocation that compresses)
template <int MODE>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_fetch_decompress_flat_staged(CodecArgs a)
{
    fetch_decompress_body<kInt8DeltaRle, MODE, false, 1, true>(a);
}
template <int MODE>
__global__ __launch_bounds__(kThreads) void k_fetch_decompress_flat_f32_staged(CodecArgs a) { fetch_decompress_body<kInt8DeltaRle, MODE, true, 1, true>(a); }

// The encoder of contiguous 4 KiB images: which block a wave owns, then compress_block (block_codec_device.hpp) from a SrcRun.
template <int SCHEME, int MODE>
__global__ __launch_bounds__(kThreads) void k_compress(CodecArgs a)
{
    SPECKV_ENC_LDS(SCHEME);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = threadIdx.x >> 6;
    const uint64_t n = a.n;
    const uint64_t per_wave = a.per_wave ? a.per_wave : 1;       // blocks per wave: see k_fetch_decompress
    const uint64_t gw = static_cast<uint64_t>(blockIdx.x) * kWaves + wave;
    const uint64_t step = a.wave_step ? a.wave_step : 1;
    const uint64_t i0 = a.wave_step ? gw : gw * per_wave;
    const uint64_t i1 = a.wave_step ? n : ((i0 + per_wave < n) ? i0 + per_wave : n);
    for (uint64_t i = i0; i < i1; i += step) {
        uint64_t page = a.page_list ? a.page_list[i] : a.first + i * (a.page_step ? a.page_step : 1);
        const uint8_t* src = a.data_list ? reinterpret_cast<const uint8_t*>(a.data_list[i])
                                         : a.data + i * a.data_stride;
        EncTarget t{a.entries, a.scale_tab, a.region_pages, a.scale_run, a.len_samples, a.recs, a.rec_stride, a.rec_bytes, a.scales};
        if (a.groups) {                                              // wave-uniform: this block's allocation
            const uint64_t gi = i / a.group_n, j = i - gi * a.group_n;
            const CompressGroup g = a.groups[gi];
            t.entries = g.entries; t.scale_tab = g.scale_tab; t.region_pages = g.region_pages; t.scale_run = g.scale_run;
            page = g.first + j * (a.page_step ? a.page_step : 1);
            src = g.data + j * a.data_stride;
        }
        compress_block<SCHEME, MODE>(t, page, SrcRun{src}, lds, lane, wave);
    }
}
} // namespace

// ===================================================================
// the other subjects of this translation unit, each in a file of its own, in the order in which their text stood here
// ===================================================================
// The compiler emits the kernels of a translation unit in the order of their definitions -- the instances of a kernel template in
// the order in which the launchers first name them -- and k_fetch_decompress calls decode_rle_general pc-relatively across all of
// them.  The headline kernel is pinned by the hash of its instructions (tests/test_build_guards.py), that call's literal
// included, so these sections are cut out of the file, not out of the translation unit, and nothing below changes its order.
#include "flush_kernels.inl"
#include "page_table_kernels.inl"
#include "qk_scores_kernels.inl"
#include "predictor_kernels.inl"

namespace {

// (k_repack and k_retarget_entries are page-table upkeep and belong to page_table_kernels.inl by subject, as k_copy16 further
// down does.  They stay where they are defined: in front of the predictor's kernels they would change the order of the code
// object.  With them stay their launchers, which need the definitions.)
// Records move to new places (compaction into packed extents and back): one wave per page copies the record's bytes, rounded up
// to 16 (k_compress zero-pads a record's last 16-byte piece), then re-points the page's table entry.
__global__ __launch_bounds__(256) void k_repack(PageEntry* __restrict__ entries, const uint64_t* __restrict__ new_addr, uint64_t n)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t p = (static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x) >> 6;
    if (p >= n) return;
    const PageEntry e = entries[p];
    const uint8_t* src = reinterpret_cast<const uint8_t*>(e.pool_addr);
    uint8_t* dst = reinterpret_cast<uint8_t*>(new_addr[p]);
    const uint32_t bytes = (e.rec_bytes + 15u) & ~15u;
    for (uint32_t b = 16u * lane; b < bytes; b += 1024u) st16(dst + b, ld16(src + b));
    if (lane == 0u) entries[p].pool_addr = new_addr[p];
}

__global__ void k_retarget_entries(PageEntry* e, uint64_t n, uint64_t base, uint64_t stride, uint64_t rec0)
{
    const uint64_t i = static_cast<uint64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (stride == kPlanarMx4) { e[i].pool_addr = base + mx4_nib_off(rec0 + i); e[i].scale = __uint_as_float(mx4_code_delta(rec0 + i)); }
    else e[i].pool_addr = base + i * stride;
}

int g_cus = 0;
int num_cus()
{
    if (g_cus == 0) {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) == hipSuccess &&
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0)
            g_cus = cus;
        else
            g_cus = 256;
    }
    return g_cus;
}
// Launch shape: the rule is codec_launch_shape (codec_launch_shape.hpp: the grid cap, the rounds, strided or consecutive, with the
// measurements behind them) under the tuning in force (wgs_per_cu, rounds_consecutive).  Every block-codec launch is sized HERE: the
// grid is returned, CodecArgs::per_wave / wave_step are filled in for the kernels' loops.
uint32_t shape_launch(CodecArgs& a)
{
    const CodecLaunchShape sh = codec_launch_shape_now(a.n, 0);
    a.per_wave = sh.per_wave;
    a.wave_step = sh.wave_step;
    return sh.grid;
}

template <int SCHEME, int MODE>
hipError_t launch_dec2(const CodecArgs& a_in, hipStream_t s)
{
    CodecArgs a = a_in;
    const uint32_t grid = shape_launch(a);
    const int ext = a.host_words ? 3 : (a.alloc_list || a.ring_owner) ? 2 : a.stripe_n ? 1 : 0;
    if (ext == 2 && a.stripe_n) return hipErrorInvalidValue;
    if (a.ring_owner && a.alloc_list) return hipErrorInvalidValue;      // the ring form reads one allocation's row (load_desc_ring)
    if (a.done_flag && (ext != 2 || a.per_wave > 1 || a.n_dev || !a.done_count)) return hipErrorInvalidValue;
    if (ext == 3 && (a.out_f32 || a.alloc_list || a.ring_owner || a.stripe_n || !a.seq0_dev || !a.data_list)) return hipErrorInvalidValue;
    if ((a.descending || a.keep_stores) && ext != 0) return hipErrorInvalidValue;      // staged, ring and host-word forms: their block index carries slot and sequence meaning
#define SPECKV_LAUNCH_DEC(F32, EXT) \
    hipLaunchKernelGGL((k_fetch_decompress<SCHEME, MODE, F32, EXT>), dim3(grid), dim3(kThreads), 0, s, a)
    if (SCHEME == kInt8DeltaRle && a.structured_hint && ext <= 1) {      // data known to compress: the FLAT instantiation (plain and copy-engine-staged forms)
        if (a.out_f32 && ext == 0) hipLaunchKernelGGL((k_fetch_decompress_flat_f32<MODE>), dim3(grid), dim3(kThreads), 0, s, a);
        else if (a.out_f32)        hipLaunchKernelGGL((k_fetch_decompress_flat_f32_staged<MODE>), dim3(grid), dim3(kThreads), 0, s, a);
        else if (ext == 0)         hipLaunchKernelGGL((k_fetch_decompress_flat<MODE>), dim3(grid), dim3(kThreads), 0, s, a);
        else                       hipLaunchKernelGGL((k_fetch_decompress_flat_staged<MODE>), dim3(grid), dim3(kThreads), 0, s, a);
        return hipGetLastError();
    }
    if (a.out_f32) { if (ext == 2) SPECKV_LAUNCH_DEC(true, 2); else if (ext == 1) SPECKV_LAUNCH_DEC(true, 1); else SPECKV_LAUNCH_DEC(true, 0); }
    else           { if (ext == 3) SPECKV_LAUNCH_DEC(false, 3); else if (ext == 2) SPECKV_LAUNCH_DEC(false, 2); else if (ext == 1) SPECKV_LAUNCH_DEC(false, 1); else SPECKV_LAUNCH_DEC(false, 0); }
#undef SPECKV_LAUNCH_DEC
    return hipGetLastError();
}
template <int SCHEME>
hipError_t launch_dec1(const CodecArgs& a, hipStream_t s)
{
    return a.quant_mode == kIntent ? launch_dec2<SCHEME, kIntent>(a, s) : launch_dec2<SCHEME, kRefExact>(a, s);
}
template <int SCHEME>
hipError_t launch_enc1(const CodecArgs& a, uint32_t grid, hipStream_t s)
{
    if (a.quant_mode == kIntent) hipLaunchKernelGGL((k_compress<SCHEME, kIntent>), dim3(grid), dim3(kThreads), 0, s, a);
    else                         hipLaunchKernelGGL((k_compress<SCHEME, kRefExact>), dim3(grid), dim3(kThreads), 0, s, a);
    return hipGetLastError();
}

} // namespace

CodecLaunchShape codec_launch_shape_now(uint64_t n, uint32_t n_cus)
{
    return codec_launch_shape(n, n_cus ? n_cus : static_cast<uint32_t>(num_cus()), tuning().wgs_per_cu, tuning().rounds_consecutive != 0,
                              static_cast<uint32_t>(kWaves));
}

hipError_t launch_decompress(const CodecArgs& a, hipStream_t s)
{
    if (a.n == 0) return hipSuccess;
    switch (a.scheme) {
    case kFp16: return launch_dec1<kFp16>(a, s);
    case kInt8: return launch_dec1<kInt8>(a, s);
    case kInt8DeltaRle: return launch_dec1<kInt8DeltaRle>(a, s);
    case kInt4G32: return launch_dec2<kInt4G32, kRefExact>(a, s);      // the quantiser mode does not apply
    case kFp8E4m3: return launch_dec2<kFp8E4m3, kRefExact>(a, s);
    case kMxFp4: return launch_dec2<kMxFp4, kRefExact>(a, s);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_compress(const CodecArgs& a, hipStream_t s)
{
    if (a.n == 0) return hipSuccess;
    CodecArgs b = a;
    const uint32_t grid = shape_launch(b);
    switch (b.scheme) {
    case kFp16: return launch_enc1<kFp16>(b, grid, s);
    case kInt8: return launch_enc1<kInt8>(b, grid, s);
    case kInt8DeltaRle: return launch_enc1<kInt8DeltaRle>(b, grid, s);
    case kInt4G32:                                                     // (these three: the quantiser mode does not apply)
        hipLaunchKernelGGL((k_compress<kInt4G32, kRefExact>), dim3(grid), dim3(kThreads), 0, s, b);
        return hipGetLastError();
    case kFp8E4m3:
        hipLaunchKernelGGL((k_compress<kFp8E4m3, kRefExact>), dim3(grid), dim3(kThreads), 0, s, b);
        return hipGetLastError();
    case kMxFp4:
        hipLaunchKernelGGL((k_compress<kMxFp4, kRefExact>), dim3(grid), dim3(kThreads), 0, s, b);
        return hipGetLastError();
    default: return hipErrorInvalidValue;
    }
}

// The launchers of flush_kernels.inl.  They stay behind launch_compress: they are the first to name k_prefetch_lookup<> and
// k_flush_mark<>, and in front of it those instances would be emitted ahead of the k_compress<> instances launch_compress names.
hipError_t launch_prefetch_lookup(const Layout& lay, uint32_t n, const uint32_t* d_req,
                                  const uint32_t* d_layer, const uint32_t* d_pos,
                                  const uint32_t* d_k, const uint32_t* d_flags, uint32_t* d_out,
                                  uint32_t cap, uint32_t* d_count, uint32_t* d_scratch,
                                  hipStream_t s)
{
    if (n == 0) return hipMemsetAsync(d_count, 0, sizeof(uint32_t), s);
    const uint32_t n_w = (n + 1u) / 2u;                 // 2 requests per wave
    uint32_t* tot = d_scratch;
    uint32_t* base = d_scratch + n_w;
    const uint32_t grid = (n_w * 64u + 255u) / 256u;
    hipLaunchKernelGGL((k_prefetch_lookup<false>), dim3(grid), dim3(256), 0, s, lay, n, d_req, d_layer,
                       d_pos, d_k, d_flags, tot, static_cast<const uint32_t*>(nullptr),
                       static_cast<uint32_t*>(nullptr), cap);
    hipLaunchKernelGGL(k_scan_totals, dim3(1), dim3(1024), 0, s, tot, base, n_w, d_count, cap);
    hipLaunchKernelGGL((k_prefetch_lookup<true>), dim3(grid), dim3(256), 0, s, lay, n, d_req, d_layer,
                       d_pos, d_k, d_flags, static_cast<uint32_t*>(nullptr), base, d_out, cap);
    return hipGetLastError();
}

hipError_t launch_flush_pipeline(const FlushArgs& a, hipStream_t s)
{
    if (a.n == 0 || a.W == 0) return hipErrorInvalidValue;
    const uint64_t total = static_cast<uint64_t>(a.n) * 32u * a.W;
    if (total >= (1ull << 24)) return hipErrorInvalidValue;        // the dedupe key carries 24 index bits
    // (test switches, tuning.hpp: the four-launch pipeline for every size / another limit for the one-workgroup form)
    const bool no_small = tuning().flush_no_small != 0;
    const uint64_t small_words = tuning().flush_small_words > 0 ? std::min<uint64_t>(static_cast<uint64_t>(tuning().flush_small_words), kFlushSmallWords) : kFlushSmallDefault;
    if (total <= small_words && !no_small) {
        hipLaunchKernelGGL(k_flush_small, dim3(1), dim3(1024), 0, s, a);
        return hipGetLastError();
    }
    const uint32_t g_lane = static_cast<uint32_t>((static_cast<uint64_t>(a.n) * 32u + 255u) / 256u);
    const uint32_t g_word = static_cast<uint32_t>((total + 255u) / 256u);
    hipLaunchKernelGGL(k_flush_candidates, dim3(g_lane), dim3(256), 0, s, a);
    hipLaunchKernelGGL((k_flush_mark<false>), dim3(g_word), dim3(256), 0, s, a, static_cast<const FlushResult*>(nullptr));
    hipLaunchKernelGGL(k_flush_assign, dim3(1), dim3(1024), 0, s, a);
    hipLaunchKernelGGL((k_flush_mark<true>), dim3(g_word), dim3(256), 0, s, a, static_cast<const FlushResult*>(a.result_dev));
    return hipGetLastError();
}

hipError_t launch_verify(uint32_t n, uint32_t k, const int32_t* d_actual,
                         const int32_t* d_predicted, uint8_t* d_hit, uint32_t* d_hit_count,
                         hipStream_t s)
{
    hipError_t e = hipMemsetAsync(d_hit_count, 0, sizeof(uint32_t), s);
    if (e != hipSuccess || n == 0) return e;
    if (k == 0 || k > 64u) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_verify, dim3((n + 255u) / 256u), dim3(256), 0, s, n, k, d_actual, d_predicted, d_hit,
                       d_hit_count);
    return hipGetLastError();
}

hipError_t launch_repack(PageEntry* d_entries, const uint64_t* d_new_addr, uint64_t n, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_repack, dim3(static_cast<uint32_t>((n + 3u) / 4u)), dim3(256), 0, s, d_entries, d_new_addr, n);
    return hipGetLastError();
}

hipError_t launch_retarget_entries(PageEntry* d_entries, uint64_t n, uint64_t base, uint64_t stride, hipStream_t s, uint64_t rec0)
{
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_retarget_entries, dim3(static_cast<uint32_t>((n + 255u) / 256u)), dim3(256), 0, s,
                       d_entries, n, base, stride, rec0);
    return hipGetLastError();
}

// 16-byte-per-lane copy (pinned host memory -> device): the request columns of a flush.  As a kernel on the flush's own
// stream it needs no copy engine and no cross-engine dependency in front of the first flush kernel.
__global__ __launch_bounds__(256) void k_copy16(const uint4* __restrict__ src, uint4* __restrict__ dst, uint32_t n16)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n16) dst[i] = src[i];
}
hipError_t launch_copy16(const void* src, void* dst, size_t bytes, hipStream_t s)
{
    const uint32_t n16 = static_cast<uint32_t>((bytes + 15u) / 16u);
    if (n16 == 0) return hipSuccess;
    hipLaunchKernelGGL(k_copy16, dim3((n16 + 255u) / 256u), dim3(256), 0, s, static_cast<const uint4*>(src), static_cast<uint4*>(dst), n16);
    return hipGetLastError();
}
} // namespace speckv
