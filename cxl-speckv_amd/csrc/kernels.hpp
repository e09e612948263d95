// cxl-speckv_amd/csrc/kernels.hpp -- launch interface of the CDNA4 kernels.
//
// One KV block = one 4 KiB page = 2048 fp16 elements.  One 64-lane wavefront
// owns one block at a time (4 wavefronts per workgroup, no workgroup barrier):
// lane l holds elements [8l + 512j, 8l + 512j + 8) for j = 0..3, so every
// global load/store instruction is one fully coalesced 1 KiB access.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "ring_rule.hpp"
#include "codec_launch_shape.hpp"

namespace speckv {

constexpr uint32_t kPageSize = 4096;
constexpr uint32_t kBlockElems = 2048;

enum Scheme : int { kFp16 = 0, kInt8 = 1, kInt8DeltaRle = 2, kInt4G32 = 3, kFp8E4m3 = 4, kMxFp4 = 5 };
constexpr uint32_t kInt4RecBytes = 128 + 1024;   // 64 fp16 group scales + 2048 nibbles
constexpr uint32_t kMx4RecBytes = 1024 + 64;     // 2048 E2M1 nibbles + 64 E8M0 group scales (OCP MX v1.0 blocks of 32)
// MXFP4 records in the POOL are tile-planar (round 6).  A record is 8.5 cache lines: at a stride of 1088 every other record starts
// in the middle of a line (a head pair's 256 bytes then span three lines: 3.38 GB fetched for 2.85 GB of records, profiles/r05_mx4.txt),
// and in line-aligned 1152-byte slots (round 5) the ninth line of every slot was fetched for half its bytes: 1.065 x the record bytes
// from DRAM and 5.9 % of the pool's capacity (profiles/r05c_mx4_mem_pmc.json).  So 16 records of a run form a TILE of exactly
// 136 lines: the 16 nibble rows (16 x 1024 B) followed by the 16 code rows (16 x 64 B, two records per line).  Record r of a
// run (runs start on a tile boundary) has its nibbles at mx4_nib_off(r) and its codes mx4_code_delta(r) bytes behind them; the
// record BYTES are the oracle's, only their placement differs.  The raw operators (speckv_ext_codec_*) keep contiguous records.
constexpr uint32_t kMx4TileRecs = 16;
constexpr uint32_t kMx4CodePlane = kMx4TileRecs * 1024u;                 // offset of the code rows inside a tile
constexpr uint32_t kMx4TileBytes = kMx4TileRecs * kMx4RecBytes;          // 17 408 B = 136 lines
__host__ __device__ inline uint64_t mx4_nib_off(uint64_t r) { return (r >> 4) * kMx4TileBytes + (r & 15u) * 1024u; }
__host__ __device__ inline uint32_t mx4_code_delta(uint64_t r) { return kMx4CodePlane - 960u * static_cast<uint32_t>(r & 15u); }
__host__ __device__ inline uint64_t mx4_run_bytes(uint64_t recs) { return (recs + 15u) / 16u * kMx4TileBytes; }
enum QuantMode : int { kRefExact = 0, kIntent = 1 };

// Device-resident page-table entry (16 B).
struct PageEntry {
    uint64_t pool_addr;   // device address of the stored record (local or peer HBM)
    uint32_t rec_bytes;   // record length in bytes (0 = never written)
    float    scale;       // per-block scale factor; MXFP4 (no block scale): the BITS are mx4_code_delta of the record, set when
                          // the entry is pointed at its place (k_init_entries / k_retarget_entries / the host) and kept by k_compress
};

// Shim layout (vllm_speckv_backend.py:87-100) of the allocation a lookup runs on.
struct Layout {
    uint32_t num_tokens, num_layers, num_heads, head_dim, bytes_per_element;
    uint64_t alloc_pages;
};

// One row of the device allocation table: what kernels that work across allocations (the prefetch pipeline, the
// ring bookkeeping of the fetch kernel) need to know about an allocation.  A freed row has entries == nullptr.
//   d_flags / d_slot : residency in HBM (bit0 L1, bit1 L2; cache slot) -- what kernels read and keep
//   h_slot           : one word per page in pinned host memory (device-visible) -- what the host reads: the ring
//                      sequence number under which a kernel fetched the page (its only host-visible store; the host
//                      derives the L2 bit from it, Engine::l2_live), or the L1 slot of a host-promoted page
//   stamp            : per-page scratch word of the flush's first-occurrence dedupe
struct DevAlloc {
    PageEntry* entries;
    uint32_t*  d_flags;
    uint32_t*  d_slot;
    uint32_t*  h_slot;
    uint32_t*  stamp;
    Layout     layout;
};
constexpr uint32_t kNoSlot = 0xFFFFFFFFu;
constexpr uint64_t kNoOwner = ~0ull;

// One allocation's share of a grouped compress launch (CodecArgs::groups): pages first + j*page_step, j < group_n, from
// data + j*data_stride.
struct CompressGroup {
    PageEntry*     entries;
    float*         scale_tab;
    uint32_t       region_pages;
    uint32_t       scale_run;         // CodecArgs::scale_run of this allocation
    uint64_t       first;
    const uint8_t* data;
};

// One position pair of one request in a pair-gather compress launch (PairArgs::pairs): block j < 2 * n_layers is page
// first + j * page_step (layer j >> 1, kind j & 1); its first 2048 bytes are row[2 * kind] + layer * layer_stride, its second
// 2048 bytes row[2 * kind + 1] + layer * layer_stride.  Rows are 16-byte aligned.
struct CommitPair {
    PageEntry*     entries;
    float*         scale_tab;
    uint32_t       region_pages;
    uint32_t       scale_run;
    uint64_t       first;
    const uint8_t* row[4];            // K even, K odd, V even, V odd
};
struct PairArgs {
    const CommitPair* pairs;          // device array
    uint32_t          n_pairs;
    uint32_t          n_layers;
    uint64_t          page_step;
    uint64_t          layer_stride;   // bytes, a multiple of 16
    int               scheme;
    int               quant_mode;
};

// One position pair of one request in a pair-read launch (ReadPairArgs::pairs), the mirror image of CommitPair: block
// j < 2 * n_layers is page first + j * page_step of the allocation in table row `table_row`; its first 2048 decoded bytes go to
// row[2 * kind] + layer * layer_stride, its second 2048 to row[2 * kind + 1] + layer * layer_stride.  A row that is nullptr is
// not wanted; the others are 16-byte aligned.
struct ReadPair {
    uint32_t table_row;               // DevAlloc row of the allocation
    uint32_t reserved;
    uint64_t first;
    uint8_t* row[4];                  // K even, K odd, V even, V odd
};
// The pair read for the split pool (k_read_pairs_kv, row_transfer_kv.hip): a pair names an FP8_E4M3 allocation with its K rows and an
// MXFP4 allocation with its V rows, each laid out as one region per layer.  Block j < 2 * n_layers (layer j >> 1, kind j & 1) is page
// first + (j >> 1) * page_step of the allocation in table row table_row[kind]; rows as in ReadPair.
struct ReadPairKV {
    uint32_t table_row[2];            // DevAlloc rows: K, V
    uint64_t first;
    uint8_t* row[4];                  // K even, K odd, V even, V odd
};
struct ReadPairKVArgs {
    const ReadPairKV* pairs;          // device array
    const DevAlloc*   tab;
    uint32_t          n_pairs;
    uint32_t          n_layers;       // real layers: one region per layer in either allocation
    uint64_t          page_step;
    uint64_t          layer_stride;   // bytes, a multiple of 16
};
struct ReadPairArgs {
    const ReadPair* pairs;            // device array
    const DevAlloc* tab;              // the device allocation table
    uint32_t        n_pairs;
    uint32_t        n_layers;
    uint64_t        page_step;
    uint64_t        layer_stride;     // bytes, a multiple of 16
    int             scheme;
    int             quant_mode;
};

// One span of a paged-cache transfer (SlotArgs::spans; k_read_slots / k_compress_slots): positions [first_token, first_token +
// n_tokens) of one allocation -- the reader finds its page table through table_row, the writer is handed entries / scale_tab /
// region_pages / scale_run as CommitPair carries them -- row t of the span lying in slot slots[slot_begin + t] of the caller's
// paged cache.  The span covers position pairs [first_token / 2, (first_token + n_tokens + 1) / 2); first_pair = the pairs of the
// spans in front of this one (the host's exclusive prefix: the kernel finds the span of a flat pair index by binary search and
// needs no atomics).  Descriptors are per span, never per pair or per token.
struct SlotSpan {
    PageEntry* entries;               // the destination (write); unused by the reader
    float*     scale_tab;
    uint32_t   region_pages;
    uint32_t   scale_run;
    uint32_t   table_row;             // DevAlloc row of the source (read)
    uint32_t   first_token;
    uint32_t   n_tokens;
    uint32_t   first_pair;            // exclusive prefix of pair counts
    uint64_t   slot_begin;
};
// Page of (layer, kind, position) = (2 * layer + kind) * page_step + position / 2, layer = layer_begin + l for l < n_layers; the
// row of slot s of that (l, kind) is caches[l] + kind * kind_stride + s * 2048.  A slot < 0 or >= n_slots is no row: not stored
// by the reader, read as `zeros` (2048 zero bytes) by the writer.
struct SlotArgs {
    const SlotSpan*  spans;           // device array, and behind it in the same staged slot ...
    const uint64_t*  caches;          // ... the n_layers cache bases (device array of device addresses)
    const int64_t*   slots;           // the caller's slot mapping (device)
    const DevAlloc*  tab;             // the device allocation table (read)
    const uint8_t*   zeros;           // 2048 zero bytes (write)
    uint64_t         n_slots;
    uint64_t         kind_stride;     // bytes, a multiple of 16
    uint64_t         page_step;
    uint32_t         n_spans;
    uint32_t         n_pairs;         // the sum of the spans' pair counts
    uint32_t         n_layers;
    uint32_t         layer_begin;
    uint32_t         kind_fast;       // the order of the waves: 0 = pair fastest inside a (layer, kind), 1 = (layer, kind) fastest
    int              scheme;
    int              quant_mode;
};
// The same launch with bf16 caches and held rows (k_read_slots_ex / k_compress_slots_ex).  A held row is one position that lives
// outside both the pool and the caches, always fp16: the row of (layer layer_begin + l, kind) at in[kind] / out[kind] +
// l * held_stride.  SlotArgs::spans then counts DECODED / ENCODED pairs only --
//   read:   in[kind] set: the span's last position (even) is copied from the held row into its slot, its page is not read; the
//           span's pairs are [first / 2, (first + n - 1) / 2)
//   write:  in[kind] set: position first_token - 1 (first_token odd) comes from the held row; out[kind] set: the last position
//           (first_token + n_tokens odd) is not encoded but written to the held row; the pairs are [first / 2, (first + n) / 2)
// -- and the positions that only move between a held row and a slot are 2 * n_layers further waves per span behind the pair
// waves (n_moves of them; those of a span without such a position leave at once).
struct SlotHeld {
    uint64_t in[2];                   // K, V; 0 = none
    uint64_t out[2];
};
struct SlotExArgs {
    SlotArgs         a;
    const SlotHeld*  held;            // device array [n_spans] in the same staged slot; nullptr = no held rows in this call
    uint64_t         held_stride;     // bytes between the layers of a held row block, a multiple of 16
    uint32_t         n_moves;         // 0 or n_spans * 2 * n_layers
    uint32_t         bf16;            // the caches' rows hold bf16
};
// The _ex launch with a per-channel K factor (the SlotKmulArgs instances of k_read_slots_ex / k_compress_slots_ex): every K
// element that crosses between a cache row and the pool side -- records and held rows -- is multiplied by the fp16 factor of its
// (layer, head, channel), the exact fp32 product rounded once to the destination's element type.  The [heads][128] factor row of
// layer layer_begin + l is k_mul + l * k_mul_stride.  Whether a wave scales is j & 1 alone (K = 0): V waves take the source and
// sink of the _ex kernels and never load a factor.  A held-in row of a write is pool-side already and is encoded as it is.
struct SlotKmulArgs {
    SlotExArgs       x;
    const uint8_t*   k_mul;           // device, 16-byte aligned, never nullptr (without a factor the call is the _ex launch)
    uint64_t         k_mul_stride;    // bytes between the layers' factor rows, a multiple of 16
};
// The _ex launch for the split pool (k_read_slots_kv / k_compress_slots_kv, row_transfer_kv.hip): a span is positions of TWO
// allocations, an FP8_E4M3 one that holds its K rows and an MXFP4 one that holds its V rows, each laid out as one region per layer.
// The waves, their (layer, kind) j, the slots, the held rows and the move waves are those of SlotExArgs; what differs is that wave j
// takes allocation and codec j & 1 (index 0 = K, 1 = V below) and that the page of (layer, position) in the chosen allocation is
// layer * page_step + position / 2, layer = layer_begin + (j >> 1): no factor 2 and no kind term.
struct SlotSpanKV {
    PageEntry* entries[2];            // the destinations (write); unused by the reader
    float*     scale_tab[2];
    uint32_t   region_pages[2];
    uint32_t   scale_run[2];
    uint32_t   table_row[2];          // DevAlloc rows of the sources (read)
    uint32_t   first_token;
    uint32_t   n_tokens;
    uint32_t   first_pair;            // exclusive prefix of pair counts
    uint32_t   reserved;
    uint64_t   slot_begin;
};
struct SlotKVArgs {
    struct Pages {                    // SlotArgs without a scheme: the codecs are fixed by the kind
        const SlotSpanKV* spans;
        const uint64_t*   caches;
        const int64_t*    slots;
        const DevAlloc*   tab;
        const uint8_t*    zeros;
        uint64_t          n_slots;
        uint64_t          kind_stride;
        uint64_t          page_step;
        uint32_t          n_spans;
        uint32_t          n_pairs;
        uint32_t          n_layers;
        uint32_t          layer_begin;
        uint32_t          kind_fast;
    } a;
    const SlotHeld*  held;            // as SlotExArgs
    uint64_t         held_stride;
    uint32_t         n_moves;
    uint32_t         bf16;
};

// One (source, destination) pair of a record-copy launch (CopyArgs::pairs; copy_records.hip): the stored records of pages
// [run_firsts[r], run_firsts[r] + n_pages), every run r of the launch, go from the allocation in table row `src_row` to the same
// pages of the allocation whose page table is `entries` -- scale_tab / region_pages / scale_run as CommitPair carries them.
// first_rec = the sum of n_runs * n_pages over the pairs in front of this one (the host's exclusive prefix: the kernel finds the pair
// of a flat record index by binary search and needs no atomics).
struct CopyPair {
    PageEntry* entries;               // destination
    float*     scale_tab;
    uint32_t   region_pages;
    uint32_t   scale_run;
    uint32_t   src_row;               // DevAlloc row of the source
    uint32_t   reserved;
    uint64_t   n_pages;
    uint64_t   first_rec;
};
struct CopyArgs {
    const CopyPair* pairs;            // device array, and behind it in the same staged slot ...
    const uint64_t* run_firsts;       // ... the first page of every run (device array)
    const DevAlloc* tab;              // the device allocation table
    uint32_t        n_pairs;
    uint32_t        n_runs;
    uint64_t        n_recs;           // n_runs * the sum of n_pages
    uint32_t        n_cus;            // compute units of the device: the grid is a few workgroups per CU, grid-stride over the records
    int             scheme;
};
// ONE launch; a source page never written leaves the destination page never written (rec_bytes 0, its slot zero bytes)
hipError_t launch_copy_records(const CopyArgs& a, hipStream_t s);
// The record copy for the split pool (k_copy_records_kv, copy_records_kv.hip): a pair is TWO (source, destination) pairs of
// allocations, index 0 = the FP8_E4M3 ones with the K rows, 1 = the MXFP4 ones with the V rows, and the same pages are copied in both.
// scale_tab / region_pages / scale_run are the K destination's (an MXFP4 allocation has no scale table).  first_rec = the sum of
// 2 * n_runs * n_pages over the pairs in front of this one; of a pair's records the first n_runs * n_pages are the K side's, run by
// run as in CopyPair, the second n_runs * n_pages the V side's.
struct CopyPairKV {
    PageEntry* entries[2];            // destinations: K, V
    float*     scale_tab;             // K destination
    uint32_t   region_pages;
    uint32_t   scale_run;
    uint32_t   src_row[2];            // DevAlloc rows of the sources: K, V
    uint64_t   n_pages;
    uint64_t   first_rec;
};
struct CopyKVArgs {
    const CopyPairKV* pairs;          // device array, and behind it in the same staged slot ...
    const uint64_t*   run_firsts;     // ... the first page of every run (device array)
    const DevAlloc*   tab;
    uint32_t          n_pairs;
    uint32_t          n_runs;
    uint64_t          n_recs;         // 2 * n_runs * the sum of n_pages
    uint32_t          n_cus;
};
// ONE launch over both allocations of every pair; per record what launch_copy_records does for its scheme
hipError_t launch_copy_records_kv(const CopyKVArgs& a, hipStream_t s);

// One sequence of a chunk-attention launch (ChunkArgs::seqs; attend_chunk.hip): pos_end (even) stored positions whose K pages are
// k_first + p / 2 and whose V pages are v_first + p / 2 of the allocation in table row `table_row`, base in {0, 1} held odd last
// positions (row tail_idx of the tail arrays) and n_q new positions.  first_block = the query blocks (ceil(n_q / (64 / rows_per_pos)))
// of the sequences in front of this one (the host's exclusive prefix: the kernel finds the sequence of a flat block index by binary
// search and needs no atomics).
// Split form (ChunkArgs::part): the sequence's pool tiles are cut into n_pieces >= 1 pieces of tiles_per_piece tiles (chunk_split.hpp),
// a work item is (query block, piece) with the piece fast, first_item = the items (blocks x pieces) of the sequences in front of this
// one, found by the same search; first_block serves the merge.
struct ChunkSeq {
    uint32_t table_row;
    uint32_t pos_end;
    uint32_t n_q;
    uint32_t first_block;
    uint64_t k_first;
    uint64_t v_first;
    int32_t  tail_idx;
    uint32_t base;
    uint32_t n_pieces;
    uint32_t tiles_per_piece;
    uint32_t first_item;
    uint32_t first_tile;              // window form: the first pool tile any block of the sequence walks (the pieces start here); else 0
    uint32_t v_table_row;             // the table row of the allocation whose pages v_first counts: table_row, but in the split pool
                                      // (ChunkArgs::v_scheme != scheme), where the V pages lie in an allocation of their own
};
// A partial of the split form, one per (work item, kv head): the un-normalised accumulator [64 rows][128] fp32 in the row order of
// `out`, then (running max, running sum) per row in the log2 domain.
constexpr size_t kChunkPartAccBytes = 64u * 128u * sizeof(float), kChunkPartBytes = kChunkPartAccBytes + 64u * 2u * sizeof(float);
struct ChunkArgs {
    const ChunkSeq* seqs;             // device array
    const DevAlloc* tab;              // the device allocation table
    const _Float16* q;                // [n_seq][C][heads][rows_per_pos][128]
    const _Float16* k_new;            // new position j of sequence i, head h: k_new + i * seq_stride + j * pos_stride + 128 h
    const _Float16* v_new;
    const _Float16* k_tail;           // tail row r, head h: k_tail + r * tail_stride + 128 h (may be null when no sequence has a tail)
    const _Float16* v_tail;
    float*          out;              // as q, fp32
    float*          lse;              // [n_seq][C][heads][rows_per_pos], natural log; may be null
    uint64_t        seq_stride, pos_stride, tail_stride;      // elements
    uint32_t        n_seq, n_blocks;  // n_blocks = the sum of the sequences' query blocks
    uint32_t        C, rows_per_pos, heads;
    float           sm_scale;
    int             scheme;           // kFp8E4m3, kInt4G32 or kMxFp4: the scheme of the K pages (and, but in the split pool, of the V pages)
    // tree form (null: causal): row (i * C + j) * mask_words of this device array = query position j of sequence i, bit t & 31 of its
    // word t >> 5 = HELD position t (the tail, if any, is 0; new position a is base + a) is visible, under the causal bound
    // t < base + j + 1 as before; a row whose own bit base + j is clear is dead: not computed to the end, not written
    const uint32_t* mask;
    uint32_t        mask_words;       // words per query position, >= (C + 1 + 31) / 32
    // split form (null: one workgroup walks all of a sequence's tiles and writes out / lse itself): n_items * heads partials of
    // kChunkPartBytes, partial (item, head) at part + (item * heads + head) * kChunkPartBytes; n_items = the sum of blocks x pieces
    uint8_t*        part;
    uint32_t        n_items;
    // window form (0: none): query position j sees the absolute positions [max(0, P + 1 - window), P], P = pos_end + base + j
    // (chunk_window.hpp); with a mask only together with `depth`
    uint32_t        window;
    // tree form under a window (null: none; needs mask and window): depth[i * C + j] = the depth of node j of sequence i in its tree
    // (0: a child of the committed context), the j of its lower bound over the STORED positions; the held part is what the mask
    // says.  The last member the kernels read: the members the other forms read keep their places.
    const uint32_t* depth;
    // the scheme of the V pages (the launcher's alone: it picks the instance).  Equal to `scheme` everywhere but in the K8V4 split pool,
    // scheme == kFp8E4m3 and v_scheme == kMxFp4 -- the one mixed pair there are instances of; any other is refused.
    int             v_scheme;
};
// part == null: ONE launch of n_blocks * heads workgroups.  Otherwise TWO: n_items * heads workgroups that write their partials, then
// the merge (k_chunk_combine) over n_blocks * heads, which reads a row's partials in ascending piece order and writes out / lse.
// Nothing is launched for n_blocks == 0.
hipError_t launch_attend_chunk(const ChunkArgs& a, hipStream_t s);

// One group of a shared-prefix launch (PrefixArgs::groups; attend_prefix.hip): a prefix allocation (table row, K / V pages as in
// ChunkSeq) and the members [first_member, first_member + n_pairs / C) of the call, whose query rows see its stored positions
// [0, prefix_len[member]).  max_len (even) = the largest prefix_len of the group's live members: the tiles a block walks.  n_pairs =
// members x C flat (member, position) pairs, cut into blocks of 64 / rows_per_pos; first_block / first_item = the host's exclusive
// prefixes over blocks and over blocks x pieces, as in ChunkSeq.  A group without a live pair has no blocks.
struct PrefixGroup {
    uint32_t table_row;
    uint32_t max_len;
    uint32_t first_member;
    uint32_t n_pairs;
    uint64_t k_first;
    uint64_t v_first;
    uint32_t first_block;
    uint32_t first_item;
    uint32_t n_pieces;
    uint32_t tiles_per_piece;
    uint32_t first_tile;              // window form: the first tile any live row of the group sees (prefix_window.hpp; the walk and
                                      // the pieces start here); else 0.  (It makes the struct 56 bytes where it was 48: the stride
                                      // of the group search changed in every instance, the plain ones included.)
    uint32_t v_table_row;             // the table row of the allocation whose pages v_first counts: table_row, but in the split pool
                                      // (PrefixArgs::v_scheme != scheme).  It takes the word that padded 52 bytes of members to 56.
};
static_assert(sizeof(PrefixGroup) == 56, "the stride of the group search (prefix_group_of) is part of every instance");
struct PrefixArgs {
    const PrefixGroup* groups;        // device array
    const uint32_t* prefix_len;       // device array [n_members]: even, the stored positions of its group's prefix the member sees
    const uint32_t* n_q;              // device array [n_members]: live positions of the member, <= C
    const DevAlloc* tab;              // the device allocation table
    const _Float16* q;                // [n_members][C][heads][rows_per_pos][128]
    float*          out;              // as q, fp32: read and written (the fold)
    float*          lse;              // [n_members][C][heads][rows_per_pos], natural log: read and written
    uint8_t*        part;             // split form (null: none): n_items * heads partials of kChunkPartBytes, as ChunkArgs::part
    uint32_t        n_groups, n_blocks, n_items;
    uint32_t        C, rows_per_pos, heads;
    float           sm_scale;
    int             scheme;           // kFp8E4m3, kInt4G32 or kMxFp4: the scheme of the K pages (and, but in the split pool, of the V pages)
    // window form (window 0: none; the engine vouches for own_seen and for depth's alignment): the row of member m and position j sees the
    // stored positions [lo, prefix_len[m]) only, lo = prefix_window_lo(prefix_len[m], own_seen[m], d, window) with d = depth[m * C + j]
    // or, where depth is null, j; a row with lo >= prefix_len[m] is dead like a pair beyond n_q[m]
    const uint32_t* own_seen;         // device array [n_members]
    const uint32_t* depth;            // device array [n_members][C], or null
    uint32_t        window;
    // the scheme of the V pages (the launcher's alone: it picks the instance), as ChunkArgs::v_scheme: equal to `scheme` everywhere but
    // in the K8V4 split pool, scheme == kFp8E4m3 and v_scheme == kMxFp4 -- the one mixed pair there are instances of; any other is refused.
    int             v_scheme;
};
// part == null: ONE launch of n_blocks * heads workgroups that fold into out / lse.  Otherwise TWO: n_items * heads workgroups that
// write their partials, then k_prefix_combine over n_blocks * heads, which merges a row's pieces in ascending order and folds.
// Nothing is launched for n_blocks == 0.
hipError_t launch_attend_prefix(const PrefixArgs& a, hipStream_t s);

// Source / destination description of one codec launch.  Exactly one of
// {entries, recs, tab+alloc_list} is used as the record source.
struct CodecArgs {
    // record side
    PageEntry*      entries;      // page table (engine form), indexed by page
    uint8_t*        recs;         // raw form: record i at recs + i*rec_stride
    uint64_t        rec_stride;
    uint32_t*       rec_bytes;    // raw form
    float*          scales;       // raw form
    // block index mapping: page = page_list ? page_list[i] : first + i  (compress only: first + i*page_step when page_step != 0)
    const uint32_t* page_list;
    uint64_t        first;
    uint64_t        page_step;
    // fp16 / fp32 side: block i at data + i*data_stride_bytes, or data_list[i]
    uint8_t*        data;
    uint64_t        data_stride;
    const uint64_t* data_list;
    // count
    uint64_t        n;
    const uint32_t* n_dev;        // optional: n read from device memory (<= n)
    uint64_t        per_wave;     // set by the launcher: blocks per wave (0 = 1) ...
    uint64_t        wave_step;    // ... consecutive (0) or this many blocks apart (one per round of the grid)
    // residency mirror update on completion (decompress only): flags[page] |= set_flags (atomic)
    uint32_t*       flags;
    uint32_t        set_flags;
    int             scheme;
    int             quant_mode;
    int             out_f32;
    // records were written by k_compress (the engine's pool): INT8_DELTA_RLE streams are then known to
    // have no zero counts and a zero-padded tail, which the decoder need not re-check per pair
    int             trusted;
    // decompress, INT8_DELTA_RLE: the caller knows the records to be short (structured data: mean record well under 512 B) --
    // the launch takes the instantiation with the flat-run fast path (decode_rle_fast<.., FLAT>); results are identical
    int             structured_hint;
    // compress only: when set, the block scale of page p is also stored at scale_tab[tile order of p] -- the
    // per-tile order the fused attention reads with one 16-byte load (attend.hip); region_pages = pages of one
    // (layer, kind) region of the shim layout, a multiple of 16
    float*          scale_tab;
    uint32_t        region_pages;
    // ... and, for an allocation striped regularly over D >= 2 runs (round 6), ALSO in run order -- the scale of page p at
    // scale_tab[-D * cap + (p % D) * cap + p / D], D = scale_run & 15, cap = scale_run >> 4 (0: no such table) -- where the
    // residue-class forms of the FP8 attention find the 16 scales of a class tile in one line (scale_run_index)
    uint32_t        scale_run;
    // compress only, INT8_DELTA_RLE: every 1024th page leaves its record length in len_samples[(page >> 10) & 15] -- 16 words of
    // the allocation's host-visible memory, plain stores -- so that the host can tell, without a copy back, whether the
    // allocation holds data that compresses (mean record well under 512 B: the flat-run decoder is then chosen for its reads;
    // CodecArgs::structured_hint).  A hint only: either decoder gives the same bytes.  Null: no samples.
    uint32_t*       len_samples;
    // compress only: blocks of several allocations in one launch -- block i belongs to groups[i / group_n] (device array)
    // as its page i % group_n; entries / scale_tab / region_pages / first / data above are then unused
    const CompressGroup* groups;
    uint64_t        group_n;
    // blocks of several allocations in one launch (decompress only): block i belongs to row alloc_list[i] of tab
    const DevAlloc* tab;
    const uint32_t* alloc_list;
    // L2-ring bookkeeping done by the fetch kernel itself (decompress only, ring_owner != nullptr): block i lands in
    // cache slot slot0 + i (dst = ring_base + slot*4096); the wave evicts the slot's previous owner (clears its L2 bit
    // if it still points at this slot), records the new owner, the page's slot and its L2 bit in HBM and the slot's ring
    // sequence number in the page's host-visible word.  slot0 / seq0 come from the *_dev pointers when set, else from
    // the values.  (Synchronous misses; the device-side flush does this in its scatter kernel, one thread per page.)
    uint64_t*       ring_owner;
    uint8_t*        ring_base;
    const uint32_t* slot0_dev;
    uint32_t        slot0;
    const uint32_t* seq0_dev;     // ring sequence number of slot0 (block i: seq0 + i), stored as the page's host-visible word
    // device-side flush (list form): block i's host-visible word *host_words[i] = *seq0_dev + i is stored by the fetch
    // itself, spread over the launch, instead of by the scatter kernel in front of it (FlushArgs::final_host)
    uint32_t* const* host_words;
    uint32_t        seq0;
    uint32_t        alloc_idx;    // row of tab for every block when alloc_list == nullptr
    uint32_t*       hand_ptr;     // optional: block 0 stores new_hand = the ring sequence number after this take (host-initiated takes keep the device's current)
    uint32_t        new_hand;
    // copy-engine fetch: the records of pool (page % stripe_n) were copied into local staging, to their pool address
    // + stripe_delta[page % stripe_n]
    uint32_t        stripe_n;
    uint64_t        stripe_magic; // floor(2^35 / stripe_n) + 1: (page * magic) >> 35 == page / stripe_n for page < 2^28
    int64_t         stripe_delta[8];
    // ring form only, launches of a few waves (speckv_access on a miss): when done_flag is set, every wave ends with a
    // system-scope fence and counts itself in *done_count (device memory, zero before and after the launch); the last one
    // stores done_token to *done_flag (pinned host memory) -- the host spins on that word instead of going through the runtime's
    // completion path (profiles/tools/probe/sync_latency.hip: 7 us against 11 us for launch + wait)
    uint32_t*       done_flag;
    uint32_t*       done_count;
    uint32_t        done_token;
    // decompress, plain forms only (range / list, raw records; the staged, ring and host-word forms are refused): the launch walks its
    // blocks from the top -- wave position i decodes block n - 1 - i (n after n_dev), page and destination alike.  The bytes written
    // are the same; the order decides what a repeated sweep finds in the Infinity Cache (fetch_sweep.hpp)
    uint32_t        descending;
    // ... and its stores to the destination are plain instead of non-temporal, so that the lines stay in the Infinity Cache for the
    // sweep that follows (block_codec_device.hpp: ImageSink).  The same forms only.
    uint32_t        keep_stores;
};

hipError_t launch_compress(const CodecArgs& a, hipStream_t s);
hipError_t launch_decompress(const CodecArgs& a, hipStream_t s);
// the shape both give a launch of n blocks under the tuning in force (codec_launch_shape.hpp; wgs_per_cu, rounds_consecutive);
// n_cus 0: the current device's CUs, or 256 without a device
CodecLaunchShape codec_launch_shape_now(uint64_t n, uint32_t n_cus);
// the pair-gather form of the encoder: n_pairs * 2 * n_layers blocks in one launch, rows read where they lie (k_compress_pairs)
hipError_t launch_compress_pairs(const PairArgs& a, hipStream_t s);
hipError_t launch_read_pairs(const ReadPairArgs& a, hipStream_t s);
// the paged-cache forms of both: n_pairs * 2 * n_layers blocks in one launch, rows addressed by a device slot mapping
hipError_t launch_compress_slots(const SlotArgs& a, hipStream_t s);
hipError_t launch_read_slots(const SlotArgs& a, hipStream_t s);
hipError_t launch_compress_slots_ex(const SlotExArgs& a, hipStream_t s);
hipError_t launch_read_slots_ex(const SlotExArgs& a, hipStream_t s);
hipError_t launch_compress_slots_kmul(const SlotKmulArgs& a, hipStream_t s);
hipError_t launch_read_slots_kmul(const SlotKmulArgs& a, hipStream_t s);
hipError_t launch_compress_slots_kv(const SlotKVArgs& a, hipStream_t s);     // (row_transfer_kv.hip)
hipError_t launch_read_slots_kv(const SlotKVArgs& a, hipStream_t s);
hipError_t launch_read_pairs_kv(const ReadPairKVArgs& a, hipStream_t s);

// FPGACacheEngine::compress / ::decompress over a tensor of any length (tensor_compress.hip, tensor_decompress.hip): one scale, one delta chain and
// one run-length stream across the whole tensor.  d_rle: 16-byte aligned, room for 2n bytes rounded up to 16; d_ws:
// 256-byte aligned scratch of tensor_*_workspace_bytes; d_n_out may be null.
size_t tensor_compress_workspace_bytes(uint64_t n);
size_t tensor_decompress_workspace_bytes(uint64_t rle_bytes);
hipError_t launch_tensor_compress(const void* d_src, uint64_t n, bool src_f32, uint8_t* d_rle, uint64_t* d_rle_bytes, float* d_scale,
                                  void* d_ws, size_t ws_bytes, int quant_mode, hipStream_t s);
hipError_t launch_tensor_decompress(const uint8_t* d_rle, uint64_t rle_bytes, float scale, void* d_dst, uint64_t dst_cap, bool out_f32,
                                    uint64_t* d_n_out, void* d_ws, size_t ws_bytes, int quant_mode, hipStream_t s);

// The same over MANY tensors in one launch each way (tensor_compress.hip: k_tcm_fused, tensor_decompress.hip: k_tdm_fused -- several workgroups per tensor,
// tensor-local look-back, max|x| by rendezvous; tensors of at most 16 tiles: k_tcb_fused / k_tdb_fused, one workgroup each).
// TensorDesc = speckv_ext_tensor_t: {data (compress: the source; decompress: the destination), n (elements; decompress: room),
// rle (the stream, 16-byte aligned), rle_cap}.  max_elems: the host's bound on n (sizes the grid); d_ws: 256-byte aligned,
// tensors_workspace_bytes(n_tensors, max_elems) bytes.
struct TensorDesc { void* data; uint64_t n; uint8_t* rle; uint64_t rle_cap; };
size_t tensors_workspace_bytes(uint32_t n_tensors, uint64_t max_elems);
hipError_t launch_tensors_compress(uint32_t n_tensors, const TensorDesc* d_desc, uint64_t max_elems, bool src_f32, uint64_t* d_rle_bytes, float* d_scales,
                                   void* d_ws, size_t ws_bytes, int quant_mode, hipStream_t s);
hipError_t launch_tensors_decompress(uint32_t n_tensors, const TensorDesc* d_desc, uint64_t max_elems, const uint64_t* d_rle_bytes, const float* d_scales, bool out_f32,
                                     uint64_t* d_n_out, void* d_ws, size_t ws_bytes, int quant_mode, hipStream_t s);

// Prefetch lookup: 3 kernels (mask+count, scan, scatter) -> compacted page list
// in request order.  scratch must hold (2*n + 2) uint32.
hipError_t launch_prefetch_lookup(const Layout& lay, uint32_t n,
                                  const uint32_t* d_req, const uint32_t* d_layer,
                                  const uint32_t* d_pos, const uint32_t* d_k,
                                  const uint32_t* d_flags, uint32_t* d_out, uint32_t cap,
                                  uint32_t* d_count, uint32_t* d_scratch, hipStream_t s);

hipError_t launch_verify(uint32_t n, uint32_t k, const int32_t* d_actual,
                         const int32_t* d_predicted, uint8_t* d_hit,
                         uint32_t* d_hit_count, hipStream_t s);

// Host-originated residency changes applied to the device mirrors: for each update,
// d_flags[page] = (d_flags[page] & and_mask) | or_mask and, unless slot == kKeepSlot, d_slot[page] = slot.
struct MirrorUpdate { uint32_t alloc_idx, page, and_mask, or_mask, slot, pad; };
constexpr uint32_t kKeepSlot = 0xFFFFFFFEu;
hipError_t launch_apply_updates(const DevAlloc* d_tab, const MirrorUpdate* d_updates, uint32_t n, hipStream_t s);

// Device-side prefetch flush (prefetch_core.v:150-241: predict -> encode -> translate -> directory check -> issue,
// without the host).  n requests (SoA: local request index inside the allocation, layer, position, depth, table row)
// -> candidate pages in request order (fixed stride of 32*W words per request), first-occurrence dedupe through the
// per-page stamps, ordered compaction, ring-slot assignment, and the final (page, row) lists a fetch launch consumes.
struct FlushResult { uint32_t m, base, total, seq; };      // pages taken, first ring slot, distinct candidates found, ring sequence number of the first slot
struct FlushArgs {
    const DevAlloc* tab;
    uint32_t        n;            // requests
    uint32_t        W;            // candidate words per lane (max new pages of one position + 1)
    const uint32_t* req;          // [n] request index inside its allocation
    const uint32_t* layer;
    const uint32_t* pos;
    const uint32_t* depth;
    const uint32_t* row;          // [n] table row (kNoSlot = unaddressable request: contributes nothing)
    uint32_t        epoch;        // 1..255, stamps of older epochs are ignored
    uint32_t*       cand;         // [n*32*W]
    uint32_t*       wave_tot;     // [n*W/2 rounded up] + same again for the bases
    // what the fetch launch reads, in list order (block i): the page's record descriptor and its ring slot's address
    PageEntry*      final_entry;  // [max_take]
    uint64_t*       final_dst;    // [max_take]
    uint64_t*       ring_owner;   // L2 ring bookkeeping, done by the scatter kernel with one THREAD per page (see there)
    uint8_t*        ring_base;
    uint32_t        max_take;     // never more than this many pages per flush
    uint32_t        n_l2;         // ring size
    uint32_t*       hand;         // device ring hand
    FlushResult*    result_dev;   // m is read by the fetch launch (n_dev)
    FlushResult*    result_host;  // the same, stored to pinned host memory
    // null: the scatter kernel stores every page's host-visible word itself (one PCIe transaction per page, all of them in
    // front of the fetch); else it lists the words' addresses and the fetch launch stores them (CodecArgs::host_words)
    uint32_t**      final_host;   // [max_take]
};
hipError_t launch_flush_pipeline(const FlushArgs& a, hipStream_t s);
// bytes rounded up to 16: both buffers must be 16-byte aligned and padded to a multiple of 16
hipError_t launch_copy16(const void* src_host_mapped, void* dst, size_t bytes, hipStream_t s);

// entries[first+i].pool_addr = base + i*stride ; rec_bytes = 0 ; scale = 1.  stride == kPlanarMx4: entry i = record rec0 + i of
// a tile-planar MXFP4 run at base (pool_addr = base + mx4_nib_off, scale bits = mx4_code_delta)
constexpr uint64_t kPlanarMx4 = 0;
hipError_t launch_init_entries(PageEntry* d_entries, uint64_t n, uint64_t base,
                               uint64_t stride, hipStream_t s, uint64_t rec0 = 0);

// Fused dequant-matvec of BASELINE config 5: q.K^T scores straight from FP8_E4M3
// records with v_mfma_f32_16x16x32_fp8_fp8 (no fp16 K is ever materialised).
// Layout requirement: one K row (all heads of one position) = 2048 B, i.e. two
// positions per 4 KiB page (H*D = 1024 elements, e.g. 8 kv heads x 128).
//   d_q8     [H][16][128] e4m3 query rows (rows >= g are zero), d_qs [H][16] their scales
//   d_out    [H][g][n_pos] fp32, n_pos = 2 * n_pages
hipError_t launch_quantize_q_e4m3(const void* d_q_f16, uint32_t heads, uint32_t g, uint32_t d,
                                  uint8_t* d_q8, float* d_qs, hipStream_t s);
hipError_t launch_qk_scores_fp8(const PageEntry* d_entries, uint64_t first_page, uint64_t layer_page_stride,
                                uint32_t n_layers, uint32_t n_pages, uint32_t heads, uint32_t g,
                                const uint8_t* d_q8, const float* d_qs, float* d_out, hipStream_t s);

// Batch form of the linear fused attention: many sequences (allocations), one layer each, one launch.  The fields
// override their AttendArgs namesakes per sequence; part_base = index of the sequence's first (head, split) partial.
struct AttendSeq {
    const uint8_t* lin_base;          // table launches (AttendArgs::table_form: a batch member without a regular placement makes the whole
                                      // launch read its addresses from the page tables): the sequence's PageEntry array instead
    const float* scale_tab;
    uint64_t k_first, v_first;        // first K / V page of the wanted layer (position 0)
    uint32_t n_pages;                 // pages of [0, pos_end)
    uint32_t n_splits;                // ceil(tiles / tiles_per_split), <= gridDim.x
    uint32_t part_base;
    uint32_t tiles_per_split;         // this sequence's own split length (its tiles divided evenly over n_splits)
    const uint64_t* stripe_bases;     // striped launches (AttendArgs::stripe_bases set): the sequence's own run bases ...
    uint32_t layer_pages;             // pages of one layer (K + V): layer l of a planned batch starts at k_first + l * layer_pages
    uint32_t stripe_n;                // ... and pool count (1 = a single run: lin_base is bases[0])
};                                    // (64 bytes: speckv_ext_attend_plan_bytes)

// Decode attention straight from FP8_E4M3 records (attend.hip): softmax(q.K^T * sm_scale) . V per kv head,
// split over the positions, partials merged by a second kernel.  Same layout requirement as the scores.
struct AttendArgs {
    const PageEntry* entries;
    uint64_t k_first, v_first;        // first K / V page of layer_begin at pos_begin
    uint64_t layer_stride;            // pages per layer (K + V)
    uint32_t n_pages;                 // pages of the position range
    uint32_t skip_pages;              // FP8 tile forms: the first skip_pages pages of the range are masked (a range that starts inside a 32-position tile)
    uint32_t heads, g;
    uint32_t n_splits, tiles_per_split;   // tile = 16 pages = 32 positions
    const uint8_t* q8;                // [layers][heads][16][128] e4m3
    const float* qs;                  // [layers][heads][16]
    float scale_log2e;                // sm_scale * log2(e)
    const uint8_t* zero_page;         // 4 KiB of zeros: stands in for pages never written (general form)
    const uint8_t* lin_base;          // non-null: record p of the allocation sits at lin_base + p*2048 and
                                      // never-written records are zero bytes (linear, pipelined form)
    const float* scale_tab;           // linear form: page scales of the whole allocation in tile order (attend.hip)
    const uint16_t* q16;              // linear form: the fp16 query rows [layers][heads][g][128] (quantised in the kernel)
    const struct AttendSeq* seqs;     // batch form: one descriptor per sequence (blockIdx.y / (heads/4)), else null
    const uint32_t* order;            // batch form, sequences of different lengths (round 6): order[i] = the sequence whose workgroups are dispatched i-th (the
                                      // engine orders them by length so that the CUs' shares even out: attend_dispatch_order), or null = as given
    float* part_acc;                  // [layers][heads][splits][16][128]
    float* part_ml;                   // [layers][heads][splits][2][16]
    // every row has exactly ONE split (set by the engine then): the attention kernel normalises and writes the final
    // [row][g][128] output and the log-sum-exp (may be null) itself, and no merge launch follows
    float* direct_out;
    float* direct_lse;
    // planned batches (descriptors resident on the device, one set for all layers of a decode step): the layer of this
    // launch, and "decide per sequence": 1 = a sequence with one split is written directly, the others through the merge
    // launch that follows; 2 = the launch geometry allows one split at most, NO merge follows: sequences without
    // positions are zeroed by the attention kernel itself (attend_zero_rows); 3 (to launch_attend_combine only, from launch_attend_k8v4_held) =
    // as 1, and the rows of a sequence WITHOUT a split are the attention kernel's as well: the merge leaves them alone
    uint32_t batch_layer;
    uint32_t direct_per_seq;
    // ... and SEVERAL layers of the planned batch in one launch (speckv_ext_attend_planned_layers: callers that have the query rows of
    // several layers at once): batch_n_seq != 0 -> grid y = layer x sequence, row block y of q / out / lse = [layer][sequence], layer
    // batch_layer + y / batch_n_seq.  Only launches whose geometry has one split per sequence (direct_per_seq == 2: no merge behind).
    uint32_t batch_n_seq;
    // striped form (lin_base == nullptr, stripe_bases != nullptr): the allocation still has the regular placement over
    // 2..8 pools -- the record of page p is stripe_bases[p % stripe_n] + (p / stripe_n) * record stride (placement.hpp),
    // never-written records zero bytes -- so every address is arithmetic here too; stripe_magic = floor(2^32 / n) + 1:
    // __umulhi(p, magic) == p / n for every p < 2^28.  The 8 run bases live in a small device array of the allocation.
    // Batch form: non-null marks a striped launch, every AttendSeq then carries its own stripe_bases / stripe_n.
    const uint64_t* stripe_bases;
    uint32_t stripe_n, stripe_magic;
    // rows-first launches: grid (rows, splits) instead of (splits, rows), so that the workgroups are dispatched split by
    // split -- split 0 of every row first.  With a long split 0 and a short split 1 per row the long pieces all start at
    // once and the short ones fill the remaining workgroup slots in turns (engine_attend.cpp: int4_unequal_split)
    uint32_t rows_first;
    uint32_t rows_real;               // rows-first batch launches of the FP8 / MXFP4 kernels: grid x is padded to an ODD number of rows, so that the pieces of one member go round
                                      // the XCDs (workgroup id % 8) instead of all landing on one; rows >= rows_real are padding and return at once
    // table form of the fast kernels (single-sequence form; lin_base and stripe_bases null): an allocation whose placement
    // is no longer regular (pages migrated one by one) but whose range is tile-aligned -- every record address comes
    // from the page-table entry, looked up one tile ahead of its request; never-written pages read zero_page
    uint32_t table_form;
    // INT4, linear form, 8 kv heads: the whole-record kernel (k_attend_int4_wg8: 8 waves = 8 heads, grid (splits, layers))
    uint32_t mx4_halves;              // MXFP4, linear batch launches of single-split sequences: 8-wave workgroups, the run cut in two (k_attend_mx4<0, 2>)
    uint32_t wg8;                     // 1: the engine's choice of form; 2: workgroups of one run (8 waves) also for batches
    // ... and its STREAM form for many layers of one sequence (see k_attend_int4_wg8): n_wgs != 0 turns it on.  The rows'
    // partials then sit at (row * max_slots + slot) and the merge takes each row's count from attend_stream_count().
    uint32_t scale_run = 0;          // FP8 class forms: the allocation's run-order scale table (CodecArgs::scale_run), 0 = none (gather from the page-order table)
    uint32_t fp8_cls = 0;            // FP8 over a regularly striped pool: k_attend_fp8_dma<2>, pages by residue class (n_splits / tiles_per_split count class-major tiles)
    using Stream = AttendStream;     // (ring_rule.hpp: {len, rem, n_wgs, max_slots, tiles})
    Stream stream;                   // tiles: per layer, 0 = ceil(n_pages / 16) (the class form of INT4_G32 over a striped pool counts by residue class)
    // planned batches, MXFP4: the position a sequence still keeps OUTSIDE the pool (the connector's odd last position, fp16 rows
    // [tail][layers][heads][128], tail_stride elements apart) is folded in by the attention kernel itself -- by the workgroup of
    // split 0, into its partial or final state, in the epilogue -- instead of by a launch of its own behind every layer's attention.
    // tail_idx[sequence] = index of its tail rows, < 0: none; null with tail_k set: sequence i has tail i.  Every sequence of such a
    // launch has at least one split (the engine sends batches with an empty member through k_attend_fold_tail as before).
    const uint16_t* tail_k;
    const uint16_t* tail_v;
    const int32_t* tail_idx;
    uint64_t tail_stride;
    // batch form under a sliding window (decode_window.hpp): seq_skip[sequence] = the leading POSITIONS (0..31, may be odd) of the
    // sequence's first tile that lie in front of its window -- their scores are -inf, as AttendArgs::skip_pages does per launch and per
    // page in the single-sequence form.  Null: no sequence of the launch is cut.  FP8: the WINDOW instances of k_attend_fp8_linear (linear,
    // striped, table) take it -- launch_attend_fp8_batch sends every launch that brings one to them, a table launch too (k_attend_fp8_dma<1>
    // has no leading mask and is passed over); INT4_G32 and MXFP4: the existing instances k_attend_int4_wg8<1|2>, k_attend_int4_wg and
    // k_attend_mx4<0|2>.  The forms by residue class have no leading mask: their launchers refuse it, the engine never plans them under a window.
    // The split pool: k_attend_k8v4<true> (launch_attend_k8v4 picks the instance by this pointer).
    const uint32_t* seq_skip;
};
// (the stream partition -- attend_stream_begin / _wg_of / _count -- is plain arithmetic the host decides with too: ring_rule.hpp)
// (the tiles of a range taken by residue class -- mx4_class_tiles / mx4_striped_tiles -- likewise: ring_rule.hpp)
#if defined(__HIPCC__)
// record address of page p in the striped form; `bases` = the allocation's run bases copied to LDS
__device__ __forceinline__ const uint8_t* attend_stripe_rec(const uint64_t* bases, uint32_t p, uint32_t n, uint32_t magic, uint32_t stride)
{
    const uint32_t q = n == 1u ? p : __umulhi(p, magic);              // (n is uniform: batches may mix single-run and striped sequences)
    return reinterpret_cast<const uint8_t*>(bases[p - q * n]) + static_cast<uint64_t>(q) * stride;
}
#endif
#if defined(__HIPCC__)
// rows of a sequence without positions in a batch launch that has no merge behind it (one wave per kv head).
// (Plain values, not the AttendArgs: a reference to the kernel's argument block makes the compiler keep it in memory,
// and the LDS-DMA kernels need its pointers in scalar registers.)
__device__ __forceinline__ void attend_zero_rows(float* direct_out, float* direct_lse, uint32_t g, uint64_t row, uint32_t lane)
{
    float* dst = direct_out + row * g * 128u;
    for (uint32_t i = lane; i < g * 128u; i += 64u) dst[i] = 0.0f;
    if (direct_lse && lane < g) direct_lse[row * g + lane] = -__builtin_inff();
}
#endif
// out / lse of rows d_rows[i] (null: i) += the position whose fp16 K / V rows are d_k_tail / d_v_tail [i][heads][128]
// (consecutive i tail_stride_elems apart); see k_attend_fold_tail
hipError_t launch_attend_fold_tail(uint32_t n_rows, const uint32_t* d_rows, uint32_t heads, uint32_t g, const void* d_q_f16,
                                   const void* d_k_tail, const void* d_v_tail, uint64_t tail_stride_elems, float sm_scale,
                                   float* d_out, float* d_lse, hipStream_t s, uint32_t n_layers = 1, uint32_t layer_rows = 0);
// (n_layers > 1: the same rows for n_layers consecutive layers in one launch -- layer l's q / out / lse row blocks start l * layer_rows
//  row blocks further on, its tail rows l * heads * 128 elements further on)
// the positions a multi-position step holds outside the pool, folded causally into rows [n_seq][heads][g][128] with g = n_q x rows_per_pos:
// query position j of sequence i += held positions 0 .. d_base[i] + j (fp16 rows at i * seq_stride + t * pos_stride + head * 128);
// positions >= d_n_q[i] (null: none) untouched; see k_attend_fold_held
hipError_t launch_attend_fold_held(uint32_t n_rows, const uint32_t* d_rows, uint32_t heads, uint32_t g, uint32_t rows_per_pos, const void* d_q_f16,
                                   const void* d_k_held, const void* d_v_held, uint64_t seq_stride_elems, uint64_t pos_stride_elems,
                                   const uint32_t* d_base, const uint32_t* d_n_q, float sm_scale, float* d_out, float* d_lse, hipStream_t s);
// the same with visibility from a mask: query position j of sequence i += the held positions t whose bit is set in d_mask[i * mask_stride + j]
// (bits >= SPECKV_HELD_MAX dropped; a word of 0 leaves the position's rows untouched); see k_attend_fold_masked
hipError_t launch_attend_fold_masked(uint32_t n_rows, const uint32_t* d_rows, uint32_t heads, uint32_t g, uint32_t rows_per_pos, const void* d_q_f16,
                                     const void* d_k_held, const void* d_v_held, uint64_t seq_stride_elems, uint64_t pos_stride_elems,
                                     const uint32_t* d_mask, uint32_t mask_stride, float sm_scale, float* d_out, float* d_lse, hipStream_t s);
// a.lin_base set: linear form (a.scale_tab, a.q16); else page-table form (a.q8 / a.qs from launch_quantize_q_e4m3); kernel: the one the engine's
// decision names (attend_geometry.hpp: seq_decide_fp8)
enum Fp8Kernel : uint32_t;
hipError_t launch_attend_fp8(const AttendArgs& a, Fp8Kernel kernel, uint32_t n_layers, float* d_out, float* d_lse, hipStream_t s);
// scale_tab[tile order of p] = entries[p].rec_bytes >= 2048 ? entries[p].scale : 0 for every page (set_layout time)
hipError_t launch_build_scale_tab(const PageEntry* d_entries, uint64_t n_pages, uint32_t region_pages, float* d_scale_tab, hipStream_t s, uint32_t scale_run = 0);
// the run-order part of a scale table (CodecArgs::scale_run): index of page p relative to scale_tab
__host__ __device__ inline int64_t scale_run_index(uint64_t p, uint32_t scale_run)
{
    const uint32_t D = scale_run & 15u, cap = scale_run >> 4;
    return -static_cast<int64_t>(D) * cap + static_cast<int64_t>(p % D) * cap + static_cast<int64_t>(p / D);
}
// position of page-in-tile j (0..15) in the tile order [kb][r]: pages 2kb, 2kb+1, 8+2kb, 9+2kb of lane group kb
__host__ __device__ inline uint32_t attend_tile_slot(uint32_t j) { return j < 8u ? ((j >> 1) << 2) + (j & 1u) : (((j - 8u) >> 1) << 2) + 2u + (j & 1u); }
// INT4_G32 records (attend_int4.hip; a.lin_base set: linear form, else page-table form with a.entries / a.zero_page;
// a.q8 = the fp16 query rows
// [layers][heads][g][128]); writes the split partials, launch_attend_combine merges them
hipError_t launch_attend_int4(const AttendArgs& a, uint32_t n_layers, hipStream_t s);
hipError_t launch_attend_combine(const AttendArgs& a, uint32_t n_layers, float* d_out, float* d_lse, hipStream_t s);
// MXFP4 records (attend_mx4.hip): a.lin_base | a.stripe_bases | a.table_form choose the address form, a.q16 = the fp16 query rows,
// a.seqs the batch descriptors; n_rows = layers or sequences.  Launches the merge itself when the rows are not final.
hipError_t launch_attend_mx4(const AttendArgs& a, uint32_t n_rows, float* d_out, float* d_lse, hipStream_t s);
// scores only, linear form (a.lin_base, a.scale_tab, a.q16, a.tiles_per_split): d_out [layers][heads][g][2*n_pages]
hipError_t launch_qk_scores_fp8_linear(const AttendArgs& a, uint32_t n_layers, float* d_out, hipStream_t s);
// batch form: a.seqs (device) holds n_seq descriptors, a.q16 = [n_seq][heads][g][128], a.n_splits = the largest
// per-sequence split count; d_out [n_seq][heads][g][128]
hipError_t launch_attend_fp8_batch(const AttendArgs& a, uint32_t n_seq, float* d_out, float* d_lse, hipStream_t s);
// The split pool's batch decode attention (attend_kv.hip: k_attend_k8v4): K from FP8_E4M3 records, V from MXFP4 records of a second
// allocation.  a.seqs carries the K side (lin_base, scale_tab, k_first) and the split bookkeeping, as for launch_attend_fp8_batch; the
// V side rides beside it, one AttendKvSide per sequence: AttendSeq stays 64 bytes and AttendArgs what every other kernel takes by value.
struct AttendKvSide {
    const uint8_t* v_base;            // the V allocation's tile-planar run (Allocation::linear_base)
    uint64_t v_first;                 // first record of the wanted layer's V region: a multiple of kMx4TileRecs
};
// a.direct_out == d_out, a.direct_per_seq == 1: sequences with one split are written final, those without positions as zeros / lse -inf;
// merge: some sequence has several splits -- launch_attend_combine follows on `s`.  a.seq_skip set: the launch under a sliding window
// (k_attend_k8v4<true>: the descriptors start at the window's tile, seq_skip[sequence] leading positions of its tile 0 masked), else the plain instance
hipError_t launch_attend_k8v4(const AttendArgs& a, const AttendKvSide* d_vside, uint32_t n_seq, bool merge, float* d_out, float* d_lse, hipStream_t s);
// The step of several positions over the split pool (k_attend_k8v4<false, true>; speckv_ext_attend_kv_spec): what the caller holds outside
// the pool, folded in by split 0 of every sequence inside the attention launch.  A struct of its own beside AttendArgs, which keeps its
// size and layout for every other kernel.  Held position t of sequence i, kv head h: fp16 at i * seq_stride + t * pos_stride + h * 128
// elements (both strides multiples of 8: a lane reads 16 bytes at a time); query position j = row / rows_per_pos of sequence i sees the held
// positions whose bit is set in mask[i * mask_stride + j] (bits >= SPECKV_HELD_MAX dropped).  No held position above the highest bit set in
// any word of a sequence is read.
struct AttendHeldArgs {
    const uint16_t* k_held;
    const uint16_t* v_held;
    uint64_t seq_stride, pos_stride;  // elements
    const uint32_t* mask;
    uint32_t mask_stride, rows_per_pos;
    // under a window only (k_attend_k8v4<true, true>): depth[i * mask_stride + j] = the depth of query position j of sequence i in the
    // step's tree (0 = a root), strided like the mask words; NULL otherwise
    const uint32_t* depth;
};
// launch_attend_k8v4 with the held positions; a.g = n_q x h.rows_per_pos.  a.seq_skip set (with h.depth): the step under a sliding window,
// k_attend_k8v4<true, true> -- seq_skip[sequence] is then the sequence's signed rel of spec_window.hpp, not a position count.
hipError_t launch_attend_k8v4_held(const AttendArgs& a, const AttendKvSide* d_vside, const AttendHeldArgs& h, uint32_t n_seq, bool merge, float* d_out,
                                   float* d_lse, hipStream_t s);

// every page's record (rec_bytes rounded up to 16) copied to d_new_addr[page], then entries[page].pool_addr = d_new_addr[page]
hipError_t launch_repack(PageEntry* d_entries, const uint64_t* d_new_addr, uint64_t n, hipStream_t s);
// entries[i].pool_addr = base + i*stride (record bytes / scale untouched): after a migration.  stride == kPlanarMx4: record
// rec0 + i of the tile-planar run at base (address and code delta, record bytes untouched)
hipError_t launch_retarget_entries(PageEntry* d_entries, uint64_t n, uint64_t base, uint64_t stride, hipStream_t s, uint64_t rec0 = 0);


// Token predictor (lstm_predictor.cpp:40-188): n histories of 16 tokens -> top-k (k <= 8) tokens and
// confidences.  d_emb [vocab][64], d_wout [vocab][128]; d_hid (n*128 floats) and d_logits (n*vocab
// floats) are scratch.
// lstm != nullptr && lstm->layers > 0: a real LSTM cell (PyTorch nn.LSTM conventions, k_lstm_cell) instead of the reference's
// degenerate one; bias[l] = b_ih[l] + b_hh[l]; out_bias may be null
struct LstmParams { const float* w_ih_t[4]; const float* w_hh_t[4]; const float* bias[4]; const float* out_bias; uint32_t layers; };   // weights arranged: lstm_arranged_index
// Where k_lstm_cell wants the weight (gate row, column) of a 512 x cols matrix.  The kernel numbers the gate rows
// v = 4 * unit + gate (the four gates of a hidden unit next to each other; nn.LSTM's row is 128 * gate + unit).  Thread
// tid = 8 * (v / 8) + s keeps the column slice s = col / (cols / 8) of the eight rows v / 8 * 8 + 0..7, as register
// q = i * (cols / 8) + col % (cols / 8) with i = (v % 8) ^ s (the xor makes the reduction over the eight slices free of
// selects); the array is [q][512 threads], read coalesced.
inline uint32_t lstm_cell_row(uint32_t row) { return 4u * (row % 128u) + row / 128u; }
inline size_t lstm_arranged_index(uint32_t row, uint32_t col, uint32_t cols)
{
    const uint32_t v = lstm_cell_row(row), cs = cols / 8u, s = col / cs, c = col % cs, i = (v & 7u) ^ s, tid = (v & ~7u) + s;
    return static_cast<size_t>(i * cs + c) * 512u + tid;
}
hipError_t launch_predict(uint32_t n, const int32_t* d_hist, const float* d_emb, const float* d_wout, uint32_t vocab,
                          uint32_t layers, uint32_t k, float* d_hid, float* d_logits, void* d_ws, int32_t* d_tok, float* d_conf,
                          hipStream_t s, const LstmParams* lstm = nullptr);
// d_wout: the output layer's weights ARRANGED by launch_arrange_wout (arranged_wout_bytes(vocab) bytes) from the row-major [vocab][128]
size_t arranged_wout_bytes(uint32_t vocab);
hipError_t launch_arrange_wout(const float* d_src, float* d_dst, uint32_t vocab, hipStream_t s);
// d_ws: predict_ws_bytes(n, vocab) bytes of scratch (the parts of the split top-k: 4096 logits each, at most 64 -- larger
// vocabularies take the one-workgroup kernel and need none)
constexpr uint32_t kPredictTopkSpan = 4096, kPredictTopkMaxParts = 64, kPredictWsPerPart = 8 + 8 * 8;
inline uint32_t predict_topk_parts(uint32_t vocab)
{
    const uint32_t parts = (vocab + kPredictTopkSpan - 1u) / kPredictTopkSpan;
    return parts <= kPredictTopkMaxParts ? parts : 0u;
}
// a handful of requests take k_predict_small: parts of 128 rows, at most kPredictSmallMaxParts of them (vocabularies up to 32 768)
constexpr uint32_t kPredictSmallN = 4, kPredictSmallMaxParts = 256;
inline size_t predict_ws_bytes(uint32_t n, uint32_t vocab)
{
    const size_t batch = static_cast<size_t>(n) * predict_topk_parts(vocab) * kPredictWsPerPart;
    const size_t small = static_cast<size_t>(kPredictSmallN) * kPredictSmallMaxParts * kPredictWsPerPart;
    return (batch > small ? batch : small) + 64;
}

} // namespace speckv
