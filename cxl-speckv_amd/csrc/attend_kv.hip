// cxl-speckv_amd/csrc/attend_kv.hip -- batch decode attention straight from the records of the SPLIT POOL ("K8V4"): a sequence's K rows
// in an FP8_E4M3 allocation, its V rows in an MXFP4 allocation (kv_split_connector.py).  One new position per sequence
// (g query rows per kv head), no fp16 K or V is materialised.  The HELD instance serves a step of SEVERAL new positions per sequence (draft
// positions to verify): the same walk for g = positions x rows per position, the rows held outside the pool folded in by split 0.
//
// The workgroup shape and the K side are k_attend_fp8_linear<false>'s (attend.hip): one wave = one kv head of one sequence over one
// contiguous split of its positions, tiles of 32 positions (16 pages), four waves = four heads of the same split; grid (splits,
// sequences x heads / 4) or rows-first.  Lane (c = lane % 16, kb = lane / 16) owns query row c:
//   scores  S^T = K . q^T on the FP8 MFMA (16x16x32): the fp16 query quantised here to E4M3 x a row scale (the FP8 kernel's own
//           functions, attend_fp8_device.hpp: the same bits), the K bytes as they lie in the record, the page scale (the K allocation's scale table, tile order) on the
//           score in fp32.  The lane ends with sc[8]: sc[j] = page slot j / 2 (pages 2kb, 2kb + 1, 8 + 2kb, 9 + 2kb of the tile), position j % 2.
//   output  O^T = V^T . P^T on v_mfma_f32_16x16x32_f16.  An MXFP4 head row of a page is 128 bytes [channel], low nibble = position 0, high
//           nibble = position 1, one E8M0 code per 16 bytes.  The lane holds bytes 8c .. 8c + 7 of its four pages; for MFMA t (channel
//           8c + t) v_cvt_scalef32_pk_f16_fp4 turns byte t of each page into the f16 pair (position 0, position 1) x 2^(code - 127): two
//           consecutive k slots, four conversions = one f16x8 in exactly the k order of the weights P[j].  The lane's 8 channels lie in
//           block c / 2: ONE code per page.  The block scale sits inside the conversion, the weights are the plain p in f16: there is no
//           per-tile V reference scale as in the FP8 kernel.
//           -> lane (c, kb) holds out[query row c][32kb + 8i + t] in acc[t][i].
// Per tile and wave: 4 sixteen-byte K loads, one load of 4 page scales, 4 eight-byte V loads, 4 code bytes (the FP8 kernel: 8 eight-byte
// V loads and a second scale load).  Register-staged like that kernel: ONE register set, K(t + 1) requested behind the scores of tile t,
// V(t + 1) behind p.V.
//
// V records are tile-planar (kernels.hpp: mx4_nib_off, mx4_code_delta, kMx4CodePlane); a region starts on a multiple of 16 records
// (num_tokens % 32 == 0), so a kernel tile is exactly one storage tile of 17 408 bytes: nibble rows at + 1024 page, code rows at
// kMx4CodePlane + 64 page.  Never-written records are zero bytes on both sides: K scale 0 -> score 0 (NOT -inf), V = 0.
#include "kernels.hpp"
#include "attend_fp8_device.hpp"     // the K side's tile arithmetic, shared with attend.hip
#include "spec_window.hpp"           // the walk rule of the held step under a window

namespace speckv {

constexpr uint32_t kHeldMax = 17;                      // SPECKV_HELD_MAX (include/speckv_ext.h)

// The held positions of a step (k_attend_k8v4<false, true>), folded into the running state of query row c by the wave of split 0.
// 64 bytes of a held row: channels 32kb .. 32kb + 31 of kv head `head`
struct HeldPiece { uint4 w[4]; };
__device__ __forceinline__ HeldPiece held_piece(const uint16_t* rows, uint64_t at)
{
    HeldPiece p;
#pragma unroll
    for (int i = 0; i < 4; ++i) p.w[i] = ldg16_temporal(reinterpret_cast<const uint8_t*>(rows + at) + 16 * i);
    return p;
}
__device__ __forceinline__ float held_f16(uint32_t w, int hi) { return static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(w >> (16 * hi)))); }

__device__ __forceinline__ void k8v4_fold_held(const AttendArgs& a, const AttendHeldArgs& h, uint32_t seq, uint32_t head, uint64_t row, uint32_t c, uint32_t kb,
                                               float& m_run, float& l_run, f32x4 (&acc)[8])
{
    // the word of the lane's query position; a lane without a query row sees nothing
    uint32_t word = 0u;
    if (c < a.g) word = *SPECKV_GP(uint32_t, h.mask + static_cast<uint64_t>(seq) * h.mask_stride + c / h.rows_per_pos) & ((1u << kHeldMax) - 1u);
    uint32_t n_held = 0u;                                                // 1 + the highest bit set in any word of the sequence (wave-uniform)
#pragma unroll
    for (uint32_t t = 0; t < kHeldMax; ++t)
        if (__builtin_amdgcn_ballot_w64((word >> t) & 1u) != 0ull) n_held = t + 1u;
    if (n_held == 0u) return;
    const uint64_t at0 = static_cast<uint64_t>(seq) * h.seq_stride + head * 128u + 32u * kb;
    // K two positions deep, V one: the next K row is requested in front of the score, the next V row behind the accumulation
    HeldPiece kn = held_piece(h.k_held, at0), vx = held_piece(h.v_held, at0);
    const HeldPiece q = held_piece(a.q16, (row * a.g + min(c, a.g - 1u)) * 128u + 32u * kb);
#pragma unroll 1
    for (uint32_t t = 0; t < n_held; ++t) {
        const HeldPiece kx = kn;
        const bool more = t + 1u < n_held;                                // scalar: nothing above the highest visible position is read
        const uint64_t at = at0 + static_cast<uint64_t>(t + 1u) * h.pos_stride;
        if (more) kn = held_piece(h.k_held, at);
        const bool sees = (word >> t) & 1u;
        float dot = 0.0f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t qw[4] = {q.w[i].x, q.w[i].y, q.w[i].z, q.w[i].w}, kw[4] = {kx.w[i].x, kx.w[i].y, kx.w[i].z, kx.w[i].w};
            // v_dot2_f32_f16 on the words as they were loaded: a query widened to 32 floats would not fit beside the accumulators
#pragma unroll
            for (int e = 0; e < 4; ++e) dot = __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2, qw[e]), __builtin_bit_cast(f16x2, kw[e]), dot, false);
        }
        const float s = sees ? sum_over_kb(dot) * a.scale_log2e : -INFINITY;
        // the loop's online-softmax step over this one position
        const float m_new = fmaxf(m_run, s);
        const float m_use = (m_new == -INFINITY) ? 0.0f : m_new;
        const float f = __builtin_amdgcn_exp2f(m_run - m_use);
        const float p = __builtin_amdgcn_exp2f(s - m_use);
        m_run = m_new;
        l_run = l_run * f + (kb == 0u ? p : 0.0f);                        // (att_store_rows8 sums l_run over kb: the weight enters one lane)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t vw[4] = {vx.w[i].x, vx.w[i].y, vx.w[i].z, vx.w[i].w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float pv = p * held_f16(vw[e >> 1], e & 1);
                acc[e][i] = acc[e][i] * f + (sees ? pv : 0.0f);
            }
        }
        if (more) vx = held_piece(h.v_held, at);
    }
}

// k_attend_k8v4<true, true>: the leading positions of the sequence's walk that the lane's query row does not see (spec_window.hpp) -- rel of
// the sequence + the depth of the row's query position, from the depth table that lies beside the mask words.  A lane without a query
// row reads no depth.
__device__ __forceinline__ uint32_t k8v4_row_skip(const AttendHeldArgs& h, uint32_t g, uint32_t seq, uint32_t c, int32_t rel)
{
    uint32_t depth = 0u;
    if (c < g) depth = *SPECKV_GP(uint32_t, h.depth + static_cast<uint64_t>(seq) * h.mask_stride + c / h.rows_per_pos);
    return spec_window_skip(rel, depth);
}

// a.seqs: the K side and the split bookkeeping of every sequence (lin_base, scale_tab, k_first of the K allocation; v_first and
// layer_pages are not read); vside[sequence]: the V allocation's run and the first record of the layer's V region (a multiple of 16).
// a.direct_out / direct_lse are always set: a sequence with ONE split is written final, one without positions as zeros / -inf, the
// others leave partials (part_acc / part_ml, true units) for launch_attend_combine, which skips the single-split sequences.
// WINDOW: the launch under a sliding window (AttendArgs::seq_skip, decode_window.hpp; speckv_ext_attend_kv_batch_window) -- the descriptors
// start at the tile of the window's lower bound, seq_skip[sequence] = the leading POSITIONS (0..31, may be odd) of the sequence's tile 0
// in front of it.  An instance of its own, for k_attend_fp8_linear<.., WINDOW>'s reason (attend.hip): carried by the plain instance the
// position mask cost the unwindowed FP8 entries 3 %.  k_attend_k8v4<false, false> is the kernel of before, instruction for instruction.
// HELD: the step of several positions (speckv_ext_attend_kv_spec) -- g = n_q x rows_per_pos query rows per kv head, row r of query position
// r / rows_per_pos; every row sees every stored position, so the walk is the plain one.  Split 0 of every sequence then folds in, in front of
// att_store_rows8, the positions the caller holds outside the pool (AttendHeldArgs: fp16 rows, one mask word per query position) with the
// online-softmax step of the loop -- into its final rows or its partial, the merge runs as ever; a sequence with nothing stored runs that
// epilogue alone.  The held scores take the FP16 query (the stand-alone folds' choice): the fp32 dot of the lane group's channels 32kb ..
// 32kb + 31, summed over kb, in log2 units; a position a row does not see is -inf and its V contribution 0, both by a select.  A lane reads
// the 64 bytes of channels 32kb .. 32kb + 31 of a held row for K and for V (acc[t][i] = channel 32kb + 8i + t: element t of the i-th 16
// bytes), one position computed while the next one's rows are under way; the loop ends at the highest bit set in any word of the sequence
// and no held position above that is read.  `held` is AttendHeldArgs for HELD and empty otherwise: the plain instances keep their argument block.
// WINDOW and HELD (speckv_ext_attend_kv_spec_window): the step of several positions on a sliding-window layer.  The rows of a wave no longer
// share a lower bound -- a node of depth d sits at length + d and sees the stored positions from length + d + 1 - W on -- so the descriptors
// start at the tile of DEPTH 0's bound, a.seq_skip[sequence] carries the signed rel of spec_window.hpp instead of a position count, and the
// lane masks its eight scores by its own row's skip = max(0, rel + depth) <= 46: in tiles 0 and 1 of the walk (the gate is wave-uniform:
// tiles whose first position lies at or behind rel + 15 carry no mask).  A row may be masked throughout a tile or a whole piece: it then
// carries m_run = -inf, l_run = 0, which att_softmax_step, k8v4_fold_held, att_store_rows8 and both merges turn into weight 0.  The held
// positions are folded as in <false, true>: what a node sees of them under the window lies in the mask words alone.
template <bool WINDOW, bool HELD, class... Held>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_attend_k8v4(AttendArgs a, const AttendKvSide* __restrict__ vside, Held... held)
{
    static_assert(sizeof...(Held) == (HELD ? 1 : 0), "instances: <false, false>, <true, false>, <false, true, AttendHeldArgs>, <true, true, AttendHeldArgs>");
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t c = lane & 15u, kb = lane >> 4;
    const uint32_t split = a.rows_first ? blockIdx.y : blockIdx.x, by = a.rows_first ? blockIdx.x : blockIdx.y;
    if (a.rows_first && by >= a.rows_real) return;                      // (padding row: see AttendArgs::rows_real)
    const uint32_t hq = a.heads / 4u;
    uint32_t seq = by / hq;
    if (a.order) seq = a.order[seq];                                     // (workgroup-uniform)
    const uint32_t head = (by % hq) * 4u + wave;
    const uint64_t row = static_cast<uint64_t>(seq) * a.heads + head;    // query / output row block
    const AttendSeq sq = a.seqs[seq];
    if (split >= sq.n_splits) {
        if constexpr (!HELD) {
            if (sq.n_splits == 0u && split == 0u) attend_zero_rows(a.direct_out, a.direct_lse, a.g, row, lane);
            return;
        } else if (sq.n_splits != 0u || split != 0u) return;             // (nothing stored: split 0 goes on to the held positions alone)
    }
    const AttendKvSide vsd = vside[seq];
    const uint64_t part = sq.part_base + static_cast<uint64_t>(head) * sq.n_splits + split;
    const uint32_t n_pages = sq.n_pages;
    const uint32_t skip_pos = (WINDOW && !HELD) ? a.seq_skip[seq] : 0u;  // (workgroup-uniform)
    // WINDOW and HELD: that word is the sequence's signed rel; row_skip = the lane's own row, cut_pos = depth 0's = the least of any row (uniform)
    uint32_t row_skip = 0u, cut_pos = 0u;
    int32_t rel = 0;
    if constexpr (WINDOW && HELD) {
        rel = static_cast<int32_t>(*SPECKV_GP(uint32_t, a.seq_skip + seq));
        row_skip = k8v4_row_skip(held..., a.g, seq, c, rel);
        cut_pos = spec_window_skip(rel, 0u);
    }

    // query operand (fp8_query_operand): row c of this head, lane kb takes d = 16kb .. 16kb + 15 of both 64-element halves, the split the
    // K loads follow; rows >= g are zero
    uint32_t qd[8];
    float qscale = 1.0f;
    auto quantise_query = [&]() { fp8_query_operand(a.q16 + (row * a.g + min(c, a.g - 1u)) * 128u + kb * 16u, c < a.g, a.scale_log2e, qd, qscale); };

    const uint32_t n_tiles = (n_pages + 15u) / 16u;
    const uint32_t t0 = split * sq.tiles_per_split;
    const uint32_t t1 = min(t0 + sq.tiles_per_split, n_tiles);
    float m_run = -INFINITY, l_run = 0.0f;
    f32x4 acc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    if (t0 < t1) {                                                       // wave-uniform
        // running pointers of the tile being requested.  K: row 16b + c of the tile, bytes [16kb, 16kb + 16) of both halves; block b: + 16 KiB
        const uint8_t* kp = sq.lin_base + sq.k_first * 2048ull + head * 128u + kb * 16u + (static_cast<uint64_t>(t0) * 32u + c) * 1024u;
        const float* kt = sq.scale_tab + (sq.k_first + static_cast<uint64_t>(t0) * 16u) + 4u * kb;
        // V: the storage tile of kernel tile t0; the lane's page slot r = page 2kb + (r & 1) + 8 (r >> 1): nibbles + 1024 page, codes behind the plane
        const uint8_t* vtile = vsd.v_base + ((vsd.v_first >> 4) + t0) * static_cast<uint64_t>(kMx4TileBytes);
        const uint8_t* vp = vtile + 2u * kb * 1024u + head * 128u + 8u * c;
        const uint8_t* vc = vtile + kMx4CodePlane + 2u * kb * 64u + head * 8u + (c >> 1);

        uint4 kx[2][2];
        uint2 vx[4];
        uint32_t vcode[4];
        f32x4 ks4;
        auto issue_k = [&]() {
#pragma unroll
            for (int b = 0; b < 2; ++b) { kx[b][0] = ldg16(kp + 16384 * b); kx[b][1] = ldg16(kp + 16384 * b + 64); }
            ks4 = ldg_f4(kt);
        };
        auto issue_v = [&]() {
#pragma unroll
            for (int r = 0; r < 4; ++r) vx[r] = ldg8(vp + 1024 * (r & 1) + 8192 * (r >> 1));
#pragma unroll
            for (int r = 0; r < 4; ++r) vcode[r] = ldg1(vc + 64 * (r & 1) + 512 * (r >> 1));
        };
        // same request order as in the loop (K before V), pinned, so that the wait at the loop head is "everything up to K" on both paths into it
        __builtin_amdgcn_sched_barrier(0);
        issue_k();
        __builtin_amdgcn_sched_barrier(0);
        issue_v();
        __builtin_amdgcn_sched_barrier(0);
        quantise_query();                                                // (its loads are the youngest: they and the tile arrive together)
        __builtin_amdgcn_sched_barrier(0);
        const bool ragged = (n_pages & 15u) != 0u;
#pragma unroll 1
        for (uint32_t tile = t0; tile < t1; ++tile) {
            // the refills are unconditional -- the last iteration re-requests its own tile -- so the loop body is one basic block
            const uint32_t step = (tile + 1u < t1) ? 1u : 0u;            // scalar
            // ---- scores
            float sc[8];
#pragma unroll
            for (int b = 0; b < 2; ++b) fp8_scores(kx[b][0], kx[b][1], qd, ks4, qscale, b, sc);
            if (ragged && tile + 1u == n_tiles) {                         // wave-uniform: pages at or beyond pos_end (even: whole pages)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const uint32_t pg = tile * 16u + att_slot_page(kb, r);
                    // (the masked page's code goes too: it may be a stale record of any magnitude, and its weight of exactly 0 must meet a finite value)
                    if (pg >= n_pages) { sc[2 * r] = -INFINITY; sc[2 * r + 1] = -INFINITY; vcode[r] = 0u; }
                }
            }
            // WINDOW: the positions of the sequence's tile 0 in front of the window.  `tile` is the absolute tile of the sequence, so only split 0
            // comes here.  Where n_pages > 0 the window's lower bound lo = skip_pos is visible and lies in tile 0: no piece is masked throughout,
            // m_run is finite from the first tile on.
            if (WINDOW && !HELD && tile == 0u && skip_pos != 0u) {        // wave-uniform
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const uint32_t pg = att_slot_page(kb, r);
                    if (2u * pg < skip_pos) sc[2 * r] = -INFINITY;
                    if (2u * pg + 1u < skip_pos) sc[2 * r + 1] = -INFINITY;
                    // a page masked in both positions loses its code as in the ragged branch (a stale or hostile record meets its weight of 0 as a
                    // small finite number).  A CUT page (skip_pos odd: position 0 masked, position 1 kept) keeps it: the kept nibble is stored in
                    // units of that code, the masked nibble's weight is exactly 0, and an MXFP4 value widened to fp16 by the conversion is finite
                    // (both positions of a page are encoded together from fp16 rows: the block's code keeps 6 x 2^(code - 127) inside fp16), so 0 x it is 0
                    if (2u * pg + 2u <= skip_pos) vcode[r] = 0u;
                }
            }
            // WINDOW and HELD: the mask is the ROW's.  Tiles whose first position lies below rel + 15, the deepest row's bound, can carry one:
            // tiles 0 and 1 (rel <= 31).  The V bytes and code bytes of a lane are not its query row's: they belong to the lane as holder of
            // channels 8c .. 8c + 7 and meet EVERY row's weights in the MFMA.  So a page's code may go only where the page is masked for every
            // row, 2 page + 2 <= cut_pos (depth 0's bound, wave-uniform) -- the windowed instance's reason: a stale or hostile record in front
            // of every window meets its weights of 0 as a small finite number.  Pages between that bound and a deeper row's own are stored,
            // encoded records some shallower row still reads in their code's units; for the deeper row a weight of exactly 0 meets a finite
            // fp16 value there (an MXFP4 value widened by the conversion is finite), and 0 x it is 0.
            if constexpr (WINDOW && HELD) {
                if (tile < 2u && static_cast<int32_t>(tile * 32u) < rel + static_cast<int32_t>(kSpecWindowMaxDepth)) {      // wave-uniform
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const uint32_t p0 = 2u * (tile * 16u + att_slot_page(kb, r));
                        if (p0 < row_skip) sc[2 * r] = -INFINITY;
                        if (p0 + 1u < row_skip) sc[2 * r + 1] = -INFINITY;
                        if (p0 + 2u <= cut_pos) vcode[r] = 0u;
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            kp += step * 32768u; kt += step * 16u;
            issue_k();
            __builtin_amdgcn_sched_barrier(0);
            // ---- online softmax of query row c
            float m_use;
            const float f = att_softmax_step(sc, m_run, m_use);
            float psum = 0.0f;
            f16x8 P;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float p = __builtin_amdgcn_exp2f(sc[j] - m_use);
                psum += p;
                P[j] = static_cast<_Float16>(p);
            }
            l_run = l_run * f + psum;
            // ---- out^T += V^T . P^T: byte t of a page = channel 8c + t of both positions -> one operand register
            float vsc[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) vsc[r] = __uint_as_float(vcode[r] << 23);        // the block's E8M0 code as a float's exponent field
#define KV_PV(T, WORD, SEL)                                                                                                       \
    {                                                                                                                              \
        const u32x4 vw = {__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(vx[0].WORD, vsc[0], SEL)),          \
                          __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(vx[1].WORD, vsc[1], SEL)),          \
                          __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(vx[2].WORD, vsc[2], SEL)),          \
                          __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(vx[3].WORD, vsc[3], SEL))};         \
        acc[T] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, vw), P, acc[T] * f, 0, 0, 0);                     \
    }
            KV_PV(0, x, 0) KV_PV(1, x, 1) KV_PV(2, x, 2) KV_PV(3, x, 3) KV_PV(4, y, 0) KV_PV(5, y, 1) KV_PV(6, y, 2) KV_PV(7, y, 3)
#undef KV_PV
            __builtin_amdgcn_sched_barrier(0);
            vp += step * kMx4TileBytes; vc += step * kMx4TileBytes;
            issue_v();
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if constexpr (HELD) {
        if (split == 0u) k8v4_fold_held(a, held..., seq, head, row, c, kb, m_run, l_run, acc);      // workgroup-uniform
    }
    // ---- a single split: the final rows; otherwise the partial of this split (acc is in true units here: unit 1)
    att_store_rows8(a, acc, m_run, l_run, 1.0f, HELD ? sq.n_splits <= 1u : sq.n_splits == 1u, row, part, c, kb);
}

// a.seqs / d_vside (device-visible) hold n_seq descriptors, a.n_splits = the largest per-sequence split count (0: no sequence has positions),
// a.direct_out = d_out and a.direct_per_seq = 1; merge = some sequence has several splits (launch_attend_combine behind the attention launch)
hipError_t launch_attend_k8v4(const AttendArgs& a, const AttendKvSide* d_vside, uint32_t n_seq, bool merge, float* d_out, float* d_lse, hipStream_t s)
{
    if (n_seq == 0) return hipSuccess;
    if (!a.seqs || !d_vside || !a.q16 || a.direct_out != d_out || a.heads % 4u || a.g == 0 || a.g > 16u) return hipErrorInvalidValue;
    AttendArgs ar = a;
    const uint32_t rows = n_seq * (a.heads / 4u), splits = a.n_splits ? a.n_splits : 1u;      // (split 0 of a sequence without positions writes its zeros)
    ar.rows_real = rows;
    const dim3 gr = a.rows_first ? dim3(rows | 1u, splits) : dim3(splits, rows);
    if (a.seq_skip) hipLaunchKernelGGL((k_attend_k8v4<true, false>), gr, dim3(256), 0, s, ar, d_vside);      // under a window that cuts a sequence
    else hipLaunchKernelGGL((k_attend_k8v4<false, false>), gr, dim3(256), 0, s, ar, d_vside);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || !merge) return e;
    return launch_attend_combine(a, n_seq, d_out, d_lse, s);
}

// The step of several positions: the launch above with the held positions of every sequence folded in by its split 0 (k_attend_k8v4<false,
// true>).  a.seq_skip set: the step on a sliding-window layer (k_attend_k8v4<true, true>) -- the descriptors start at the tile of depth 0's
// bound, seq_skip[sequence] is the sequence's SIGNED rel (spec_window.hpp) and h.depth the depth table beside the mask words.
hipError_t launch_attend_k8v4_held(const AttendArgs& a, const AttendKvSide* d_vside, const AttendHeldArgs& h, uint32_t n_seq, bool merge, float* d_out,
                                   float* d_lse, hipStream_t s)
{
    if (n_seq == 0) return hipSuccess;
    if (!a.seqs || !d_vside || !a.q16 || a.direct_out != d_out || a.heads % 4u || a.g == 0 || a.g > 16u || (a.seq_skip && !h.depth)) return hipErrorInvalidValue;
    if (!h.k_held || !h.v_held || !h.mask || h.rows_per_pos == 0 || a.g % h.rows_per_pos || a.g / h.rows_per_pos > kHeldMax - 1u ||
        h.mask_stride < a.g / h.rows_per_pos || h.seq_stride % 8u || h.pos_stride % 8u)
        return hipErrorInvalidValue;
    AttendArgs ar = a;
    const uint32_t rows = n_seq * (a.heads / 4u), splits = a.n_splits ? a.n_splits : 1u;      // (split 0 of a sequence without positions folds its held ones)
    ar.rows_real = rows;
    const dim3 gr = a.rows_first ? dim3(rows | 1u, splits) : dim3(splits, rows);
    if (a.seq_skip) hipLaunchKernelGGL((k_attend_k8v4<true, true, AttendHeldArgs>), gr, dim3(256), 0, s, ar, d_vside, h);
    else hipLaunchKernelGGL((k_attend_k8v4<false, true, AttendHeldArgs>), gr, dim3(256), 0, s, ar, d_vside, h);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || !merge) return e;
    ar.direct_per_seq = 3u;                                              // the merge passes over the sequences without a split too: their rows are the softmax over the held positions
    return launch_attend_combine(ar, n_seq, d_out, d_lse, s);
}

} // namespace speckv
