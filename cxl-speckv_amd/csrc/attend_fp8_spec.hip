// cxl-speckv_amd/csrc/attend_fp8_spec.hip -- the draft step of an FP8_E4M3 pool on a SLIDING-WINDOW layer (speckv_ext_attend_spec_window):
// k_attend_fp8_spec, up to 16 query rows per kv head (g = positions x rows per position) over ONE FP8 allocation in one pass over the
// records, every row under its own lower bound, and the rows the caller holds outside the pool folded in inside the same launch.
//
// The workgroup shape, the operand maps, the grid and the descriptors are the FP8 batch form's (attend.hip, k_attend_fp8_linear<false>):
// one wave = one kv head of one sequence over one contiguous piece of its walk, tiles of 32 positions (16 pages), four waves = four
// heads of the same piece; grid (pieces, sequences x heads / 4) or rows-first (a.rows_first, a.rows_real), a.order the dispatch order,
// a.seqs one AttendSeq per sequence -- lin_base, scale_tab (tile order), k_first / v_first the first page of the layer's K / V region
// as that kernel reads them.  Linear placement only.  Lane (c = lane % 16, kb = lane / 16) owns query row c.  The arithmetic is
// attend_fp8_device.hpp's, called, not restated: fp8_query_operand behind the first tile's requests, fp8_scores on the K bytes as
// they lie, fp8_v_weights / fp8_pv8 with the V page scales on the f16 weights against the tile's reference scale, att_store_rows8.
// Register-staged like the linear batch instance: ONE register set, K(t + 1) requested behind the scores of tile t, V(t + 1) behind
// the accumulation, the refills unconditional and the request order pinned, so the s_waitcnt counts are exact.
//
// The mask is per ROW (spec_window.hpp).  The descriptor starts at the tile of depth 0's bound in both regions (begin / 2 pages in:
// a multiple of 16 records, so a kernel tile stays one group of the scale table), a.seq_skip[sequence] carries the member's SIGNED
// rel, and a lane masks its eight scores by its own row's skip = spec_window_skip(rel, depth of the row's query position) <= 46, the
// depth read from the table beside the mask words.  Only tiles 0 and 1 of a walk can carry a mask (rel <= 31); the gate is
// wave-uniform, and a window that cuts no row passes no gate: it pays the gate's scalar compare per tile and nothing else.  ONE instance.
// The V side: a lane's four V page scales are not its query row's -- they ride on the weights of EVERY row of the wave.  A scale may go
// to 0 only where the page is masked for every row, 2 page + 2 <= cut_pos = spec_window_skip(rel, 0): a stale or hostile record in front
// of every window (a scale of any magnitude, inf, NaN) then meets its weights of 0 as a finite number, and it stands for no election as
// the tile's reference scale.  The page CUT by depth 0's bound (cut_pos odd) stands with 2^-10 of its scale, k_attend_fp8_linear<..,
// WINDOW>'s rule and reason.  Pages between cut_pos and a deeper row's own bound are stored records with finite scales that some
// shallower row reads: the deeper row gives them a weight of exactly 0.  A row masked throughout a tile or a whole piece carries
// m_run = -inf, l_run = 0, which att_softmax_step, the held fold, att_store_rows8 and both merges turn into weight 0.
//
// Held rows: split 0 of every member folds in the positions held outside the pool -- the odd last position, then the new ones; fp16
// rows, one mask word per query position (AttendHeldArgs) -- in front of att_store_rows8, into its final rows or its partial:
// k8v4_fold_held (attend_kv_device.hpp), which depends on the accumulator map acc[t][i] = channel 32kb + 8i + t alone, the one
// att_store_rows8 fixes for the FP8 kernels too.  It works in true units, so the wave first leaves the reference scale's units
// (acc x vref).  A member with nothing walked -- nothing stored, or a window in which no row sees a pool position -- runs that epilogue alone.
//
// Resources (gfx950, -O3): 115 VGPRs, 0 AGPRs, no LDS, no scratch -- inside the 128 registers of four waves per SIMD, the linear batch
// instance's occupancy, which is the hint; five waves would leave 102 and spill the tile.  The build fails on scratch.
#include "attend_kv_device.hpp"      // k8v4_fold_held, k8v4_row_skip; with it attend_fp8_device.hpp and spec_window.hpp

namespace speckv {

__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void k_attend_fp8_spec(AttendArgs a, AttendHeldArgs h)
{
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
    if (split >= sq.n_splits && (sq.n_splits != 0u || split != 0u)) return;      // (nothing walked: split 0 goes on to the held positions alone)
    const uint64_t part = sq.part_base + static_cast<uint64_t>(head) * sq.n_splits + split;
    const uint32_t n_pages = sq.n_pages;
    // the member's signed rel; row_skip = the lane's own row, cut_pos = depth 0's = the least of any row (wave-uniform)
    const int32_t rel = static_cast<int32_t>(*SPECKV_GP(uint32_t, a.seq_skip + seq));
    const uint32_t row_skip = k8v4_row_skip(h, a.g, seq, c, rel), cut_pos = spec_window_skip(rel, 0u);

    uint32_t qd[8];
    float qscale = 1.0f;
    const uint32_t n_tiles = (n_pages + 15u) / 16u;
    const uint32_t t0 = split * sq.tiles_per_split;
    const uint32_t t1 = min(t0 + sq.tiles_per_split, n_tiles);
    float m_run = -INFINITY, l_run = 0.0f, vref = 1.0f;
    f32x4 acc[8];
#pragma unroll
    for (int t = 0; t < 8; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    if (t0 < t1) {                                                       // wave-uniform
        // running pointers of the tile being requested.  K: row 16b + c of the tile, bytes [16kb, 16kb + 16) of both halves; block b: + 16 KiB.
        // V: bytes 8c .. 8c + 7 of position slot j: + (j & 3) KiB + (j >> 2) x 16 KiB.  The scales of the lane's four slot pages: one load each.
        const uint8_t* kp = sq.lin_base + sq.k_first * 2048ull + head * 128u + kb * 16u + (static_cast<uint64_t>(t0) * 32u + c) * 1024u;
        const uint8_t* vp = sq.lin_base + sq.v_first * 2048ull + head * 128u + 8u * c + (static_cast<uint64_t>(t0) * 32u + 4u * kb) * 1024u;
        const float* kt = sq.scale_tab + (sq.k_first + static_cast<uint64_t>(t0) * 16u) + 4u * kb;
        const float* vt = sq.scale_tab + (sq.v_first + static_cast<uint64_t>(t0) * 16u) + 4u * kb;
        uint4 kx[2][2];
        uint2 vx[8];
        f32x4 ks4, vs4;
        auto issue_k = [&]() {
#pragma unroll
            for (int b = 0; b < 2; ++b) { kx[b][0] = ldg16(kp + 16384 * b); kx[b][1] = ldg16(kp + 16384 * b + 64); }
            ks4 = ldg_f4(kt);
        };
        auto issue_v = [&]() {
#pragma unroll
            for (int j = 0; j < 8; ++j) vx[j] = ldg8(vp + 1024 * (j & 3) + 16384 * (j >> 2));
            vs4 = ldg_f4(vt);
        };
        // same request order as in the loop (K before V), pinned, so that the wait at the loop head is "everything up to K" on both paths into it
        __builtin_amdgcn_sched_barrier(0);
        issue_k();
        __builtin_amdgcn_sched_barrier(0);
        issue_v();
        __builtin_amdgcn_sched_barrier(0);
        // (the query's loads are the youngest: they and the tile arrive together)
        fp8_query_operand(a.q16 + (row * a.g + min(c, a.g - 1u)) * 128u + kb * 16u, c < a.g, a.scale_log2e, qd, qscale);
        __builtin_amdgcn_sched_barrier(0);
        const bool ragged = (n_pages & 15u) != 0u;
#pragma unroll 1
        for (uint32_t tile = t0; tile < t1; ++tile) {
            // the refills are unconditional -- the last iteration re-requests its own tile -- so the requests of the body never sit under a branch
            const uint32_t step = (tile + 1u < t1) ? 1u : 0u;            // scalar
            // ---- scores
            float sc[8];
#pragma unroll
            for (int b = 0; b < 2; ++b) fp8_scores(kx[b][0], kx[b][1], qd, ks4, qscale, b, sc);
            // the lane's candidate for the tile's reference V scale: the largest scale among its four pages
            float vcand = max4(vs4);
            // The edges of the walk, wave-uniform.  `tile` is the absolute tile of the member's walk.  The ragged last tile: pages at or beyond
            // pos_end (even: whole pages), as in the batch kernel.  The window: tiles whose first position lies below rel + 15, the deepest
            // row's bound -- tiles 0 and 1 at most.  Outside the gate every comparison below is false (row_skip <= rel + 15 <= 32 tile).
            if ((ragged && tile + 1u == n_tiles) || (tile < 2u && static_cast<int32_t>(tile * 32u) < rel + static_cast<int32_t>(kSpecWindowMaxDepth))) {
                vcand = 0.0f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const uint32_t pg = tile * 16u + att_slot_page(kb, r), p0 = 2u * pg;
                    const bool beyond = pg >= n_pages;
                    if (beyond || p0 < row_skip) sc[2 * r] = -INFINITY;                 // the ROW's bound
                    if (beyond || p0 + 1u < row_skip) sc[2 * r + 1] = -INFINITY;
                    // the scale goes only where the page is masked for EVERY row: it may be a stale record of any magnitude, and its weights of 0
                    // must meet a finite number; it leaves the election of the reference scale with it
                    if (beyond || p0 + 2u <= cut_pos) vs4[r] = 0.0f;
                    // the page cut by depth 0's bound (its first position in front of every window, its second kept) stands with 2^-10 of its scale:
                    // the masked row may have set it, and as the reference it would push the other weights into the fp16 subnormals
                    vcand = fmaxf(vcand, p0 + 1u == cut_pos ? vs4[r] * 0.0009765625f : vs4[r]);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            kp += step * 32768u; kt += step * 16u;
            issue_k();
            __builtin_amdgcn_sched_barrier(0);
            // ---- online softmax of query row c; the tile's V reference scale and the weights in units of it
            float m_use;
            const float f = att_softmax_step(sc, m_run, m_use);
            f16x8 P;
            const float fa = fp8_v_weights(sc, m_use, f, vs4, vcand, vref, l_run, P);
            // ---- out^T += V^T . P^T, accumulated in place
            fp8_pv8(vx, P, fa, acc);
            __builtin_amdgcn_sched_barrier(0);
            vp += step * 32768u; vt += step * 16u;
            issue_v();
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (split == 0u) {                                                   // workgroup-uniform
        // the held positions enter in true units: leave the reference scale's (a member with nothing walked: vref = 1, acc = 0)
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[t] = acc[t] * vref;
        vref = 1.0f;
        k8v4_fold_held(a, h, seq, head, row, c, kb, m_run, l_run, acc);
    }
    // ---- a single piece (or none): the final rows; otherwise the partial of this piece, back in true units
    att_store_rows8(a, acc, m_run, l_run, vref, sq.n_splits <= 1u, row, part, c, kb);
}

// The draft step of an FP8 pool under a window: a.seqs (device-visible) holds n_seq descriptors that start at the tile of depth 0's bound,
// a.seq_skip the members' signed rel (always: one instance), h.depth the depth table beside the mask words; a.n_splits = the largest
// per-sequence piece count (0: no member walks anything), a.direct_out = d_out.  merge = some member has several pieces:
// launch_attend_combine follows on `s` and passes over the members with one piece or none, whose rows the kernel wrote itself.
hipError_t launch_attend_fp8_spec(const AttendArgs& a, const AttendHeldArgs& h, uint32_t n_seq, bool merge, float* d_out, float* d_lse, hipStream_t s)
{
    if (n_seq == 0) return hipSuccess;
    if (!a.seqs || !a.seq_skip || !a.q16 || a.direct_out != d_out || a.heads % 4u || a.g == 0 || a.g > 16u) return hipErrorInvalidValue;
    if (!h.k_held || !h.v_held || !h.mask || !h.depth || h.rows_per_pos == 0 || a.g % h.rows_per_pos || a.g / h.rows_per_pos > kHeldMax - 1u ||
        h.mask_stride < a.g / h.rows_per_pos || h.seq_stride % 8u || h.pos_stride % 8u)
        return hipErrorInvalidValue;
    AttendArgs ar = a;
    const uint32_t rows = n_seq * (a.heads / 4u), splits = a.n_splits ? a.n_splits : 1u;      // (split 0 of a member that walks nothing folds its held positions)
    ar.rows_real = rows;
    const dim3 gr = a.rows_first ? dim3(rows | 1u, splits) : dim3(splits, rows);
    hipLaunchKernelGGL(k_attend_fp8_spec, gr, dim3(256), 0, s, ar, h);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || !merge) return e;
    ar.direct_per_seq = 3u;                                              // the merge passes over the members without a piece too: their rows are the softmax over the held positions
    return launch_attend_combine(ar, n_seq, d_out, d_lse, s);
}

} // namespace speckv
