// cxl-speckv_amd/csrc/attend_fp8_wide.hip -- the draft step of an FP8_E4M3 pool with up to 32 query rows per kv head in ONE pass over the
// records (speckv_ext_attend_spec_wide): k_attend_fp8_wide<WINDOW>, the WIDE form of k_attend_fp8_spec (attend_fp8_spec.hip), on a global
// layer (plain instance) or under a sliding window (WINDOW instance), the rows held outside the pool folded in inside the same launch.
// A translation unit of its own, built with -packed-fp32-ops off (Makefile) like attend_fp8_spec.hip; that kernel is not touched.
//
// One wave is still one kv head of one sequence over one contiguous piece of its walk (the workgroup shape, the grid with its rows-first
// form, the descriptors, the ONE register-staged tile and the pinned request order of k_attend_fp8_spec: K(t + 1) behind the scores of
// tile t, V(t + 1) behind the accumulation, refills unconditional), but it carries TWO blocks of 16 query rows: block b = rows 16b ..
// 16b + 15 of the group, lane (c, kb) owns row c of both.
//   once per tile    the K loads and K page scales, the V loads and V page scales; the v_perm_b32 pairing of the V bytes and the FP8 ->
//                    f16 operand conversion (fp8_pv8's w[][] and V, built once and issued against both blocks' weights); the election of
//                    the tile's V reference scale
//   once per block   fp8_query_operand (a row scale of its own); the four score MFMAs per K row block (16 per tile instead of 8);
//                    att_softmax_step, the f16 weights with the V page scales riding on them, l_run and m_run; the eight
//                    mfma_f32_16x16x32_f16 into that block's accumulators
// so a step of 17..32 rows reads every stored byte and converts every V value once, where two 16-row calls do both twice.
//
// The reference scale is the TILE's, not a block's: the lane candidates do not depend on the query row and cut_pos is depth 0's, so every
// row of both blocks elects the same vref_t.  fp8_v_weights (attend_fp8_device.hpp) elects it AND overwrites vref; called once per block
// it would hand the second block an accumulator factor of f x 1.  Here: fp8_vref_elect once per tile, fp8_block_weights per block with
// fa[b] = f[b] x (vref_old x rinv), vref assigned once behind both.  Operation for operation a block's arithmetic is fp8_v_weights' and
// fp8_pv8's, so a row's bits are those of k_attend_fp8_spec over the same pieces.
//
// WINDOW: the mask is the row's, so it is per block (row_skip[b] = k8v4_row_skip of row 16b + c); the gate (wave-uniform, tiles 0 and 1
// only) and the V-scale rule are k_attend_fp8_spec's: a scale goes to 0 only where 2 page + 2 <= cut_pos, the page cut by depth 0's bound
// stands with 2^-10 of its scale, pages beyond pos_end are cleared in the ragged last tile.  The plain instance (a.seq_skip == nullptr)
// carries the ragged-tile rule alone, reads no depth table and pays no gate.
//
// Held rows and stores: every split first leaves the reference scale's units (acc x vref, 64 multiplies per wave at the end: the product
// att_store_rows8 forms with unit = vref, so partials and final rows keep the 16-row kernel's bits); split 0 then folds the held rows into
// both blocks (k8v4_fold_held_wide) and both blocks leave through k8v4_store_block, block 1's partials `block_parts` behind block 0's
// (attend_wide_device.hpp, shared with attend_kv_wide.hip).  A member with nothing walked runs that epilogue alone.  The second block may
// be partly empty (g < 32): those lanes carry the zero query, m_run = -inf, l_run = 0, and write nothing.
//
// Resources (gfx950, -O3, as the compiler reports them): plain instance 162 VGPRs, 0 AGPRs, 63 SGPRs; WINDOW instance 168 VGPRs, 0 AGPRs,
// 69 SGPRs; no LDS, no scratch, no spill in either -- at the 168 registers of THREE waves per SIMD, so waves_per_eu(3, 3), the occupancy of
// k_attend_k8v4_wide (k_attend_fp8_spec runs four at 115).  The V operand is paired and converted per channel pair (fp8_pv8_wide holds four
// paired words, not fp8_pv8's sixteen); the WINDOW instance sits exactly on the limit, so anything added to it has to be paid for or it
// drops to two waves.  The build fails on scratch (Makefile).  DESIGN section 4.
#include "attend_wide_device.hpp"    // k8v4_fold_held_wide, k8v4_store_block; with it attend_kv_device.hpp, attend_fp8_device.hpp, spec_window.hpp

namespace speckv {

// The tile's V reference scale: fp8_v_weights' election (the largest lane candidate of the row's four lanes; vref stays when that is 0),
// once for every query block of the wave.
__device__ __forceinline__ float fp8_vref_elect(float vcand, float vref)
{
    const float vmx = max_over_kb(vcand);
    return vmx > 0.0f ? vmx : vref;
}
// fp8_v_weights for ONE block of a wave against a reference scale already elected (rinv = 1 / vref_t): the block's weights and running
// sum; returns its accumulator factor f x vref_old / vref_t.  vref_old is not touched -- the caller assigns vref behind its last block.
__device__ __forceinline__ float fp8_block_weights(const float (&sc)[8], float m_use, float f, const f32x4& vs4, float vref_old, float rinv, float& l_run, f16x8& P)
{
    float psum = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float p = __builtin_amdgcn_exp2f(sc[j] - m_use);
        psum += p;
        P[j] = static_cast<_Float16>(p * (vs4[j >> 1] * rinv));
    }
    l_run = l_run * f + psum;
    return f * (vref_old * rinv);
}
// fp8_pv8 for two blocks: the byte pairing and each channel's f16 operand are built once and meet both blocks' weights and accumulators.
__device__ __forceinline__ void fp8_pv8_wide(const uint2 (&vx)[8], const f16x8 (&P)[2], const float (&fa)[2], f32x4 (&acc)[2][8])
{
    constexpr uint32_t kEven = 0x05010400u, kOdd = 0x07030602u;          // fp8_pv8's selectors
#pragma unroll
    for (int tp = 0; tp < 4; ++tp) {                                      // channels 8c + 2tp, 8c + 2tp + 1: one paired word per row pair
        uint32_t w[4];
#pragma unroll
        for (int jp = 0; jp < 4; ++jp) {
            const uint32_t hi = (tp & 2) ? vx[2 * jp + 1].y : vx[2 * jp + 1].x, lo = (tp & 2) ? vx[2 * jp].y : vx[2 * jp].x;
            w[jp] = __builtin_amdgcn_perm(hi, lo, (tp & 1) ? kOdd : kEven);
        }
#pragma unroll
        for (int o = 0; o < 2; ++o) {
            const int t = 2 * tp + o;
            f16x8 V;
#pragma unroll
            for (int jp = 0; jp < 4; ++jp) {
                const f16x2 h = o ? __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w[jp], 1.0f, true) : __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w[jp], 1.0f, false);
                V[2 * jp] = h.x;
                V[2 * jp + 1] = h.y;
            }
            acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(V, P[0], acc[0][t] * fa[0], 0, 0, 0);
            acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(V, P[1], acc[1][t] * fa[1], 0, 0, 0);
        }
    }
}

// The arguments, the descriptors and the walk are k_attend_fp8_spec's; 17 <= a.g <= 32.  WINDOW: a.seq_skip carries the members' signed rel
// and h.depth the depth table; the plain instance reads neither.  block_parts: the partials of ONE block of the launch (what assign_pieces
// counted); block 1's lie that many further on.
template <bool WINDOW>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_attend_fp8_wide(AttendArgs a, AttendHeldArgs h, uint32_t block_parts)
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
    const uint64_t row = static_cast<uint64_t>(seq) * a.heads + head;    // query / output row block (32 rows at most)
    const AttendSeq sq = a.seqs[seq];
    if (split >= sq.n_splits && (sq.n_splits != 0u || split != 0u)) return;      // (nothing walked: split 0 goes on to the held positions alone)
    const uint64_t part = sq.part_base + static_cast<uint64_t>(head) * sq.n_splits + split;
    const uint32_t n_pages = sq.n_pages;
    // WINDOW: the member's signed rel; row_skip[b] = the lane's own row of block b, cut_pos = depth 0's = the least of any row (wave-uniform)
    uint32_t row_skip[2] = {0u, 0u}, cut_pos = 0u;
    int32_t rel = 0;
    if constexpr (WINDOW) {
        rel = static_cast<int32_t>(*SPECKV_GP(uint32_t, a.seq_skip + seq));
#pragma unroll
        for (uint32_t b = 0; b < 2u; ++b) row_skip[b] = k8v4_row_skip(h, a.g, seq, 16u * b + c, rel);
        cut_pos = spec_window_skip(rel, 0u);
    }

    uint32_t qd[2][8];
    float qscale[2] = {1.0f, 1.0f};
    const uint32_t n_tiles = (n_pages + 15u) / 16u;
    const uint32_t t0 = split * sq.tiles_per_split;
    const uint32_t t1 = min(t0 + sq.tiles_per_split, n_tiles);
    float m_run[2] = {-INFINITY, -INFINITY}, l_run[2] = {0.0f, 0.0f}, vref = 1.0f;
    f32x4 acc[2][8];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[b][t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    if (t0 < t1) {                                                       // wave-uniform
        // the running pointers, the register set and the request order of k_attend_fp8_spec: the load schedule is not touched
        const uint8_t* kp = sq.lin_base + sq.k_first * 2048ull + head * 128u + kb * 16u + (static_cast<uint64_t>(t0) * 32u + c) * 1024u;
        const uint8_t* vp = sq.lin_base + sq.v_first * 2048ull + head * 128u + 8u * c + (static_cast<uint64_t>(t0) * 32u + 4u * kb) * 1024u;
        const float* kt = sq.scale_tab + (sq.k_first + static_cast<uint64_t>(t0) * 16u) + 4u * kb;
        const float* vt = sq.scale_tab + (sq.v_first + static_cast<uint64_t>(t0) * 16u) + 4u * kb;
        uint4 kx[2][2];
        uint2 vx[8];
        f32x4 ks4, vs4;
        auto issue_k = [&]() {
#pragma unroll
            for (int kr = 0; kr < 2; ++kr) { kx[kr][0] = ldg16(kp + 16384 * kr); kx[kr][1] = ldg16(kp + 16384 * kr + 64); }
            ks4 = ldg_f4(kt);
        };
        auto issue_v = [&]() {
#pragma unroll
            for (int j = 0; j < 8; ++j) vx[j] = ldg8(vp + 1024 * (j & 3) + 16384 * (j >> 2));
            vs4 = ldg_f4(vt);
        };
        __builtin_amdgcn_sched_barrier(0);
        issue_k();
        __builtin_amdgcn_sched_barrier(0);
        issue_v();
        __builtin_amdgcn_sched_barrier(0);
        // (the queries' loads are the youngest: they and the tile arrive together); rows >= g are zero
#pragma unroll
        for (uint32_t b = 0; b < 2u; ++b)
            fp8_query_operand(a.q16 + (row * a.g + min(16u * b + c, a.g - 1u)) * 128u + kb * 16u, 16u * b + c < a.g, a.scale_log2e, qd[b], qscale[b]);
        __builtin_amdgcn_sched_barrier(0);
        const bool ragged = (n_pages & 15u) != 0u;
#pragma unroll 1
        for (uint32_t tile = t0; tile < t1; ++tile) {
            const uint32_t step = (tile + 1u < t1) ? 1u : 0u;            // scalar: the last iteration re-requests its own tile
            // ---- scores: the K bytes of the tile against both blocks' query operands
            float sc[2][8];
#pragma unroll
            for (int b = 0; b < 2; ++b)
#pragma unroll
                for (int kr = 0; kr < 2; ++kr) fp8_scores(kx[kr][0], kx[kr][1], qd[b], ks4, qscale[b], kr, sc[b]);
            // the lane's candidate for the tile's reference V scale: the largest scale among its four pages
            float vcand = max4(vs4);
            // The edges of the walk, wave-uniform, k_attend_fp8_spec's rules: the ragged last tile (pages at or beyond pos_end) and, WINDOW, the
            // tiles whose first position lies below rel + 15 -- tiles 0 and 1 at most.  The score mask is the ROW's, so per block; what becomes
            // of a V scale depends on cut_pos alone, so it is the tile's.
            bool edge = ragged && tile + 1u == n_tiles;
            if constexpr (WINDOW) edge = edge || (tile < 2u && static_cast<int32_t>(tile * 32u) < rel + static_cast<int32_t>(kSpecWindowMaxDepth));
            if (edge) {
                vcand = 0.0f;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const uint32_t pg = tile * 16u + att_slot_page(kb, r), p0 = 2u * pg;
                    const bool beyond = pg >= n_pages;
#pragma unroll
                    for (int b = 0; b < 2; ++b) {
                        if (beyond || p0 < row_skip[b]) sc[b][2 * r] = -INFINITY;
                        if (beyond || p0 + 1u < row_skip[b]) sc[b][2 * r + 1] = -INFINITY;
                    }
                    // masked for EVERY row of both blocks: the scale goes, and leaves the election with it
                    if (beyond || p0 + 2u <= cut_pos) vs4[r] = 0.0f;
                    // the page cut by depth 0's bound stands with 2^-10 of its scale
                    vcand = fmaxf(vcand, p0 + 1u == cut_pos ? vs4[r] * 0.0009765625f : vs4[r]);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            kp += step * 32768u; kt += step * 16u;
            issue_k();
            __builtin_amdgcn_sched_barrier(0);
            // ---- the tile's V reference scale, once; then the online softmax and the weights of rows c and 16 + c in units of it
            const float vref_t = fp8_vref_elect(vcand, vref);
            const float rinv = __builtin_amdgcn_rcpf(vref_t);
            float fa[2];
            f16x8 P[2];
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                float m_use;
                const float f = att_softmax_step(sc[b], m_run[b], m_use);
                fa[b] = fp8_block_weights(sc[b], m_use, f, vs4, vref, rinv, l_run[b], P[b]);
            }
            vref = vref_t;
            // ---- out^T += V^T . P^T: the operand of channel 8c + t is built once and meets both blocks' weights
            fp8_pv8_wide(vx, P, fa, acc);
            __builtin_amdgcn_sched_barrier(0);
            vp += step * 32768u; vt += step * 16u;
            issue_v();
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    // every split leaves the reference scale's units (a member with nothing walked: vref = 1, acc = 0): the held positions and the stores
    // of attend_wide_device.hpp work in true units
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[b][t] = acc[b][t] * vref;
    if (split == 0u) k8v4_fold_held_wide(a, h, seq, head, row, c, kb, m_run, l_run, acc);       // workgroup-uniform
    // ---- a single piece (or none): the final rows; otherwise the two partials of this piece
    const bool final_rows = sq.n_splits <= 1u;
    k8v4_store_block(a, acc[0], m_run[0], l_run[0], final_rows, row, part, 0u, c, kb);
    k8v4_store_block(a, acc[1], m_run[1], l_run[1], final_rows, row, part + block_parts, 1u, c, kb);
}

// launch_attend_fp8_spec for 17 <= a.g <= 32 query rows: the same grid (a wave per kv head, sequence and piece), the wide kernel -- the
// WINDOW instance exactly when a.seq_skip is set, which then needs the depth table -- and where some member has several pieces the merge
// over both blocks' partials (a.part_acc / part_ml hold 2 x block_parts of them).
hipError_t launch_attend_fp8_wide(const AttendArgs& a, const AttendHeldArgs& h, uint32_t n_seq, uint32_t block_parts, bool merge, float* d_out, float* d_lse, hipStream_t s)
{
    if (n_seq == 0) return hipSuccess;
    if (!a.seqs || !a.q16 || a.direct_out != d_out || a.heads % 4u || a.g <= 16u || a.g > 32u || (a.seq_skip != nullptr) != (h.depth != nullptr)) return hipErrorInvalidValue;
    if (!h.k_held || !h.v_held || !h.mask || h.rows_per_pos < 2u || a.g % h.rows_per_pos || a.g / h.rows_per_pos > kHeldMax - 1u ||
        h.mask_stride < a.g / h.rows_per_pos || h.seq_stride % 8u || h.pos_stride % 8u)
        return hipErrorInvalidValue;
    AttendArgs ar = a;
    const uint32_t rows = n_seq * (a.heads / 4u), splits = a.n_splits ? a.n_splits : 1u;      // (split 0 of a member that walks nothing folds its held positions)
    ar.rows_real = rows;
    const dim3 gr = a.rows_first ? dim3(rows | 1u, splits) : dim3(splits, rows);
    if (a.seq_skip) hipLaunchKernelGGL((k_attend_fp8_wide<true>), gr, dim3(256), 0, s, ar, h, block_parts);
    else hipLaunchKernelGGL((k_attend_fp8_wide<false>), gr, dim3(256), 0, s, ar, h, block_parts);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || !merge) return e;
    ar.direct_per_seq = 3u;                                              // the merge passes over the members without a piece too: their rows are the softmax over the held positions
    return launch_attend_combine(ar, n_seq, d_out, d_lse, s, 0u, 0u, block_parts);
}

} // namespace speckv
