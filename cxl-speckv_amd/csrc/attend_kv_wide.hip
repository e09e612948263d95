// cxl-speckv_amd/csrc/attend_kv_wide.hip -- the split pool's multi-position step with up to 32 query rows per kv head in ONE pass over the
// records (speckv_ext_attend_kv_spec_wide): k_attend_k8v4_wide, the WIDE form of k_attend_k8v4's held step (attend_kv_device.hpp), and its
// launcher.  A translation unit of its own, built with -packed-fp32-ops off (Makefile): the five instances of attend_kv.hip and
// attend_kv_layers.hip keep their units, their flags and their code -- the header they share is not touched.
//
// One wave is still one kv head of one sequence over one piece of its tiles (the workgroup shape, the grid, the descriptors and the
// request order of k_attend_k8v4), but it carries TWO blocks of 16 query rows: block b = rows 16b .. 16b + 15 of the group, lane (c, kb)
// owns row c of both.  Per tile the K loads, the page scales, the V loads, the code bytes and the eight v_cvt_scalef32_pk_f16_fp4 operand
// builds happen once; what is per block is arithmetic on operands already in registers:
//   scores   the four FP8 MFMAs of each K row block run once per query block, against that block's E4M3 query operand (a row scale of
//            its own: fp8_query_operand twice), 16 score MFMAs per tile instead of 8
//   softmax  att_softmax_step once per block: m_run, l_run, f and the f16 weights P of its own
//   output   each mfma_f32_16x16x32_f16 is issued twice with the SAME widened V operand, once per block's P and accumulators: 16 instead of 8
// so a step of 17..32 rows reads every stored byte and widens every MXFP4 value once, where two 16-row calls do both twice.
// Registers: 64 accumulator registers, two query operands, two score sets and two sets of weights beside the one tile in flight: the
// compiler reports 160 (plain) and 161 (WINDOW) VGPRs, no AGPRs, no LDS and no scratch -- under the 168 of THREE waves per SIMD, so
// waves_per_eu(3, 3) (k_attend_k8v4 runs four at 128; two would leave the third wave's registers unused).  DESIGN section 4.
// The second block may be partly empty (g < 32): those lanes carry the zero query, m_run = -inf, l_run = 0, and write nothing.
#include "attend_wide_device.hpp"    // k8v4_fold_held_wide, k8v4_store_block (shared with attend_fp8_wide.hip); with it attend_kv_device.hpp

namespace speckv {

// The arguments, the descriptors, the walk and the window rule are k_attend_k8v4<WINDOW, true>'s (attend_kv_device.hpp); 17 <= a.g <= 32.
// block_parts: the partials of ONE block of the launch (what assign_pieces counted); block 1's lie that many further on.
template <bool WINDOW>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_attend_k8v4_wide(AttendArgs a, const AttendKvSide* __restrict__ vside, AttendHeldArgs h,
                                                                                                     uint32_t block_parts)
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
    if (split >= sq.n_splits && (sq.n_splits != 0u || split != 0u)) return;      // (nothing stored: split 0 goes on to the held positions alone)
    const AttendKvSide vsd = vside[seq];
    const uint64_t part = sq.part_base + static_cast<uint64_t>(head) * sq.n_splits + split;
    const uint32_t n_pages = sq.n_pages;
    // WINDOW: the sequence's signed rel; row_skip[b] = the lane's own row of block b, cut_pos = depth 0's = the least of any row (uniform)
    uint32_t row_skip[2] = {0u, 0u}, cut_pos = 0u;
    int32_t rel = 0;
    if constexpr (WINDOW) {
        rel = static_cast<int32_t>(*SPECKV_GP(uint32_t, a.seq_skip + seq));
#pragma unroll
        for (uint32_t b = 0; b < 2u; ++b) row_skip[b] = k8v4_row_skip(h, a.g, seq, 16u * b + c, rel);
        cut_pos = spec_window_skip(rel, 0u);
    }

    // query operands (fp8_query_operand): row 16b + c of this head per block, each with its own row scale; rows >= g are zero
    uint32_t qd[2][8];
    float qscale[2] = {1.0f, 1.0f};
    auto quantise_queries = [&]() {
#pragma unroll
        for (uint32_t b = 0; b < 2u; ++b)
            fp8_query_operand(a.q16 + (row * a.g + min(16u * b + c, a.g - 1u)) * 128u + kb * 16u, 16u * b + c < a.g, a.scale_log2e, qd[b], qscale[b]);
    };

    const uint32_t n_tiles = (n_pages + 15u) / 16u;
    const uint32_t t0 = split * sq.tiles_per_split;
    const uint32_t t1 = min(t0 + sq.tiles_per_split, n_tiles);
    float m_run[2] = {-INFINITY, -INFINITY}, l_run[2] = {0.0f, 0.0f};
    f32x4 acc[2][8];
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int t = 0; t < 8; ++t) acc[b][t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    if (t0 < t1) {                                                       // wave-uniform
        // the running pointers, the register set and the request order of k_attend_k8v4: the load schedule is not touched
        const uint8_t* kp = sq.lin_base + sq.k_first * 2048ull + head * 128u + kb * 16u + (static_cast<uint64_t>(t0) * 32u + c) * 1024u;
        const float* kt = sq.scale_tab + (sq.k_first + static_cast<uint64_t>(t0) * 16u) + 4u * kb;
        const uint8_t* vtile = vsd.v_base + ((vsd.v_first >> 4) + t0) * static_cast<uint64_t>(kMx4TileBytes);
        const uint8_t* vp = vtile + 2u * kb * 1024u + head * 128u + 8u * c;
        const uint8_t* vc = vtile + kMx4CodePlane + 2u * kb * 64u + head * 8u + (c >> 1);

        uint4 kx[2][2];
        uint2 vx[4];
        uint32_t vcode[4];
        f32x4 ks4;
        auto issue_k = [&]() {
#pragma unroll
            for (int kr = 0; kr < 2; ++kr) { kx[kr][0] = ldg16(kp + 16384 * kr); kx[kr][1] = ldg16(kp + 16384 * kr + 64); }
            ks4 = ldg_f4(kt);
        };
        auto issue_v = [&]() {
#pragma unroll
            for (int r = 0; r < 4; ++r) vx[r] = ldg8(vp + 1024 * (r & 1) + 8192 * (r >> 1));
#pragma unroll
            for (int r = 0; r < 4; ++r) vcode[r] = ldg1(vc + 64 * (r & 1) + 512 * (r >> 1));
        };
        __builtin_amdgcn_sched_barrier(0);
        issue_k();
        __builtin_amdgcn_sched_barrier(0);
        issue_v();
        __builtin_amdgcn_sched_barrier(0);
        quantise_queries();                                              // (their loads are the youngest: they and the tile arrive together)
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
            if (ragged && tile + 1u == n_tiles) {                         // wave-uniform: pages at or beyond pos_end; per tile, as in k_attend_k8v4
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const uint32_t pg = tile * 16u + att_slot_page(kb, r);
                    if (pg >= n_pages) {
#pragma unroll
                        for (int b = 0; b < 2; ++b) { sc[b][2 * r] = -INFINITY; sc[b][2 * r + 1] = -INFINITY; }
                        vcode[r] = 0u;
                    }
                }
            }
            // WINDOW: the mask is the row's, so it is per block; the gate and the code-clearing rule (pages in front of depth 0's bound) are
            // k_attend_k8v4<true, true>'s -- a step has at most 16 positions, kSpecWindowMaxDepth holds
            if constexpr (WINDOW) {
                if (tile < 2u && static_cast<int32_t>(tile * 32u) < rel + static_cast<int32_t>(kSpecWindowMaxDepth)) {      // wave-uniform
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const uint32_t p0 = 2u * (tile * 16u + att_slot_page(kb, r));
#pragma unroll
                        for (int b = 0; b < 2; ++b) {
                            if (p0 < row_skip[b]) sc[b][2 * r] = -INFINITY;
                            if (p0 + 1u < row_skip[b]) sc[b][2 * r + 1] = -INFINITY;
                        }
                        if (p0 + 2u <= cut_pos) vcode[r] = 0u;
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            kp += step * 32768u; kt += step * 16u;
            issue_k();
            __builtin_amdgcn_sched_barrier(0);
            // ---- online softmax of rows c and 16 + c
            float f[2];
            f16x8 P[2];
#pragma unroll
            for (int b = 0; b < 2; ++b) {
                float m_use;
                f[b] = att_softmax_step(sc[b], m_run[b], m_use);
                float psum = 0.0f;
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float p = __builtin_amdgcn_exp2f(sc[b][j] - m_use);
                    psum += p;
                    P[b][j] = static_cast<_Float16>(p);
                }
                l_run[b] = l_run[b] * f[b] + psum;
            }
            // ---- out^T += V^T . P^T: the operand of channel 8c + T is built once and meets both blocks' weights
            float vsc[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) vsc[r] = __uint_as_float(vcode[r] << 23);        // the block's E8M0 code as a float's exponent field
#define KV_PV2(T, WORD, SEL)                                                                                                      \
    {                                                                                                                              \
        const u32x4 vw = {__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(vx[0].WORD, vsc[0], SEL)),          \
                          __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(vx[1].WORD, vsc[1], SEL)),          \
                          __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(vx[2].WORD, vsc[2], SEL)),          \
                          __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(vx[3].WORD, vsc[3], SEL))};         \
        acc[0][T] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, vw), P[0], acc[0][T] * f[0], 0, 0, 0);         \
        acc[1][T] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, vw), P[1], acc[1][T] * f[1], 0, 0, 0);         \
    }
            KV_PV2(0, x, 0) KV_PV2(1, x, 1) KV_PV2(2, x, 2) KV_PV2(3, x, 3) KV_PV2(4, y, 0) KV_PV2(5, y, 1) KV_PV2(6, y, 2) KV_PV2(7, y, 3)
#undef KV_PV2
            __builtin_amdgcn_sched_barrier(0);
            vp += step * kMx4TileBytes; vc += step * kMx4TileBytes;
            issue_v();
            __builtin_amdgcn_sched_barrier(0);
        }
    }
    if (split == 0u) k8v4_fold_held_wide(a, h, seq, head, row, c, kb, m_run, l_run, acc);       // workgroup-uniform
    // ---- a single split: the final rows; otherwise the two partials of this split
    const bool final_rows = sq.n_splits <= 1u;
    k8v4_store_block(a, acc[0], m_run[0], l_run[0], final_rows, row, part, 0u, c, kb);
    k8v4_store_block(a, acc[1], m_run[1], l_run[1], final_rows, row, part + block_parts, 1u, c, kb);
}

// launch_attend_k8v4_held for 17 <= a.g <= 32 query rows: the same grid (a wave per kv head, sequence and piece), the wide kernel, and
// where some sequence has several pieces the merge over both blocks' partials (a.part_acc / part_ml hold 2 x block_parts of them).
hipError_t launch_attend_k8v4_wide(const AttendArgs& a, const AttendKvSide* d_vside, const AttendHeldArgs& h, uint32_t n_seq, uint32_t block_parts, bool merge,
                                   float* d_out, float* d_lse, hipStream_t s)
{
    if (n_seq == 0) return hipSuccess;
    if (!a.seqs || !d_vside || !a.q16 || a.direct_out != d_out || a.heads % 4u || a.g <= 16u || a.g > 32u || (a.seq_skip && !h.depth)) return hipErrorInvalidValue;
    if (!h.k_held || !h.v_held || !h.mask || h.rows_per_pos < 2u || a.g % h.rows_per_pos || a.g / h.rows_per_pos > kHeldMax - 1u ||
        h.mask_stride < a.g / h.rows_per_pos || h.seq_stride % 8u || h.pos_stride % 8u)
        return hipErrorInvalidValue;
    AttendArgs ar = a;
    const uint32_t rows = n_seq * (a.heads / 4u), splits = a.n_splits ? a.n_splits : 1u;      // (split 0 of a sequence without positions folds its held ones)
    ar.rows_real = rows;
    const dim3 gr = a.rows_first ? dim3(rows | 1u, splits) : dim3(splits, rows);
    if (a.seq_skip) hipLaunchKernelGGL((k_attend_k8v4_wide<true>), gr, dim3(256), 0, s, ar, d_vside, h, block_parts);
    else hipLaunchKernelGGL((k_attend_k8v4_wide<false>), gr, dim3(256), 0, s, ar, d_vside, h, block_parts);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || !merge) return e;
    ar.direct_per_seq = 3u;                                              // (launch_attend_k8v4_held: the merge passes over the sequences without a split too)
    return launch_attend_combine(ar, n_seq, d_out, d_lse, s, 0u, 0u, block_parts);
}

} // namespace speckv
