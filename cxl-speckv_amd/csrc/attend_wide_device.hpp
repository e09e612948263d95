// cxl-speckv_amd/csrc/attend_wide_device.hpp -- what the WIDE draft-step kernels share (two blocks of 16 query rows per wave:
// k_attend_k8v4_wide, attend_kv_wide.hip, and k_attend_fp8_wide, attend_fp8_wide.hip): the fold of the held positions into both blocks and
// the store of one block.  Both depend on the accumulator map acc[b][t][i] = channel 32kb + 8i + t of row 16b + c alone, and on accumulators
// in TRUE units.  Device code only; the functions moved here from attend_kv_wide.hip, text unchanged.
#pragma once
#include "attend_kv_device.hpp"

namespace speckv {

// The held positions of the step folded into BOTH blocks by the wave of split 0: k8v4_fold_held's loop with each held K and V row loaded
// once per position and used twice.  word[b] = the mask word of the query position of row 16b + c, (16b + c) / rows_per_pos; the loop ends
// at the highest bit set in any word of either block.  The arithmetic per (block, position) is k8v4_fold_held's.
__device__ __forceinline__ void k8v4_fold_held_wide(const AttendArgs& a, const AttendHeldArgs& h, uint32_t seq, uint32_t head, uint64_t row, uint32_t c, uint32_t kb,
                                                    float (&m_run)[2], float (&l_run)[2], f32x4 (&acc)[2][8])
{
    uint32_t word[2] = {0u, 0u};
#pragma unroll
    for (uint32_t b = 0; b < 2u; ++b)
        if (16u * b + c < a.g) word[b] = *SPECKV_GP(uint32_t, h.mask + static_cast<uint64_t>(seq) * h.mask_stride + (16u * b + c) / h.rows_per_pos) & ((1u << kHeldMax) - 1u);
    uint32_t n_held = 0u;                                                // 1 + the highest bit set in any word of the sequence (wave-uniform)
#pragma unroll
    for (uint32_t t = 0; t < kHeldMax; ++t)
        if (__builtin_amdgcn_ballot_w64(((word[0] | word[1]) >> t) & 1u) != 0ull) n_held = t + 1u;
    if (n_held == 0u) return;
    const uint64_t at0 = static_cast<uint64_t>(seq) * h.seq_stride + head * 128u + 32u * kb;
    HeldPiece kn = held_piece(h.k_held, at0), vx = held_piece(h.v_held, at0);
    const HeldPiece q[2] = {held_piece(a.q16, (row * a.g + min(c, a.g - 1u)) * 128u + 32u * kb),
                            held_piece(a.q16, (row * a.g + min(16u + c, a.g - 1u)) * 128u + 32u * kb)};
#pragma unroll 1
    for (uint32_t t = 0; t < n_held; ++t) {
        const HeldPiece kx = kn;
        const bool more = t + 1u < n_held;                                // scalar: nothing above the highest visible position is read
        const uint64_t at = at0 + static_cast<uint64_t>(t + 1u) * h.pos_stride;
        if (more) kn = held_piece(h.k_held, at);
        float f[2], p[2];
        bool sees[2];
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            sees[b] = (word[b] >> t) & 1u;
            float dot = 0.0f;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t qw[4] = {q[b].w[i].x, q[b].w[i].y, q[b].w[i].z, q[b].w[i].w}, kw[4] = {kx.w[i].x, kx.w[i].y, kx.w[i].z, kx.w[i].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) dot = __builtin_amdgcn_fdot2(__builtin_bit_cast(f16x2, qw[e]), __builtin_bit_cast(f16x2, kw[e]), dot, false);
            }
            const float s = sees[b] ? sum_over_kb(dot) * a.scale_log2e : -INFINITY;
            const float m_new = fmaxf(m_run[b], s);
            const float m_use = (m_new == -INFINITY) ? 0.0f : m_new;
            f[b] = __builtin_amdgcn_exp2f(m_run[b] - m_use);
            p[b] = __builtin_amdgcn_exp2f(s - m_use);
            m_run[b] = m_new;
            l_run[b] = l_run[b] * f[b] + (kb == 0u ? p[b] : 0.0f);       // (the store sums l_run over kb: the weight enters one lane)
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t vw[4] = {vx.w[i].x, vx.w[i].y, vx.w[i].z, vx.w[i].w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float v = held_f16(vw[e >> 1], e & 1);             // widened once, weighted per block
#pragma unroll
                for (int b = 0; b < 2; ++b) acc[b][e][i] = acc[b][e][i] * f[b] + (sees[b] ? p[b] * v : 0.0f);
            }
        }
        if (more) vx = held_piece(h.v_held, at);
    }
}

// att_store_rows8 for block b of the wave: the merge and the output are laid out for 16 rows per (head, piece), so the two blocks leave as
// two 16-row row blocks -- final rows row * g + 16b + c, partials as two parts, block b's `block_parts` partials behind block 0's.  Rows at
// or beyond g are not written (their m / l slots of the partial are: -inf and 0, which the merge turns into weight 0).
__device__ __forceinline__ void k8v4_store_block(const AttendArgs& a, const f32x4 (&acc)[8], float m_run, float l_run, bool final_rows, uint64_t row, uint64_t part,
                                                 uint32_t b, uint32_t c, uint32_t kb)
{
    const float l_tot = sum_over_kb(l_run);
    const uint32_t rc = 16u * b + c;
    if (final_rows) {
        if (rc < a.g) {
            const float w = l_tot > 0.0f ? 1.0f / l_tot : 0.0f;
            float* dst = a.direct_out + (row * a.g + rc) * 128u + 32u * kb;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                *reinterpret_cast<f32x4*>(dst + 8 * i) = f32x4{acc[0][i], acc[1][i], acc[2][i], acc[3][i]} * w;
                *reinterpret_cast<f32x4*>(dst + 8 * i + 4) = f32x4{acc[4][i], acc[5][i], acc[6][i], acc[7][i]} * w;
            }
            if (a.direct_lse && kb == 0) a.direct_lse[row * a.g + rc] = l_tot > 0.0f ? (m_run + log2f(l_tot)) * 0.6931471805599453f : -INFINITY;
        }
        return;
    }
    if (kb == 0) {
        a.part_ml[part * 32u + c] = m_run;
        a.part_ml[part * 32u + 16u + c] = l_tot;
    }
    if (rc < a.g) {
        float* dst = a.part_acc + (part * 16u + c) * 128u + 32u * kb;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<f32x4*>(dst + 8 * i) = f32x4{acc[0][i], acc[1][i], acc[2][i], acc[3][i]};
            *reinterpret_cast<f32x4*>(dst + 8 * i + 4) = f32x4{acc[4][i], acc[5][i], acc[6][i], acc[7][i]};
        }
    }
}

} // namespace speckv
