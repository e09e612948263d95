// cxl-speckv_amd/csrc/attend_fp8_device.hpp -- the tile arithmetic of the decode attention kernels that read FP8_E4M3 keys
// (attend.hip: k_attend_fp8, k_attend_fp8_linear, k_attend_fp8_dma, k_qk_scores_fp8_linear; attend_kv.hip: k_attend_k8v4), each block
// once: query operand, score MFMAs, slot pages, online-softmax step, FP8 V weights and p.V, epilogue.  The kernels keep what differs
// between them: descriptors, requests, waits, mask rules.  Operand maps: attend.hip.  The translation units build with
// -ffp-contract=off: the same operations in the same order give the same bits in every kernel, whatever the schedule.  Device code only.
#pragma once
#include "attend_device.hpp"
#include "codec_device.hpp"          // the exact reciprocal divide of the codecs (div_by_scale and friends)

namespace speckv {
namespace {

// ---- query operand
// The score MFMAs' B operand of lane (c, kb) from the four 16-byte pieces of fp16 row c that the lane feeds (d = 16kb .. 16kb + 15 of
// both 64-element halves), quantised exactly as k_quantize_q_e4m3 does (row scale = max|q| / 448, 1 if zero; e4m3 of clamp(q / scale));
// a dead row (c >= g) is zero.  The 32 quotients go through the row's reciprocal: div_by_scale is bit-identical to the IEEE divide
// for an fp16 dividend and a scale m / 448 (exhaustive device check: test_fast_division_is_exact); rows with inf / NaN keep the divide.
__device__ __forceinline__ void fp8_quantize_query(const u32x4 (&w4)[4], bool live, uint32_t (&qd)[8], float& row_scale)
{
    float xq[32];
    float mx = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t ws[4] = {w4[i].x, w4[i].y, w4[i].z, w4[i].w};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            xq[8 * i + k] = static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(ws[k >> 1] >> (16 * (k & 1)))));
            mx = fmaxf(mx, fabsf(xq[8 * i + k]));
        }
    }
    mx = max_over_kb(mx);
    const bool finite = mx < INFINITY;
    const float sc = (mx > 0.0f) ? (finite ? div448_of_f16_value(mx) : mx / 448.0f) : 1.0f;
    const float rcp = finite ? rcp_of_scale(sc) : 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float x = xq[4 * i + k];
            const float qt = finite ? __builtin_copysignf(div_by_scale(x, sc, rcp), x) : x / sc;
            v[k] = live ? fminf(fmaxf(qt, -448.0f), 448.0f) : 0.0f;
        }
        int pk = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], 0, false);
        pk = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], pk, true);
        qd[i] = static_cast<uint32_t>(pk);
    }
    row_scale = live ? sc : 1.0f;
}
// The same with the row's four loads (qsrc = row + 16 kb); qscale = row scale x sm_scale x log2(e).  The register-staged kernels call
// it BEHIND their first tile's requests: descriptor -> {tile, query} -> scores instead of descriptor -> query -> tile -> scores -- a
// launch of 256 x 1k lasts 100 us, and 32 IEEE divides behind a load of their own stood in front of every workgroup's first request.
__device__ __forceinline__ void fp8_query_operand(const uint16_t* qsrc, bool live, float scale_log2e, uint32_t (&qd)[8], float& qscale)
{
    u32x4 w4[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint4 w = *reinterpret_cast<const uint4*>(qsrc + 8 * (i & 1) + 64 * (i >> 1));
        w4[i] = u32x4{w.x, w.y, w.z, w.w};
    }
    float row_scale;
    fp8_quantize_query(w4, live, qd, row_scale);
    qscale = row_scale * scale_log2e;
}

// ---- scores
// The four score MFMAs of block b of a tile (K row 16b + c) from the lane's two 16-byte pieces of that row: the raw sums of query row
// c over the positions 16b + 4kb + i.  Piece: uint4 (loaded) or u32x4 (read from LDS).
template <typename Piece>
__device__ __forceinline__ f32x4 fp8_scores_raw(const Piece& k0, const Piece& k1, const uint32_t (&qd)[8])
{
    const uint32_t kd[8] = {k0.x, k0.y, k0.z, k0.w, k1.x, k1.y, k1.z, k1.w};
    f32x4 s = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
    for (int st = 0; st < 4; ++st)
        s = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(pack64(kd[2 * st], kd[2 * st + 1]), pack64(qd[2 * st], qd[2 * st + 1]), s, 0, 0, 0);
    return s;
}
// ... as sc[4b .. 4b + 3] in the log2 domain: sum x (page scale x query scale), in this association (k_attend_fp8 and
// k_qk_scores_fp8_linear multiply (sum x page scale) x query scale on the raw form: the two round differently).  ks4: the scales of the
// lane's four slot pages.
template <typename Piece>
__device__ __forceinline__ void fp8_scores(const Piece& k0, const Piece& k1, const uint32_t (&qd)[8], const f32x4& ks4, float qscale, int b,
                                           float (&sc)[8])
{
    const f32x4 s = fp8_scores_raw(k0, k1, qd);
#pragma unroll
    for (int i = 0; i < 4; ++i) sc[4 * b + i] = s[i] * (ks4[2 * b + (i >> 1)] * qscale);
}

// ---- slot pages
// page of the tile behind page slot r (0..3) of lane group kb: 2kb, 2kb + 1, 8 + 2kb, 9 + 2kb; its two positions are the lane's score
// slots 2r and 2r + 1
__device__ __forceinline__ uint32_t att_slot_page(uint32_t kb, int r) { return r < 2 ? 2u * kb + r : 8u + 2u * kb + (r - 2); }

// ---- online softmax of query row c (its 32 positions of a tile sit in lanes c, c + 16, c + 32, c + 48)
// The row's running max (log2 domain) over one more tile: m_use is what the tile's weights are taken against (0 for a row that is
// still fully masked: it stays at weight 0), the return value the factor that brings the running sum and accumulators to the new max.
__device__ __forceinline__ float att_softmax_step(const float (&sc)[8], float& m_run, float& m_use)
{
    float mx = sc[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) mx = fmaxf(mx, sc[j]);
    mx = max_over_kb(mx);
    const float m_new = fmaxf(m_run, mx);
    m_use = (m_new == -INFINITY) ? 0.0f : m_new;
    const float f = __builtin_amdgcn_exp2f(m_run - m_use);
    m_run = m_new;
    return f;
}
// The weights of a tile over FP8 V, for accumulators kept in units of the tile's V reference scale vref_t: the largest lane candidate
// vcand of the row's four lanes (a lane's largest V page scale among its pages inside the range; vref stays when that is 0).  The V
// page scales ride on the f16 weights as vs / vref_t <= 1.  Returns the one per-tile factor of the accumulators, f x vref_{t-1} /
// vref_t (old max -> new max, old V reference -> new).
__device__ __forceinline__ float fp8_v_weights(const float (&sc)[8], float m_use, float f, const f32x4& vs4, float vcand, float& vref,
                                               float& l_run, f16x8& P)
{
    const float vmx = max_over_kb(vcand);
    const float vref_t = vmx > 0.0f ? vmx : vref;
    const float rinv = __builtin_amdgcn_rcpf(vref_t);
    float psum = 0.0f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float p = __builtin_amdgcn_exp2f(sc[j] - m_use);
        psum += p;
        P[j] = static_cast<_Float16>(p * (vs4[j >> 1] * rinv));
    }
    l_run = l_run * f + psum;
    const float fa = f * (vref * rinv);
    vref = vref_t;
    return fa;
}
__device__ __forceinline__ float max4(const f32x4& v) { return fmaxf(fmaxf(v[0], v[1]), fmaxf(v[2], v[3])); }

// ---- out^T += V^T . P^T over FP8 V in the d = 8c + t map, accumulated in place (C = acc x fa): vx[j] = bytes 8c .. 8c + 7 of position
// slot j; v_perm_b32 pairs the bytes of two positions of one d column, the conversion to f16 is exact.  Pair: uint2 or u32x2.
template <typename Pair>
__device__ __forceinline__ void fp8_pv8(const Pair (&vx)[8], const f16x8& P, float fa, f32x4 (&acc)[8])
{
    uint32_t w[4][4];                                                     // [row pair][byte pair of the 8 d]
#pragma unroll
    for (int jp = 0; jp < 4; ++jp) {
        constexpr uint32_t kEven = 0x05010400u, kOdd = 0x07030602u;      // [lo.b0, hi.b0, lo.b1, hi.b1] / [lo.b2, hi.b2, lo.b3, hi.b3]
        w[jp][0] = __builtin_amdgcn_perm(vx[2 * jp + 1].x, vx[2 * jp].x, kEven);
        w[jp][1] = __builtin_amdgcn_perm(vx[2 * jp + 1].x, vx[2 * jp].x, kOdd);
        w[jp][2] = __builtin_amdgcn_perm(vx[2 * jp + 1].y, vx[2 * jp].y, kEven);
        w[jp][3] = __builtin_amdgcn_perm(vx[2 * jp + 1].y, vx[2 * jp].y, kOdd);
    }
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        f16x8 V;
#pragma unroll
        for (int jp = 0; jp < 4; ++jp) {
            const f16x2 h = (t & 1) ? __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w[jp][t >> 1], 1.0f, true)
                                    : __builtin_amdgcn_cvt_scalef32_pk_f16_fp8(w[jp][t >> 1], 1.0f, false);
            V[2 * jp] = h.x;
            V[2 * jp + 1] = h.y;
        }
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(V, P, acc[t] * fa, 0, 0, 0);
    }
}

// ---- epilogue in the d = 8c + t map (lane (c, kb) holds out[row c][32kb + 8i + t] in acc[t][i], in units of `unit`)
// final_rows: the wave's split is the whole range -- the normalised rows and their lse go to direct_out / direct_lse; otherwise the
// partial of this split in true units: part_acc [..][splits][16][128] (unnormalised), part_ml [..][splits][2][16] (running max in the
// log2 domain, running sum) for the merge.
__device__ __forceinline__ void att_store_rows8(const AttendArgs& a, const f32x4 (&acc)[8], float m_run, float l_run, float unit,
                                                bool final_rows, uint64_t row, uint64_t part, uint32_t c, uint32_t kb)
{
    const float l_tot = sum_over_kb(l_run);
    if (final_rows) {
        if (c < a.g) {
            const float w = l_tot > 0.0f ? unit / l_tot : 0.0f;
            float* dst = a.direct_out + (row * a.g + c) * 128u + 32u * kb;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                *reinterpret_cast<f32x4*>(dst + 8 * i) = f32x4{acc[0][i], acc[1][i], acc[2][i], acc[3][i]} * w;
                *reinterpret_cast<f32x4*>(dst + 8 * i + 4) = f32x4{acc[4][i], acc[5][i], acc[6][i], acc[7][i]} * w;
            }
            if (a.direct_lse && kb == 0)
                a.direct_lse[row * a.g + c] = l_tot > 0.0f ? (m_run + log2f(l_tot)) * 0.6931471805599453f : -INFINITY;
        }
        return;
    }
    if (kb == 0) {
        a.part_ml[part * 32u + c] = m_run;
        a.part_ml[part * 32u + 16u + c] = l_tot;
    }
    if (c < a.g) {
        float* dst = a.part_acc + (part * 16u + c) * 128u + 32u * kb;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            *reinterpret_cast<f32x4*>(dst + 8 * i) = f32x4{acc[0][i], acc[1][i], acc[2][i], acc[3][i]} * unit;
            *reinterpret_cast<f32x4*>(dst + 8 * i + 4) = f32x4{acc[4][i], acc[5][i], acc[6][i], acc[7][i]} * unit;
        }
    }
}

} // namespace
} // namespace speckv
