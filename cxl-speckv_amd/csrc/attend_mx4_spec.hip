// cxl-speckv_amd/csrc/attend_mx4_spec.hip -- the draft step of a batch over an MXFP4 pool (speckv_ext_attend_spec_mx4): k_attend_mx4_spec, up to
// 16 query rows per kv head (g = positions x rows per position) over ONE MXFP4 allocation per sequence in one pass over the records, and the
// rows the caller holds outside the pool folded in inside the same launch.  Records in one run only (k_attend_mx4's FORM 0).
//
// The workgroup, the fetch and the stage are k_attend_mx4<0>'s (attend_mx4.hip, attend_mx4_device.hpp): 4 waves x 2 kv heads = the 8 heads
// of a 32-position tile, every byte by LDS-DMA in ten 1 KiB requests per wave and tile into a stage of 8704 bytes, kStages tiles deep, one
// workgroup per CU, the request order K(t), V(t), K(t + 1), ... counted by hand in s_waitcnt vmcnt(N).  Both regions of a layer start on a
// storage tile (layouts with num_tokens % 32 == 0: the engine's condition), so a kernel tile is ONE storage tile.  grid (pieces, sequences)
// or rows-first (a.rows_first, a.rows_real), a.order the dispatch order, a.seqs one AttendSeq per sequence.  No z dimension.
//
// What differs is the column of the MFMAs.  k_attend_mx4 spends its 16 columns on (8 query rows x 2 position parities) with half of the
// query operand and half of the weights zero, and adds the parities in its epilogue.  Here the column IS the query row c = lane % 16:
//   scores  per head and tile 2 channel halves x 2 parities of v_mfma_scale_f32_16x16x128_f8f6f4: A = the K block as it lies in the record
//           with its E8M0 code (row = page, k = 2 x channel + position), B_w = the query row in MXFP8 per 16 channels -- k_attend_mx4's
//           quantisation, the same codes, the same bits -- in the k slots of parity w and zeros in the other parity's.
//           D_w[page 4kb + r][row c] leaves lane (c, kb) with the 8 scores of its OWN row: pages 4kb .. 4kb + 3 x positions 0 | 1.
//           Rows >= g are zero columns.  The four B operands per head are built once and HELD: 64 VGPRs per wave -- one wave per SIMD
//           has 512, and rebuilding them per tile would cost 32 v_perm per head in a loop that has nothing to hide them behind.
//   softmax per row over the lane's 8 scores, the row maximum over kb.  k_attend_mx4's LAZY reference maximum is kept: it moves only when a
//           tile's maximum passes it by more than 2^8 (weights <= 256: no concern in f16, the accumulators are fp32), so the 64 accumulator
//           registers are left alone once a split has settled -- att_softmax_step would rescale them every tile, 64 multiplies a tile on
//           the one wave of a SIMD.  (m_run, l_run, acc) stay a consistent triple: the held fold, att_store_rows8 and the merge take any.
//   P . V   the lane's 8 weights ARE the B operand of v_mfma_f32_16x16x32_f16 in k order (page 4kb + i, position 0 | 1): no zero padding and
//           no parity merge.  V is widened by v_cvt_scalef32_pk_f16_fp4 with the block code inside the conversion, as in k_attend_mx4: 8
//           MFMAs per head and tile.  acc[t][i] = channel 32kb + 8i + t of row c, k_attend_k8v4's map, so att_store_rows8 and
//           k8v4_fold_held serve each of the wave's two heads unchanged.
// The records are fetched once for 16 rows where k_attend_mx4 (grid z = 2) walks them twice and a fold launch follows.
//
// Edges: a ragged last tile (n_pages % 16 != 0) masks the scores of pages >= n_pages by a select -- a hostile K code there is a NaN in that
// page's row of D alone -- and drops those pages' V codes, as k_attend_k8v4 does, so that a weight of exactly 0 meets a finite value.  A
// member with nothing stored runs the held fold alone in split 0; a row that sees nothing is exactly 0 with lse -inf.  Split 0 folds the
// held rows into its final rows or into its partial (part_acc / part_ml, true units, 16 rows); launch_attend_combine merges.
//
// Resources (gfx950, -O3; the compiler's report): 198 VGPRs, 224 AGPRs (k_attend_mx4<0>: 214 and 200 -- the compiler parks what the three
// unrolled tile bodies keep live in the second half of the one wave's 512 registers), no scratch, no spill, no static LDS, 104 448 bytes
// of dynamic LDS (4 waves x 3 stages x 8704), one wave per SIMD.  The build fails on scratch: its vmcnt accounting would be wrong.
#include "attend_mx4_device.hpp"
#include "attend_kv_device.hpp"      // k8v4_fold_held; with it attend_fp8_device.hpp: att_store_rows8
#include <atomic>

namespace speckv {

__global__ __launch_bounds__(64 * kWavesPerWg) __attribute__((amdgpu_waves_per_eu(1, 1))) void k_attend_mx4_spec(AttendArgs a, AttendHeldArgs h)
{
    constexpr uint32_t kStages = kStagesDefault;
    extern __shared__ __attribute__((aligned(16))) uint8_t lds_dyn[];                  // kWavesPerWg x kStages stages (102 KiB: beyond the static limit)
    uint8_t (*lds)[kStages * kStage] = reinterpret_cast<uint8_t (*)[kStages * kStage]>(lds_dyn);
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t c = lane & 15u, kb = lane >> 4;                       // query row c; pages 4kb .. 4kb + 3 of a tile, channels 32kb .. 32kb + 31 of the output
    const uint32_t split = a.rows_first ? blockIdx.y : blockIdx.x;
    uint32_t seq = a.rows_first ? blockIdx.x : blockIdx.y;
    if (a.rows_first && seq >= a.rows_real) return;                      // (padding row: see AttendArgs::rows_real)
    if (a.order) seq = a.order[seq];                                     // (workgroup-uniform)
    const uint32_t h0 = wave * 2u;                                       // first of this wave's two kv heads
    const uint64_t row0 = static_cast<uint64_t>(seq) * 8u + h0;          // query / output row block of head 0 (head 1: + 1)
    const AttendSeq sq = a.seqs[seq];
    if (split >= sq.n_splits && (sq.n_splits != 0u || split != 0u)) return;      // (nothing stored: split 0 goes on to the held positions alone)
    const uint64_t part0 = sq.part_base + static_cast<uint64_t>(h0) * sq.n_splits + split;      // partials of head 0 | head 1: part0, part0 + n_splits
    const uint32_t n_pages = sq.n_pages;
    const uint32_t n_tiles = (n_pages + 15u) / 16u;
    const uint32_t t0 = split * sq.tiles_per_split;
    const uint32_t t1 = min(t0 + sq.tiles_per_split, n_tiles);
    float m_run[2] = {-INFINITY, -INFINITY}, l_run[2] = {0.0f, 0.0f};
    f32x4 acc[2][8];
#pragma unroll
    for (int hh = 0; hh < 2; ++hh)
#pragma unroll
        for (int s = 0; s < 8; ++s) acc[hh][s] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    if (t0 < t1) {                                                       // wave-uniform
        const uint32_t lbase = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(reinterpret_cast<uintptr_t>(&lds[wave][0])));
        const uint8_t* const lptr = &lds[wave][0];
        // ---- staging, as in k_attend_mx4: DMA instruction i (0..3) of a region fills page rows 4i .. 4i+3: lane l -> row 4i + l/16, 16-byte
        // slot l%16, which holds piece (slot ^ row) of the two heads' 256 bytes -- the XOR spreads the operand reads below over the banks.
        // Byte offsets from the nibble row of the tile's first record (a scalar base): row r at r * 1024, its codes at 16384 + r * 64
        const uint32_t srow = lane >> 4, sslot = lane & 15u;
        uint32_t goff[4];
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) goff[i] = (4u * i + srow) * 1024u + h0 * 128u + ((sslot ^ ((4u * i + srow) & 15u)) * 16u);
        const uint32_t goffc = kMx4CodePlane + (lane >> 2) * 64u + h0 * 8u + (lane & 3u) * 4u;      // codes: lane l -> page l/4, dword l%4 of the two heads' 16
        const uint32_t last = t1 - 1u;
        const uint8_t* const run = uniform_ptr(sq.lin_base);
        // (multiples of 16: a kernel tile is one storage tile; scalar, as the DMA statements take their base)
        const uint32_t kfirst = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(sq.k_first)), vfirst = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(sq.v_first));
        // one region's share of a tile (rg = 0: K rows + K codes, 1: V rows + V codes) into stage `buf`: 5 DMA instructions; a request past
        // the piece repeats its last tile
        auto stage = [&](uint32_t tt, uint32_t buf, uint32_t rg) __attribute__((always_inline)) {
            const uint32_t dst = lbase + buf * kStage;
            const uint64_t R = static_cast<uint64_t>(rg ? vfirst : kfirst) + 16ull * min(tt, last);
            dma_region(dst + (rg ? kStV : kStK), dst + (rg ? kStVC : kStKC), run + mx4_nib_off(R), goff, goffc);
        };
        // request order K(t), V(t), K(t+1), V(t+1), ...: five instructions each, so "all but the 25 youngest" is "this region has landed"
#pragma unroll
        for (uint32_t sg = 0; sg < kStages; ++sg) { stage(t0 + sg, sg, 0u); stage(t0 + sg, sg, 1u); }

        // ---- query operands (MXFP8, blocks of 16 channels): lane (c, kb) takes channels 8kb + 32 gq + 0..7 (gq = 0..3) of query row c of both
        // heads; operand [head][half hf][parity w] bytes 0..15 <- gq = 2 hf, bytes 16..31 <- gq = 2 hf + 1, the row's bytes in the k slots of w
        v8i QB[2][2][2];
        int q_code[2][2];
        {
            const bool live = c < a.g;
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                const uint16_t* qrow = a.q16 + ((row0 + hh) * a.g + min(c, a.g - 1u)) * 128u;
                float x[4][8];
                uint32_t code[4];
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    const u32x4 wv = *SPECKV_GP(u32x4, qrow + 8u * kb + 32u * gq);
                    const uint32_t ws[4] = {wv.x, wv.y, wv.z, wv.w};
                    float amax = 0.0f;
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        x[gq][k] = q_clean((ws[k >> 1] >> (16 * (k & 1))) & 0xFFFFu);
                        amax = fmaxf(amax, fabsf(x[gq][k]));
                    }
                    // the block of 16 channels = this lane's 8 and lane ^ 16's 8 (kb ^ 1)
                    const auto sw = __builtin_amdgcn_permlane16_swap(__float_as_uint(amax), __float_as_uint(amax), false, false);
                    amax = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
                    code[gq] = (live && amax > 0.0f) ? (__float_as_uint(amax) >> 23) - 8u : 0u;            // floor(log2 amax) - 8 + 127
                }
                uint32_t qd[2][16];
#pragma unroll
                for (int gq = 0; gq < 4; ++gq) {
                    const float mul = __uint_as_float((254u - code[gq]) << 23);                             // 2^(127 - code), exact
                    float v[8];
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[k] = live ? fminf(fmaxf(x[gq][k] * mul, -448.0f), 448.0f) : 0.0f;
                    int p0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], 0, false);
                    p0 = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], p0, true);
                    int p1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[4], v[5], 0, false);
                    p1 = __builtin_amdgcn_cvt_pk_fp8_f32(v[6], v[7], p1, true);
                    // bytes b0..b7 -> (b0, 0, b1, 0, ...) for parity 0, (0, b0, 0, b1, ...) for parity 1   (selector 0x0c = a zero byte)
#pragma unroll
                    for (int w = 0; w < 2; ++w) {
                        const uint32_t sl = w ? 0x010C000Cu : 0x0C010C00u, sh = w ? 0x030C020Cu : 0x0C030C02u;
                        qd[w][4 * gq + 0] = __builtin_amdgcn_perm(0u, static_cast<uint32_t>(p0), sl);
                        qd[w][4 * gq + 1] = __builtin_amdgcn_perm(0u, static_cast<uint32_t>(p0), sh);
                        qd[w][4 * gq + 2] = __builtin_amdgcn_perm(0u, static_cast<uint32_t>(p1), sl);
                        qd[w][4 * gq + 3] = __builtin_amdgcn_perm(0u, static_cast<uint32_t>(p1), sh);
                    }
                }
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {
#pragma unroll
                    for (int w = 0; w < 2; ++w)
                        QB[hh][hf][w] = v8i{static_cast<int>(qd[w][8 * hf + 0]), static_cast<int>(qd[w][8 * hf + 1]), static_cast<int>(qd[w][8 * hf + 2]),
                                            static_cast<int>(qd[w][8 * hf + 3]), static_cast<int>(qd[w][8 * hf + 4]), static_cast<int>(qd[w][8 * hf + 5]),
                                            static_cast<int>(qd[w][8 * hf + 6]), static_cast<int>(qd[w][8 * hf + 7])};
                    // the lane's scale operand: hardware block kb of this instruction = channels 64 hf + 16 kb .. + 15 = the block lanes
                    // (kb' = 2 (kb & 1), 2 (kb & 1) + 1) computed as their group gq = 2 hf + (kb >> 1)
                    const uint32_t src = c + 32u * (kb & 1u);
                    const uint32_t s0 = __shfl(code[2 * hf], src), s1 = __shfl(code[2 * hf + 1], src);
                    q_code[hh][hf] = static_cast<int>((kb >> 1) ? s1 : s0);
                }
            }
        }
        // ---- where the lane reads its operands in a stage (k_attend_mx4's: the A operands of both products are the same)
        uint32_t rk[2][2], rkc[2][2], rv[2][4], rvc[2][4];
#pragma unroll
        for (uint32_t hh = 0; hh < 2; ++hh) {
#pragma unroll
            for (uint32_t hf = 0; hf < 2; ++hf) {
                rk[hh][hf] = kStK + c * 256u + (((hh * 8u + hf * 4u + kb) ^ c) * 16u);                  // row = page c: one 16-byte MX block
                rkc[hh][hf] = kStKC + c * 16u + hh * 8u + hf * 4u + kb;
            }
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) {
                const uint32_t pg = 4u * kb + i;
                rv[hh][i] = kStV + pg * 256u + (((hh * 8u + (c >> 1)) ^ pg) * 16u) + (c & 1u) * 8u;      // bytes 8c .. 8c+7 of the head's row
                rvc[hh][i] = kStVC + pg * 16u + hh * 8u + (c >> 1);
            }
        }
        const bool ragged = (n_pages & 15u) != 0u;
        const float scale_log2e = a.scale_log2e;
        // one tile out of stage BUF (a compile-time constant: the LDS reads then carry the stage as an immediate offset)
        auto tile_body = [&](uint32_t tile, auto buf_c) __attribute__((always_inline)) {
            const uint32_t buf = buf_c;
            const uint8_t* st = lptr + buf * kStage;
            // ---- K of this tile has landed (younger requests: V of this tile, K and V of the next ones): both heads' blocks and codes
            // to registers, and the region goes straight back to the DMA for the tile kStages further on
            wait_all_but<10u * kStages - 5u>();
            u32x4 kx[2][2];
            uint32_t kc[2][2];
#pragma unroll
            for (int hh = 0; hh < 2; ++hh)
#pragma unroll
                for (int hf = 0; hf < 2; ++hf) {
                    kx[hh][hf] = *reinterpret_cast<const u32x4*>(st + rk[hh][hf]);
                    kc[hh][hf] = st[rkc[hh][hf]];
                }
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(kx[0][0]), "+v"(kx[0][1]), "+v"(kx[1][0]), "+v"(kx[1][1]), "+v"(kc[0][0]), "+v"(kc[0][1]), "+v"(kc[1][0]), "+v"(kc[1][1]) :: "memory");
            stage(tile + kStages, buf, 0u);
            const bool edge = ragged && tile + 1u == n_tiles;           // wave-uniform: pages at or beyond pos_end (even: whole pages)
            f16x8 P[2];
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                // ---- scores: per parity two block-scaled MFMAs (channels 0..63, 64..127) over the tile's 16 pages
                float sc[8];
#pragma unroll
                for (int w = 0; w < 2; ++w) {
                    f32x4 s = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                    for (int hf = 0; hf < 2; ++hf) {
                        const v8i A = {static_cast<int>(kx[hh][hf].x), static_cast<int>(kx[hh][hf].y), static_cast<int>(kx[hh][hf].z), static_cast<int>(kx[hh][hf].w), 0, 0, 0, 0};
                        s = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(A, QB[hh][hf][w], s, 4 /* A: e2m1 */, 0 /* B: e4m3 */, 0, static_cast<int>(kc[hh][hf]), 0, q_code[hh][hf]);
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) sc[2 * r + w] = s[r] * scale_log2e;
                }
                if (edge) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (tile * 16u + 4u * kb + r >= n_pages) { sc[2 * r] = -INFINITY; sc[2 * r + 1] = -INFINITY; }
                }
                // ---- online softmax of query row c (its 32 positions of the tile sit in lanes c, c + 16, c + 32, c + 48) against the lazy
                // reference maximum
                float mx = sc[0];
#pragma unroll
                for (int j = 1; j < 8; ++j) mx = fmaxf(mx, sc[j]);
                mx = max_over_kb(mx);
                if (__builtin_expect(__ballot(mx > m_run[hh] + 8.0f) != 0ull, 0)) {         // (wave-uniform; -inf + 8 = -inf: the first tile comes here)
                    const float m_new = (mx > m_run[hh] + 8.0f) ? mx : m_run[hh];
                    const float f = (m_new == -INFINITY) ? 1.0f : __builtin_amdgcn_exp2f(m_run[hh] - m_new);
                    m_run[hh] = m_new;
                    l_run[hh] *= f;
#pragma unroll
                    for (int t = 0; t < 8; ++t) acc[hh][t] *= f;
                }
                const float m_use = (m_run[hh] == -INFINITY) ? 0.0f : m_run[hh];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float p = __builtin_amdgcn_exp2f(sc[j] - m_use);
                    l_run[hh] += p;
                    P[hh][j] = static_cast<_Float16>(p);                  // k slot j = (page 4kb + j / 2, position j % 2)
                }
            }
            // ---- V of this tile has landed (younger: K and V of the next tiles): both heads' pieces and codes
            wait_all_but<10u * kStages - 5u>();
            u32x2 vx[2][4];
            uint32_t vcode[2][4];
#pragma unroll
            for (int hh = 0; hh < 2; ++hh)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    vx[hh][i] = *reinterpret_cast<const u32x2*>(st + rv[hh][i]);
                    vcode[hh][i] = st[rvc[hh][i]];
                }
            asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(vx[0][0]), "+v"(vx[0][1]), "+v"(vx[0][2]), "+v"(vx[0][3]), "+v"(vx[1][0]), "+v"(vx[1][1]), "+v"(vx[1][2]), "+v"(vx[1][3]),
                         "+v"(vcode[0][0]), "+v"(vcode[0][1]), "+v"(vcode[0][2]), "+v"(vcode[0][3]), "+v"(vcode[1][0]), "+v"(vcode[1][1]), "+v"(vcode[1][2]), "+v"(vcode[1][3]) :: "memory");
            stage(tile + kStages, buf, 1u);
            // ---- out^T += V^T . P^T: a byte of the record = channel d of both positions of a page -> one operand register
#pragma unroll
            for (int hh = 0; hh < 2; ++hh) {
                float vsc[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    // (a masked page's code goes too: it may be a stale record of any magnitude, and its weight of exactly 0 must meet a finite value)
                    if (edge && tile * 16u + 4u * kb + i >= n_pages) vcode[hh][i] = 0u;
                    vsc[i] = __uint_as_float(vcode[hh][i] << 23);          // the block's E8M0 code as a float's exponent field
                }
#define MX_PV(S, WORD, SEL)                                                                                                          \
    {                                                                                                                                \
        const u32x4 vw = {__builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(vx[hh][0].WORD, vsc[0], SEL)),        \
                          __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(vx[hh][1].WORD, vsc[1], SEL)),        \
                          __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(vx[hh][2].WORD, vsc[2], SEL)),        \
                          __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp4(vx[hh][3].WORD, vsc[3], SEL))};       \
        acc[hh][S] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, vw), P[hh], acc[hh][S], 0, 0, 0);               \
    }
                MX_PV(0, x, 0) MX_PV(1, x, 1) MX_PV(2, x, 2) MX_PV(3, x, 3) MX_PV(4, y, 0) MX_PV(5, y, 1) MX_PV(6, y, 2) MX_PV(7, y, 3)
#undef MX_PV
            }
        };
#pragma unroll 1
        for (uint32_t tile = t0; tile < t1; tile += kStages) {
            tile_body(tile, std::integral_constant<uint32_t, 0u>{});
            if (tile + 1u >= t1) break;
            tile_body(tile + 1u, std::integral_constant<uint32_t, 1u>{});
            if (kStages > 2u) {
                if (tile + 2u >= t1) break;
                tile_body(tile + 2u, std::integral_constant<uint32_t, (kStages > 2u ? 2u : 0u)>{});
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                 // the re-requested last tiles: nothing may land after the wave ends
    }
    // ---- split 0 folds the held positions (workgroup-uniform); then a single piece (or none): the final rows, else the partial of this piece
#pragma unroll
    for (uint32_t hh = 0; hh < 2u; ++hh) {
        if (split == 0u) k8v4_fold_held(a, h, seq, h0 + hh, row0 + hh, c, kb, m_run[hh], l_run[hh], acc[hh]);
        att_store_rows8(a, acc[hh], m_run[hh], l_run[hh], 1.0f, sq.n_splits <= 1u, row0 + hh, part0 + hh * sq.n_splits, c, kb);
    }
}

// The draft step of an MXFP4 pool: a.seqs (device-visible) holds n_seq descriptors as launch_attend_mx4 takes them in the linear batch form
// (lin_base, k_first / v_first multiples of 16); a.n_splits = the largest per-sequence piece count (0: no member walks anything),
// a.direct_out = d_out.  merge = some member has several pieces: launch_attend_combine follows on `s` and passes over the members with one
// piece or none, whose rows the kernel wrote itself.
hipError_t launch_attend_mx4_spec(const AttendArgs& a, const AttendHeldArgs& h, uint32_t n_seq, bool merge, float* d_out, float* d_lse, hipStream_t s)
{
    if (n_seq == 0) return hipSuccess;
    if (!a.seqs || !a.q16 || a.direct_out != d_out || a.heads != 8u || a.g == 0 || a.g > 16u) return hipErrorInvalidValue;
    if (!h.k_held || !h.v_held || !h.mask || h.rows_per_pos == 0 || a.g % h.rows_per_pos || a.g / h.rows_per_pos > kHeldMax - 1u ||
        h.mask_stride < a.g / h.rows_per_pos || h.seq_stride % 8u || h.pos_stride % 8u)
        return hipErrorInvalidValue;
    AttendArgs ar = a;
    const uint32_t splits = a.n_splits ? a.n_splits : 1u;               // (split 0 of a member that walks nothing folds its held positions)
    ar.rows_real = n_seq;
    const dim3 gr = a.rows_first ? dim3(n_seq | 1u, splits) : dim3(splits, n_seq);
    constexpr size_t lds_bytes = static_cast<size_t>(kWavesPerWg) * kStagesDefault * kStage;
    // more than 64 KiB of dynamic LDS has to be allowed per function AND per device: once for every device this process launches on
    static std::atomic<uint64_t> allowed{0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev > 63) return hipErrorInvalidDevice;
    if (!(allowed.load(std::memory_order_acquire) >> dev & 1ull)) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_attend_mx4_spec), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
        if (e != hipSuccess) return e;
        allowed.fetch_or(1ull << dev, std::memory_order_release);
    }
    hipLaunchKernelGGL(k_attend_mx4_spec, gr, dim3(64 * kWavesPerWg), lds_bytes, s, ar, h);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || !merge) return e;
    ar.direct_per_seq = 3u;                                              // the merge passes over the members without a piece too: their rows are the softmax over the held positions
    return launch_attend_combine(ar, n_seq, d_out, d_lse, s);
}

} // namespace speckv
