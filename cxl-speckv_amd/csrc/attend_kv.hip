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
#include "attend_kv_device.hpp"     // the kernel: shared with attend_kv_layers.hip

namespace speckv {

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
