// cxl-speckv_amd/csrc/attend_kv_layers.hip -- the split pool's decode step of SEVERAL layers in one launch (speckv_ext_attend_kv_layers): the LAYERS
// instance of k_attend_k8v4 (attend_kv_device.hpp) and its launcher.  A translation unit of its own, built with -packed-fp32-ops off (Makefile):
// the instances of attend_kv.hip keep their unit, their flags and their code.
#include "attend_kv_device.hpp"

namespace speckv {

// The decode step of several layers (kernels.hpp: AttendKvLayers): a.seqs / d_vside hold n_seq descriptors for region 0, a.batch_n_seq = n_seq,
// a.batch_layer = the first layer, a.order (if set) n_layers x n_seq members, a.n_splits = the largest per-sequence split count (0: nothing
// stored anywhere), a.direct_out = d_out.  At most two launches: the attention and, where some sequence has several pieces, ONE merge over
// all the layers, which passes over the members of one piece and of none (their rows are the attention kernel's).
hipError_t launch_attend_k8v4_layers(const AttendArgs& a, const AttendKvSide* d_vside, uint32_t n_seq, uint32_t n_layers, uint32_t layer_parts, bool merge,
                                     float* d_out, float* d_lse, hipStream_t s)
{
    if (n_seq == 0 || n_layers == 0) return hipSuccess;
    if (!a.seqs || !d_vside || !a.q16 || a.direct_out != d_out || a.heads % 4u || a.g == 0 || a.g > 16u || a.seq_skip || a.batch_n_seq != n_seq)
        return hipErrorInvalidValue;
    if (a.tail_idx && (!a.tail_k || !a.tail_v || a.tail_stride % 8u)) return hipErrorInvalidValue;
    const uint64_t rows = static_cast<uint64_t>(n_seq) * n_layers * (a.heads / 4u);
    const uint32_t splits = a.n_splits ? a.n_splits : 1u;                // (split 0 of a member with nothing stored folds its tail or writes its zeros)
    if (rows > (a.rows_first ? 0x7FFFFFFEull : 65535ull) || (a.rows_first && splits > 65535u)) return hipErrorInvalidValue;
    AttendArgs ar = a;
    ar.rows_real = static_cast<uint32_t>(rows);
    const dim3 gr = a.rows_first ? dim3(ar.rows_real | 1u, splits) : dim3(splits, ar.rows_real);
    hipLaunchKernelGGL((k_attend_k8v4<false, false, AttendKvLayers>), gr, dim3(256), 0, s, ar, d_vside, AttendKvLayers{layer_parts});
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || !merge) return e;
    ar.direct_per_seq = 3u;
    return launch_attend_combine(ar, n_seq * n_layers, d_out, d_lse, s, n_seq, layer_parts);
}

} // namespace speckv
