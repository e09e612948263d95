// cxl-speckv_amd/csrc/tensor_codec_device.hpp -- what the two directions of the whole-tensor codec share (tensor_compress.hip,
// tensor_decompress.hip, nobody else): the tile, the workgroup shapes that size the many-tensor workspace from both sides, the
// status words of the look-back chains, and the ONE place where (quant_mode, fp32?) turns into template arguments.
#pragma once
#include "kernels.hpp"
#include "tuning.hpp"
#include "codec_device.hpp"
#include "encode_device.hpp"
#include <algorithm>
#include <type_traits>

namespace speckv {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr uint32_t kTile = 2048;            // elements per tile (one wave)
#ifndef SPECKV_TF_WAVES
#define SPECKV_TF_WAVES 16
#endif
constexpr uint32_t kTfWaves = SPECKV_TF_WAVES;        // compress: tiles per workgroup
#ifndef SPECKV_TDF_LB_WAVE
#define SPECKV_TDF_LB_WAVE 0
#endif
constexpr uint32_t kTdfLbWave = SPECKV_TDF_LB_WAVE;   // 1: wave 0 of a workgroup takes no chunk, it only looks back (kTdfWaves - 1 chunks per workgroup)
// The many-streams kernels (k_tdm_fused / k_tdb_fused) take 8-wave workgroups: four of them per CU wait less at their barriers than
// two of 16 waves (4096 x 131 072 to fp32 0.63 -> 0.65, to fp16 0.56 -> 0.59); ONE long stream wants the 16 -- half as many status
// words to look back over (32 Mi elements: 0.37 against 0.30 with 8).
#ifndef SPECKV_TDM_WAVES
#define SPECKV_TDM_WAVES 8
#endif
constexpr uint32_t kTdmWaves = SPECKV_TDM_WAVES, kTdmChunks = kTdmWaves - kTdfLbWave;
constexpr uint32_t kScanWaves = 16, kScanMaxSteps = 2048;                // the one-workgroup scans (k_tc_scan_wg, k_td_scan_wg)
__device__ __forceinline__ uint64_t shfl64(uint64_t v, uint32_t src)
{
    const uint32_t lo = __shfl(static_cast<uint32_t>(v), static_cast<int>(src)), hi = __shfl(static_cast<uint32_t>(v >> 32), static_cast<int>(src));
    return (static_cast<uint64_t>(hi) << 32) | lo;
}
__device__ __forceinline__ unsigned long long lanes_above(uint32_t lane) { return lane == 63u ? 0ull : ~((2ull << lane) - 1ull); }

// A status word of a look-back chain: state << 62 | value (the states: tensor_compress.hip); each direction looks back its own way
typedef unsigned long long __attribute__((address_space(1))) tc_gu64;
__device__ __forceinline__ void tc_lb_store(uint64_t* w, uint64_t state, uint64_t value)
{
    __hip_atomic_store(reinterpret_cast<tc_gu64*>(reinterpret_cast<uintptr_t>(w)), (state << 62) | value, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint64_t tc_lb_load(const uint64_t* w)
{
    return __hip_atomic_load(reinterpret_cast<const tc_gu64*>(reinterpret_cast<uintptr_t>(w)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
constexpr uint64_t kTcLbMask = (1ull << 62) - 1ull;

struct TcbDesc { void* data; uint64_t n; uint8_t* rle; uint64_t rle_cap; };        // = speckv_ext_tensor_t (include/speckv_ext.h)
size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// (the two directions cut a tensor into workgroups of their own size: kTfWaves tiles to compress, kTdmChunks chunks to decompress)
static uint64_t tensors_wpt(uint64_t max_elems, uint32_t per_wg)
{
    return std::max<uint64_t>(1, (max_elems + static_cast<uint64_t>(per_wg) * kTile - 1) / (static_cast<uint64_t>(per_wg) * kTile));
}

// One kernel instance per (quantiser mode, fp32 or fp16 on the tensor's side): a launch site hands by_mode_f32 a generic lambda
// that takes the pair as two integral constants, (auto mode, auto f32), and launches k_...<mode(), f32()>.
template <class LAUNCH>
void by_mode_f32(int quant_mode, bool f32, const LAUNCH& launch)
{
    using intent = std::integral_constant<int, kIntent>; using ref_exact = std::integral_constant<int, kRefExact>;
    if (quant_mode == kIntent) { if (f32) launch(intent{}, std::true_type{}); else launch(intent{}, std::false_type{}); }
    else                       { if (f32) launch(ref_exact{}, std::true_type{}); else launch(ref_exact{}, std::false_type{}); }
}

} // namespace
} // namespace speckv
