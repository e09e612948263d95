// cxl-speckv_amd/csrc/attend_device.hpp -- device primitives shared by the attention translation units (attend.hip,
// attend_int4.hip, attend_mx4.hip; pack64 also by qk_scores_kernels.inl): vector types, global-address-space loads, the
// reductions over a query row's four lanes, wave-uniform pointers and the LDS-DMA issue statements.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace speckv {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

namespace {

// two dwords as the 64-bit operand of the fp8 MFMAs
__device__ __forceinline__ long pack64(uint32_t lo, uint32_t hi)
{
    return static_cast<long>(static_cast<uint64_t>(lo) | (static_cast<uint64_t>(hi) << 32));
}

// Record loads go through an explicit GLOBAL-address-space pointer.  A pointer the compiler cannot trace back to a kernel argument
// (one that is assigned under a template condition, or read from a page-table entry) otherwise becomes a FLAT load: flat loads
// count in lgkmcnt as well as vmcnt, the waits in front of the loop's scalar and LDS reads then drain every record load in
// flight, and the compiler's own vmcnt(N) bookkeeping collapses to vmcnt(0) -- the linear FP8 kernel lost 15 % that way when
// its pointers were initialised as nullptr for the striped instantiation (128 x 2k batch: 0.73 -> 0.62 of HBM peak).
#ifdef SPECKV_ABL_FLAT_LDG      // (A/B only: the loads as they were, flat wherever the pointer's origin is not visible)
#define SPECKV_GP(T, p) reinterpret_cast<const T*>(p)
#else
#define SPECKV_GP(T, p) ((const T __attribute__((address_space(1)))*)(reinterpret_cast<uintptr_t>(p)))
#endif
// 16 bytes of a record, non-temporal: every wave reads whole lines of its own
__device__ __forceinline__ uint4 ldg16(const uint8_t* p)
{
    const u32x4 v = __builtin_nontemporal_load(SPECKV_GP(u32x4, p));
    return make_uint4(v.x, v.y, v.z, v.w);
}
// 8 / 4 bytes of a record, non-temporal
__device__ __forceinline__ uint2 ldg8(const uint8_t* p)
{
    const u32x2 v = __builtin_nontemporal_load(SPECKV_GP(u32x2, p));
    return make_uint2(v.x, v.y);
}
__device__ __forceinline__ uint32_t ldg4(const uint8_t* p) { return __builtin_nontemporal_load(SPECKV_GP(uint32_t, p)); }
// one byte of a record (temporal)
__device__ __forceinline__ uint32_t ldg1(const uint8_t* p) { return *SPECKV_GP(uint8_t, p); }
// four floats of a scale table (temporal: the table is small and every workgroup of a layer or sequence reads it)
__device__ __forceinline__ f32x4 ldg_f4(const float* p) { return *SPECKV_GP(f32x4, p); }
// 16 bytes as a plain (temporal) load, for lines that a neighbouring wave reads too; always through the global address space
__device__ __forceinline__ uint4 ldg16_temporal(const uint8_t* p)
{
    typedef const u32x4 __attribute__((address_space(1)))* gp;
    const u32x4 v = *(gp)(reinterpret_cast<uintptr_t>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
}

// max over the four lanes {c, c+16, c+32, c+48}
__device__ __forceinline__ float max_over_kb(float v)
{
    // lane ^ 16 and lane ^ 32 through gfx950's row / half swaps (v_permlane16_swap / v_permlane32_swap: both operands the same
    // register -> the two rows, then the two halves, side by side), not through the LDS crossbar (ds_bpermute)
    const uint32_t u = __float_as_uint(v);
    const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    const uint32_t m = __float_as_uint(fmaxf(__uint_as_float(a[0]), __uint_as_float(a[1])));
    const auto b = __builtin_amdgcn_permlane32_swap(m, m, false, false);
    return fmaxf(__uint_as_float(b[0]), __uint_as_float(b[1]));
}
__device__ __forceinline__ float sum_over_kb(float v)
{
    const uint32_t u = __float_as_uint(v);
    const auto a = __builtin_amdgcn_permlane16_swap(u, u, false, false);
    const uint32_t m = __float_as_uint(__uint_as_float(a[0]) + __uint_as_float(a[1]));
    const auto b = __builtin_amdgcn_permlane32_swap(m, m, false, false);
    return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

// a pointer that is the same in every lane, pinned to scalar registers (the LDS-DMA statements below take their base
// address as an SGPR pair; a value loaded from a per-sequence descriptor is wave-uniform, but the compiler only proves
// that while no store of the kernel could alias the descriptor)
template <typename T> __device__ __forceinline__ T* uniform_ptr(T* p)
{
    const uint64_t v = reinterpret_cast<uint64_t>(p);
    const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v)), hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v >> 32));
    return reinterpret_cast<T*>((static_cast<uint64_t>(hi) << 32) | lo);
}

// One LDS-DMA: lane l's 16 (4) bytes at base + voff land at LDS address lds_dst + 16 (4) l; a lane that is not active fetches
// nothing.  M0 (the destination) belongs to the compiler: saved and restored inside the statement.  The caller counts the
// instruction in its s_waitcnt vmcnt(N).
__device__ __forceinline__ void dma16(uint32_t lds_dst, const uint8_t* base, uint32_t voff)
{
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %3\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(lds_dst), "v"(voff), "s"(base) : "memory");
}
__device__ __forceinline__ void dma4(uint32_t lds_dst, const uint8_t* base, uint32_t voff)
{
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %2, %3\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(lds_dst), "v"(voff), "s"(base) : "memory");
}
// the same with a full 64-bit address per lane (striped and page-table forms: a lane's rows may lie anywhere)
__device__ __forceinline__ void dma16v(uint32_t lds_dst, const uint8_t* addr)
{
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(lds_dst), "v"(addr) : "memory");
}
__device__ __forceinline__ void dma4v(uint32_t lds_dst, const uint8_t* addr)
{
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %2, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(lds_dst), "v"(addr) : "memory");
}
// dma16v with the non-temporal cache policy ("nt" on the instruction): rows that no other workgroup reads
__device__ __forceinline__ void dma16v_nt(uint32_t lds_dst, const uint8_t* addr)
{
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, off nt\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(lds_dst), "v"(addr) : "memory");
}

} // namespace
} // namespace speckv
