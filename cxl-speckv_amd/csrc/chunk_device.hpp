// cxl-speckv_amd/csrc/chunk_device.hpp -- what the chunk walk's translation units share (attend_chunk.hip: k_attend_chunk;
// attend_prefix.hip: k_attend_prefix): the LDS layout of a tile, global-address-space loads and stores, the undecoded bytes a thread
// keeps in flight for the next tile (Raw), and the three small decoders restated for ONE head's 8 elements of both positions of a
// page; they give the fp16 values speckv_ext_fetch_range gives (the fp32 product rounded once to fp16, pack_half2) -- but for the K
// rows of an FP8 pool, staged unscaled with the block scale applied to the score (decode_pool).  The decoders take the scheme of ONE
// side: k_attend_chunk names the K side's and the V side's apart (the split pool: FP8 keys, MXFP4 values).  Device code only.
#pragma once
#include "kernels.hpp"
#include "codec_device.hpp"          // pack_half2, half_bits_to_float
#include "attend_device.hpp"

namespace speckv {
namespace {

constexpr uint32_t kChunkThreads = 256;
constexpr uint32_t kKRow = 128 + 8;                       // fp16 elements of a K row in LDS
constexpr uint32_t kVRow = 32 + 4;                        // fp16 elements of a V^T row in LDS
constexpr uint32_t kKTile = 32 * kKRow, kVTile = 128 * kVRow, kBufElems = kKTile + kVTile;
constexpr float kLog2e = 1.4426950408889634f, kLn2 = 0.6931471805599453f;

typedef u32x4 __attribute__((address_space(1))) gk_u32x4;
typedef u32x2 __attribute__((address_space(1))) gk_u32x2;
template <typename T> __device__ __forceinline__ T ck_ld(const void* p) { return *SPECKV_GP(T, p); }
template <typename T> __device__ __forceinline__ void ck_st(void* p, T v)
{
    typedef T __attribute__((address_space(1))) G;
    *(G*)(reinterpret_cast<uintptr_t>(p)) = v;
}
__device__ __forceinline__ uint64_t ck_uniform(uint64_t v)
{
    const uint32_t lo = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v)), hi = __builtin_amdgcn_readfirstlane(static_cast<uint32_t>(v >> 32));
    return (static_cast<uint64_t>(hi) << 32) | lo;
}

// What a thread has in flight for one kind (K or V) of the next tile: the undecoded bytes of its 8 elements of both positions.
//   pool, FP8  : a.xy / b.xy = the 8 bytes of the even / odd position, aux = the block scale
//   pool, INT4 : a.x / b.x = the 4 nibble bytes, a.y / b.y = the group scale (fp16 bits)
//   pool, MXFP4: a.xy = the 8 bytes (low nibble even, high nibble odd position), a.z = the E8M0 code
//   held       : a / b = the 8 fp16 elements of the two rows
// len = the record length (0: zeros).
struct Raw { u32x4 a, b; uint32_t aux, len; };

template <int SCHEME>
__device__ __forceinline__ Raw load_pool(const PageEntry* e, uint32_t p0, bool live)
{
    Raw r{{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, 0u, 0u};
    if (!live) return r;
    const u32x4 w = ck_ld<u32x4>(e);
    const uint8_t* rec = reinterpret_cast<const uint8_t*>((static_cast<uint64_t>(w.y) << 32) | w.x);
    r.len = w.z;
    r.aux = w.w;
    if (SCHEME == kFp8E4m3) {
        if (r.len > kBlockElems) r.len = kBlockElems;
        if (p0 < r.len) { const u32x2 v = ck_ld<u32x2>(rec + p0); r.a.x = v.x; r.a.y = v.y; }
        if (p0 + 1024u < r.len) { const u32x2 v = ck_ld<u32x2>(rec + p0 + 1024u); r.b.x = v.x; r.b.y = v.y; }
    } else if (SCHEME == kInt4G32) {
        if (r.len >= kInt4RecBytes) {
            r.a.x = ck_ld<uint32_t>(rec + 128u + (p0 >> 1));
            r.b.x = ck_ld<uint32_t>(rec + 128u + ((p0 + 1024u) >> 1));
            r.a.y = ck_ld<uint16_t>(rec + 2u * (p0 >> 5));
            r.b.y = ck_ld<uint16_t>(rec + 2u * ((p0 + 1024u) >> 5));
        } else {
            r.len = 0u;
        }
    } else {
        if (r.len >= kMx4RecBytes) {
            const u32x2 v = ck_ld<u32x2>(rec + p0);
            r.a.x = v.x; r.a.y = v.y;
            r.a.z = ck_ld<uint8_t>(rec + r.aux + (p0 >> 4));         // PageEntry::scale of an MXFP4 page: the distance to its code row
        } else {
            r.len = 0u;
        }
    }
    return r;
}

// the 8 + 8 fp16 values of a Raw: ev / od = the even / odd position, two elements per word
// UNSCALED (the K rows of an FP8 pool): the E4M3 values themselves, exact in fp16 -- the block scale (pool_k_scale) multiplies the
// SCORE in fp32 instead.  value x scale rounded to fp16 costs every K element a relative 2^-12, and the score error that makes grows
// with |k|: rows of magnitude 3 took the output past the 2e-3 sum p|v| bound of this path.  The other formats decode exactly or are
// judged against their fp16 values, and V rows keep the rounded product (its error is relative to v: within the bound at any size).
template <int SCHEME, bool UNSCALED = false>
__device__ __forceinline__ void decode_pool(const Raw& r, uint32_t p0, uint32_t (&ev)[4], uint32_t (&od)[4])
{
    float y0[8], y1[8];
    if (SCHEME == kFp8E4m3) {
        const float s = UNSCALED ? 1.0f : __uint_as_float(r.aux);
#define CK_FP8(K, W, SEL) { y0[K] = __builtin_amdgcn_cvt_f32_fp8(static_cast<int>(r.a.W), SEL); y1[K] = __builtin_amdgcn_cvt_f32_fp8(static_cast<int>(r.b.W), SEL); }
        CK_FP8(0, x, 0) CK_FP8(1, x, 1) CK_FP8(2, x, 2) CK_FP8(3, x, 3) CK_FP8(4, y, 0) CK_FP8(5, y, 1) CK_FP8(6, y, 2) CK_FP8(7, y, 3)
#undef CK_FP8
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) {
            y0[k] = (p0 + k < r.len) ? y0[k] * s : 0.0f;
            y1[k] = (p0 + 1024u + k < r.len) ? y1[k] * s : 0.0f;
        }
    } else if (SCHEME == kInt4G32) {
        const float s0 = half_bits_to_float(r.a.y), s1 = half_bits_to_float(r.b.y);
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) {
            const int q0 = static_cast<int>(r.a.x << (28u - 4u * k)) >> 28, q1 = static_cast<int>(r.b.x << (28u - 4u * k)) >> 28;
            y0[k] = r.len ? static_cast<float>(q0) * s0 : 0.0f;
            y1[k] = r.len ? static_cast<float>(q1) * s1 : 0.0f;
        }
    } else {
        typedef float f32x2c __attribute__((ext_vector_type(2)));
        const uint32_t code = r.len ? r.a.z : 127u;
        const float s = __uint_as_float(code == 0u ? 0x00400000u : code == 255u ? 0x7FC00000u : code << 23);
#define CK_MX(K, W, SEL) { const f32x2c f = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(r.a.W, 1.0f, SEL); y0[K] = f.x * s; y1[K] = f.y * s; }
        CK_MX(0, x, 0) CK_MX(1, x, 1) CK_MX(2, x, 2) CK_MX(3, x, 3) CK_MX(4, y, 0) CK_MX(5, y, 1) CK_MX(6, y, 2) CK_MX(7, y, 3)
#undef CK_MX
    }
#pragma unroll
    for (uint32_t k = 0; k < 4u; ++k) {
        ev[k] = pack_half2(y0[2 * k], y0[2 * k + 1]);
        od[k] = pack_half2(y1[2 * k], y1[2 * k + 1]);
    }
}

// what the scores of a staged page are multiplied by: the block scale of an FP8 K page (decode_pool<FP8, true>), 1 otherwise
template <int SCHEME>
__device__ __forceinline__ float pool_k_scale(const Raw& r)
{
    return SCHEME == kFp8E4m3 && r.len ? __uint_as_float(r.aux) : 1.0f;
}

// the same piece of two held rows: addresses of 0 (beyond the sequence's held positions) give zeros
__device__ __forceinline__ Raw load_held(const _Float16* r0, const _Float16* r1)
{
    Raw r{{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, 0u, 1u};
    if (r0) r.a = ck_ld<u32x4>(r0);
    if (r1) r.b = ck_ld<u32x4>(r1);
    return r;
}

} // namespace
} // namespace speckv
