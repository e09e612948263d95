// cxl-speckv_amd/csrc/block_codec_device.hpp -- the device code of the block codec (device code only): what turns one record
// into a block's 4 KiB image and back, without the kernels that say which block a wave owns.  Streaming global loads and stores,
// the destination forms of a decoder (a contiguous image, the two rows of a RowSink / RowSinkBf16), every decode_* helper, the RLE
// encoder, the source forms of an encoder (SrcRun, SrcPair, SrcPairMixed, SrcPairScaled) and compress_block, the one body of every encoder kernel.
// Included by kernels.hip (k_fetch_decompress*, k_compress) and by row_transfer.hip (the pair and slot kernels); the
// instruction-level helpers underneath are codec_device.hpp and encode_device.hpp.
//
// Everything here is __forceinline__ but decode_rle_general, encode_rle_general and absmax_with_nonfinite in their contiguous
// forms, which only kernels.hip calls: a translation unit that uses the sink and source forms alone gets no out-of-line function.
#pragma once
#include "kernels.hpp"
#include "codec_device.hpp"
#include "encode_device.hpp"
#include "attend_device.hpp"         // u32x4, u32x2

#include <hip/hip_fp16.h>

#include <type_traits>

namespace speckv {
namespace {

#ifndef SPECKV_WAVES
#define SPECKV_WAVES 4
#endif
constexpr int kWaves = SPECKV_WAVES;      // wavefronts per workgroup (independent of each other)
constexpr int kThreads = 64 * kWaves;
constexpr int kDecLdsWords = 528;         // per wave: 2 KiB byte table + 64 B of write-only dummies
constexpr int kEncLdsHalves = 2064;        // per wave: 4128 B (see kEncWaveBytes)

// Streaming accesses: every record byte is read once and every output byte
// written once per launch, so both are marked non-temporal (measured on MI355X,
// 131072 blocks: nt stores +4..8 %, nt loads+stores +6..10 % over plain accesses;
// -DSPECKV_PLAIN_LOAD / -DSPECKV_PLAIN_STORE restore the plain forms for A/B).
#if !defined(SPECKV_PLAIN_LOAD)
#define SPECKV_NT_LOAD 1
#endif
#if !defined(SPECKV_PLAIN_STORE)
#define SPECKV_NT_STORE 1
#endif
// Records and block images are reached through pointers read from page-table entries / pointer lists, which the compiler cannot
// trace back to a kernel argument: plain C++ dereferences of them become FLAT loads and stores (an address-space check per
// access, and every one counts in lgkmcnt as well as vmcnt, so the waits in front of LDS and scalar reads wait for them too).
// The codec's accesses therefore go through explicit global-address-space pointers (attend.hip: the same hazard cost the
// linear FP8 attention kernel 15 %).
typedef u32x4 __attribute__((address_space(1))) g_u32x4;
template <typename T> __device__ __forceinline__ T gload(const void* p)
{
    typedef T __attribute__((address_space(1))) G;
    return *(const G*)(reinterpret_cast<uintptr_t>(p));
}
template <typename T> __device__ __forceinline__ void gstore(void* p, T v)
{
    typedef T __attribute__((address_space(1))) G;
    *(G*)(reinterpret_cast<uintptr_t>(p)) = v;
}
__device__ __forceinline__ uint2 gload_u2(const void* p)
{
    typedef uint32_t v2 __attribute__((ext_vector_type(2)));
    const v2 v = gload<v2>(p);
    return make_uint2(v.x, v.y);
}
__device__ __forceinline__ uint4 ld16(const uint8_t* p)
{
    const g_u32x4* gp = (const g_u32x4*)(reinterpret_cast<uintptr_t>(p));
#if defined(SPECKV_NT_LOAD)
    const u32x4 v = __builtin_nontemporal_load(gp);
#else
    const u32x4 v = *gp;
#endif
    return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st16(uint8_t* p, uint4 v)
{
    g_u32x4* gp = (g_u32x4*)(reinterpret_cast<uintptr_t>(p));
    const u32x4 t = {v.x, v.y, v.z, v.w};
#if defined(SPECKV_NT_STORE)
    __builtin_nontemporal_store(t, gp);
#else
    *gp = t;
#endif
}
// The compress direction streams too: every source byte is read once, every record byte written once (the fp16 "compress"
// is a plain copy and ran at 0.65-0.67 of HBM peak with temporal accesses against 0.77 for the same copy in the decode
// direction; -DSPECKV_ENC_PLAIN restores them for the A/B).
__device__ __forceinline__ uint4 enc_ld16(const uint8_t* p)
{
#if defined(SPECKV_ENC_PLAIN)
    const u32x4 v = *(const g_u32x4*)(reinterpret_cast<uintptr_t>(p));
    return make_uint4(v.x, v.y, v.z, v.w);
#else
    return ld16(p);
#endif
}
__device__ __forceinline__ void enc_st16(uint8_t* p, uint4 v)
{
#if defined(SPECKV_ENC_PLAIN)
    *(g_u32x4*)(reinterpret_cast<uintptr_t>(p)) = u32x4{v.x, v.y, v.z, v.w};
#else
    st16(p, v);
#endif
}
__device__ __forceinline__ void enc_st8(uint8_t* p, uint2 v)
{
    typedef u32x2 __attribute__((address_space(1))) g_u32x2;
    g_u32x2* gp = (g_u32x2*)(reinterpret_cast<uintptr_t>(p));
    const u32x2 t = {v.x, v.y};
#if defined(SPECKV_ENC_PLAIN)
    *gp = t;
#else
    __builtin_nontemporal_store(t, gp);
#endif
}
// fp32 output: a lane's eight values are 32 bytes, so two 16-byte stores per lane at a 32-byte stride -- every store instruction
// of the wave then writes a 16-byte piece of every other 32, half of each 64-byte sector of memory, and the sector is written again by
// the second instruction: 512 MiB of fp32 output took 558 us where the fp16 form of the same blocks takes 171 (0.36 of the HBM
// roofline against 0.78).  The values go through 2 KiB of the wave's LDS instead (written per lane, read back 16 bytes x 64 lanes in
// a row), so that each instruction writes one contiguous KiB, as the fp16 form does.  p0 = 512 j + 8 lane (every caller's layout).
__device__ __forceinline__ void store8_f32(uint8_t* dst, uint32_t p0, const float (&y)[8])
{
    __shared__ __attribute__((aligned(16))) uint4 stage[kWaves][128];
    const uint32_t lane = threadIdx.x & 63u;
    uint4* st = stage[(threadIdx.x >> 6) % kWaves];
    wave_lds_fence();                                       // (the reads of the chunk before are done: LDS is in order per wave)
    st[2u * lane] = make_uint4(__float_as_uint(y[0]), __float_as_uint(y[1]), __float_as_uint(y[2]), __float_as_uint(y[3]));
    st[2u * lane + 1u] = make_uint4(__float_as_uint(y[4]), __float_as_uint(y[5]), __float_as_uint(y[6]), __float_as_uint(y[7]));
    wave_lds_fence();
    const uint4 a = st[lane], b = st[64u + lane];
    uint8_t* base = dst + 4ull * (p0 - 8u * lane) + 16u * lane;
    st16(base, a);
    st16(base + 1024, b);
}
// Where a decoder puts a block's fp16 image.  Every decoder below takes its destination as a type: a plain pointer is the
// contiguous 4 KiB image (fetch, ring, flush), a RowSink the two position rows of a page where a caller holds them apart
// (k_read_pairs).  The decoders ask wants() per 512-element chunk before they load anything of it and hand whole chunks to
// put16 / store8 -- p0 = 512 j + 8 lane, so a chunk lies in one half of the block and `p0 < 1024` is wave-uniform.
struct RowSink {
    uint8_t* even;      // elements [0, 1024): the even position's [heads][128] row; nullptr = not wanted
    uint8_t* odd;       // elements [1024, 2048)
    __device__ __forceinline__ uint8_t* row(uint32_t p) const { return p < 1024u ? even : odd; }
};
// (how a decoder declares its destination parameter: a plain pointer keeps the __restrict__ it always had)
template <class DST> struct dst_arg { typedef const DST& type; };
template <> struct dst_arg<uint8_t*> { typedef uint8_t* __restrict__ type; };
__device__ __forceinline__ bool wants(const uint8_t*, uint32_t) { return true; }
__device__ __forceinline__ bool wants(const RowSink& d, uint32_t p0) { return d.row(p0) != nullptr; }
__device__ __forceinline__ void put16(const RowSink& d, uint32_t p0, uint4 v)
{
    uint8_t* r = d.row(p0);
    if (r) st16(r + 2ull * (p0 & 1023u), v);
}
// The same two rows where the caller's cache holds bf16 (k_read_slots_ex): a decoder still hands over the fp16 bits that
// speckv_ext_fetch_range writes, and the sink rounds THOSE once to bf16 (nearest even; fp16 -> fp32 is exact, so the one rounding
// is fp32 -> bf16 of the fp16 value, never of the decoder's fp32 intermediate) -- eight elements in registers, then the same one
// 16-byte store per lane, 1 KiB per instruction.  A NaN stays a NaN.
struct RowSinkBf16 {
    uint8_t* even;
    uint8_t* odd;
    __device__ __forceinline__ uint8_t* row(uint32_t p) const { return p < 1024u ? even : odd; }
};
template <class DST> struct is_row_sink { static constexpr bool value = false; };
template <> struct is_row_sink<RowSink> { static constexpr bool value = true; };
template <> struct is_row_sink<RowSinkBf16> { static constexpr bool value = true; };
__device__ __forceinline__ uint32_t pack_bf16x2(float a, float b)                        // one packed conversion for the two
{
    typedef float pair_f32 __attribute__((ext_vector_type(2)));
    typedef __bf16 pair_bf16 __attribute__((ext_vector_type(2)));
    const pair_f32 f = {a, b};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(f, pair_bf16));
}
__device__ __forceinline__ uint32_t half2_to_bf16x2(uint32_t w) { return pack_bf16x2(half_bits_to_float(w & 0xFFFFu), half_bits_to_float(w >> 16)); }
// ... and backwards, a bf16 row read by the encoder or moved into a held fp16 row: the exact value rounded once to fp16 (nearest
// even; overflow gives inf, a NaN stays a NaN, fp16 subnormals are kept and what is smaller rounds to +-0) -- pack_half2's rounding
__device__ __forceinline__ uint32_t bf16x2_to_half2(uint32_t w)
{
    return pack_half2(__uint_as_float(w << 16), __uint_as_float(w & 0xFFFF0000u));
}
__device__ __forceinline__ uint4 half8_to_bf16(uint4 v) { return make_uint4(half2_to_bf16x2(v.x), half2_to_bf16x2(v.y), half2_to_bf16x2(v.z), half2_to_bf16x2(v.w)); }
__device__ __forceinline__ uint4 bf16_to_half8(uint4 v) { return make_uint4(bf16x2_to_half2(v.x), bf16x2_to_half2(v.y), bf16x2_to_half2(v.z), bf16x2_to_half2(v.w)); }
__device__ __forceinline__ bool wants(const RowSinkBf16& d, uint32_t p0) { return d.row(p0) != nullptr; }
__device__ __forceinline__ void put16(const RowSinkBf16& d, uint32_t p0, uint4 v)
{
    uint8_t* r = d.row(p0);
    if (r) st16(r + 2ull * (p0 & 1023u), half8_to_bf16(v));
}
// The per-channel K factor of a paged-cache transfer (k_read_slots_ex / k_compress_slots_ex on a SlotKmulArgs): an element that
// crosses between a cache row and the pool side is multiplied by the fp16 factor of its channel.  The product is taken in fp32,
// where it is exact (11 x 11 or 8 x 11 significand bits), and rounded ONCE, to nearest even, to the destination's element type --
// the three forms below: fp16 x factor -> fp16 (what torch's half multiply gives), fp16 x factor -> bf16, bf16 x factor -> fp16.
__device__ __forceinline__ uint32_t mul_half2(uint32_t w, uint32_t m)
{
    return pack_half2(half_bits_to_float(w & 0xFFFFu) * half_bits_to_float(m & 0xFFFFu), half_bits_to_float(w >> 16) * half_bits_to_float(m >> 16));
}
__device__ __forceinline__ uint32_t mul_half2_to_bf16x2(uint32_t w, uint32_t m)
{
    return pack_bf16x2(half_bits_to_float(w & 0xFFFFu) * half_bits_to_float(m & 0xFFFFu), half_bits_to_float(w >> 16) * half_bits_to_float(m >> 16));
}
__device__ __forceinline__ uint32_t mul_bf16x2_to_half2(uint32_t w, uint32_t m)
{
    return pack_half2(__uint_as_float(w << 16) * half_bits_to_float(m & 0xFFFFu), __uint_as_float(w & 0xFFFF0000u) * half_bits_to_float(m >> 16));
}
__device__ __forceinline__ uint4 mul_half8(uint4 v, uint4 m) { return make_uint4(mul_half2(v.x, m.x), mul_half2(v.y, m.y), mul_half2(v.z, m.z), mul_half2(v.w, m.w)); }
__device__ __forceinline__ uint4 mul_half8_to_bf16(uint4 v, uint4 m)
{
    return make_uint4(mul_half2_to_bf16x2(v.x, m.x), mul_half2_to_bf16x2(v.y, m.y), mul_half2_to_bf16x2(v.z, m.z), mul_half2_to_bf16x2(v.w, m.w));
}
__device__ __forceinline__ uint4 mul_bf16_to_half8(uint4 v, uint4 m)
{
    return make_uint4(mul_bf16x2_to_half2(v.x, m.x), mul_bf16x2_to_half2(v.y, m.y), mul_bf16x2_to_half2(v.z, m.z), mul_bf16x2_to_half2(v.w, m.w));
}
// RowSink / RowSinkBf16 with that factor: `mul` is the [heads][128] fp16 factor row of the block's layer, shared by the two
// position rows (element p of the block takes factor element p & 1023).  A decoder still hands over the fp16 bits that
// speckv_ext_fetch_range writes; the sink multiplies THOSE -- the lane's 16 bytes of factors lie at its chunk's own offset, one more
// 16-byte load per store.
struct RowSinkMul {
    uint8_t* even;
    uint8_t* odd;
    const uint8_t* mul;
    __device__ __forceinline__ uint8_t* row(uint32_t p) const { return p < 1024u ? even : odd; }
};
struct RowSinkBf16Mul {
    uint8_t* even;
    uint8_t* odd;
    const uint8_t* mul;
    __device__ __forceinline__ uint8_t* row(uint32_t p) const { return p < 1024u ? even : odd; }
};
template <> struct is_row_sink<RowSinkMul> { static constexpr bool value = true; };
template <> struct is_row_sink<RowSinkBf16Mul> { static constexpr bool value = true; };
__device__ __forceinline__ bool wants(const RowSinkMul& d, uint32_t p0) { return d.row(p0) != nullptr; }
__device__ __forceinline__ bool wants(const RowSinkBf16Mul& d, uint32_t p0) { return d.row(p0) != nullptr; }
__device__ __forceinline__ void put16(const RowSinkMul& d, uint32_t p0, uint4 v)
{
    uint8_t* r = d.row(p0);
    if (r) st16(r + 2ull * (p0 & 1023u), mul_half8(v, ld16(d.mul + 2ull * (p0 & 1023u))));
}
__device__ __forceinline__ void put16(const RowSinkBf16Mul& d, uint32_t p0, uint4 v)
{
    uint8_t* r = d.row(p0);
    if (r) st16(r + 2ull * (p0 & 1023u), mul_half8_to_bf16(v, ld16(d.mul + 2ull * (p0 & 1023u))));
}
// The contiguous image of a fetch whose LAUNCH chooses how its stores are marked (k_fetch_decompress, the plain forms: CodecArgs::
// keep_stores).  Non-temporal stores are the faster ones for an image nobody touches again before it has left the Infinity Cache; a
// range that is fetched again at once, walked the other way (fetch_sweep.hpp), overwrites the lines its previous sweep wrote last
// while they are still on die -- if they were allocated there, which plain stores do and non-temporal ones do not (profiles/
// sweep_direction.txt).  keep is wave-uniform (a kernel argument): a scalar branch per store instruction, both forms in one kernel.
struct ImageSink {
    uint8_t* p;
    uint32_t keep;
};
template <> struct is_row_sink<ImageSink> { static constexpr bool value = true; };      // (stores through put16)
__device__ __forceinline__ bool wants(const ImageSink&, uint32_t) { return true; }
__device__ __forceinline__ void st16(const ImageSink& d, uint8_t* p, uint4 v)
{
    if (d.keep) *(g_u32x4*)(reinterpret_cast<uintptr_t>(p)) = u32x4{v.x, v.y, v.z, v.w};
    else st16(p, v);
}
__device__ __forceinline__ void put16(const ImageSink& d, uint32_t p0, uint4 v) { st16(d, d.p + 2ull * p0, v); }
__device__ __forceinline__ void store8_f32(const ImageSink& d, uint32_t p0, const float (&y)[8])       // store8_f32 above, the policy per store
{
    __shared__ __attribute__((aligned(16))) uint4 stage[kWaves][128];
    const uint32_t lane = threadIdx.x & 63u;
    uint4* st = stage[(threadIdx.x >> 6) % kWaves];
    wave_lds_fence();
    st[2u * lane] = make_uint4(__float_as_uint(y[0]), __float_as_uint(y[1]), __float_as_uint(y[2]), __float_as_uint(y[3]));
    st[2u * lane + 1u] = make_uint4(__float_as_uint(y[4]), __float_as_uint(y[5]), __float_as_uint(y[6]), __float_as_uint(y[7]));
    wave_lds_fence();
    const uint4 a = st[lane], b = st[64u + lane];
    uint8_t* base = d.p + 4ull * (p0 - 8u * lane) + 16u * lane;
    st16(d, base, a);
    st16(d, base + 1024, b);
}
template <bool F32, class DST>
__device__ __forceinline__ void store8(const DST& dst, uint32_t p0, const float (&y)[8])
{
    if constexpr (F32) {
        store8_f32(dst, p0, y);
    } else if constexpr (!is_row_sink<DST>::value) {                   // (the address in front of the conversions, as it always stood)
        st16(dst + 2ull * p0, make_uint4(pack_half2(y[0], y[1]), pack_half2(y[2], y[3]),
                                         pack_half2(y[4], y[5]), pack_half2(y[6], y[7])));
    } else {
        put16(dst, p0, make_uint4(pack_half2(y[0], y[1]), pack_half2(y[2], y[3]),
                                  pack_half2(y[4], y[5]), pack_half2(y[6], y[7])));
    }
}

// ===================================================================
// decode: INT8_DELTA_RLE  (cache_engine.cpp:241-284)
// ===================================================================
// float(q)/127.0f without a divide, 2 ops: fma(q, hi, q*lo) with hi = fl(1/127),
// lo = fl(1/127 - hi) is correctly rounded for every int8 q (exhaustive check in
// tests/test_cabi_boundary.py::test_div127_identity).
template <int MODE>
__device__ __forceinline__ float dequant_q8(uint32_t q8, float scale)
{
    const float fq = static_cast<float>(static_cast<int>(static_cast<int8_t>(q8 & 0xFFu)));
    if (MODE == kRefExact) {
        const float hi = 0x1.020408p-7f, lo = 0x1.020408p-35f;
        const float r = __builtin_fmaf(fq, hi, fq * lo);
        return r * scale;                                  // cache_engine.cpp:279-280
    }
    return fq * scale;
}

// ---- sub-dword VALU forms (SDWA): one instruction extracts a byte AND uses it ----
// (pure register ops, no memory, no hazards beyond what the hardware interlocks)
#define SPECKV_SDWA2(NAME, OP, S0, S1)                                                          \
    __device__ __forceinline__ uint32_t NAME(uint32_t a, uint32_t b)                            \
    {                                                                                           \
        uint32_t r;                                                                             \
        asm(OP " %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:" S0 " src1_sel:" S1   \
            : "=v"(r) : "v"(a), "v"(b));                                                        \
        return r;                                                                               \
    }
SPECKV_SDWA2(add_b0, "v_add_u32_sdwa", "DWORD", "BYTE_0")
SPECKV_SDWA2(add_b1, "v_add_u32_sdwa", "DWORD", "BYTE_1")
SPECKV_SDWA2(add_b2, "v_add_u32_sdwa", "DWORD", "BYTE_2")
SPECKV_SDWA2(add_b3, "v_add_u32_sdwa", "DWORD", "BYTE_3")
SPECKV_SDWA2(min_b1, "v_min_u32_sdwa", "DWORD", "BYTE_1")
SPECKV_SDWA2(min_b3, "v_min_u32_sdwa", "DWORD", "BYTE_3")
SPECKV_SDWA2(sub_b0_b2, "v_sub_u32_sdwa", "BYTE_0", "BYTE_2")   // a.b0 - b.b2
SPECKV_SDWA2(sub_b2_b0, "v_sub_u32_sdwa", "BYTE_2", "BYTE_0")   // a.b2 - b.b0
#undef SPECKV_SDWA2
template <int K> __device__ __forceinline__ uint32_t add_byte(uint32_t a, uint32_t lo, uint32_t hi)
{
    return K == 0 ? add_b0(a, lo) : K == 1 ? add_b1(a, lo) : K == 2 ? add_b2(a, lo) : K == 3 ? add_b3(a, lo)
         : K == 4 ? add_b0(a, hi) : K == 5 ? add_b1(a, hi) : K == 6 ? add_b2(a, hi) : add_b3(a, hi);
}
__device__ __forceinline__ void lds_store_b8(uint32_t addr, uint32_t v)
{
    *reinterpret_cast<lds_u8*>(static_cast<uintptr_t>(addr)) = static_cast<uint8_t>(v);
}

// ---- fast path: well-formed block (every count >= 1, counts sum to 2048) ----
// The decoded int8 sequence is the SECOND-order prefix sum (mod 256) of
//   E[start_r] = value_r - value_{r-1},  0 elsewhere,
// because the expanded deltas are piecewise constant (first prefix sum of E)
// and q is their running sum (second prefix sum).  So each run scatters ONE
// byte into a 2 KiB table at its start position, and every lane then walks its
// 8 table bytes with two adds per element; lane carries come from two DPP
// add-scans per 512-element chunk (v_sad_u8 / v_dot4_u32_u8 give the lane totals).
// Per pair the VALU work is three SDWA instructions: next address, E, min count.
//
// One 512-pair chunk of the pair phase.  A pair dword is  v0 | c0<<8 | v1<<16 | c1<<24.
// Returns false when the running count passes 2048 (caller falls back).
template <bool FULL, bool CHECK>
__device__ __forceinline__ bool rle_pair_chunk(const uint4 wv, uint32_t pair0, uint32_t npairs,
                                               uint32_t tab_addr, uint32_t& ccarry, uint32_t& wtail,
                                               uint32_t& mn)
{
    uint32_t w[4] = {wv.x, wv.y, wv.z, wv.w};
    uint32_t wm[4] = {wv.x, wv.y, wv.z, wv.w};              // count bytes as seen by the zero-count test
    if (!FULL) {
        // pairs at or beyond npairs are not pairs: count 0 for addressing, 0xFF for the min test
        const int nv = static_cast<int>(npairs) - static_cast<int>(pair0);     // valid pairs of this lane
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const uint32_t keep = 0x00FF00FFu | (nv > 2 * t ? 0x0000FF00u : 0u) | (nv > 2 * t + 1 ? 0xFF000000u : 0u);
            w[t] &= keep;
            wm[t] |= ~keep;
        }
    }
    // lane total of the 8 counts (bytes 1 and 3 of each dword)
    uint32_t run = __builtin_amdgcn_udot4(w[0], 0x01000100u, 0u, false);
    run = __builtin_amdgcn_udot4(w[1], 0x01000100u, run, false);
    run = __builtin_amdgcn_udot4(w[2], 0x01000100u, run, false);
    run = __builtin_amdgcn_udot4(w[3], 0x01000100u, run, false);
    const uint32_t incl = wave_incl_add(run);
    const uint32_t base = ccarry + incl - run;              // start position of this lane's first pair
    ccarry += lane63(incl);
    if (ccarry > kBlockElems) return false;                 // wave-uniform; nothing of this chunk is scattered
    // every start below is <= 2048; 2048 itself is a dummy byte behind the table
    const uint32_t prevw = wave_shr1(w[3], wtail);          // previous pair's dword (value in byte 2)
    wtail = lane63(w[3]);
    uint32_t a = tab_addr + base;
    lds_store_b8(a, sub_b0_b2(w[0], prevw)); a = add_b1(a, w[0]);
    lds_store_b8(a, sub_b2_b0(w[0], w[0]));  a = add_b3(a, w[0]);
    lds_store_b8(a, sub_b0_b2(w[1], w[0]));  a = add_b1(a, w[1]);
    lds_store_b8(a, sub_b2_b0(w[1], w[1]));  a = add_b3(a, w[1]);
    lds_store_b8(a, sub_b0_b2(w[2], w[1]));  a = add_b1(a, w[2]);
    lds_store_b8(a, sub_b2_b0(w[2], w[2]));  a = add_b3(a, w[2]);
    lds_store_b8(a, sub_b0_b2(w[3], w[2]));  a = add_b1(a, w[3]);
    lds_store_b8(a, sub_b2_b0(w[3], w[3]));
    if (CHECK) {
#pragma unroll
        for (int t = 0; t < 4; ++t) { mn = min_b1(mn, wm[t]); mn = min_b3(mn, wm[t]); }
    }
    return true;
}

// Returns false (nothing stored) when the block is not well-formed.
// `trusted` (wave-uniform): the stream comes from k_compress -- no zero counts, and the
// bytes between len and the next 16-byte boundary are zero pairs, which scatter into
// the dummy byte; every chunk then takes the unmasked, unchecked form.
// FLAT (the kernel of its own that launches hinted "structured" run, k_fetch_decompress_flat: CodecArgs::structured_hint; the
// kernels the headline fetch runs are instantiated without it): blocks that are piecewise constant on 8-element boundaries
// skip the scans, recurrences and conversions of the general loop -- see the whole-block path in front of it.
template <int MODE, bool F32, bool FLAT = false, class DST = uint8_t*>
__device__ __forceinline__ bool decode_rle_fast(const uint8_t* __restrict__ rec, uint32_t len,
                                                float scale, typename dst_arg<DST>::type dst,
                                                uint8_t* tab, uint32_t lane, bool trusted)
{
    const uint32_t npairs = len >> 1;                       // odd trailing byte dropped
    uint4 w[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t pair0 = 512u * j + 8u * lane;
        w[j] = make_uint4(0u, 0u, 0u, 0u);
        if (pair0 < npairs) w[j] = ld16(rec + 2ull * pair0);
    }
    // A stream whose value bytes are all zero (a block of zeros, a never-written page: len 0) decodes to +0 whatever its
    // counts are -- 0/127 * scale with a finite scale of positive sign -- and needs neither table nor scans: plain vector stores.
    // (Otherwise such blocks take the full constant-work path below, or, with len 0, the element-wise general path.)
    {
        uint32_t anyv = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) anyv |= (w[j].x | w[j].y | w[j].z | w[j].w) & 0x00FF00FFu;
        if (__builtin_amdgcn_ballot_w64(anyv != 0u) == 0ull && __float_as_uint(scale) < 0x7F800000u) {    // sign clear (not -0 either), finite
            const float z[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int j = 0; j < 4; ++j) store8<F32>(dst, 512u * j + 8u * lane, z);
            return true;
        }
    }
    // clear the byte table (2 KiB); byte 2048 is a write-only dummy
    uint4* t4 = reinterpret_cast<uint4*>(tab);
    t4[lane] = make_uint4(0u, 0u, 0u, 0u);
    t4[64 + lane] = make_uint4(0u, 0u, 0u, 0u);
    const uint32_t tab_addr = static_cast<uint32_t>(reinterpret_cast<uintptr_t>((lds_u8*)tab));

    uint32_t ccarry = 0;        // running count total
    uint32_t wtail = 0;         // last pair dword of the previous chunk (value 0 before the first run)
    uint32_t mn = 255u;         // min count over valid pairs
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (512u * j >= npairs) break;                      // wave-uniform
        const uint32_t pair0 = 512u * j + 8u * lane;
        bool go;
        if (trusted)                       go = rle_pair_chunk<true, false>(w[j], pair0, npairs, tab_addr, ccarry, wtail, mn);
        else if (512u * (j + 1) <= npairs) go = rle_pair_chunk<true, true>(w[j], pair0, npairs, tab_addr, ccarry, wtail, mn);
        else                               go = rle_pair_chunk<false, true>(w[j], pair0, npairs, tab_addr, ccarry, wtail, mn);
        if (!go) return false;
    }
    const bool ok = (ccarry == kBlockElems) && (__ballot(mn == 0u) == 0ull);
    if (!ok) return false;
    wave_lds_fence();

    if (FLAT && npairs <= 256u) {                            // (wave-uniform)
        // The whole block piecewise constant on 8-element boundaries: every lane's table bytes are (+d, -d, 0 x 6) in all four
        // chunks.  Then no slope enters any lane (each lane's bytes sum to 0), a lane's eight elements are ONE value, and that
        // value is the inclusive prefix sum of the +d bytes: one packed scan per two chunks (fields of 16 bits: 64 x 255 fits),
        // one conversion and plain 16-byte stores per chunk -- instead of two scans, eight recurrences and eight conversions.
        // A block that breaks the pattern in any lane takes the general loop below.
        uint2 xs[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) xs[j] = *reinterpret_cast<const uint2*>(tab + 512u * j + 8u * lane);
        uint32_t bad = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) bad |= (xs[j].x & 0xFFFF0000u) | xs[j].y | ((xs[j].x + (xs[j].x >> 8)) & 0xFFu);
        if (__builtin_amdgcn_ballot_w64(bad != 0u) == 0ull) {
            const uint32_t ia = wave_incl_add(__builtin_amdgcn_perm(xs[1].x, xs[0].x, 0x0C040C00u));     // chunk 0 | chunk 1 << 16
            const uint32_t ib = wave_incl_add(__builtin_amdgcn_perm(xs[3].x, xs[2].x, 0x0C040C00u));     // chunk 2 | chunk 3 << 16
            const uint32_t ta = lane63(ia), tb = lane63(ib);
            const uint32_t carry1 = ta & 0xFFFFu, carry2 = carry1 + (ta >> 16), carry3 = carry2 + (tb & 0xFFFFu);
            const uint32_t qv[4] = {ia, (ia >> 16) + carry1, ib + carry2, (ib >> 16) + carry3};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float v = dequant<MODE>(static_cast<int>(static_cast<int8_t>(qv[j] & 0xFFu)), scale);
                const float y8[8] = {v, v, v, v, v, v, v, v};
                store8<F32>(dst, 512u * j + 8u * lane, y8);
            }
            wave_lds_fence();
            return true;
        }
    }
    uint32_t c1 = 0, c2 = 0;    // S1 / S2 at the end of the previous chunk
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t p0 = 512u * j + 8u * lane;
        const uint2 x = *reinterpret_cast<const uint2*>(tab + p0);
        const uint32_t t1 = __builtin_amdgcn_sad_u8(x.x, 0u, __builtin_amdgcn_sad_u8(x.y, 0u, 0u));
        const uint32_t t2 = __builtin_amdgcn_udot4(x.x, 0x05060708u,
                                                   __builtin_amdgcn_udot4(x.y, 0x01020304u, 0u, false), false);
        const uint32_t i1 = wave_incl_add(t1);
        const uint32_t x1 = c1 + i1 - t1;                   // S1 entering this lane
        const uint32_t u = t2 + 8u * x1;                    // this lane's S2 increment
        const uint32_t i2 = wave_incl_add(u);
        const uint32_t x2 = c2 + i2 - u;                    // S2 entering this lane
        c1 += lane63(i1);
        c2 += lane63(i2);
        uint32_t s1 = x1, s2 = x2;
        uint32_t q[8];
        s1 = add_byte<0>(s1, x.x, x.y); s2 += s1; q[0] = s2;
        s1 = add_byte<1>(s1, x.x, x.y); s2 += s1; q[1] = s2;
        s1 = add_byte<2>(s1, x.x, x.y); s2 += s1; q[2] = s2;
        s1 = add_byte<3>(s1, x.x, x.y); s2 += s1; q[3] = s2;
        s1 = add_byte<4>(s1, x.x, x.y); s2 += s1; q[4] = s2;
        s1 = add_byte<5>(s1, x.x, x.y); s2 += s1; q[5] = s2;
        s1 = add_byte<6>(s1, x.x, x.y); s2 += s1; q[6] = s2;
        s1 = add_byte<7>(s1, x.x, x.y); s2 += s1; q[7] = s2;
        float y[8];
#pragma unroll
        for (int k = 0; k < 8; k += 2) {
            f32x2 fq;
            fq.x = static_cast<float>(static_cast<int>(static_cast<int8_t>(q[k] & 0xFFu)));
            fq.y = static_cast<float>(static_cast<int>(static_cast<int8_t>(q[k + 1] & 0xFFu)));
            f32x2 r;
            if (MODE == kRefExact) {
                const f32x2 hi = {0x1.020408p-7f, 0x1.020408p-7f}, lo = {0x1.020408p-35f, 0x1.020408p-35f};
                r = __builtin_elementwise_fma(fq, hi, fq * lo);        // float(q)/127.0f, correctly rounded
            } else {
                r = fq;
            }
            const f32x2 sc = {scale, scale};
            r = r * sc;
            y[k] = r.x;
            y[k + 1] = r.y;
        }
        store8<F32>(dst, p0, y);
    }
    wave_lds_fence();
    return true;
}

// ---- general path: any byte stream (zero counts, short or overlong streams) ----
// Rare, so it is written for size, not speed, and needs no LDS at all: one pair
// per lane per step; an add-scan of (value*count mod 256)<<24 | count gives each
// run its start position and the int8 prefix of all earlier deltas, and the lane
// then writes the run's elements itself:  q[start+m] = prefix + (m+1)*value (mod 256).
// Zero counts emit nothing, an odd trailing byte is dropped, output is clipped at
// the block and zero-filled behind the last run (cache_engine.cpp:241-284).
template <bool F32>
__device__ __forceinline__ void store_elem(uint8_t* dst, uint32_t p, float y)
{
    if (F32) {
        gstore<float>(dst + 4ull * p, y);
    } else {
        float a = y, z = 0.0f;
        gstore<uint16_t>(dst + 2ull * p, static_cast<uint16_t>(pack_half2(a, z) & 0xFFFFu));
    }
}
template <bool F32>
__device__ __forceinline__ void store_elem(const RowSink& d, uint32_t p, float y)
{
    static_assert(!F32, "position rows are fp16");
    uint8_t* r = d.row(p);
    if (r) store_elem<false>(r, p & 1023u, y);
}
template <bool F32>
__device__ __forceinline__ void store_elem(const RowSinkBf16& d, uint32_t p, float y)
{
    static_assert(!F32, "position rows are 16-bit");
    uint8_t* r = d.row(p);
    float a = y, z = 0.0f;
    if (r) gstore<uint16_t>(r + 2ull * (p & 1023u), static_cast<uint16_t>(half2_to_bf16x2(pack_half2(a, z) & 0xFFFFu) & 0xFFFFu));
}
template <bool F32>
__device__ __forceinline__ void store_elem(const RowSinkMul& d, uint32_t p, float y)
{
    static_assert(!F32, "position rows are fp16");
    uint8_t* r = d.row(p);
    float a = y, z = 0.0f;
    if (r) gstore<uint16_t>(r + 2ull * (p & 1023u), static_cast<uint16_t>(mul_half2(pack_half2(a, z) & 0xFFFFu, gload<uint16_t>(d.mul + 2ull * (p & 1023u))) & 0xFFFFu));
}
template <bool F32>
__device__ __forceinline__ void store_elem(const RowSinkBf16Mul& d, uint32_t p, float y)
{
    static_assert(!F32, "position rows are 16-bit");
    uint8_t* r = d.row(p);
    float a = y, z = 0.0f;
    if (r) gstore<uint16_t>(r + 2ull * (p & 1023u), static_cast<uint16_t>(mul_half2_to_bf16x2(pack_half2(a, z) & 0xFFFFu, gload<uint16_t>(d.mul + 2ull * (p & 1023u))) & 0xFFFFu));
}
template <int MODE, bool F32, class DST>
__device__ __forceinline__ void decode_rle_general_to(const uint8_t* __restrict__ rec, uint32_t len,
                                                      float scale, typename dst_arg<DST>::type dst, uint32_t lane)
{
    const uint32_t npairs = len >> 1;
    uint32_t carry = 0;                                     // (sum v*c mod 256)<<24 | sum c
#pragma unroll 1
    for (uint32_t b = 0; b < npairs; b += 64u) {
        const uint32_t i = b + lane;
        uint32_t bits = 0;
        if (i < npairs) bits = gload<uint16_t>(rec + 2ull * i);
        const uint32_t v = bits & 0xFFu, c = bits >> 8;
        const uint32_t packed = ((v * c) << 24) | c;
        const uint32_t incl = wave_incl_add(packed);
        const uint32_t e = carry + incl - packed;
        carry += lane63(incl);
        const uint32_t start = e & 0xFFFFFFu;
        uint32_t q = e >> 24;
#pragma unroll 1
        for (uint32_t m = 0; m < c; ++m) {
            const uint32_t p = start + m;
            if (p >= kBlockElems) break;
            q += v;
            store_elem<F32>(dst, p, dequant_q8<MODE>(q, scale));
        }
        if ((carry & 0xFFFFFFu) >= kBlockElems) break;      // wave-uniform: the block is full
    }
    const uint32_t total = carry & 0xFFFFFFu;
#pragma unroll 1
    for (uint32_t p = total + lane; p < kBlockElems; p += 64u) store_elem<F32>(dst, p, 0.0f);
}
// (out of line for the block images: one copy per quantiser mode and output width, called from every fetch kernel; a RowSink
// caller takes the body above inline, so that no further function comes to lie between these and the kernels that call them)
template <int MODE, bool F32>
__device__ __noinline__ void decode_rle_general(const uint8_t* __restrict__ rec, uint32_t len,
                                                float scale, uint8_t* __restrict__ dst, uint32_t lane)
{
    decode_rle_general_to<MODE, F32, uint8_t*>(rec, len, scale, dst, lane);
}

// decode: INT8 (quantise only)
template <int MODE, bool F32, class DST = uint8_t*>
__device__ __forceinline__ void decode_int8(const uint8_t* __restrict__ rec, uint32_t len,
                                            float scale, typename dst_arg<DST>::type dst, uint32_t lane)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t p0 = 512u * j + 8u * lane;
        if (!wants(dst, p0)) continue;
        uint2 w = make_uint2(0u, 0u);
        if (p0 < len) w = gload_u2(rec + p0);
        float y[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t b = ((k < 4 ? w.x : w.y) >> ((k & 3) * 8)) & 0xFFu;
            const int q = static_cast<int>(static_cast<int8_t>(b));
            y[k] = (p0 + k < len) ? dequant<MODE>(q, scale) : 0.0f;
        }
        store8<F32>(dst, p0, y);
    }
}

// decode: FP16 (raw copy, optional widening)
template <bool F32, class DST = uint8_t*>
__device__ __forceinline__ void decode_fp16(const uint8_t* __restrict__ rec, uint32_t len,
                                            typename dst_arg<DST>::type dst, uint32_t lane)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t p0 = 512u * j + 8u * lane;
        if (!wants(dst, p0)) continue;
        uint4 w = make_uint4(0u, 0u, 0u, 0u);
        if (2u * p0 < len) w = ld16(rec + 2ull * p0);
        if constexpr (!F32) {
            // mask a ragged tail at element granularity
            const uint32_t words[4] = {w.x, w.y, w.z, w.w};
            uint32_t o[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                uint32_t lo = (2u * (p0 + 2 * t) + 1u < len) ? (words[t] & 0xFFFFu) : 0u;
                uint32_t hi = (2u * (p0 + 2 * t + 1) + 1u < len) ? (words[t] & 0xFFFF0000u) : 0u;
                o[t] = lo | hi;
            }
            if constexpr (!is_row_sink<DST>::value) st16(dst + 2ull * p0, make_uint4(o[0], o[1], o[2], o[3]));
            else put16(dst, p0, make_uint4(o[0], o[1], o[2], o[3]));
        } else {
            const uint32_t words[4] = {w.x, w.y, w.z, w.w};
            float y[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t h = (words[k >> 1] >> ((k & 1) * 16)) & 0xFFFFu;
                y[k] = (2u * (p0 + k) + 1u < len) ? half_bits_to_float(h) : 0.0f;
            }
            store8<true>(dst, p0, y);
        }
    }
}

// decode: INT4_G32 (config 5 extension; record = 64 fp16 scales + 1024 B nibbles)
template <bool F32, class DST = uint8_t*>
__device__ __forceinline__ void decode_int4(const uint8_t* __restrict__ rec, uint32_t len,
                                            typename dst_arg<DST>::type dst, uint32_t lane)
{
    const bool ok = len >= kInt4RecBytes;                    // short record decodes to zeros
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t p0 = 512u * j + 8u * lane;
        if (!wants(dst, p0)) continue;                       // (a row's 32 group scales are words 32 (p0 >> 10) .. + 31: only they are read)
        uint32_t nib = 0;
        float s = 0.0f;
        if (ok) {
            nib = gload<uint32_t>(rec + 128u + (p0 >> 1));
            s = half_bits_to_float(gload<uint16_t>(rec + 2u * (p0 >> 5)));
        }
        float y[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const int q = (static_cast<int>(nib << (28 - 4 * k))) >> 28;       // sign-extended nibble
            y[k] = ok ? static_cast<float>(q) * s : 0.0f;
        }
        store8<F32>(dst, p0, y);
    }
}

// decode: MXFP4 (OCP MX v1.0 elements and scales; record = 1024 nibble bytes + 64 E8M0 codes; oracle: compress_mxfp4 / ORC_COMP_MXFP4)
// The two halves of the block are interleaved element by element: byte i = element i (low nibble) and element 1024 + i (high),
// code j scales bytes 16j .. 16j+15.  y = e2m1(nibble) * 2^(code - 127): the nibble pairs widen through
// v_cvt_scalef32_pk_f32_fp4 (exact), the scale is a float whose exponent field is the code (a subnormal for code 0, NaN for
// 255) -- the product is exact in fp32.  A lane takes bytes 8l .. 8l+7 of both 512-byte halves of the nibble area: elements
// [512 j + 8 l, + 8) for j = 0, 1 and their partners 1024 further on (j = 2, 3 of every other decoder's lane map).
typedef float f32x2v __attribute__((ext_vector_type(2)));
// (A byte carries both positions, so a RowSink that wants one of them still reads all 1024 nibble bytes and the 64 codes, and the
// conversion widens both nibbles of a byte at once: both planes are computed, only the store of the plane nobody wants is left out.)
template <bool F32, class DST = uint8_t*>
__device__ __forceinline__ void decode_mx4(const uint8_t* __restrict__ rec, const uint8_t* __restrict__ codes, uint32_t len,
                                           typename dst_arg<DST>::type dst, uint32_t lane)
{
    const bool ok = len >= kMx4RecBytes;                     // short record decodes to zeros
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const uint32_t p0 = 512u * j + 8u * lane;
        uint2 nib = make_uint2(0u, 0u);
        uint32_t code = 127u;
        if (ok) {
            nib = gload_u2(rec + p0);
            code = gload<uint8_t>(codes + (p0 >> 4));
        }
        const float s = __uint_as_float(code == 0u ? 0x00400000u : code == 255u ? 0x7FC00000u : code << 23);
        float y0[8], y1[8];
#define MX_DEC(K, W, SEL) { const f32x2v f = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(W, 1.0f, SEL); y0[K] = f.x * s; y1[K] = f.y * s; }
        MX_DEC(0, nib.x, 0) MX_DEC(1, nib.x, 1) MX_DEC(2, nib.x, 2) MX_DEC(3, nib.x, 3)
        MX_DEC(4, nib.y, 0) MX_DEC(5, nib.y, 1) MX_DEC(6, nib.y, 2) MX_DEC(7, nib.y, 3)
#undef MX_DEC
        store8<F32>(dst, p0, y0);
        store8<F32>(dst, p0 + 1024u, y1);
    }
}

// decode: FP8_E4M3 (config 5 extension; per-block scale)
template <bool F32, class DST = uint8_t*>
__device__ __forceinline__ void decode_fp8(const uint8_t* __restrict__ rec, uint32_t len,
                                           float scale, typename dst_arg<DST>::type dst, uint32_t lane)
{
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t p0 = 512u * j + 8u * lane;
        if (!wants(dst, p0)) continue;
        uint2 w = make_uint2(0u, 0u);
        if (p0 < len) w = gload_u2(rec + p0);
        float y[8];
        y[0] = __builtin_amdgcn_cvt_f32_fp8(static_cast<int>(w.x), 0);
        y[1] = __builtin_amdgcn_cvt_f32_fp8(static_cast<int>(w.x), 1);
        y[2] = __builtin_amdgcn_cvt_f32_fp8(static_cast<int>(w.x), 2);
        y[3] = __builtin_amdgcn_cvt_f32_fp8(static_cast<int>(w.x), 3);
        y[4] = __builtin_amdgcn_cvt_f32_fp8(static_cast<int>(w.y), 0);
        y[5] = __builtin_amdgcn_cvt_f32_fp8(static_cast<int>(w.y), 1);
        y[6] = __builtin_amdgcn_cvt_f32_fp8(static_cast<int>(w.y), 2);
        y[7] = __builtin_amdgcn_cvt_f32_fp8(static_cast<int>(w.y), 3);
#pragma unroll
        for (int k = 0; k < 8; ++k) y[k] = (p0 + k < len) ? y[k] * scale : 0.0f;
        store8<F32>(dst, p0, y);
    }
}

// ===================================================================
// RLE encode of the delta stream (cache_engine.cpp:198-239)
// ===================================================================
// Wave LDS layout (bytes): [0,16) lead (the count byte "before the first pair" lands here), [16, 16+4096) pair
// buffer.  Both paths scatter, per RUN START at position p, the value byte of its own pair and the count byte of the
// PREVIOUS pair (p - previous start); the last pair is closed after the loop.  No read-back from LDS.
// (kEncPairOff / kEncFail, quantize8 and the SDWA / EXEC-predicated helpers of this path: encode_device.hpp, shared with
// tensor_compress.hip)

// Fast path: no stretch of equal deltas reaches 255 elements, so every change of the delta starts a run and no run
// has to be split (count < 255 rule).  Returns the number of runs, or kEncFail when a long stretch may exist (>= 14
// lanes of a chunk without any run start: a 255-stretch needs 30 such lanes in two chunks) -- the caller then runs
// the SPLIT form, which starts over.  The block must be finite (quantize8).
// SPLIT (round 4; its own instantiation, the plain one is untouched): stretches of any length.  A run also starts at every
// 255th element of a stretch (cache_engine.cpp:224).  A lane holds 8 consecutive elements, so at most one such element falls
// into the part of the lane in front of its first change of the delta -- the part that belongs to the stretch ENTERING the lane,
// whose start is the last change in front of the lane (a second max-scan, over change positions only): if the entering
// stretch has offset o0 at the lane's element 0, the split start is element (255 - o0 % 255) % 255 when that is one of the
// lane's.  Everything behind that -- run indices, "count = distance to the previous start" -- is the plain path's, with the
// split start as one more start.  (Blocks of long runs took the element-wise path before: 745 us per 131 072 blocks, four
// times a block of noise, for the data that compresses 100 : 1.  profiles/r04_long_runs.txt)
template <int MODE, bool SPLIT = false>
__device__ __forceinline__ uint32_t encode_rle_fast(const uint4 (&raw)[4], float scale, float rcp, uint8_t* wl, uint32_t lane)
{
    const uint32_t pair_m1 = lds_addr_of(wl + kEncPairOff) - 1u;
    uint32_t qtail = 0, dtail = 0x100u, mcarry = 0, icarry = 0;  // dtail 0x100: no delta precedes element 0 (it starts a run)
    bool prev_sparse = false;                                    // mcarry: position+1 of the last run start
    uint32_t ccarry = 0;                                         // SPLIT: position+1 of the last CHANGE of the delta
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t p0 = 512u * j + 8u * lane;
        uint32_t q[8];
        quantize8<MODE>(raw[j], scale, rcp, q);
        const uint32_t prevq = wave_shr1(q[7], qtail);
        qtail = lane63(q[7]);
        uint32_t d[8];
        d[0] = sub_bytes(q[0], prevq);
#pragma unroll
        for (int k = 1; k < 8; ++k) d[k] = sub_bytes(q[k], q[k - 1]);
        const uint32_t prevd = wave_shr1(d[7], dtail);
        dtail = lane63(d[7]);
        bool st[8];                                              // element k starts a run (a v_cmp result: an SGPR pair)
        uint32_t mask = 0;                                       // bit 7-k = element k starts a run
        unsigned long long sm[8];                                // the same as lane masks
        st[0] = d[0] != prevd;
#pragma unroll
        for (int k = 1; k < 8; ++k) st[k] = d[k] != d[k - 1];
        if (SPLIT) {
            uint32_t cmask = 0;                                  // the changes alone
#pragma unroll
            for (int k = 0; k < 8; ++k) shift_in(cmask, __builtin_amdgcn_ballot_w64(st[k]));
            const uint32_t lmc = cmask ? p0 + 8u - static_cast<uint32_t>(__builtin_ctz(cmask)) : 0u;
            const uint32_t imc = wave_incl_max(lmc);
            const uint32_t mc = umax(wave_shr1(imc, 0u), ccarry);                // last change in front of the lane, position+1 (0: none)
            ccarry = umax(ccarry, lane63(imc));
            const uint32_t o0 = p0 + 1u - mc;                                    // offset of element 0 in the entering stretch (>= 1)
            const uint32_t r = o0 - 255u * ((o0 * 0x8081u) >> 23);                // o0 % 255 (exact below 4096)
            uint32_t ks = r ? 255u - r : 0u;                                      // the lane's element at a multiple of 255, if < 8
            const uint32_t kfirst = cmask ? static_cast<uint32_t>(__builtin_clz(cmask)) - 24u : 8u;     // the lane's first change
            if (mc == 0u || ks >= kfirst) ks = 8u;                               // (behind a change the offsets are < 8: never a split)
#pragma unroll
            for (int k = 0; k < 8; ++k) st[k] = st[k] || ks == static_cast<uint32_t>(k);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) { sm[k] = __builtin_amdgcn_ballot_w64(st[k]); shift_in(mask, sm[k]); }
        const uint32_t cnt = static_cast<uint32_t>(__builtin_popcount(mask));
        // last start of the lane, as position+1 (0 = none): element 7 - ctz(mask)
        const uint32_t lm = mask ? p0 + 8u - static_cast<uint32_t>(__builtin_ctz(mask)) : 0u;
        // cheap pre-filter: a run longer than 248 elements needs >= 28 start-free lanes in this chunk and the previous
        // one together, i.e. >= 14 in one of them
        const bool sparse = !SPLIT && __popcll(__ballot(mask == 0u)) >= 14;            // wave-uniform
        const bool suspicious = sparse || prev_sparse;
        prev_sparse = sparse;
        const uint32_t ic = wave_incl_add(cnt);
        uint32_t idx = icarry + ic - cnt;
        icarry += lane63(ic);
        const uint32_t im = wave_incl_max(lm);
        const uint32_t m = umax(wave_shr1(im, 0u), mcarry);      // last start before this lane, position+1
        mcarry = umax(mcarry, lane63(im));
        // A count is "position of this run start - previous run start"; only a lane's FIRST start of the chunk can
        // close a long run, and that run is shorter than (end of the lane's 8 elements - previous start).  If that
        // bound passes 255 anywhere the run may need splitting (cache_engine.cpp:224), which the SPLIT form does.
        // (wave-uniform: the SPLIT form starts over, nothing of this attempt is used)
        if (!SPLIT && suspicious) {
            if (__ballot(mask != 0u && p0 + 8u - m > 255u) != 0ull) return kEncFail;
            // ... or the run that is open at the end of the chunk is too long already (then its last 31 lanes hold no start: sparse)
            if (512u * static_cast<uint32_t>(j + 1) + 1u - mcarry > 255u) return kEncFail;
        }
        // rel = (last start, position+1) - (p0 + 1): count of the run closed by a start at element k is k - rel
        uint32_t rel = m - p0 - 1u;
        uint32_t addr[8], cntv[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            addr[k] = lshl1_add(idx, pair_m1);                   // count byte of the previous pair; +1 = value byte of this one
            cntv[k] = static_cast<uint32_t>(k) - rel;
            rel = st[k] ? static_cast<uint32_t>(k) : rel;
            add_pred(idx, sm[k]);
        }
#pragma unroll
        for (int k = 0; k < 8; ++k) store_pair_if(sm[k], addr[k], cntv[k], d[k]);
    }
    lds_store_b8(pair_m1 + 2u * icarry, kBlockElems + 1u - mcarry);         // close the last run
    return icarry;
}

// Where a block's 4096 source bytes lie.  SrcRun: one contiguous image.  SrcPair: two rows of 2048 bytes anywhere -- the even
// and the odd position of a position pair, gathered by the encoder itself (k_compress_pairs) instead of being copied into a
// page image first.  chunk(j, lane): this lane's j-th 16-byte load (elements [512 j + 8 lane, + 8)); elem(p): element p.  The
// half a load falls into is a compile-time (chunk) or wave-uniform (elem: the out-of-line paths step 64 elements at a time) choice.
struct SrcRun {
    const uint8_t* p;
    __device__ __forceinline__ const uint8_t* chunk(int j, uint32_t lane) const { return p + 2ull * (512u * j + 8u * lane); }
    __device__ __forceinline__ const uint8_t* elem(uint32_t e) const { return p + 2ull * e; }
};
struct SrcPair {
    const uint8_t* lo;
    const uint8_t* hi;
    __device__ __forceinline__ const uint8_t* chunk(int j, uint32_t lane) const { return (j < 2 ? lo : hi) + 2ull * (512u * (j & 1) + 8u * lane); }
    __device__ __forceinline__ const uint8_t* elem(uint32_t e) const { return e < 1024u ? lo + 2ull * e : hi + 2ull * (e - 1024u); }
};
// How the encoder reads a source: the fp16 bits of a lane's chunk (the fast paths) or of one element (the out-of-line paths).
template <class SRC> __device__ __forceinline__ uint4 src_ld16(const SRC& src, int j, uint32_t lane) { return enc_ld16(src.chunk(j, lane)); }
template <class SRC> __device__ __forceinline__ uint32_t src_half(const SRC& src, uint32_t e) { return gload<uint16_t>(src.elem(e)); }
// SrcPair whose rows each say what they hold (k_compress_slots_ex): fp16, or bf16 that becomes fp16 by bf16x2_to_half2's one
// rounding as it is loaded -- on both access paths, so a bf16 row with inf / NaN in it is encoded as row.to(fp16) would be.  A pair
// made of a held fp16 row and a row of a bf16 cache is mixed; the type of a row is the same for all lanes of the wave.
struct SrcPairMixed {
    const uint8_t* lo;
    const uint8_t* hi;
    bool lo_bf16, hi_bf16;
};
__device__ __forceinline__ uint4 src_ld16(const SrcPairMixed& src, int j, uint32_t lane)
{
    const uint4 v = enc_ld16((j < 2 ? src.lo : src.hi) + 2ull * (512u * (j & 1) + 8u * lane));
    return (j < 2 ? src.lo_bf16 : src.hi_bf16) ? bf16_to_half8(v) : v;
}
__device__ __forceinline__ uint32_t src_half(const SrcPairMixed& src, uint32_t e)
{
    const bool low = e < 1024u;
    const uint32_t b = gload<uint16_t>(low ? src.lo + 2ull * e : src.hi + 2ull * (e - 1024u));
    return (low ? src.lo_bf16 : src.hi_bf16) ? (bf16x2_to_half2(b) & 0xFFFFu) : b;
}
// SrcPairMixed whose rows also say whether they are scaled (the K waves of k_compress_slots_ex on a SlotKmulArgs): lo_mul / hi_mul
// = the [heads][128] fp16 factor row of the block's layer, or nullptr for a row that is pool-side already (a held-in row is
// neither bf16 nor scaled).  The encoder sees fp16_rne(float(x) * float(m)) of the cache element x, fp16 or bf16 -- one rounding,
// never bf16 -> fp16 -> scaled -- on both access paths; the lane's 16 bytes of factors lie at its chunk's own offset in the row.
struct SrcPairScaled {
    const uint8_t* lo;
    const uint8_t* hi;
    bool lo_bf16, hi_bf16;
    const uint8_t* lo_mul;
    const uint8_t* hi_mul;
};
__device__ __forceinline__ uint4 src_ld16(const SrcPairScaled& src, int j, uint32_t lane)
{
    const uint32_t off = 2u * (512u * (j & 1) + 8u * lane);
    const uint4 v = enc_ld16((j < 2 ? src.lo : src.hi) + off);
    const bool bf16 = j < 2 ? src.lo_bf16 : src.hi_bf16;
    const uint8_t* mul = j < 2 ? src.lo_mul : src.hi_mul;
    if (!mul) return bf16 ? bf16_to_half8(v) : v;
    const uint4 m = ld16(mul + off);
    return bf16 ? mul_bf16_to_half8(v, m) : mul_half8(v, m);
}
__device__ __forceinline__ uint32_t src_half(const SrcPairScaled& src, uint32_t e)
{
    const bool low = e < 1024u;
    const uint32_t r = low ? e : e - 1024u;
    const uint32_t b = gload<uint16_t>((low ? src.lo : src.hi) + 2ull * r);
    const bool bf16 = low ? src.lo_bf16 : src.hi_bf16;
    const uint8_t* mul = low ? src.lo_mul : src.hi_mul;
    if (!mul) return bf16 ? (bf16x2_to_half2(b) & 0xFFFFu) : b;
    const uint32_t m = gload<uint16_t>(mul + 2ull * r);
    return (bf16 ? mul_bf16x2_to_half2(b, m) : mul_half2(b, m)) & 0xFFFFu;
}

// General path (long stretches: zeros, constants; blocks with inf / NaN): one element per lane per step, rolled,
// quantised with the exact scalar form straight from the source; stretch starts by max-scan, a run starts every 255
// elements of a stretch.
template <int MODE, class SRC>
__device__ __forceinline__ uint32_t encode_rle_general_from(const SRC src, float scale, uint8_t* wl, uint32_t lane)
{
    const uint32_t pair_addr = lds_addr_of(wl + kEncPairOff);
    uint32_t qtail = 0, dtail = 0, scarry = 0, mcarry = 0, icarry = 0;
#pragma unroll 1
    for (uint32_t step = 0; step < kBlockElems / 64u; ++step) {
        const uint32_t p = 64u * step + lane;
        const uint32_t qv = quantize<MODE>(half_bits_to_float(src_half(src, p)), scale);
        const uint32_t prevq = wave_shr1(qv, qtail);
        qtail = lane63(qv);
        const uint32_t d = (qv - prevq) & 0xFFu;
        const uint32_t prevd = wave_shr1(d, dtail);
        dtail = lane63(d);
        const bool neq = (p == 0u) || (d != prevd);
        const uint32_t is = wave_incl_max(neq ? p + 1u : 0u);
        const uint32_t ss = umax(is, scarry);                      // stretch start, position+1
        scarry = umax(scarry, lane63(is));
        const bool isrun = ((p + 1u - ss) % 255u) == 0u;           // count < 255 rule (cache_engine.cpp:224)
        const uint32_t ic = wave_incl_add(isrun ? 1u : 0u);
        const uint32_t idx = icarry + ic - (isrun ? 1u : 0u);
        icarry += lane63(ic);
        const uint32_t im = wave_incl_max(isrun ? p + 1u : 0u);
        const uint32_t prev = umax(wave_shr1(im, 0u), mcarry);
        mcarry = umax(mcarry, lane63(im));
        if (isrun) {
            lds_store_b8(pair_addr + 2u * idx - 1u, p + 1u - prev);
            lds_store_b8(pair_addr + 2u * idx, d);
        }
    }
    lds_store_b8(pair_addr + 2u * icarry - 1u, kBlockElems + 1u - mcarry);
    return icarry;
}
// Out of line for a contiguous image.  The pair form takes the body inline: device functions are emitted in front of the
// kernels, and one more of them would move every kernel away from decode_rle_general (the note on emission order below).
template <int MODE>
__device__ __noinline__ uint32_t encode_rle_general(const uint8_t* __restrict__ src, float scale, uint8_t* wl, uint32_t lane)
{
    return encode_rle_general_from<MODE>(SrcRun{src}, scale, wl, lane);
}
template <int MODE>
__device__ __forceinline__ uint32_t encode_rle_general(const SrcRun src, float scale, uint8_t* wl, uint32_t lane) { return encode_rle_general<MODE>(src.p, scale, wl, lane); }
template <int MODE>
__device__ __forceinline__ uint32_t encode_rle_general(const SrcPair src, float scale, uint8_t* wl, uint32_t lane) { return encode_rle_general_from<MODE>(src, scale, wl, lane); }
template <int MODE>
__device__ __forceinline__ uint32_t encode_rle_general(const SrcPairMixed src, float scale, uint8_t* wl, uint32_t lane) { return encode_rle_general_from<MODE>(src, scale, wl, lane); }
template <int MODE>
__device__ __forceinline__ uint32_t encode_rle_general(const SrcPairScaled src, float scale, uint8_t* wl, uint32_t lane) { return encode_rle_general_from<MODE>(src, scale, wl, lane); }

// the reference's own rule for blocks that hold inf / NaN: a NaN never wins the '>' compare (cache_engine.cpp:176-180).
// Rare, out of line, and fed from memory again (a register array passed by reference would move to scratch).
template <class SRC>
__device__ __forceinline__ float absmax_with_nonfinite_from(const SRC src, uint32_t lane)
{
    float mx = 0.0f;
#pragma unroll 1
    for (uint32_t p = lane; p < kBlockElems; p += 64u)
        mx = __builtin_fmaxf(mx, fabsf(half_bits_to_float(src_half(src, p))));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float other = __shfl_xor(mx, o);
        mx = (other > mx) ? other : mx;
    }
    return mx;
}
__device__ __noinline__ float absmax_with_nonfinite(const uint8_t* __restrict__ src, uint32_t lane) { return absmax_with_nonfinite_from(SrcRun{src}, lane); }
__device__ __forceinline__ float absmax_with_nonfinite(const SrcRun src, uint32_t lane) { return absmax_with_nonfinite(src.p, lane); }
__device__ __forceinline__ float absmax_with_nonfinite(const SrcPair src, uint32_t lane) { return absmax_with_nonfinite_from(src, lane); }
__device__ __forceinline__ float absmax_with_nonfinite(const SrcPairMixed src, uint32_t lane) { return absmax_with_nonfinite_from(src, lane); }
__device__ __forceinline__ float absmax_with_nonfinite(const SrcPairScaled src, uint32_t lane) { return absmax_with_nonfinite_from(src, lane); }

// ===================================================================
// encode  (cache_engine.cpp:40-82,172-239)
// ===================================================================
// Where one block's record goes: the page table of its allocation (engine form) or the raw arrays of the codec operators.
struct EncTarget {
    PageEntry* entries;
    float*     scale_tab;
    uint32_t   region_pages, scale_run;
    uint32_t*  len_samples;
    uint8_t*   recs;              // raw form (entries == nullptr)
    uint64_t   rec_stride;
    uint32_t*  rec_bytes;
    float*     scales;
};

// One block: 4096 source bytes (SRC says where they are) -> the record of `page`, its length, scale and table words.  The one
// body of every encoder kernel: k_compress reads a contiguous image, k_compress_pairs two rows.
template <int SCHEME, int MODE, class SRC>
__device__ __forceinline__ void compress_block(const EncTarget& t, const uint64_t page, const SRC src, uint16_t* lds, const uint32_t lane, const uint32_t wave)
{
    PageEntry* const entries = t.entries;
    float* const scale_tab = t.scale_tab;
    const uint32_t region_pages = t.region_pages, scale_run = t.scale_run;
    uint8_t* rec = entries ? reinterpret_cast<uint8_t*>(gload<uint64_t>(&entries[page].pool_addr))
                           : t.recs + page * t.rec_stride;
    // MXFP4 in the pool is tile-planar (kernels.hpp): the codes go mx4_code_delta behind the nibbles -- the entry's scale word
    uint8_t* rec_codes = rec + 1024u;
    if (SCHEME == kMxFp4 && entries) rec_codes = rec + gload<uint32_t>(reinterpret_cast<const uint32_t*>(&entries[page].scale));
    uint32_t out_len;
    float scale = 1.0f;

    uint4 raw[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        raw[j] = src_ld16(src, j, lane);

    if (SCHEME == kFp16) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            enc_st16(rec + 2ull * (512u * j + 8u * lane), raw[j]);
        out_len = 2u * kBlockElems;
    } else if (SCHEME == kInt4G32) {
        // per group of 32 elements (4 lanes x 8): s = fp16(max|x|/7), q = clamp(round(x/s), -7, 7).  The group's max|x| and
        // its "all finite" test come from the fp16 bit patterns (v_pk_max_u16, two elements per instruction), the
        // quantisation runs in packed fp32 (the same multiply / fma / fma / add / truncate per element as the scalar form,
        // so the same bits).  Round 4, instruction count (the kernel ran 18 % over what the chip moves at its read : write
        // mix, profiles/r04_store_shape.txt): max|x| / 7 and 1 / s without the IEEE divide (codec_device.hpp: two and three
        // operations, bit-identical for fp16-valued operands); no clamp when every scale of the chunk is a normal fp16
        // (then no quotient reaches 7.5); the nibbles summed as signed i << 4k and un-biased once per dword.
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t words[4] = {raw[j].x, raw[j].y, raw[j].z, raw[j].w};
            u16x2 m2 = {0, 0};
#pragma unroll
            for (int t = 0; t < 4; ++t) m2 = __builtin_elementwise_max(m2, __builtin_bit_cast(u16x2, words[t] & 0x7FFF7FFFu));
            uint32_t mbits = m2.x > m2.y ? m2.x : m2.y;                 // largest |bits| of the lane's 8 elements
            mbits = umax(mbits, dpp<0xB1>(0u, mbits));                  // quad_perm [1,0,3,2]: lane ^ 1
            mbits = umax(mbits, dpp<0x4E>(0u, mbits));                  // quad_perm [2,3,0,1]: lane ^ 2 -> the group of 32
            const bool finite = __ballot(mbits >= 0x7C00u) == 0ull;     // wave-uniform: no inf / NaN in any group of this chunk
            uint32_t nib = 0;
            _Float16 s16;
            if (finite) {
                float sdiv = div7_of_f16_value(half_bits_to_float(mbits));
                asm volatile("" : "+v"(sdiv));                      // keep the fp32 rounding of the divide
                s16 = static_cast<_Float16>(sdiv);
                const float sc = static_cast<float>(s16);
                // |x| <= 7.5*sc in a finite group: the reciprocal divide is exact (test_fast_division_is_exact); a scale that
                // rounds to zero (subnormal groups) gives rcp = 0 and every quotient 0, as the definition says
                const float rcp = sc != 0.0f ? rcp_of_f16_value(sc) : 0.0f;
                const f32x2 ss = {sc, sc}, rr = {rcp, rcp};
                // a subnormal scale may be off by more than half a step: only then can a quotient leave [-7.5, 7.5]
                const uint32_t sbits = __builtin_bit_cast(uint16_t, s16);
                const bool clamp = __ballot(sbits - 1u < 0x3FFu) != 0ull;                   // (wave-uniform)
                int iq[8];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    f32x2 x;
                    x.x = half_bits_to_float(words[t] & 0xFFFFu);
                    x.y = half_bits_to_float(words[t] >> 16);
                    const f32x2 q0 = x * rr;
                    const f32x2 e = __builtin_elementwise_fma(-q0, ss, x);
                    const f32x2 y = __builtin_elementwise_fma(e, rr, q0);
                    f32x2 h;
                    h.x = __builtin_copysignf(0.5f, y.x);
                    h.y = __builtin_copysignf(0.5f, y.y);
                    const f32x2 r = y + h;                          // round half away from zero = truncate(y + copysign(0.5, y))
                    iq[2 * t] = static_cast<int>(r.x);
                    iq[2 * t + 1] = static_cast<int>(r.y);
                }
                if (clamp) {
#pragma unroll
                    for (int k = 0; k < 8; ++k) iq[k] = min(max(iq[k], -7), 7);
                }
                // nibble k = iq[k] & 0xF:  sum of iq[k] << 4k  =  sum of (iq[k] + 8) << 4k  -  0x88888888, and (i + 8) ^ 8 = i & 0xF
                uint32_t acc = 0x88888888u;
#pragma unroll
                for (int k = 0; k < 8; ++k) acc += static_cast<uint32_t>(iq[k]) << (4 * k);
                nib = acc ^ 0x88888888u;
            } else {
                float xv[8];
                float mx = 0.0f, nanacc = 0.0f;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    xv[k] = half_bits_to_float((words[k >> 1] >> ((k & 1) * 16)) & 0xFFFFu);
                    absmax_finite(xv[k], mx, nanacc);
                }
                float o = __shfl_xor(mx, 1); mx = (o > mx) ? o : mx;
                o = __shfl_xor(mx, 2);       mx = (o > mx) ? o : mx;
                float sdiv = mx / 7.0f;
                asm volatile("" : "+v"(sdiv));
                s16 = static_cast<_Float16>(sdiv);
                const float sc = static_cast<float>(s16);
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    float r = 0.0f;
                    if (sc != 0.0f && sc == sc) {
                        r = roundf(xv[k] / sc);
                        if (!(r == r)) r = 0.0f;
                        r = fminf(fmaxf(r, -7.0f), 7.0f);
                    }
                    nib |= (static_cast<uint32_t>(static_cast<int>(r)) & 0xFu) << (4 * k);
                }
            }
            // The record is assembled in LDS and leaves as whole 16-byte pieces per lane: written straight from the
            // registers it took eight store instructions of 4 / 2 bytes per lane (0.63-0.65 of HBM peak).
            const uint32_t p0 = 512u * j + 8u * lane;
            uint8_t* wl = reinterpret_cast<uint8_t*>(lds) + wave * kInt4RecBytes;
            *reinterpret_cast<uint32_t*>(wl + 128u + (p0 >> 1)) = nib;
            if ((lane & 3u) == 0u)
                *reinterpret_cast<uint16_t*>(wl + 2u * (p0 >> 5)) = __builtin_bit_cast(uint16_t, s16);
        }
        {
            uint8_t* wl = reinterpret_cast<uint8_t*>(lds) + wave * kInt4RecBytes;
            wave_lds_fence();
            enc_st16(rec + 128u + 16u * lane, *reinterpret_cast<const uint4*>(wl + 128u + 16u * lane));
            if (lane < 8u) enc_st16(rec + 16u * lane, *reinterpret_cast<const uint4*>(wl + 16u * lane));
            wave_lds_fence();
        }
        out_len = kInt4RecBytes;
    } else if (SCHEME == kMxFp4) {
        // OCP MX v1.0 conversion (oracle: compress_mxfp4) over the block's two halves interleaved element by element: byte i of the
        // record = element i (low nibble) and element 1024 + i (high), one E8M0 code per 16 bytes.  This lane's raw[j] and
        // raw[j + 2] (j = 0, 1) are exactly such partners -- elements [512 j + 8 l, + 8) and the same 1024 further on -- so the
        // interleave never leaves the lane; a block of 32 = this lane's and lane ^ 1's 8 + 8 elements of both halves.
        //   code = floor(log2 max|x|) - 2 + 127 = the exponent field of max|x| as a float, minus 2
        //   q    = E2M1 of x / 2^(code-127), nearest even, saturating: one v_cvt_scalef32_pk_fp4_f16 per element pair (it divides
        //          by the power of two its scale operand's exponent names: profiles/probes/mxprobe.hip)
        typedef _Float16 f16x2v __attribute__((ext_vector_type(2)));
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const uint32_t w0[4] = {raw[j].x, raw[j].y, raw[j].z, raw[j].w};                    // first half: elements 2t, 2t+1 per word
            const uint32_t w1[4] = {raw[j + 2].x, raw[j + 2].y, raw[j + 2].z, raw[j + 2].w};    // their partners in the second half
            u16x2 m2 = {0, 0};
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                m2 = __builtin_elementwise_max(m2, __builtin_bit_cast(u16x2, w0[t] & 0x7FFF7FFFu));
                m2 = __builtin_elementwise_max(m2, __builtin_bit_cast(u16x2, w1[t] & 0x7FFF7FFFu));
            }
            uint32_t mbits = m2.x > m2.y ? m2.x : m2.y;                 // largest |bits| of the lane's 16 elements
            mbits = umax(mbits, dpp<0xB1>(0u, mbits));                  // lane ^ 1 -> the block of 32
            const bool finite = __ballot(mbits >= 0x7C00u) == 0ull;     // wave-uniform: no inf / NaN in any block of this chunk
            uint32_t nib[2] = {0u, 0u}, code = 0;
            if (finite) {
                code = mbits ? (__float_as_uint(half_bits_to_float(mbits)) >> 23) - 2u : 0u;
                const float sc = mbits ? __uint_as_float(code << 23) : 1.0f;      // (code >= 101 for any non-zero fp16: a normal float)
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    // (element 2t of both halves), (element 2t+1 of both halves) -> bytes 2t, 2t+1
                    const f16x2v ea = __builtin_bit_cast(f16x2v, __builtin_amdgcn_perm(w1[t], w0[t], 0x05040100u));
                    const f16x2v eb = __builtin_bit_cast(f16x2v, __builtin_amdgcn_perm(w1[t], w0[t], 0x07060302u));
                    uint32_t& o = nib[t >> 1];
                    if (t & 1) { o = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(o, ea, sc, 2); o = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(o, eb, sc, 3); }
                    else       { o = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(o, ea, sc, 0); o = __builtin_amdgcn_cvt_scalef32_pk_fp4_f16(o, eb, sc, 1); }
                }
            } else {
                // a chunk with inf / NaN somewhere: NaN elements are skipped in the maximum and store +0, inf counts as 65504
                float x0[8], x1[8];
                float mx = 0.0f;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    float a0 = half_bits_to_float((w0[k >> 1] >> ((k & 1) * 16)) & 0xFFFFu), a1 = half_bits_to_float((w1[k >> 1] >> ((k & 1) * 16)) & 0xFFFFu);
                    a0 = (a0 == a0) ? fminf(fmaxf(a0, -65504.0f), 65504.0f) : 0.0f;
                    a1 = (a1 == a1) ? fminf(fmaxf(a1, -65504.0f), 65504.0f) : 0.0f;
                    x0[k] = a0; x1[k] = a1;
                    mx = fmaxf(mx, fmaxf(fabsf(a0), fabsf(a1)));
                }
                const float o = __shfl_xor(mx, 1);
                mx = (o > mx) ? o : mx;
                code = mx > 0.0f ? (__float_as_uint(mx) >> 23) - 2u : 0u;
                const float sc = mx > 0.0f ? __uint_as_float(code << 23) : 1.0f;
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    uint32_t& ob = nib[k >> 2];
                    switch (k & 3) {
                    case 0: ob = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(ob, x0[k], x1[k], sc, 0); break;
                    case 1: ob = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(ob, x0[k], x1[k], sc, 1); break;
                    case 2: ob = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(ob, x0[k], x1[k], sc, 2); break;
                    default: ob = __builtin_amdgcn_cvt_scalef32_pk_fp4_f32(ob, x0[k], x1[k], sc, 3); break;
                    }
                    // a NaN element keeps no sign: +0
                    if (((w0[k >> 1] >> ((k & 1) * 16)) & 0x7FFFu) > 0x7C00u) ob &= ~(0x0Fu << (8 * (k & 3)));
                    if (((w1[k >> 1] >> ((k & 1) * 16)) & 0x7FFFu) > 0x7C00u) ob &= ~(0xF0u << (8 * (k & 3)));
                }
            }
            // the record is assembled in LDS and leaves as whole 16-byte pieces per lane (as the INT4 record does)
            const uint32_t p0 = 512u * j + 8u * lane;
            uint8_t* wl = reinterpret_cast<uint8_t*>(lds) + wave * kMx4RecBytes;
            *reinterpret_cast<uint2*>(wl + p0) = make_uint2(nib[0], nib[1]);
            if ((lane & 1u) == 0u) wl[1024u + (p0 >> 4)] = static_cast<uint8_t>(code);
        }
        {
            uint8_t* wl = reinterpret_cast<uint8_t*>(lds) + wave * kMx4RecBytes;
            wave_lds_fence();
            enc_st16(rec + 16u * lane, *reinterpret_cast<const uint4*>(wl + 16u * lane));
            if (lane < 4u) enc_st16(rec_codes + 16u * lane, *reinterpret_cast<const uint4*>(wl + 1024u + 16u * lane));
            wave_lds_fence();
        }
        out_len = kMx4RecBytes;
    } else if (SCHEME == kFp8E4m3) {
        float x[4][8];
        float mx = 0.0f, nanacc = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t words[4] = {raw[j].x, raw[j].y, raw[j].z, raw[j].w};
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                x[j][k] = half_bits_to_float((words[k >> 1] >> ((k & 1) * 16)) & 0xFFFFu);
                absmax_finite(x[j][k], mx, nanacc);
            }
        }
        // (mx is never a NaN and never negative: its bit pattern orders like its value -- the DPP max scan of the encoders
        // instead of six trips through the LDS crossbar)
        mx = __uint_as_float(lane63(wave_incl_max(__float_as_uint(mx))));
        const bool finite = __ballot(!(nanacc == 0.0f)) == 0ull;       // wave-uniform
        // a finite block's max|x| is an fp16 value: its scale and the reciprocal without the IEEE divide, bit-identical
        // (codec_device.hpp; exhaustive: test_fast_division_is_exact)
        scale = (mx > 0.0f) ? (finite ? div448_of_f16_value(mx) : mx / 448.0f) : 1.0f;
        const float rcp = finite ? rcp_of_scale(scale) : 1.0f / scale;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v[8];
            if (finite) {
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    v[k] = fminf(fmaxf(__builtin_copysignf(div_by_scale(x[j][k], scale, rcp), x[j][k]), -448.0f), 448.0f);
            } else {
#pragma unroll
                for (int k = 0; k < 8; ++k) v[k] = fminf(fmaxf(x[j][k] / scale, -448.0f), 448.0f);
            }
            int lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[0], v[1], 0, false);
            lo = __builtin_amdgcn_cvt_pk_fp8_f32(v[2], v[3], lo, true);
            int hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[4], v[5], 0, false);
            hi = __builtin_amdgcn_cvt_pk_fp8_f32(v[6], v[7], hi, true);
            enc_st8(rec + 512u * j + 8u * lane, make_uint2(static_cast<uint32_t>(lo), static_cast<uint32_t>(hi)));
        }
        out_len = kBlockElems;
    } else {
        const uint32_t mbits = absmax_bits(raw);                       // wave-uniform
        const bool finite = mbits < 0x7C00u;
        const float mx = finite ? half_bits_to_float(mbits) : absmax_with_nonfinite(src, lane);
        scale = (mx > 0.0f) ? (finite ? div127_of_f16_value(mx) : mx / 127.0f) : 1.0f;     // cache_engine.cpp:172-183 (finite: an fp16 value
        const float rcp = finite ? rcp_of_scale(scale) : 1.0f / scale;                      //  over 127 without the IEEE divide, same bits)

        if (SCHEME == kInt8) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                uint32_t q[8];
                if (finite) {
                    quantize8<MODE>(raw[j], scale, rcp, q);
                } else {
                    const uint32_t words[4] = {raw[j].x, raw[j].y, raw[j].z, raw[j].w};
#pragma unroll
                    for (int k = 0; k < 8; ++k)
                        q[k] = quantize<MODE>(half_bits_to_float((words[k >> 1] >> ((k & 1) * 16)) & 0xFFFFu), scale);
                }
                uint2 o;
                o.x = (q[0] & 0xFFu) | ((q[1] & 0xFFu) << 8) | ((q[2] & 0xFFu) << 16) | (q[3] << 24);
                o.y = (q[4] & 0xFFu) | ((q[5] & 0xFFu) << 8) | ((q[6] & 0xFFu) << 16) | (q[7] << 24);
                enc_st8(rec + 512u * j + 8u * lane, o);
            }
            out_len = kBlockElems;
        } else if (mx == 0.0f) {
            // every element is +-0 (or a NaN, which quantises to 0 as well): all deltas are 0, so the record is
            // eight runs of 255 zeros and one of 8 (cache_engine.cpp:208-239) -- no need to encode anything
            if (lane < 16u)
                reinterpret_cast<uint16_t*>(rec)[lane] = lane < 8u ? 0xFF00u : (lane == 8u ? 0x0800u : 0u);
            out_len = 18u;
        } else {
            uint8_t* wl = reinterpret_cast<uint8_t*>(lds) + wave * kEncWaveBytes;
            uint32_t nruns = finite ? encode_rle_fast<MODE>(raw, scale, rcp, wl, lane) : kEncFail;
            wave_lds_fence();
            if (nruns == kEncFail) {
                if (finite) {                                        // long stretches: the fast path's SPLIT form, from the source again
                    uint4 again[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) again[j] = src_ld16(src, j, lane);
                    nruns = encode_rle_fast<MODE, true>(again, scale, rcp, wl, lane);
                } else {
                    nruns = encode_rle_general<MODE>(src, scale, wl, lane);
                }
                wave_lds_fence();
            }
            uint8_t* pairbuf = wl + kEncPairOff;
            // zero the tail of the last 16-byte chunk so the stored slot is deterministic
            {
                const uint32_t idx = nruns + lane;
                if (lane < 8u && idx < ((nruns + 7u) & ~7u)) reinterpret_cast<uint16_t*>(pairbuf)[idx] = 0;
            }
            wave_lds_fence();
            out_len = 2u * nruns;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t b = 1024u * j + 16u * lane;
                if (b < out_len)
                    enc_st16(rec + b, *reinterpret_cast<const uint4*>(pairbuf + b));
            }
            wave_lds_fence();
        }
    }
    if (lane == 0u) {
        if (entries) {
            gstore<uint32_t>(&entries[page].rec_bytes, out_len);
            if (SCHEME != kMxFp4) gstore<float>(&entries[page].scale, scale);       // (MXFP4: the word holds the code delta)
            if (SCHEME == kInt8DeltaRle && t.len_samples && (page & 1023u) == 0u) gstore<uint32_t>(&t.len_samples[(page >> 10) & 15u], out_len);
            if (scale_tab) {
                const uint32_t j = static_cast<uint32_t>(page % region_pages) & 15u;
                gstore<float>(&scale_tab[page - j + attend_tile_slot(j)], scale);
                if (scale_run) gstore<float>(scale_tab + scale_run_index(page, scale_run), scale);
            }
        } else {
            t.rec_bytes[page] = out_len;
            if (t.scales) t.scales[page] = scale;
        }
    }
}

#define SPECKV_ENC_LDS(SCHEME) \
    __shared__ __attribute__((aligned(16))) uint16_t lds[SCHEME == kInt8DeltaRle ? kWaves * kEncLdsHalves : SCHEME == kInt4G32 ? kWaves * (kInt4RecBytes / 2) \
                                                         : SCHEME == kMxFp4 ? kWaves * (kMx4RecBytes / 2) : 8]

} // namespace
} // namespace speckv
