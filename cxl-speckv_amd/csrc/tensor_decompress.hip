// cxl-speckv_amd/csrc/tensor_decompress.hip -- FPGACacheEngine::decompress over a stream of ANY length, as the reference defines
// it (src/fpga_engine/cache_engine.cpp:84-116): pairs (delta, count) expand to the int8 delta chain (:241-258), its running sum is
// q (:260-273), one scale dequantises; an odd trailing byte is dropped (:245).  The other direction, with the vocabulary, is
// tensor_compress.hip; what both use is tensor_codec_device.hpp.  Production, chosen by launch_tensor_decompress (see there):
//   by pairs   k_td_fused: ONE pass, a chunk of 2048 pairs per wave;   many streams: k_tdb_fused (one workgroup each) or k_tdm_fused
//   by output  k_td_summary -> k_td_scan_local/_apply -> k_td_expand_scatter: 2048 OUTPUT elements per wave (no pairs: k_td_scan alone)
// Reached through tuning switches only (the tests run them), under a banner of their own: k_td_scan_wg (SPECKV_TC_SCAN=1; =2 is
// k_td_scan) and k_td_expand (SPECKV_TD_EXPAND_PER_ELEMENT).  SPECKV_TC_MULTIPASS / SPECKV_TD_ONE_PASS force a production form.
#include "tensor_codec_device.hpp"

namespace speckv {
namespace {

// ---------------------------------------------------------------- decompress in ONE pass over the stream
// The by-output form of rounds 2-3 (k_td_summary, a scan, k_td_expand) reads the stream twice and stores a byte per ELEMENT.  This form
// reads it once and expands the way the pool's block decoder does (kernels.hip: decode_rle_fast) -- one byte scattered per RUN, the rest constant work:
//   the expanded deltas are piecewise constant, so the decoded int8 sequence is the SECOND prefix sum (mod 256) of
//       E[start of run r] = value_r - value_{r-1},   0 elsewhere        (cache_engine.cpp:241-273)
//   a wave owns a chunk of 2048 pairs (4 KiB of the stream: four 16-byte loads per lane, kept in registers) and sums its counts and
//   value x count products; a workgroup of kTdfWaves waves takes that many consecutive chunks (ticket counter: ascending order, so
//   a workgroup's predecessors are finished or resident) and publishes ONE 8-byte status word (state << 62 | int8 prefix << 54 |
//   elements; the value is the word -- agent-scope relaxed store / load, nothing to fence); wave 0 looks back over the
//   predecessors' words 64 at a time; every wave then knows where its stretch of the output starts and what q was in front of it.
//   The stretch goes out window by window (4096 elements, aligned to 8 elements of the OUTPUT so that whole groups are 16-byte
//   stores; a chunk of data that does not compress is one window): clear the window's byte table, scatter E for the pairs that
//   start in it, then 512 elements per step: two packed wave scans + eight byte recurrences per lane, dequantise, store.  The
//   groups at the two ragged ends of the stretch are stored element by element (their neighbours belong to the next chunk's wave).
// A chunk that holds a ZERO count (nothing our encoders or the reference's emit; cache_engine.cpp:262 just skips it) would put two
// runs on one table byte: such a chunk is expanded pair by pair, straight to memory (td_chunk_general).
#ifndef SPECKV_TDF_WAVES
#define SPECKV_TDF_WAVES 16
#endif
constexpr uint32_t kTdfWaves = SPECKV_TDF_WAVES;
constexpr uint32_t kTdfChunks = kTdfWaves - kTdfLbWave;
constexpr uint32_t kTdfWin = 4096;           // elements per window
#define SPECKV_TD_SDWA2(NAME, OP, S0, S1)                                                       \
    __device__ __forceinline__ uint32_t NAME(uint32_t a, uint32_t b)                            \
    {                                                                                           \
        uint32_t r;                                                                             \
        asm(OP " %0, %1, %2 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:" S0 " src1_sel:" S1   \
            : "=v"(r) : "v"(a), "v"(b));                                                        \
        return r;                                                                               \
    }
SPECKV_TD_SDWA2(td_add_b0, "v_add_u32_sdwa", "DWORD", "BYTE_0")
SPECKV_TD_SDWA2(td_add_b1, "v_add_u32_sdwa", "DWORD", "BYTE_1")
SPECKV_TD_SDWA2(td_add_b2, "v_add_u32_sdwa", "DWORD", "BYTE_2")
SPECKV_TD_SDWA2(td_add_b3, "v_add_u32_sdwa", "DWORD", "BYTE_3")
SPECKV_TD_SDWA2(td_sub_b0_b2, "v_sub_u32_sdwa", "BYTE_0", "BYTE_2")   // a.b0 - b.b2
SPECKV_TD_SDWA2(td_sub_b2_b0, "v_sub_u32_sdwa", "BYTE_2", "BYTE_0")   // a.b2 - b.b0
#undef SPECKV_TD_SDWA2
template <int K> __device__ __forceinline__ uint32_t td_add_byte(uint32_t a, uint32_t lo, uint32_t hi)
{
    return K == 0 ? td_add_b0(a, lo) : K == 1 ? td_add_b1(a, lo) : K == 2 ? td_add_b2(a, lo) : K == 3 ? td_add_b3(a, lo)
         : K == 4 ? td_add_b0(a, hi) : K == 5 ? td_add_b1(a, hi) : K == 6 ? td_add_b2(a, hi) : td_add_b3(a, hi);
}
__device__ __forceinline__ void td_lds_b8(uint32_t addr, uint32_t v) { *reinterpret_cast<lds_u8*>(static_cast<uintptr_t>(addr)) = static_cast<uint8_t>(v); }

// Exclusive prefix in front of workgroup `t` (t > 0): elements (low 54 bits of the words) and the int8 prefix (the 8 bits above,
// summed modulo 256 by the caller).  An aggregate's element count is < 2^24 x kTdfWaves.
__device__ __forceinline__ void td_look_back(const uint64_t* status, uint64_t t, uint32_t lane, uint64_t& elems, uint32_t& qsum)
{
    constexpr uint64_t kLo = (1ull << 54) - 1ull;
    elems = 0; qsum = 0;
    uint64_t end = t;                                                    // words [.., end) are still to be looked at
    for (;;) {
        const bool have = lane < end;
        uint64_t w;
        unsigned long long ready, incl;
        uint32_t first_incl;
        for (;;) {                                                       // this window: every word in front of the nearest prefix must be there
            w = have ? tc_lb_load(status + (end - 1u - lane)) : (2ull << 62);        // (in front of workgroup 0: a prefix of nothing)
            ready = __ballot((w >> 62) != 0ull);
            incl = __ballot((w >> 62) == 2ull);
            first_incl = incl ? static_cast<uint32_t>(__builtin_ctzll(incl)) : 64u;
            const unsigned long long need = first_incl >= 63u ? ~0ull : ((2ull << first_incl) - 1ull);
            if ((ready & need) == need) break;
            __builtin_amdgcn_s_sleep(8);
        }
        const uint64_t v = w & kTcLbMask;
        const bool mine = lane < first_incl;                            // aggregates in front of the prefix
        const uint32_t lo_lo = lane63(wave_incl_add(mine ? static_cast<uint32_t>(v & 0xFFFFu) : 0u));
        const uint32_t lo_hi = lane63(wave_incl_add(mine ? static_cast<uint32_t>((v & kLo) >> 16) : 0u));
        elems += (static_cast<uint64_t>(lo_hi) << 16) + lo_lo;
        qsum += lane63(wave_incl_add(mine ? static_cast<uint32_t>(v >> 54) : 0u));
        if (first_incl < 64u) {
            const uint32_t pl = static_cast<uint32_t>(__shfl(static_cast<int>(v & 0xFFFFFFFFull), static_cast<int>(first_incl)));
            const uint32_t ph = static_cast<uint32_t>(__shfl(static_cast<int>(v >> 32), static_cast<int>(first_incl)));
            const uint64_t pv = (static_cast<uint64_t>(ph) << 32) | pl;
            elems += pv & kLo; qsum += static_cast<uint32_t>(pv >> 54);
            return;
        }
        end -= 64u;
    }
}

// A chunk with zero counts in it: pair by pair, 64 pairs per step (an add-scan of (value x count mod 256) << 24 | count gives each
// run its start and the int8 prefix of all earlier deltas; the lane writes its run element by element), clipped at `end`.
template <int MODE, bool F32>
__device__ __noinline__ void td_chunk_general(const uint8_t* __restrict__ rle, uint64_t p0, uint64_t n_pairs, uint64_t start, uint64_t end,
                                              uint32_t qp, float scale, uint8_t* __restrict__ dst, uint32_t lane)
{
    uint64_t pos = start;
    uint32_t q0 = qp;
#pragma unroll 1
    for (uint32_t b = 0; b < kTile && pos < end; b += 64u) {
        const uint64_t i = p0 + b + lane;
        uint32_t bits = 0;
        if (i < n_pairs) bits = *reinterpret_cast<const uint16_t*>(rle + 2ull * i);
        const uint32_t v = bits & 0xFFu, c = bits >> 8;
        const uint32_t packed = ((v * c) << 24) | c;
        const uint32_t incl = wave_incl_add(packed);
        const uint32_t e = incl - packed;
        uint64_t p = pos + (e & 0xFFFFFFu);
        uint32_t q = q0 + (e >> 24);
#pragma unroll 1
        for (uint32_t m = 0; m < c && p < end; ++m, ++p) {
            q += v;
            const float y = dequant<MODE>(static_cast<int>(static_cast<int8_t>(q & 0xFFu)), scale);
            if (F32) reinterpret_cast<float*>(dst)[p] = y;
            else { float a = y, z = 0.0f; reinterpret_cast<uint16_t*>(dst)[p] = static_cast<uint16_t>(pack_half2(a, z) & 0xFFFFu); }
        }
        const uint32_t tot = lane63(incl);
        pos += tot & 0xFFFFFFu;
        q0 = (q0 + (tot >> 24)) & 0xFFu;
    }
}

// The pairs of chunk `p0 / 2048`: dword = v0 | c0 << 8 | v1 << 16 | c1 << 24, pairs p0 + 512 j + 8 lane .. + 7 in w[j]; pairs behind
// the stream's end read as (0, 0).  mn: the smallest count among the lane's pairs that exist.
__device__ __forceinline__ void td_load_pairs(const uint8_t* __restrict__ rle, uint64_t p0, uint64_t n_pairs, bool live, uint32_t lane,
                                              uint32_t (&w)[4][4], uint32_t& mn)
{
    const bool wide = (reinterpret_cast<uintptr_t>(rle) & 15u) == 0u;
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
        const uint64_t i = p0 + 512u * j + 8u * lane;
        w[j][0] = w[j][1] = w[j][2] = w[j][3] = 0u;
        if (live && i < n_pairs) {
            if (wide && i + 8u <= n_pairs) {
                const u32x4 x = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(rle + 2ull * i));
                w[j][0] = x.x; w[j][1] = x.y; w[j][2] = x.z; w[j][3] = x.w;
#pragma unroll
                for (int t = 0; t < 4; ++t) mn = umin(mn, umin((w[j][t] >> 8) & 0xFFu, w[j][t] >> 24));
            } else {
#pragma unroll
                for (uint32_t e = 0; e < 8u; ++e)
                    if (i + e < n_pairs) {
                        const uint32_t bits = *reinterpret_cast<const uint16_t*>(rle + 2ull * (i + e));
                        w[j][e >> 1] |= bits << (16u * (e & 1u));
                        mn = umin(mn, bits >> 8);
                    }
            }
        }
    }
}
// Per step of 512 pairs: the lane's count and value x count sums scanned across the wave.  ex: exclusive prefix of the lane in its
// step, st: the step's total; both (sum v c mod 256) << 24 | sum c (counts < 2^24 per step).
__device__ __forceinline__ void td_scan_pairs(const uint32_t (&w)[4][4], uint32_t (&ex)[4], uint32_t (&st)[4])
{
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
        uint32_t sc = 0, sv = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const uint32_t counts = (w[j][t] >> 8) & 0x00FF00FFu;
            sc = __builtin_amdgcn_udot4(counts, 0x00010001u, sc, false);
            sv = __builtin_amdgcn_udot4(w[j][t], counts, sv, false);
        }
        const uint32_t lt = (sv << 24) | sc;
        const uint32_t incl = wave_incl_add(lt);
        ex[j] = incl - lt;
        st[j] = lane63(incl);
    }
}
// One window of a chunk: elements [wo, wo + 4096) counted from the chunk's OWN first element, as int8 values relative to the q in
// front of the chunk, into the wave's table (byte p = element wo + p).  Needs nothing from outside the chunk.
// c1 / c2: S1 (the delta) / S2 (q - q in front of the chunk) at the end of the previous window.
__device__ __forceinline__ void td_window_values(const uint32_t (&w)[4][4], const uint32_t (&ex)[4], const uint32_t (&st)[4], uint32_t wo,
                                                 uint32_t tot_c, uint8_t* tab, uint32_t lane, uint32_t& c1, uint32_t& c2)
{
    const uint32_t tab_addr = lds_addr_of(tab);
    const uint32_t cnt = tot_c - wo < kTdfWin ? tot_c - wo : kTdfWin;      // elements of the chunk in this window
    {
        u32x4* t4 = reinterpret_cast<u32x4*>(tab);
        const u32x4 z = {0u, 0u, 0u, 0u};
#pragma unroll
        for (uint32_t k = 0; k < kTdfWin / 1024u; ++k) t4[64u * k + lane] = z;
    }
    int32_t tot = -static_cast<int32_t>(wo);                             // first element of step 0, relative to the window (> -2^24)
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
        const int32_t step_c = static_cast<int32_t>(st[j] & 0xFFFFFFu);
        if (tot + step_c > 0 && tot < static_cast<int32_t>(kTdfWin)) {      // (wave-uniform) the step has pairs that start in the window
            const int32_t base = tot + static_cast<int32_t>(ex[j] & 0xFFFFFFu);
            // value of the pair in front of the lane's first (0 in front of the chunk: E of the first run is its value)
            const uint32_t pwj = wave_shr1(w[j][3], j == 0u ? 0u : lane63(w[j == 0u ? 0u : j - 1u][3]));
            const uint32_t d0 = td_sub_b0_b2(w[j][0], pwj), d1 = td_sub_b2_b0(w[j][0], w[j][0]);
            const uint32_t d2 = td_sub_b0_b2(w[j][1], w[j][0]), d3 = td_sub_b2_b0(w[j][1], w[j][1]);
            const uint32_t d4 = td_sub_b0_b2(w[j][2], w[j][1]), d5 = td_sub_b2_b0(w[j][2], w[j][2]);
            const uint32_t d6 = td_sub_b0_b2(w[j][3], w[j][2]), d7 = td_sub_b2_b0(w[j][3], w[j][3]);
            if (tot >= 0 && tot + step_c <= static_cast<int32_t>(kTdfWin)) {    // all of them do: plain addresses
                uint32_t a = tab_addr + static_cast<uint32_t>(base);
                td_lds_b8(a, d0); a = td_add_b1(a, w[j][0]);
                td_lds_b8(a, d1); a = td_add_b3(a, w[j][0]);
                td_lds_b8(a, d2); a = td_add_b1(a, w[j][1]);
                td_lds_b8(a, d3); a = td_add_b3(a, w[j][1]);
                td_lds_b8(a, d4); a = td_add_b1(a, w[j][2]);
                td_lds_b8(a, d5); a = td_add_b3(a, w[j][2]);
                td_lds_b8(a, d6); a = td_add_b1(a, w[j][3]);
                td_lds_b8(a, d7);                                       // (pairs behind the stream's end have count 0: they land on the byte behind
                                                                        //  the chunk's last element -- nobody's, or the spare byte at the window's end)
            } else {                                                    // a run may start in front of the window or behind it: those go to the spare bytes
                int32_t a = base;
                const uint32_t dd[8] = {d0, d1, d2, d3, d4, d5, d6, d7};
#pragma unroll
                for (uint32_t e = 0; e < 8u; ++e) {
                    const uint32_t off = static_cast<uint32_t>(a) < kTdfWin ? static_cast<uint32_t>(a) : kTdfWin;
                    td_lds_b8(tab_addr + off, dd[e]);
                    a += static_cast<int32_t>((w[j][e >> 1] >> (8u + 16u * (e & 1u))) & 0xFFu);
                }
            }
        }
        tot += step_c;
    }
    wave_lds_fence();
    // E -> q (relative), in place: 512 elements per step, two packed wave scans + eight byte recurrences per lane
#pragma unroll 1
    for (uint32_t g0 = 0; g0 < kTdfWin; g0 += 512u) {
        if (g0 >= cnt) break;                                            // (wave-uniform) nothing of this chunk behind here
        uint2* cell = reinterpret_cast<uint2*>(tab + g0 + 8u * lane);
        const uint2 x = *cell;
        const uint32_t t1 = __builtin_amdgcn_sad_u8(x.x, 0u, __builtin_amdgcn_sad_u8(x.y, 0u, 0u));
        const uint32_t t2 = __builtin_amdgcn_udot4(x.x, 0x05060708u, __builtin_amdgcn_udot4(x.y, 0x01020304u, 0u, false), false);
        const uint32_t i1 = wave_incl_add(t1);
        const uint32_t x1 = c1 + i1 - t1;                                // S1 entering this lane
        const uint32_t u = t2 + 8u * x1;                                 // this lane's S2 increment
        const uint32_t i2 = wave_incl_add(u);
        const uint32_t x2 = c2 + i2 - u;                                 // S2 entering this lane
        c1 += lane63(i1);
        c2 += lane63(i2);
        uint32_t s1 = x1, s2 = x2;
        uint32_t q[8];
        s1 = td_add_byte<0>(s1, x.x, x.y); s2 += s1; q[0] = s2;
        s1 = td_add_byte<1>(s1, x.x, x.y); s2 += s1; q[1] = s2;
        s1 = td_add_byte<2>(s1, x.x, x.y); s2 += s1; q[2] = s2;
        s1 = td_add_byte<3>(s1, x.x, x.y); s2 += s1; q[3] = s2;
        s1 = td_add_byte<4>(s1, x.x, x.y); s2 += s1; q[4] = s2;
        s1 = td_add_byte<5>(s1, x.x, x.y); s2 += s1; q[5] = s2;
        s1 = td_add_byte<6>(s1, x.x, x.y); s2 += s1; q[6] = s2;
        s1 = td_add_byte<7>(s1, x.x, x.y); s2 += s1; q[7] = s2;
        uint2 o;                                                         // byte k = q[k] & 0xFF (v_perm: two low bytes, then two halves)
        o.x = __builtin_amdgcn_perm(__builtin_amdgcn_perm(q[3], q[2], 0x0c0c0400u), __builtin_amdgcn_perm(q[1], q[0], 0x0c0c0400u), 0x05040100u);
        o.y = __builtin_amdgcn_perm(__builtin_amdgcn_perm(q[7], q[6], 0x0c0c0400u), __builtin_amdgcn_perm(q[5], q[4], 0x0c0c0400u), 0x05040100u);
        *cell = o;
    }
    wave_lds_fence();
}
// ... and out (round 6): groups of one 16-byte store -- 4 fp32 / 8 fp16 elements -- aligned in the OUTPUT, from a table that is
// aligned to the chunk: the group's bytes re-aligned with v_alignbyte from aligned dwords (group G of the window covers table
// bytes [g G - al, g G - al + g), al = start mod g), and every byte turned into its output value by ONE LDS read: `lut_q` = LDS
// address of entry qp of the workgroup's 512-entry table, entry i = the output bits of int8(i & 0xFF) under the tensor's scale
// (dequant<MODE>, converted once; the table byte is q - qp mod 256, so byte + qp < 512 needs no wrap).  Before: byte extract, add,
// sign extension, conversion, the exact division by 127 and the scale per element, and for fp32 a lane's 8 elements exchanged
// inside the quad so that a store instruction writes whole sectors -- 92 vector instructions per 8 elements, a third of the
// kernel's; now a lane takes 4 consecutive fp32 elements per store (lanes 16 bytes apart: a contiguous KiB per instruction).
// The groups at the window's two ends that hold fewer of its elements than a whole group go element by element (the others belong
// to the neighbouring chunk's wave, or to the window before / behind).
template <bool F32>
__device__ __forceinline__ uint32_t td_lut_entry(uint32_t lut_q, uint32_t bytes, int k)
{
    typedef const uint32_t __attribute__((address_space(3)))* l_u32_p;
    return *(l_u32_p)(static_cast<uintptr_t>(lut_q + (((bytes >> (8 * k)) & 0xFFu) << 2)));
}
template <int MODE, bool F32>
__device__ __forceinline__ void td_window_store(const uint8_t* tab, uint32_t wo, uint64_t start, uint64_t end, uint32_t lut_q,
                                                uint8_t* __restrict__ dst, uint32_t lane)
{
    constexpr uint32_t kG = F32 ? 4u : 8u;                              // elements per 16-byte store
    const uint32_t al = static_cast<uint32_t>(start) & (kG - 1u);
    const uint64_t obase = (start & ~static_cast<uint64_t>(kG - 1u)) + wo;      // output position of group 0's first element
    const int32_t lo_i = static_cast<int32_t>(al);                      // group-relative bounds of what this window stores
    const uint64_t wend = start + wo + kTdfWin < end ? start + wo + kTdfWin : end;
    const int32_t hi_i = static_cast<int32_t>(wend - obase);
    const uint32_t tab_addr = lds_addr_of(tab);
    typedef const uint32_t __attribute__((address_space(3)))* l_u32_p;
    typedef u32x4 __attribute__((address_space(1)))* g_u32x4_p;
    const uint32_t sh = (0u - al) & 3u;                                 // (table byte of a group's first element) mod 4: the same for every group
#pragma unroll 1
    for (uint32_t g0 = 0; static_cast<int32_t>(g0) < hi_i; g0 += 512u) {
#pragma unroll
        for (uint32_t part = 0; part < (F32 ? 2u : 1u); ++part) {
            const int32_t q0 = static_cast<int32_t>(g0 + (F32 ? 256u * part + 4u * lane : 8u * lane));     // group-relative element index of the lane's group
            if (q0 + static_cast<int32_t>(kG) <= lo_i || q0 >= hi_i) continue;
            const int32_t tb = q0 - static_cast<int32_t>(al);            // table byte of its first element (>= 1 - kG)
            const uint32_t da = tab_addr + static_cast<uint32_t>((tb >> 2) << 2);      // (arithmetic shift: -1 -> the dword in front)
            const uint32_t a0 = *(l_u32_p)(static_cast<uintptr_t>(da)), a1 = *(l_u32_p)(static_cast<uintptr_t>(da + 4u));
            const uint32_t lo4 = __builtin_amdgcn_alignbyte(a1, a0, sh);
            uint32_t hi4 = 0u;
            if (!F32) { const uint32_t a2 = *(l_u32_p)(static_cast<uintptr_t>(da + 8u)); hi4 = __builtin_amdgcn_alignbyte(a2, a1, sh); }
            uint32_t y[8];
#pragma unroll
            for (int e = 0; e < static_cast<int>(kG); ++e) y[e] = td_lut_entry<F32>(lut_q, e < 4 ? lo4 : hi4, e & 3);
            const uint64_t o = obase + static_cast<uint64_t>(q0);
            if (q0 >= lo_i && q0 + static_cast<int32_t>(kG) <= hi_i) {
                u32x4 v;
                if (F32) { v.x = y[0]; v.y = y[1]; v.z = y[2]; v.w = y[3]; }
                else { v.x = y[0] | (y[1] << 16); v.y = y[2] | (y[3] << 16); v.z = y[4] | (y[5] << 16); v.w = y[6] | (y[7] << 16); }
                __builtin_nontemporal_store(v, (g_u32x4_p)(reinterpret_cast<uintptr_t>(dst) + (F32 ? 4ull : 2ull) * o));
            } else {
                for (int e = 0; e < static_cast<int>(kG); ++e) {
                    if (q0 + e < lo_i || q0 + e >= hi_i) continue;
                    if (F32) reinterpret_cast<uint32_t*>(dst)[o + e] = y[e];
                    else reinterpret_cast<uint16_t*>(dst)[o + e] = static_cast<uint16_t>(y[e]);
                }
            }
        }
    }
    wave_lds_fence();
}
// A chunk of long runs: its windows behind the first, with the pairs read again (kept in registers over the first store pass
// they would cost the kernel a workgroup per CU).  Out of line: data that does not compress never gets here.
template <int MODE, bool F32>
__device__ __noinline__ void td_windows_behind_the_first(const uint8_t* __restrict__ rle, uint64_t p0, uint64_t n_pairs, uint64_t start,
                                                         uint64_t end, uint32_t lut_q, uint32_t tot_c, uint32_t c1, uint32_t c2, uint8_t* tab,
                                                         uint8_t* __restrict__ dst, uint32_t lane)
{
    uint32_t w[4][4], ex[4], st[4], mn = 255u;
    td_load_pairs(rle, p0, n_pairs, true, lane, w, mn);
    td_scan_pairs(w, ex, st);
#pragma unroll 1
    for (uint32_t wo = kTdfWin; start + wo < end; wo += kTdfWin) {
        td_window_values(w, ex, st, wo, tot_c, tab, lane, c1, c2);
        td_window_store<MODE, F32>(tab, wo, start, end, lut_q, dst, lane);
    }
}

// BATCH (speckv_ext_codec_decompress_tensors): one workgroup per stream, rounds of kTdfChunks chunks, the prefix in front of a
// round carried in LDS (see tc_fused_body).
template <int MODE, bool F32, bool BATCH, uint32_t WAVES = kTdfWaves>
__device__ __forceinline__ void td_fused_body(const uint8_t* __restrict__ rle, uint64_t n_pairs, uint64_t n_chunks, uint64_t wg0, uint64_t* __restrict__ status,
                                              uint64_t cap, uint64_t* __restrict__ out_n, float scale, uint8_t* __restrict__ dst)
{
    constexpr uint32_t kFront = 16;           // bytes in front of a wave's table (the store pass may read up to 7 of them: never used)
    __shared__ __attribute__((aligned(16))) uint8_t tabs[WAVES][kFront + kTdfWin + 16];      // (+16 behind: written, never used)
    __shared__ uint32_t s_tot[WAVES];
    __shared__ uint64_t s_start[WAVES];
    __shared__ uint32_t s_qp[WAVES];
    __shared__ uint64_t s_carry_before;                                 // BATCH: elements / int8 prefix in front of the round
    __shared__ uint32_t s_carry_q;
    __shared__ uint32_t s_lut[512];                                     // output bits of int8(i & 0xFF) under this tensor's scale (td_window_store)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < 512u; i += 64u * WAVES) {    // (published by the first barrier of round 0)
        const float y = dequant<MODE>(static_cast<int>(static_cast<int8_t>(i & 0xFFu)), scale);
        float a = y, z = 0.0f;
        s_lut[i] = F32 ? __float_as_uint(y) : (pack_half2(a, z) & 0xFFFFu);
    }
    if (BATCH && threadIdx.x == 0u) { s_carry_before = 0ull; s_carry_q = 0u; }       // (published by the first barrier of round 0)
    const uint64_t n_rounds = BATCH ? (n_chunks + (WAVES - kTdfLbWave) - 1u) / (WAVES - kTdfLbWave) : 1u;
#pragma unroll 1
    for (uint64_t round = 0; round < n_rounds; ++round) {
    const uint64_t wg = BATCH ? round : wg0;
    const uint64_t chunk = wg * (WAVES - kTdfLbWave) + wave - kTdfLbWave;
    const bool live = wave >= kTdfLbWave && chunk < n_chunks;           // (waves behind the last chunk only keep the barriers company)
    const uint64_t p0 = chunk * kTile;
    uint32_t w[4][4], ex[4], st[4], mn = 255u;
    td_load_pairs(rle, p0, n_pairs, live, lane, w, mn);
    td_scan_pairs(w, ex, st);
    const uint32_t tot_c = (st[0] & 0xFFFFFFu) + (st[1] & 0xFFFFFFu) + (st[2] & 0xFFFFFFu) + (st[3] & 0xFFFFFFu);     // < 2^24 (2048 x 255)
    const uint32_t tot_v = ((st[0] >> 24) + (st[1] >> 24) + (st[2] >> 24) + (st[3] >> 24)) & 0xFFu;
    const bool has_zero = __ballot(mn == 0u) != 0ull;
    if (lane == 0u) s_tot[wave] = (tot_v << 24) | tot_c;
    __syncthreads();
    // ---- wave 0: the workgroup's aggregate goes out at once (nobody in front of it is needed for that)
    if (wave == 0u) {
        const uint32_t wt = lane < WAVES ? s_tot[lane] : 0u;
        const uint32_t agg_c = lane63(wave_incl_add(wt & 0xFFFFFFu)), agg_v = lane63(wave_incl_add(wt >> 24)) & 0xFFu;      // < 2^24 x 16
        if (!BATCH && lane == 0u) tc_lb_store(status + wg, wg == 0u ? 2ull : 1ull, (static_cast<uint64_t>(agg_v) << 54) | agg_c);
    }
    // ---- the first window's values: nothing in them needs the look-back, which they therefore hide
    uint8_t* tab = tabs[wave] + kFront;
    uint32_t c1 = 0u, c2 = 0u;
    if (live && tot_c != 0u && !has_zero) td_window_values(w, ex, st, 0u, tot_c, tab, lane, c1, c2);
    // ---- wave 0: the prefix in front of the workgroup by look-back, every wave's own start; then everybody knows where it writes
    if (wave == 0u) {
        const uint32_t wt = lane < WAVES ? s_tot[lane] : 0u;         // (again: cheaper than keeping them over the window)
        const uint32_t wic = wave_incl_add(wt & 0xFFFFFFu), wiv = wave_incl_add(wt >> 24);
        const uint32_t agg_c = lane63(wic), agg_v = lane63(wiv) & 0xFFu;
        uint64_t before = 0;
        uint32_t qb = 0;
        if (BATCH) {
            before = s_carry_before; qb = s_carry_q;
            if (lane == 0u) { s_carry_before = before + agg_c; s_carry_q = (qb + agg_v) & 0xFFu; }
        } else if (wg != 0u) {
#ifdef SPECKV_TD_NO_LB
            before = wg * (WAVES - kTdfLbWave) * 2048ull;                         // (timing builds only: wrong output)
#else
            td_look_back(status, wg, lane, before, qb);
#endif
            qb &= 0xFFu;
            if (lane == 0u) tc_lb_store(status + wg, 2ull, (static_cast<uint64_t>((qb + agg_v) & 0xFFu) << 54) | (before + agg_c));
        }
        if (lane < WAVES) {
            s_start[lane] = before + (wic - (wt & 0xFFFFFFu));
            s_qp[lane] = (qb + wiv - (wt >> 24)) & 0xFFu;
        }
        if (lane == 0u && (wg + 1u) * (WAVES - kTdfLbWave) >= n_chunks) { const uint64_t total = before + agg_c; *out_n = total < cap ? total : cap; }
    }
    __syncthreads();
    if (!live) continue;
    const uint64_t start = s_start[wave];
    const uint32_t qp = s_qp[wave];
    const uint64_t end = (start + tot_c < cap) ? start + tot_c : cap;
    if (start >= end) continue;
    if (has_zero) { td_chunk_general<MODE, F32>(rle, p0, n_pairs, start, end, qp, scale, dst, lane); continue; }
    const uint32_t lut_q = lds_addr_of(reinterpret_cast<const uint8_t*>(s_lut)) + 4u * qp;
    td_window_store<MODE, F32>(tab, 0u, start, end, lut_q, dst, lane);
    if (start + kTdfWin < end) td_windows_behind_the_first<MODE, F32>(rle, p0, n_pairs, start, end, lut_q, tot_c, c1, c2, tab, dst, lane);
    }   // rounds
}

template <int MODE, bool F32>
__global__ __launch_bounds__(64 * kTdfWaves) __attribute__((amdgpu_waves_per_eu(8, 8)))
void k_td_fused(const uint8_t* __restrict__ rle, uint64_t n_pairs, uint64_t n_chunks, uint64_t* __restrict__ status, uint32_t* __restrict__ ticket,
                uint64_t cap, uint64_t* __restrict__ out_n, float scale, uint8_t* __restrict__ dst)
{
    __shared__ uint32_t s_ticket;
    if (threadIdx.x == 0u) s_ticket = atomicAdd(ticket, 1u);
    __syncthreads();
    td_fused_body<MODE, F32, false>(rle, n_pairs, n_chunks, s_ticket, status, cap, out_n, scale, dst);
}

// Many streams, one workgroup each (speckv_ext_codec_decompress_tensors): stream i = desc[i].rle, rle_bytes[i] bytes, scale
// scales[i], decoded into desc[i].data (room for desc[i].n elements); n_out[i] = elements the stream holds, clipped to the room.
template <int MODE, bool F32>
__global__ __launch_bounds__(64 * kTdmWaves) __attribute__((amdgpu_waves_per_eu(8, 8)))
void k_tdb_fused(const TcbDesc* __restrict__ desc, const uint64_t* __restrict__ rle_bytes, const float* __restrict__ scales, uint64_t* __restrict__ n_out)
{
    __shared__ uint64_t s_none;
    const TcbDesc d = desc[blockIdx.x];
    const uint64_t n_pairs = rle_bytes[blockIdx.x] >> 1;                 // an odd trailing byte is dropped (cache_engine.cpp:245)
    const uint64_t chunks = (n_pairs + kTile - 1u) / kTile;
    uint64_t* on = n_out ? n_out + blockIdx.x : &s_none;
    if (chunks == 0u || d.n == 0u) { if (threadIdx.x == 0u) *on = 0ull; return; }
    td_fused_body<MODE, F32, true, kTdmWaves>(d.rle, n_pairs, chunks, 0ull, nullptr, d.n, on, scales[blockIdx.x], static_cast<uint8_t*>(d.data));
}

// ... and with several workgroups per stream (see k_tcm_fused): stream t = ticket / wpt, its workgroup ticket % wpt takes 16 chunks of
// 2048 pairs, the prefix in front of it by look-back over the stream's own status words.
template <int MODE, bool F32>
__global__ __launch_bounds__(64 * kTdmWaves) __attribute__((amdgpu_waves_per_eu(8, 8)))
void k_tdm_fused(const TcbDesc* __restrict__ desc, uint32_t wpt, uint32_t* __restrict__ ticket, uint64_t* __restrict__ status,
                 const uint64_t* __restrict__ rle_bytes, const float* __restrict__ scales, uint64_t* __restrict__ n_out)
{
    __shared__ uint32_t s_ticket;
    __shared__ uint64_t s_none;
    if (threadIdx.x == 0u) s_ticket = atomicAdd(ticket, 1u);
    __syncthreads();
    const uint32_t t = s_ticket / wpt, l = s_ticket - t * wpt;
    const TcbDesc d = desc[t];
    const uint64_t n_pairs = rle_bytes[t] >> 1;                           // an odd trailing byte is dropped (cache_engine.cpp:245)
    const uint64_t chunks = (n_pairs + kTile - 1u) / kTile;
    const uint64_t my_wgs = (chunks + kTdmChunks - 1u) / kTdmChunks;
    uint64_t* on = n_out ? n_out + t : &s_none;
    if (l >= my_wgs || d.n == 0u) {
        if (l == 0u && threadIdx.x == 0u) *on = 0ull;
        return;
    }
    td_fused_body<MODE, F32, false, kTdmWaves>(d.rle, n_pairs, chunks, l, status + static_cast<uint64_t>(t) * wpt, d.n, on, scales[t], static_cast<uint8_t*>(d.data));
}

// ---------------------------------------------------------------- decompress by OUTPUT: summary, scan, expand (streams of few pairs)
struct TdSummary { uint32_t sum_c, sum_v; };           // of one chunk of 2048 pairs: elements it emits, sum of value*count mod 256
struct TdCarry { uint64_t start; uint32_t q_pre, pad; }; // elements / int8 prefix in front of the chunk

__global__ __launch_bounds__(256) void k_td_summary(const uint8_t* __restrict__ rle, uint64_t n_pairs, TdSummary* __restrict__ summ)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t chunk = static_cast<uint64_t>(blockIdx.x) * 4u + wave;
    const uint64_t p0 = chunk * kTile;
    if (p0 >= n_pairs) return;
    uint32_t sc = 0, sv = 0;
    // 8 pairs (16 bytes) per lane and step where the stream allows it (the chunk starts 4 KiB into the stream: aligned with it)
    const bool wide = (reinterpret_cast<uintptr_t>(rle) & 15u) == 0u;
#pragma unroll 1
    for (uint32_t step = 0; step < kTile / 512u; ++step) {
        const uint64_t i = p0 + 512u * step + 8u * lane;
        if (wide && i + 8u <= n_pairs) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(rle + 2ull * i);      // (temporal: the expand pass reads the stream again)
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int t = 0; t < 4; ++t) {                               // dword = v0 | c0 << 8 | v1 << 16 | c1 << 24
                const uint32_t counts = (w[t] >> 8) & 0x00FF00FFu;
                sc = __builtin_amdgcn_udot4(counts, 0x00010001u, sc, false);
                sv = __builtin_amdgcn_udot4(w[t], counts, sv, false);  // v0 c0 + v1 c1
            }
        } else {
            for (uint32_t k = 0; k < 8u; ++k) {
                uint32_t bits = 0;
                if (i + k < n_pairs) bits = *reinterpret_cast<const uint16_t*>(rle + 2ull * (i + k));
                sc += bits >> 8;
                sv += (bits & 0xFFu) * (bits >> 8);
            }
        }
    }
    sc = lane63(wave_incl_add(sc));
    sv = lane63(wave_incl_add(sv & 0xFFu));
    if (lane == 0u) summ[chunk] = TdSummary{sc, sv & 0xFFu};
}

__global__ __launch_bounds__(64) void k_td_scan(const TdSummary* __restrict__ summ, TdCarry* __restrict__ carry, uint64_t n_chunks,
                                               uint64_t cap, uint64_t* __restrict__ out_n)
{
    const uint32_t lane = threadIdx.x;
    uint64_t start = 0;
    uint32_t qpre = 0;
    for (uint64_t base = 0; base < n_chunks; base += 64u) {
        const uint64_t c = base + lane;
        TdSummary s{0u, 0u};
        if (c < n_chunks) s = summ[c];
        // 64 x 2048 x 255 elements per step do not fit 32 bits: scan the two halves of the count separately
        const uint32_t lo = wave_incl_add(s.sum_c & 0xFFFFu), hi = wave_incl_add(s.sum_c >> 16);
        const uint64_t inc = static_cast<uint64_t>(lo) + (static_cast<uint64_t>(hi) << 16);
        const uint32_t vinc = wave_incl_add(s.sum_v);
        if (c < n_chunks) carry[c] = TdCarry{start + inc - s.sum_c, (qpre + vinc - s.sum_v) & 0xFFu, 0u};
        start += static_cast<uint64_t>(lane63(lo)) + (static_cast<uint64_t>(lane63(hi)) << 16);
        qpre = (qpre + lane63(vinc)) & 0xFFu;
    }
    if (lane == 0u) {
        carry[n_chunks] = TdCarry{start, qpre, 0u};
        *out_n = start < cap ? start : cap;                          // elements written (the stream's total, clipped at the buffer)
    }
}

// The decode scan as two grids (a wave per step of 64 chunks): the one-workgroup form (k_td_scan_wg) is bound by the instruction issue of
// the single CU it runs on (14 us for 16 384 chunks); the scan over the step totals is short enough for every wave to redo.
struct TdStepTotal { uint64_t cnt; uint32_t val, pad; };
__global__ __launch_bounds__(256) void k_td_scan_local(const TdSummary* __restrict__ summ, TdCarry* __restrict__ carry, uint64_t n_chunks,
                                                      TdStepTotal* __restrict__ step_tot)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t st = static_cast<uint64_t>(blockIdx.x) * 4u + (threadIdx.x >> 6);
    const uint64_t c = st * 64u + lane;
    if (st * 64u >= n_chunks) return;
    TdSummary s{0u, 0u};
    if (c < n_chunks) s = summ[c];
    const uint32_t lo = wave_incl_add(s.sum_c & 0xFFFFu), hi = wave_incl_add(s.sum_c >> 16);
    const uint64_t inc = static_cast<uint64_t>(lo) + (static_cast<uint64_t>(hi) << 16);
    const uint32_t vinc = wave_incl_add(s.sum_v);
    if (c < n_chunks) carry[c] = TdCarry{inc - s.sum_c, (vinc - s.sum_v) & 0xFFu, 0u};
    if (lane == 0u) step_tot[st] = TdStepTotal{static_cast<uint64_t>(lane63(lo)) + (static_cast<uint64_t>(lane63(hi)) << 16), lane63(vinc) & 0xFFu, 0u};
}
__global__ __launch_bounds__(256) void k_td_scan_apply(TdCarry* __restrict__ carry, uint64_t n_chunks, const TdStepTotal* __restrict__ step_tot,
                                                      uint64_t cap, uint64_t* __restrict__ out_n)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t st = static_cast<uint64_t>(blockIdx.x) * 4u + (threadIdx.x >> 6);
    const uint64_t n_steps = (n_chunks + 63u) / 64u;
    if (st >= n_steps) return;
    uint64_t cnt = 0;                                               // totals of the steps in front of this one (< 2^25 each)
    uint32_t val = 0;
    for (uint64_t j0 = 0; j0 < st; j0 += 64u) {
        const uint64_t j = j0 + lane;
        if (j < st) { const TdStepTotal t = step_tot[j]; cnt += t.cnt; val += t.val; }
    }
    const uint32_t lo = lane63(wave_incl_add(static_cast<uint32_t>(cnt) & 0xFFFFu)), mid = lane63(wave_incl_add(static_cast<uint32_t>(cnt >> 16) & 0xFFFFu));
    const uint32_t hi = lane63(wave_incl_add(static_cast<uint32_t>(cnt >> 32)));
    const uint64_t before = static_cast<uint64_t>(lo) + (static_cast<uint64_t>(mid) << 16) + (static_cast<uint64_t>(hi) << 32);
    const uint32_t qbefore = lane63(wave_incl_add(val)) & 0xFFu;
    const uint64_t c = st * 64u + lane;
    if (c < n_chunks) {
        const TdCarry mine = carry[c];
        carry[c] = TdCarry{mine.start + before, (mine.q_pre + qbefore) & 0xFFu, 0u};
    }
    if (st + 1u == n_steps && lane == 0u) {
        const TdStepTotal t = step_tot[st];
        const uint64_t total = before + t.cnt;
        carry[n_chunks] = TdCarry{total, (qbefore + t.val) & 0xFFu, 0u};
        *out_n = total < cap ? total : cap;                          // elements written (the stream's total, clipped at the buffer)
    }
}

// The output-centric expand with the run scatter.  k_td_expand (under the banner below) lets a lane write the part of its run that falls into the tile element by element: a tile covered by three
// runs of 700 elements is three lanes storing 700 bytes each.  On tensors that compress (long runs, few pairs) BOTH decoders
// collapse -- the one-pass kernel because its work is cut by PAIRS (a chunk of 2048 pairs is a megabyte of output walked by one
// wave), this one because of that loop: 128 Mi elements at 155 : 1 took 0.67-0.71 ms, 5 % of the roofline.  Here a wave owns 2048
// OUTPUT elements as before, but fills its table the block decoder's way: E[start of run] = value - previous value for the runs
// that start inside the tile (one byte per run), the state in front of the tile (q and the delta of element -1) from the packed
// sums of the pairs in front of it, then two wave scans + eight byte recurrences per 512 elements.  Constant work per tile
// whatever the run lengths.  A tile that meets a zero count (hand-made streams) takes td_tile_general.
template <int MODE, bool F32>
__device__ __noinline__ void td_tile_general(const uint8_t* __restrict__ rle, uint64_t n_pairs, uint64_t i0, uint64_t pos0, uint32_t q0,
                                             uint64_t o0, uint64_t o1, float scale, uint8_t* __restrict__ dst, uint32_t lane)
{
    uint64_t pos = pos0;                                                 // element index of pair i0's first element
    uint32_t qa = q0;
#pragma unroll 1
    for (uint64_t b = i0; b < n_pairs && pos < o1; b += 64u) {
        const uint64_t i = b + lane;
        uint32_t bits = 0;
        if (i < n_pairs) bits = *reinterpret_cast<const uint16_t*>(rle + 2ull * i);
        const uint32_t v = bits & 0xFFu, c = bits >> 8;
        const uint32_t packed = ((v * c) << 24) | c;
        const uint32_t incl = wave_incl_add(packed);
        const uint32_t e = incl - packed;
        uint64_t p = pos + (e & 0xFFFFFFu);
        uint32_t q = qa + (e >> 24);
#pragma unroll 1
        for (uint32_t m = 0; m < c && p < o1; ++m, ++p) {
            q += v;
            if (p < o0) continue;
            const float y = dequant<MODE>(static_cast<int>(static_cast<int8_t>(q & 0xFFu)), scale);
            if (F32) reinterpret_cast<float*>(dst)[p] = y;
            else { float a = y, z = 0.0f; reinterpret_cast<uint16_t*>(dst)[p] = static_cast<uint16_t>(pack_half2(a, z) & 0xFFFFu); }
        }
        const uint32_t tot = lane63(incl);
        pos += tot & 0xFFFFFFu;
        qa = (qa + (tot >> 24)) & 0xFFu;
    }
}
template <int MODE, bool F32>
__global__ __launch_bounds__(256) void k_td_expand_scatter(const uint8_t* __restrict__ rle, uint64_t n_pairs, const TdCarry* __restrict__ carry,
                                                          uint64_t n_chunks, const uint64_t* __restrict__ n_out_p, float scale, uint8_t* __restrict__ dst)
{
    __shared__ __attribute__((aligned(16))) uint8_t tabs[4][kTile + 16];      // (+16: bytes that may be written and are never read)
    __shared__ __attribute__((aligned(16))) uint8_t stage[4][F32 ? 2048 : 16];   // fp32 output: the step's values on their way to whole-KiB stores
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t n_out = *n_out_p;
    const uint64_t o0 = (static_cast<uint64_t>(blockIdx.x) * 4u + wave) * kTile;
    if (o0 >= n_out) return;
    const uint64_t o1 = (n_out - o0 < kTile) ? n_out : o0 + kTile;
    uint8_t* tab = tabs[wave];
    const uint32_t tab_addr = lds_addr_of(tab);
    uint64_t lo = 0, hi = n_chunks;                                      // last chunk whose first element is at or before o0 (64-ary search)
    while (hi - lo > 1u) {
        const uint64_t span = hi - lo, step = (span + 63u) / 64u;
        const uint64_t c = lo + static_cast<uint64_t>(lane + 1u) * step;
        const bool le = c < hi && carry[c].start <= o0;
        const uint32_t kk = static_cast<uint32_t>(__popcll(__ballot(le)));
        const uint64_t nlo = lo + static_cast<uint64_t>(kk) * step, nhi = lo + static_cast<uint64_t>(kk + 1u) * step;
        lo = nlo;
        hi = nhi < hi ? nhi : hi;
    }
    const uint32_t valid = static_cast<uint32_t>(o1 - o0);
    const uint64_t chunk_start = carry[lo].start;
    const uint32_t chunk_q = carry[lo].q_pre;
    int32_t tot = -static_cast<int32_t>(o0 - chunk_start);               // first element of the step's first pair, relative to o0
    uint32_t qm1 = chunk_q;                                               // becomes q[-1]: everything in front of the tile
    uint32_t dm1 = 0u;                                                   // the delta of element -1 (value of the pair that covers it)
    uint32_t tail = 0u;                                                  // the dword of the pair in front of the step's first (value in byte 2)
    if (lo != 0u) {                                                      // (the last pair of the chunk before: it exists and has been read by the summary pass)
        const uint32_t b = *reinterpret_cast<const uint16_t*>(rle + 2ull * (lo * kTile - 1u));
        tail = (b & 0xFFu) << 16;
        dm1 = b & 0xFFu;
        if ((b >> 8) == 0u) { td_tile_general<MODE, F32>(rle, n_pairs, lo * kTile, chunk_start, chunk_q, o0, o1, scale, dst, lane); return; }
    }
    {
        u32x4* t4 = reinterpret_cast<u32x4*>(tab);
        const u32x4 z = {0u, 0u, 0u, 0u};
        t4[lane] = z; t4[64u + lane] = z;
    }
    const bool wide = (reinterpret_cast<uintptr_t>(rle) & 15u) == 0u;
    bool zero_seen = false;
#pragma unroll 1
    for (uint64_t i0 = lo * kTile; i0 < n_pairs && tot < static_cast<int32_t>(valid); i0 += 512u) {
        const uint64_t i = i0 + 8u * lane;
        uint32_t w[4] = {0u, 0u, 0u, 0u};                                // pairs i, i+1 | i+2, i+3 | ... (v | c << 8 | v << 16 | c << 24)
        uint32_t mn = 255u;
        if (wide && i + 8u <= n_pairs) {
            const u32x4 x = *reinterpret_cast<const u32x4*>(rle + 2ull * i);
            w[0] = x.x; w[1] = x.y; w[2] = x.z; w[3] = x.w;
#pragma unroll
            for (int t = 0; t < 4; ++t) mn = umin(mn, umin((w[t] >> 8) & 0xFFu, w[t] >> 24));
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 8u; ++k)
                if (i + k < n_pairs) {
                    const uint32_t bits = *reinterpret_cast<const uint16_t*>(rle + 2ull * (i + k));
                    w[k >> 1] |= bits << (16u * (k & 1u));
                    mn = umin(mn, bits >> 8);
                }
        }
        if (__ballot(mn == 0u) != 0ull) { zero_seen = true; break; }
        uint32_t sc = 0, sv = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const uint32_t counts = (w[t] >> 8) & 0x00FF00FFu;
            sc = __builtin_amdgcn_udot4(counts, 0x00010001u, sc, false);
            sv = __builtin_amdgcn_udot4(w[t], counts, sv, false);
        }
        const uint32_t lt = (sv << 24) | sc;
        const uint32_t incl = wave_incl_add(lt);
        const uint32_t stp = lane63(incl);
        const int32_t step_c = static_cast<int32_t>(stp & 0xFFFFFFu);
        const uint32_t last_dw = lane63(w[3]);
        if (tot + step_c <= 0) {                                         // (wave-uniform) every element of the step lies in front of the tile
            qm1 += stp >> 24;
            if (step_c != 0) dm1 = (last_dw >> 16) & 0xFFu;              // (a full step: its last pair exists and covers the last element so far)
            tot += step_c;
            tail = last_dw;
            continue;
        }
        const uint32_t ex = incl - lt;
        int32_t a = tot + static_cast<int32_t>(ex & 0xFFFFFFu);           // first element of the lane's first pair
        const uint32_t pwj = wave_shr1(w[3], tail);
        const uint32_t dd[8] = {td_sub_b0_b2(w[0], pwj), td_sub_b2_b0(w[0], w[0]), td_sub_b0_b2(w[1], w[0]), td_sub_b2_b0(w[1], w[1]),
                                td_sub_b0_b2(w[2], w[1]), td_sub_b2_b0(w[2], w[2]), td_sub_b0_b2(w[3], w[2]), td_sub_b2_b0(w[3], w[3])};
        if (tot < 0) {
            // the step straddles the tile's first element: what its pairs put IN FRONT of the tile goes into q[-1], and the last
            // pair that starts in front of the tile is the one that covers element -1
            uint32_t qb = 0u, cov = 0u, has = 0u;
            int32_t st_e = a;
#pragma unroll
            for (uint32_t e = 0; e < 8u; ++e) {
                const uint32_t v = (w[e >> 1] >> (16u * (e & 1u))) & 0xFFu, c = (w[e >> 1] >> (8u + 16u * (e & 1u))) & 0xFFu;
                const int32_t nb = st_e < 0 ? ((-st_e) < static_cast<int32_t>(c) ? -st_e : static_cast<int32_t>(c)) : 0;
                qb += v * static_cast<uint32_t>(nb);
                if (st_e < 0 && c != 0u) { cov = v; has = 1u; }
                st_e += static_cast<int32_t>(c);
            }
            qm1 += lane63(wave_incl_add(qb & 0xFFu));
            const unsigned long long hm = __ballot(has != 0u);
            if (hm) dm1 = static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int>(cov), 63 - __builtin_clzll(hm)));
        }
        if (tot >= 0 && tot + step_c <= static_cast<int32_t>(valid)) {      // (wave-uniform) every pair of the step starts inside the tile: plain addresses
            uint32_t ad = tab_addr + static_cast<uint32_t>(a);
            td_lds_b8(ad, dd[0]); ad = td_add_b1(ad, w[0]);
            td_lds_b8(ad, dd[1]); ad = td_add_b3(ad, w[0]);
            td_lds_b8(ad, dd[2]); ad = td_add_b1(ad, w[1]);
            td_lds_b8(ad, dd[3]); ad = td_add_b3(ad, w[1]);
            td_lds_b8(ad, dd[4]); ad = td_add_b1(ad, w[2]);
            td_lds_b8(ad, dd[5]); ad = td_add_b3(ad, w[2]);
            td_lds_b8(ad, dd[6]); ad = td_add_b1(ad, w[3]);
            td_lds_b8(ad, dd[7]);                                         // (pairs behind the stream's end: count 0, they land on the byte behind the last element)
        } else {
#pragma unroll
            for (uint32_t e = 0; e < 8u; ++e) {
                const uint32_t off = static_cast<uint32_t>(a) < valid ? static_cast<uint32_t>(a) : kTile;  // in front of / behind the tile: the spare byte
                td_lds_b8(tab_addr + off, dd[e]);
                a += static_cast<int32_t>((w[e >> 1] >> (8u + 16u * (e & 1u))) & 0xFFu);
            }
        }
        tot += step_c;
        tail = last_dw;
    }
    if (zero_seen) { td_tile_general<MODE, F32>(rle, n_pairs, lo * kTile, chunk_start, chunk_q, o0, o1, scale, dst, lane); return; }
    wave_lds_fence();
    uint32_t c1 = dm1, c2 = qm1;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t p0 = 512u * j + 8u * lane;
        if (512u * j >= valid) break;                                    // (wave-uniform)
        const uint2 x = *reinterpret_cast<const uint2*>(tab + p0);
        const uint32_t t1 = __builtin_amdgcn_sad_u8(x.x, 0u, __builtin_amdgcn_sad_u8(x.y, 0u, 0u));
        const uint32_t t2 = __builtin_amdgcn_udot4(x.x, 0x05060708u, __builtin_amdgcn_udot4(x.y, 0x01020304u, 0u, false), false);
        const uint32_t i1 = wave_incl_add(t1);
        const uint32_t x1 = c1 + i1 - t1;
        const uint32_t u = t2 + 8u * x1;
        const uint32_t i2 = wave_incl_add(u);
        const uint32_t x2 = c2 + i2 - u;
        c1 += lane63(i1);
        c2 += lane63(i2);
        if (!F32 && p0 >= valid) continue;                               // (fp32: the lane may have to store a neighbour's values, below)
        uint32_t s1 = x1, s2 = x2;
        uint32_t q[8];
        s1 = td_add_byte<0>(s1, x.x, x.y); s2 += s1; q[0] = s2;
        s1 = td_add_byte<1>(s1, x.x, x.y); s2 += s1; q[1] = s2;
        s1 = td_add_byte<2>(s1, x.x, x.y); s2 += s1; q[2] = s2;
        s1 = td_add_byte<3>(s1, x.x, x.y); s2 += s1; q[3] = s2;
        s1 = td_add_byte<4>(s1, x.x, x.y); s2 += s1; q[4] = s2;
        s1 = td_add_byte<5>(s1, x.x, x.y); s2 += s1; q[5] = s2;
        s1 = td_add_byte<6>(s1, x.x, x.y); s2 += s1; q[6] = s2;
        s1 = td_add_byte<7>(s1, x.x, x.y); s2 += s1; q[7] = s2;
        float y[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) y[e] = dequant<MODE>(static_cast<int>(static_cast<int8_t>(q[e] & 0xFFu)), scale);
        if (F32) {
            // fp32: a lane's eight values are 32 bytes; stored from the lane, every instruction of the wave would write half of each
            // 64-byte sector (the block decoders lost two thirds of their rate that way: kernels.hip store8_f32).  Through 2 KiB of
            // LDS instead: written per lane, read back 16 bytes x 64 lanes in a row -- one contiguous KiB per store instruction.
            // Piece t of the step (16 bytes) holds half of lane t / 2's group and goes out only if that group is whole.
            typedef float f32x4v __attribute__((ext_vector_type(4)));
            f32x4v* stg = reinterpret_cast<f32x4v*>(stage[wave]);
            wave_lds_fence();
            stg[2u * lane] = f32x4v{y[0], y[1], y[2], y[3]};
            stg[2u * lane + 1u] = f32x4v{y[4], y[5], y[6], y[7]};
            wave_lds_fence();
            const f32x4v a4 = stg[lane], b4 = stg[64u + lane];
            float* ob = reinterpret_cast<float*>(dst) + o0 + 512u * j;
            const uint32_t g0 = 512u * j + 8u * (lane >> 1), g1 = g0 + 256u;       // first element of the groups the two pieces belong to
            if (g0 + 8u <= valid) __builtin_nontemporal_store(a4, reinterpret_cast<f32x4v*>(ob + 4u * lane));
            if (g1 + 8u <= valid) __builtin_nontemporal_store(b4, reinterpret_cast<f32x4v*>(ob + 256u + 4u * lane));
            if (p0 < valid && p0 + 8u > valid)
                for (uint32_t e = 0; e < 8u && p0 + e < valid; ++e) reinterpret_cast<float*>(dst)[o0 + p0 + e] = y[e];
            continue;
        }
        if (p0 + 8u <= valid) {
            {
                const u32x4 pk = {pack_half2(y[0], y[1]), pack_half2(y[2], y[3]), pack_half2(y[4], y[5]), pack_half2(y[6], y[7])};
                __builtin_nontemporal_store(pk, reinterpret_cast<u32x4*>(reinterpret_cast<uint16_t*>(dst) + o0 + p0));
            }
        } else {
            for (uint32_t e = 0; e < 8u && p0 + e < valid; ++e) {
                if (F32) reinterpret_cast<float*>(dst)[o0 + p0 + e] = y[e];
                else { float a2 = y[e], z = 0.0f; reinterpret_cast<uint16_t*>(dst)[o0 + p0 + e] = static_cast<uint16_t>(pack_half2(a2, z) & 0xFFFFu); }
            }
        }
    }
}

// ================================================================ cross-check forms (rounds 2-3): reached through tuning switches only
// The decode scan by one workgroup of 16 waves (see k_tc_scan_wg, tensor_compress.hip; up to kScanMaxSteps x 64 chunks of 2048 pairs).
__global__ __launch_bounds__(64 * kScanWaves) void k_td_scan_wg(const TdSummary* __restrict__ summ, TdCarry* __restrict__ carry, uint64_t n_chunks,
                                                                uint64_t cap, uint64_t* __restrict__ out_n)
{
    __shared__ uint64_t s_cnt[kScanMaxSteps];
    __shared__ uint32_t s_val[kScanMaxSteps];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t n_steps = static_cast<uint32_t>((n_chunks + 63u) / 64u);
    // (a wave's steps are taken eight at a time, their loads issued together: one step after the other the kernel was a chain
    // of load latencies -- 21 us for 16 384 chunks)
    for (uint32_t st0 = wave; st0 < n_steps; st0 += 8u * kScanWaves) {
        TdSummary sb[8];
#pragma unroll
        for (uint32_t u = 0; u < 8u; ++u) {
            const uint64_t c = static_cast<uint64_t>(st0 + u * kScanWaves) * 64u + lane;
            sb[u] = TdSummary{0u, 0u};
            if (st0 + u * kScanWaves < n_steps && c < n_chunks) sb[u] = summ[c];
        }
#pragma unroll
        for (uint32_t u = 0; u < 8u; ++u) {
            const uint32_t st = st0 + u * kScanWaves;
            if (st >= n_steps) break;
            const uint64_t c = static_cast<uint64_t>(st) * 64u + lane;
            const TdSummary s = sb[u];
            const uint32_t lo = wave_incl_add(s.sum_c & 0xFFFFu), hi = wave_incl_add(s.sum_c >> 16);
            const uint64_t inc = static_cast<uint64_t>(lo) + (static_cast<uint64_t>(hi) << 16);
            const uint32_t vinc = wave_incl_add(s.sum_v);
            if (c < n_chunks) carry[c] = TdCarry{inc - s.sum_c, (vinc - s.sum_v) & 0xFFu, 0u};
            if (lane == 0u) {
                s_cnt[st] = static_cast<uint64_t>(lane63(lo)) + (static_cast<uint64_t>(lane63(hi)) << 16);
                s_val[st] = lane63(vinc) & 0xFFu;
            }
        }
    }
    __syncthreads();
    if (wave == 0u) {
        uint64_t start = 0;
        uint32_t qpre = 0;
        for (uint32_t j = 0; j < n_steps; j += 64u) {
            const uint32_t i = j + lane;
            const uint64_t v = i < n_steps ? s_cnt[i] : 0ull;          // <= 64 * 2048 * 255 < 2^25
            const uint32_t q = i < n_steps ? s_val[i] : 0u;
            const uint32_t lo = wave_incl_add(static_cast<uint32_t>(v) & 0xFFFFu), hi = wave_incl_add(static_cast<uint32_t>(v >> 16));
            const uint64_t inc = static_cast<uint64_t>(lo) + (static_cast<uint64_t>(hi) << 16);
            const uint32_t qinc = wave_incl_add(q);
            if (i < n_steps) { s_cnt[i] = start + inc - v; s_val[i] = (qpre + qinc - q) & 0xFFu; }
            start += static_cast<uint64_t>(lane63(lo)) + (static_cast<uint64_t>(lane63(hi)) << 16);
            qpre = (qpre + lane63(qinc)) & 0xFFu;
        }
        if (lane == 0u) {
            carry[n_chunks] = TdCarry{start, qpre, 0u};
            *out_n = start < cap ? start : cap;
        }
    }
    __syncthreads();
    for (uint32_t st0 = wave; st0 < n_steps; st0 += 8u * kScanWaves) {
        TdCarry cb[8];
#pragma unroll
        for (uint32_t u = 0; u < 8u; ++u) {
            const uint64_t c = static_cast<uint64_t>(st0 + u * kScanWaves) * 64u + lane;
            cb[u] = TdCarry{0ull, 0u, 0u};
            if (st0 + u * kScanWaves < n_steps && c < n_chunks) cb[u] = carry[c];
        }
#pragma unroll
        for (uint32_t u = 0; u < 8u; ++u) {
            const uint32_t st = st0 + u * kScanWaves;
            const uint64_t c = static_cast<uint64_t>(st) * 64u + lane;
            if (st < n_steps && c < n_chunks) carry[c] = TdCarry{cb[u].start + s_cnt[st], (cb[u].q_pre + s_val[st]) & 0xFFu, 0u};
        }
    }
}

// Output-centric expand: a wave owns 2048 consecutive output elements.  It finds the chunk of pairs its first element
// lies in, walks the pairs 64 per step (add-scan of (value*count mod 256) << 24 | count gives each run its start and the
// int8 prefix of all earlier deltas), and every lane writes the part of its run that falls into the tile:
//     q[start + m] = prefix + (m + 1) * value  (mod 256)        (cache_engine.cpp:241-273)
// into a 2 KiB byte table; dequantisation and the stores are then one coalesced pass.
template <int MODE, bool F32>
__global__ __launch_bounds__(256) void k_td_expand(const uint8_t* __restrict__ rle, uint64_t n_pairs, const TdCarry* __restrict__ carry,
                                                  uint64_t n_chunks, const uint64_t* __restrict__ n_out_p, float scale, uint8_t* __restrict__ dst)
{
    __shared__ __attribute__((aligned(16))) uint8_t tabs[4][kTile];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t n_out = *n_out_p;
    const uint64_t o0 = (static_cast<uint64_t>(blockIdx.x) * 4u + wave) * kTile;
    if (o0 >= n_out) return;
    const uint64_t o1 = (n_out - o0 < kTile) ? n_out : o0 + kTile;
    uint8_t* tab = tabs[wave];
    // last chunk whose first element is at or before o0 (chunks that emit nothing share their successor's start), found by the
    // whole wave at once: 64 probes per step of a 64-ary search (3 steps for 16 384 chunks; a binary search was 14 dependent
    // loads in front of everything else the wave does)
    uint64_t lo = 0, hi = n_chunks;                                 // carry[n_chunks].start = total > o0; start is non-decreasing
    while (hi - lo > 1u) {
        const uint64_t span = hi - lo, step = (span + 63u) / 64u;
        const uint64_t c = lo + static_cast<uint64_t>(lane + 1u) * step;
        const bool le = c < hi && carry[c].start <= o0;
        const uint32_t kk = static_cast<uint32_t>(__popcll(__ballot(le)));
        const uint64_t nlo = lo + static_cast<uint64_t>(kk) * step, nhi = lo + static_cast<uint64_t>(kk + 1u) * step;
        lo = nlo;
        hi = nhi < hi ? nhi : hi;
    }
    // positions relative to the tile from here on (32-bit): the chunk starts at or before o0, by less than 2048 x 255 elements
    const int32_t valid_i = static_cast<int32_t>(o1 - o0);
    int32_t tot = -static_cast<int32_t>(o0 - carry[lo].start);       // elements in front of pair `i0`, relative to o0
    uint32_t qp = carry[lo].q_pre;
    // eight pairs per lane and step (one 16-byte load where the stream is aligned): a lane sums its own eight, one add-scan over
    // the lane totals places them
    const bool wide = (reinterpret_cast<uintptr_t>(rle) & 15u) == 0u;
#pragma unroll 1
    for (uint64_t i0 = lo * kTile; i0 < n_pairs && tot < valid_i; i0 += 512u) {
        const uint64_t i = i0 + 8u * lane;
        uint32_t w[4] = {0u, 0u, 0u, 0u};                              // pairs i, i+1 | i+2, i+3 | ...
        if (wide && i + 8u <= n_pairs) {
            const u32x4 x = *reinterpret_cast<const u32x4*>(rle + 2ull * i);
            w[0] = x.x; w[1] = x.y; w[2] = x.z; w[3] = x.w;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 8u; ++k)
                if (i + k < n_pairs) w[k >> 1] |= static_cast<uint32_t>(*reinterpret_cast<const uint16_t*>(rle + 2ull * (i + k))) << (16u * (k & 1u));
        }
        uint32_t sc = 0, sv = 0;                                       // the lane's counts and value x count sums (dword = v0 | c0 << 8 | v1 << 16 | c1 << 24)
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const uint32_t counts = (w[t] >> 8) & 0x00FF00FFu;
            sc = __builtin_amdgcn_udot4(counts, 0x00010001u, sc, false);
            sv = __builtin_amdgcn_udot4(w[t], counts, sv, false);
        }
        const uint32_t lane_total = (sv << 24) | sc;                   // counts: < 2^24 per step, the value sums wrap mod 256
        const uint32_t incl = wave_incl_add(lane_total);
        const uint32_t e = incl - lane_total;
        int32_t start = tot + static_cast<int32_t>(e & 0xFFFFFFu);
        uint32_t q = qp + (e >> 24);
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) {
            const uint32_t bits = (w[k >> 1] >> (16u * (k & 1u))) & 0xFFFFu;
            const uint32_t v = bits & 0xFFu;
            const int32_t c = static_cast<int32_t>(bits >> 8);
            // the part of [start, start + c) inside [0, valid): the run's first element by itself (data that does not compress
            // is runs of one: no loop, no bounds arithmetic), the rest of a longer run in a loop
            if (c != 0) {
                if (static_cast<uint32_t>(start) < static_cast<uint32_t>(valid_i)) tab[start] = static_cast<uint8_t>(q + v);
                if (c > 1) {
                    const int32_t a0 = start + 1 > 0 ? start + 1 : 0, bnd = (start + c < valid_i) ? start + c : valid_i;
                    uint32_t qq = q + static_cast<uint32_t>(a0 - start) * v;
#pragma unroll 1
                    for (int32_t p = a0; p < bnd; ++p) { qq += v; tab[p] = static_cast<uint8_t>(qq); }
                }
            }
            start += c;
            q += v * static_cast<uint32_t>(c);
        }
        const uint32_t step_tot = lane63(incl);
        tot += static_cast<int32_t>(step_tot & 0xFFFFFFu);
        qp = (qp + (step_tot >> 24)) & 0xFFu;
    }
    wave_lds_fence();
    const uint32_t valid = static_cast<uint32_t>(o1 - o0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t p0 = 512u * j + 8u * lane;
        if (p0 >= valid) continue;
        const uint2 x = *reinterpret_cast<const uint2*>(tab + p0);
        float y[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t b = ((k < 4 ? x.x : x.y) >> ((k & 3) * 8)) & 0xFFu;
            y[k] = dequant<MODE>(static_cast<int>(static_cast<int8_t>(b)), scale);
        }
        if (p0 + 8u <= valid) {
            if (F32) {
                float* o = reinterpret_cast<float*>(dst) + o0 + p0;
                *reinterpret_cast<float4*>(o) = make_float4(y[0], y[1], y[2], y[3]);
                *reinterpret_cast<float4*>(o + 4) = make_float4(y[4], y[5], y[6], y[7]);
            } else {
                *reinterpret_cast<uint4*>(reinterpret_cast<uint16_t*>(dst) + o0 + p0) =
                    make_uint4(pack_half2(y[0], y[1]), pack_half2(y[2], y[3]), pack_half2(y[4], y[5]), pack_half2(y[6], y[7]));
            }
        } else {
            for (uint32_t k = 0; k < 8u && p0 + k < valid; ++k) {
                if (F32) reinterpret_cast<float*>(dst)[o0 + p0 + k] = y[k];
                else { float a = y[k], z = 0.0f; reinterpret_cast<uint16_t*>(dst)[o0 + p0 + k] = static_cast<uint16_t>(pack_half2(a, z) & 0xFFFFu); }
            }
        }
    }
}
} // namespace

size_t tensor_decompress_workspace_bytes(uint64_t rle_bytes)
{
    const uint64_t chunks = ((rle_bytes >> 1) + kTile - 1) / kTile;
    return align_up(chunks * sizeof(TdSummary), 256) + align_up((chunks + 1) * sizeof(TdCarry), 256) + 256 + align_up(((chunks + 63) / 64) * 16, 256);   // (the last: step totals of the two-grid scan)
}
hipError_t launch_tensor_decompress(const uint8_t* d_rle, uint64_t rle_bytes, float scale, void* d_dst, uint64_t dst_cap, bool out_f32,
                                    uint64_t* d_n_out, void* d_ws, size_t ws_bytes, int quant_mode, hipStream_t s)
{
    if (ws_bytes < tensor_decompress_workspace_bytes(rle_bytes) || (reinterpret_cast<uintptr_t>(d_ws) & 255u)) return hipErrorInvalidValue;
    const uint64_t n_pairs = rle_bytes >> 1;                         // an odd trailing byte is dropped (cache_engine.cpp:245)
    const uint64_t chunks = (n_pairs + kTile - 1) / kTile;
    uint8_t* w = static_cast<uint8_t*>(d_ws);
    TdSummary* summ = reinterpret_cast<TdSummary*>(w); w += align_up(chunks * sizeof(TdSummary), 256);
    TdCarry* carry = reinterpret_cast<TdCarry*>(w); w += align_up((chunks + 1) * sizeof(TdCarry), 256);
    uint64_t* n_out = d_n_out ? d_n_out : reinterpret_cast<uint64_t*>(w);
    // Which form: the one-pass kernel cuts the work by PAIRS (a chunk of 2048 pairs per wave) -- right for data that does not
    // compress, but ONE wave per megabyte of output wherever the data does: a stream that is noise with a tail of zero padding
    // leaves a few dozen waves walking hundreds of windows each.  The multi-launch form cuts the work by OUTPUT (2048 elements per
    // wave, constant work per tile whatever the run lengths: k_td_expand_scatter) and pays a summary pass over the stream for it:
    // 20 % behind the one-pass kernel on runs of 4, five times ahead of it on a tensor that is one third noise and two thirds long
    // runs (profiles/r04_long_runs.txt).  So: one pass only for streams that are practically incompressible (at most 1.02 elements
    // per pair), by output otherwise.  SPECKV_TC_MULTIPASS=1 / SPECKV_TD_ONE_PASS=1 force a form (tests, A/B).
    const bool few_pairs = n_pairs * 51u < std::min<uint64_t>(dst_cap, n_pairs * 255u) * 50u;
    const Tuning& tn = tuning();
    if (chunks && dst_cap && !tn.tc_multipass && (!few_pairs || tn.td_one_pass)) {
        // single pass: a memset node (ticket, element count, one status word per workgroup), then ONE kernel
        const uint64_t wgs = (chunks + kTdfChunks - 1) / kTdfChunks;
        uint32_t* ticket = reinterpret_cast<uint32_t*>(d_ws);
        uint64_t* n_out1 = d_n_out ? d_n_out : reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(d_ws) + 128);
        uint64_t* status = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(d_ws) + 256);
        if (const hipError_t e = hipMemsetAsync(d_ws, 0, 256 + wgs * 8, s); e != hipSuccess) return e;
        by_mode_f32(quant_mode, out_f32, [&](auto mode, auto f32) { hipLaunchKernelGGL((k_td_fused<mode(), f32()>), dim3(static_cast<uint32_t>(wgs)), dim3(64 * kTdfWaves), 0, s, d_rle, n_pairs,
                                                                                       chunks, status, ticket, dst_cap, n_out1, scale, static_cast<uint8_t*>(d_dst)); });
        return hipGetLastError();
    }
    if (chunks) hipLaunchKernelGGL(k_td_summary, dim3(static_cast<uint32_t>((chunks + 3) / 4)), dim3(256), 0, s, d_rle, n_pairs, summ);
    const uint64_t n_steps = (chunks + 63) / 64;
    if (chunks == 0 || tn.tc_scan == 2) hipLaunchKernelGGL(k_td_scan, dim3(1), dim3(64), 0, s, summ, carry, chunks, dst_cap, n_out);
    else if (tn.tc_scan == 1 && n_steps <= kScanMaxSteps) hipLaunchKernelGGL(k_td_scan_wg, dim3(1), dim3(64 * kScanWaves), 0, s, summ, carry, chunks, dst_cap, n_out);
    else {
        TdStepTotal* step_tot = reinterpret_cast<TdStepTotal*>(w + 256);
        const uint32_t g = static_cast<uint32_t>((n_steps + 3) / 4);
        hipLaunchKernelGGL(k_td_scan_local, dim3(g), dim3(256), 0, s, summ, carry, chunks, step_tot);
        hipLaunchKernelGGL(k_td_scan_apply, dim3(g), dim3(256), 0, s, carry, chunks, step_tot, dst_cap, n_out);
    }
    if (chunks && dst_cap) {
        // grid: the output can hold at most min(dst_cap, 255 * n_pairs) elements; waves behind the stream's total return at once
        const uint64_t max_out = std::min<uint64_t>(dst_cap, n_pairs * 255u);
        const uint32_t g = static_cast<uint32_t>(((max_out + kTile - 1) / kTile + 3) / 4);
        by_mode_f32(quant_mode, out_f32, [&](auto mode, auto f32) {
            if (tn.td_expand_per_element) hipLaunchKernelGGL((k_td_expand<mode(), f32()>), dim3(g), dim3(256), 0, s, d_rle, n_pairs, carry, chunks, n_out, scale, static_cast<uint8_t*>(d_dst));
            else hipLaunchKernelGGL((k_td_expand_scatter<mode(), f32()>), dim3(g), dim3(256), 0, s, d_rle, n_pairs, carry, chunks, n_out, scale, static_cast<uint8_t*>(d_dst));
        });
    }
    return hipGetLastError();
}

// Many streams per launch (workspace and descriptors: launch_tensors_compress, tensor_compress.hip): a status word per (stream, workgroup)
hipError_t launch_tensors_decompress(uint32_t n_tensors, const TensorDesc* d_desc, uint64_t max_elems, const uint64_t* d_rle_bytes, const float* d_scales, bool out_f32,
                                     uint64_t* d_n_out, void* d_ws, size_t ws_bytes, int quant_mode, hipStream_t s)
{
    if (n_tensors == 0) return hipSuccess;
    const TcbDesc* dd = reinterpret_cast<const TcbDesc*>(d_desc);
    const uint64_t wpt = tensors_wpt(max_elems, kTdmChunks);
    if (wpt == 1 || tuning().tc_batch_one_wg) {
        by_mode_f32(quant_mode, out_f32, [&](auto mode, auto f32) { hipLaunchKernelGGL((k_tdb_fused<mode(), f32()>), dim3(n_tensors), dim3(64 * kTdmWaves), 0, s, dd, d_rle_bytes, d_scales, d_n_out); });
        return hipGetLastError();
    }
    if (!d_ws || ws_bytes < tensors_workspace_bytes(n_tensors, max_elems) || (reinterpret_cast<uintptr_t>(d_ws) & 255u) || n_tensors * wpt > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (const hipError_t e = hipMemsetAsync(d_ws, 0, 256 + n_tensors * wpt * 8ull, s); e != hipSuccess) return e;
    uint32_t* ticket = static_cast<uint32_t*>(d_ws);
    uint64_t* status = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(d_ws) + 256);
    const uint32_t g = static_cast<uint32_t>(n_tensors * wpt), w = static_cast<uint32_t>(wpt);
    by_mode_f32(quant_mode, out_f32, [&](auto mode, auto f32) { hipLaunchKernelGGL((k_tdm_fused<mode(), f32()>), dim3(g), dim3(64 * kTdmWaves), 0, s, dd, w, ticket, status, d_rle_bytes, d_scales, d_n_out); });
    return hipGetLastError();
}

} // namespace speckv
