// cxl-speckv_amd/csrc/attend_mx4_device.hpp -- what the kernels over MXFP4 pool records share (attend_mx4.hip: k_attend_mx4; attend_mx4_spec.hip:
// k_attend_mx4_spec): the workgroup and stage geometry of the LDS-DMA pipeline, a region's share of a tile as one statement, the vmcnt
// waits, and the query element as the MX conversion sees it.  The record, the operand maps and the reasons stand at the head of
// attend_mx4.hip; the text below moved here from there unchanged.  Device code only.
#pragma once
#include "kernels.hpp"
#include "attend_device.hpp"

#ifndef MX4_CODES_POLICY
#define MX4_CODES_POLICY ""        // the 64 bytes of codes of a record are read by all four waves of the workgroup: default cache policy (the rows: nt)
#endif

namespace speckv {

typedef int v8i __attribute__((ext_vector_type(8)));

namespace {

// Records in the pool are tile-planar (kernels.hpp): 16 records of a run = 16 nibble rows (1024 B each) + 16 code rows (64 B each)
// = 136 whole cache lines.  A 16-page tile of the kernel that starts at record R of its run reads rows R .. R+15; with R a multiple
// of 16 (every tile-aligned range of a layout whose regions are multiples of 16 pages) that is ONE storage tile: the ten 1 KiB
// requests below touch exactly its 136 lines, and nothing else (round 5's 1152-byte slots: 144).  Any other phase R % 16 works
// too: rows past the storage tile's 16th continue in the next one (lane offsets + one tile's codes, tile_offsets).
constexpr uint32_t kWavesPerWg = 4;                          // two heads per wave: a workgroup covers the 8 kv heads -- the four waves that read a
                                                             // record's 64 bytes of codes then sit on one CU (one L2): measured with two workgroups per
                                                             // record, each code line came from HBM up to four times (profiles/r05_mx4.txt)
// per wave and stage: K rows [16 pages][256 B] | V rows [16 pages][256 B] | K codes [16][16 B] | V codes [16][16 B]
constexpr uint32_t kStK = 0, kStV = 4096, kStKC = 8192, kStVC = 8448, kStage = 8704;
#ifndef MX4_STAGES
#define MX4_STAGES 3          // (2: two workgroups per CU fit; measured 0.71-0.75 of the HBM roofline against 0.73-0.77 with 3 and one workgroup per CU)
#endif
constexpr uint32_t kStagesDefault = MX4_STAGES;              // tiles a wave keeps in LDS: the one it works on and kStages - 1 on their way
constexpr uint32_t kTabEnt = 2u * 512u;                      // page-table form: the 32 entries (16 K pages, 16 V pages) of a tile, for the two tiles ahead

// a region's share of a tile in one statement: four 1 KiB pieces of rows + the codes; M0 saved and restored once
__device__ __forceinline__ void dma_region(uint32_t lds_rows, uint32_t lds_codes, const uint8_t* base, const uint32_t (&goff)[4], uint32_t goffc)
{
    uint32_t keep;
    asm volatile("s_mov_b32 %0, m0\n\t"
                 "s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %3, %8 nt\n\t"
                 "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %4, %8 nt\n\t"
                 "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %5, %8 nt\n\t"
                 "s_add_u32 m0, m0, 0x400\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %6, %8 nt\n\t"
                 "s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dword %7, %8" MX4_CODES_POLICY "\n\t"
                 "s_mov_b32 m0, %0"
                 : "=&s"(keep) : "s"(lds_rows), "s"(lds_codes), "v"(goff[0]), "v"(goff[1]), "v"(goff[2]), "v"(goff[3]), "v"(goffc), "s"(base) : "memory", "scc");
}
template <uint32_t N> __device__ __forceinline__ void wait_all_but()
{
    static_assert(N == 15u || N == 25u, "vmcnt immediate");
    if (N == 15u) asm volatile("s_waitcnt vmcnt(15)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(25)" ::: "memory");
}
// an fp16 query element as the MX conversion sees it: NaN counts as 0, inf as 65504 (oracle: orc_quantize_rows_mxfp8)
__device__ __forceinline__ float q_clean(uint32_t half_bits)
{
    const float x = static_cast<float>(__builtin_bit_cast(_Float16, static_cast<uint16_t>(half_bits)));
    return (x == x) ? fminf(fmaxf(x, -65504.0f), 65504.0f) : 0.0f;
}

} // namespace
} // namespace speckv
