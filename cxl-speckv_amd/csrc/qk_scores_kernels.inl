// cxl-speckv_amd/csrc/qk_scores_kernels.inl -- the two stand-alone attention helpers over FP8_E4M3 records: k_quantize_q_e4m3 and
// k_qk_scores_fp8 (q.K^T alone, through the page table), and their launchers.  The fused kernels are in attend.hip.
//
// A section of the translation unit kernels.hip, which includes it inside namespace speckv at the place where the text stood (why
// it is not a translation unit of its own yet: see there).  As one it would need
//   kernels.hpp         PageEntry, kBlockElems and the launch declarations
//   attend_device.hpp   f32x4, pack64
//   codec_device.hpp    half_bits_to_float, wave_lds_fence
// and nothing of kernels.hip itself.

namespace {

// ===================================================================
// fused dequant-matvec (BASELINE config 5): q.K^T from FP8 records on the matrix cores
// ===================================================================
// per query row: scale = max|q|/448 (1 if zero), e4m3 bytes of clamp(q/scale); rows >= g are zero
__global__ __launch_bounds__(64) void k_quantize_q_e4m3(const uint16_t* __restrict__ q16, uint32_t g,
                                                        uint32_t d, uint8_t* __restrict__ q8,
                                                        float* __restrict__ qs)
{
    // blockIdx.x runs over (layer, head, row): q16 is [layers][heads][g][d], q8 [layers][heads][16][d]
    const uint32_t lane = threadIdx.x, h = blockIdx.x / 16u, m = blockIdx.x % 16u;
    uint8_t* out = q8 + (static_cast<uint64_t>(h) * 16u + m) * d;
    if (m >= g) {
        for (uint32_t i = lane; i < d; i += 64u) out[i] = 0;
        if (lane == 0) qs[h * 16u + m] = 1.0f;
        return;
    }
    const uint16_t* row = q16 + (static_cast<uint64_t>(h) * g + m) * d;
    float mx = 0.0f;
    for (uint32_t i = lane; i < d; i += 64u) { const float a = fabsf(half_bits_to_float(row[i])); mx = (a > mx) ? a : mx; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const float t = __shfl_xor(mx, o); mx = (t > mx) ? t : mx; }
    const float sc = (mx > 0.0f) ? (mx / 448.0f) : 1.0f;
    for (uint32_t i = lane; i < d; i += 64u) {
        const float v = fminf(fmaxf(half_bits_to_float(row[i]) / sc, -448.0f), 448.0f);
        out[i] = static_cast<uint8_t>(__builtin_amdgcn_cvt_pk_fp8_f32(v, 0.0f, 0, false) & 0xFF);
    }
    if (lane == 0) qs[h * 16u + m] = sc;
}

// One wave = 8 pages = 16 positions, all 8 kv heads, K tile staged in LDS.
//   * fetch: the 16 KiB tile goes pool -> LDS with 16 global_load_lds_dwordx4 (1 KiB
//     each, no VGPRs); instruction i brings the row block of position i (8 heads x
//     128 B).  Whole 128-byte lines per instruction, pages read exactly once.
//   * LDS image: row block i sits at i*1024; its 16-byte chunks are XOR-swizzled with
//     i ON THE SOURCE SIDE (lane l fetches chunk l^i), because the MFMA reader walks
//     16 row blocks at the same in-row offset (1 KiB stride = one bank otherwise).
//   * MFMA 16x16x32 fp8: lane (c = l%16, kb = l/16) feeds 8 consecutive d of query
//     row c (A) / position c (B); the d axis is permuted so lane kb owns
//     d in [32kb, 32kb+32) -> two ds_read_b64 per 16-byte chunk.
__global__ __launch_bounds__(128) void k_qk_scores_fp8(const PageEntry* __restrict__ entries,
        uint64_t first_page, uint64_t layer_page_stride, uint32_t n_pages, uint32_t heads, uint32_t g,
        const uint8_t* __restrict__ q8, const float* __restrict__ qs, float* __restrict__ out)
{
    __shared__ __attribute__((aligned(1024))) uint8_t tiles[2][16384];
    // blockIdx.y = layer (several layers of one sequence in one launch)
    first_page += blockIdx.y * layer_page_stride;
    q8 += static_cast<uint64_t>(blockIdx.y) * heads * 16u * 128u;
    qs += static_cast<uint64_t>(blockIdx.y) * heads * 16u;
    out += static_cast<uint64_t>(blockIdx.y) * heads * g * 2u * n_pages;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t page0 = (blockIdx.x * 2u + wave) * 8u;            // wave-uniform
    if (page0 >= n_pages) return;
    uint8_t* tile = tiles[wave];
    const uint32_t n_pos = 2u * n_pages;
    // ---- fetch: 8 pages x 2 positions, descriptors through the scalar cache
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t pg = page0 + j;
        PageEntry e{0, 0, 0.0f};
        if (pg < n_pages) e = entries[first_page + pg];
        const bool ok = pg < n_pages && e.rec_bytes >= kBlockElems;       // wave-uniform
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) {
            const int i = 2 * j + sl;
            if (ok) {
                const uint8_t* src = reinterpret_cast<const uint8_t*>(e.pool_addr) + sl * 1024 + ((lane ^ i) * 16u);
                __builtin_amdgcn_global_load_lds(
                    (const __attribute__((address_space(1))) void*)(src),
                    (__attribute__((address_space(3))) void*)(tile + i * 1024), 16, 0, 0);
            } else {
                *reinterpret_cast<uint4*>(tile + i * 1024 + lane * 16u) = make_uint4(0u, 0u, 0u, 0u);
            }
        }
    }
    const uint32_t c = lane & 15u, kb = lane >> 4;
    const uint32_t pgc = page0 + (c >> 1);
    const bool live = pgc < n_pages;
    float ks = 0.0f;
    if (live) {
        const PageEntry ec = entries[first_page + pgc];
        ks = ec.rec_bytes >= kBlockElems ? ec.scale : 0.0f;
    }
    // query operands and row scales of all 8 heads: requested while the tile is in flight
    uint4 a0[8], a1[8];
    f32x4 qsc[8];
#pragma unroll
    for (int h = 0; h < 8; ++h) {
        const uint8_t* qrow = q8 + (static_cast<uint64_t>(h) * 16u + c) * 128u + kb * 32u;
        a0[h] = *reinterpret_cast<const uint4*>(qrow);
        a1[h] = *reinterpret_cast<const uint4*>(qrow + 16);
        qsc[h] = *reinterpret_cast<const f32x4*>(qs + h * 16u + 4u * kb);
    }
    const uint32_t t = page0 * 2u + c;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                    // DMA landed, operands loaded
    wave_lds_fence();
#pragma unroll
    for (int h = 0; h < 8; ++h) {
        // B: chunks h*8 + kb*2 (+1) of row block c, at their swizzled place
        const uint32_t q0 = (static_cast<uint32_t>(h) * 8u + kb * 2u) ^ c, q1 = (static_cast<uint32_t>(h) * 8u + kb * 2u + 1u) ^ c;
        const uint2 b00 = *reinterpret_cast<const uint2*>(tile + c * 1024u + q0 * 16u);
        const uint2 b01 = *reinterpret_cast<const uint2*>(tile + c * 1024u + q0 * 16u + 8u);
        const uint2 b10 = *reinterpret_cast<const uint2*>(tile + c * 1024u + q1 * 16u);
        const uint2 b11 = *reinterpret_cast<const uint2*>(tile + c * 1024u + q1 * 16u + 8u);
        f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
        acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(pack64(a0[h].x, a0[h].y), pack64(b00.x, b00.y), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(pack64(a0[h].z, a0[h].w), pack64(b01.x, b01.y), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(pack64(a1[h].x, a1[h].y), pack64(b10.x, b10.y), acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x32_fp8_fp8(pack64(a1[h].z, a1[h].w), pack64(b11.x, b11.y), acc, 0, 0, 0);
        // accumulator: lane holds rows m = 4*kb + i (i = 0..3) of column c
        if (live) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const uint32_t m = 4u * kb + i;
                if (m < g) out[(static_cast<uint64_t>(h) * g + m) * n_pos + t] = acc[i] * ks * qsc[h][i];
            }
        }
    }
}

} // namespace

hipError_t launch_quantize_q_e4m3(const void* d_q_f16, uint32_t heads, uint32_t g, uint32_t d,
                                  uint8_t* d_q8, float* d_qs, hipStream_t s)
{
    if (heads == 0 || g == 0 || g > 16u || d != 128u) return hipErrorInvalidValue;
    // `heads` may be layers*heads: rows are independent
    hipLaunchKernelGGL(k_quantize_q_e4m3, dim3(heads * 16u), dim3(64), 0, s,
                       static_cast<const uint16_t*>(d_q_f16), g, d, d_q8, d_qs);
    return hipGetLastError();
}

hipError_t launch_qk_scores_fp8(const PageEntry* d_entries, uint64_t first_page, uint64_t layer_page_stride,
                                uint32_t n_layers, uint32_t n_pages, uint32_t heads, uint32_t g,
                                const uint8_t* d_q8, const float* d_qs, float* d_out, hipStream_t s)
{
    if (n_pages == 0 || n_layers == 0) return hipSuccess;
    const uint32_t waves = (n_pages + 7u) / 8u;
    hipLaunchKernelGGL(k_qk_scores_fp8, dim3((waves + 1u) / 2u, n_layers), dim3(128), 0, s, d_entries, first_page,
                       layer_page_stride, n_pages, heads, g, d_q8, d_qs, d_out);
    return hipGetLastError();
}
