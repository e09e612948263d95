// cxl-speckv_amd/csrc/predictor_kernels.inl -- the token predictor: k_lstm_hidden, k_lstm_cell, k_arrange_wout, k_lstm_logits,
// k_softmax_topk, k_softmax_topk_small, k_softmax_topk_merge, k_predict_small, k_predict_small_merge; launch_arrange_wout,
// launch_predict.
//
// A section of the translation unit kernels.hip, which includes it inside namespace speckv at the place where the text stood (why
// it is not a translation unit of its own yet: see there).  As one it would need
//   kernels.hpp         LstmParams, the kPredict* constants, predict_topk_parts and the launch declarations
//   tuning.hpp          tuning().predict_batch_path
//   encode_device.hpp   f32x2 (the typedef alone)
// and nothing of kernels.hip or codec_device.hpp.

namespace {

// ===================================================================
// token predictor  (src/prefetcher/lstm_predictor.cpp:40-188)
// ===================================================================
// The reference's "LSTM" is degenerate: gates fixed at 0.5, recurrent weights unused,
// candidate g = sum_j 0.1*embedding[token][j] (lstm_predictor.cpp:117-146).  These
// kernels compute exactly that maths for a batch of 16-token histories, then the
// 128 x vocab output mat-vec, softmax and top-k.  fp tolerance vs the oracle: the
// device tanhf/expf and the reduction order differ from glibc's (tests state 1e-4).
constexpr uint32_t kPredHist = 16, kPredEmb = 64, kPredHidden = 128;
// All-lanes reductions over the wave for the top-k rounds, written for latency (a round is a chain of six exchanges): the
// four steps inside a row of 16 lanes are DPP moves (quad_perm xor 1, xor 2, row_half_mirror, row_mirror: a few clocks each);
// rows 16 apart and the two halves of the wave meet through gfx950's v_permlane16_swap / v_permlane32_swap -- with both operands
// the same register they return the two rows (halves) side by side in every lane, still in the vector ALU.  (ds_swizzle and
// ds_bpermute, two trips through the LDS crossbar per reduction, were most of a one-request prediction: 15.7 us with them.)
template <int CTRL> __device__ __forceinline__ uint32_t tk_dpp(uint32_t v) { return static_cast<uint32_t>(__builtin_amdgcn_update_dpp(0, static_cast<int>(v), CTRL, 0xf, 0xf, false)); }
template <int STEP> __device__ __forceinline__ uint32_t tk_exchange(uint32_t v)
{
    static_assert(STEP < 4, "rows and halves: tk_rows / tk_halves");
    if constexpr (STEP == 0) return tk_dpp<0xB1>(v);                 // quad_perm [1,0,3,2]
    else if constexpr (STEP == 1) return tk_dpp<0x4E>(v);            // quad_perm [2,3,0,1]
    else if constexpr (STEP == 2) return tk_dpp<0x141>(v);           // row_half_mirror: the other quad of each 8
    else return tk_dpp<0x140>(v);                                    // row_mirror: the other 8 of each 16
}
struct TkPair { uint32_t a, b; };                                    // a lane's own value and its partner's (in no particular order)
__device__ __forceinline__ TkPair tk_rows(uint32_t v) { const auto r = __builtin_amdgcn_permlane16_swap(v, v, false, false); return TkPair{r[0], r[1]}; }      // lane ^ 16
__device__ __forceinline__ TkPair tk_halves(uint32_t v) { const auto r = __builtin_amdgcn_permlane32_swap(v, v, false, false); return TkPair{r[0], r[1]}; }    // lane ^ 32
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t k)
{
#define SPECKV_TK_STEP(S) { const uint64_t other = (static_cast<uint64_t>(tk_exchange<S>(static_cast<uint32_t>(k >> 32))) << 32) | tk_exchange<S>(static_cast<uint32_t>(k)); k = other > k ? other : k; }
    SPECKV_TK_STEP(0) SPECKV_TK_STEP(1) SPECKV_TK_STEP(2) SPECKV_TK_STEP(3)
#undef SPECKV_TK_STEP
    {
        const TkPair hi = tk_rows(static_cast<uint32_t>(k >> 32)), lo = tk_rows(static_cast<uint32_t>(k));
        const uint64_t x = (static_cast<uint64_t>(hi.a) << 32) | lo.a, y = (static_cast<uint64_t>(hi.b) << 32) | lo.b;
        k = x > y ? x : y;
    }
    {
        const TkPair hi = tk_halves(static_cast<uint32_t>(k >> 32)), lo = tk_halves(static_cast<uint32_t>(k));
        const uint64_t x = (static_cast<uint64_t>(hi.a) << 32) | lo.a, y = (static_cast<uint64_t>(hi.b) << 32) | lo.b;
        k = x > y ? x : y;
    }
    return k;
}
__device__ __forceinline__ float wave_max_f32(float v)
{
    v = fmaxf(v, __uint_as_float(tk_exchange<0>(__float_as_uint(v))));
    v = fmaxf(v, __uint_as_float(tk_exchange<1>(__float_as_uint(v))));
    v = fmaxf(v, __uint_as_float(tk_exchange<2>(__float_as_uint(v))));
    v = fmaxf(v, __uint_as_float(tk_exchange<3>(__float_as_uint(v))));
    const TkPair r = tk_rows(__float_as_uint(v));
    v = fmaxf(__uint_as_float(r.a), __uint_as_float(r.b));
    const TkPair h = tk_halves(__float_as_uint(v));
    return fmaxf(__uint_as_float(h.a), __uint_as_float(h.b));
}
__device__ __forceinline__ float wave_sum_f32(float v)
{
    v += __uint_as_float(tk_exchange<0>(__float_as_uint(v)));
    v += __uint_as_float(tk_exchange<1>(__float_as_uint(v)));
    v += __uint_as_float(tk_exchange<2>(__float_as_uint(v)));
    v += __uint_as_float(tk_exchange<3>(__float_as_uint(v)));
    const TkPair r = tk_rows(__float_as_uint(v));
    v = __uint_as_float(r.a) + __uint_as_float(r.b);
    const TkPair h = tk_halves(__float_as_uint(v));
    return __uint_as_float(h.a) + __uint_as_float(h.b);
}
// tanh(x) = 1 - 2 / (exp(2x) + 1) on the hardware exponential and reciprocal: absolute error ~1e-7, i.e. 1e-5 relative at the
// |x| ~ 0.01 the reference's cell states have (tests: confidences within 5e-4 of the oracle).  libm's tanhf is ~100 instructions,
// and the recurrence is a chain of 16 x layers x 2 of them.
// exp(x) for the softmax terms (x <= 0): the hardware's exp2 on x log2(e), relative error ~1e-6 at |x| ~ 20 (libm's expf is ~20
// instructions and every logit of every request takes one; tests state 5e-4 on the confidences against the oracle).
__device__ __forceinline__ float pred_fast_exp(float x) { return __builtin_amdgcn_exp2f(x * 1.4426950408889634f); }
__device__ __forceinline__ float pred_fast_tanh(float x)
{
    x = fminf(fmaxf(x, -15.0f), 15.0f);
    const float e = __builtin_amdgcn_exp2f(x * 2.8853900817779268f);         // exp(2x)
    return 1.0f - 2.0f * __builtin_amdgcn_rcpf(e + 1.0f);
}

// one wave per request: lane 0 walks the history; every lane stores 2 of the 128 hidden values
__global__ __launch_bounds__(64) void k_lstm_hidden(const int32_t* __restrict__ hist, uint32_t n,
        const float* __restrict__ emb, uint32_t vocab, uint32_t layers, float* __restrict__ hid)
{
    const uint32_t r = blockIdx.x, lane = threadIdx.x;
    if (r >= n) return;
    // candidate g_t = sum_j 0.1*embedding[token_t][j]: lane j holds entry j of every token's row
    // (16 independent loads in flight), one wave reduction per token
    float g[kPredHist];
#pragma unroll
    for (uint32_t t = 0; t < kPredHist; ++t) {
        const uint32_t tok = static_cast<uint32_t>(hist[r * kPredHist + t]);
        g[t] = (tok < vocab) ? emb[static_cast<uint64_t>(tok) * kPredEmb + lane] * 0.1f : 0.0f;
    }
    float tg[kPredHist];
#pragma unroll
    for (uint32_t t = 0; t < kPredHist; ++t) tg[t] = 0.5f * pred_fast_tanh(wave_sum_f32(g[t]));      // (independent of the chain)
    float h = 0.0f, c = 0.0f;
#pragma unroll
    for (uint32_t t = 0; t < kPredHist; ++t)
        for (uint32_t l = 0; l < layers; ++l) {
            c = 0.5f * c + tg[t];
            h = 0.5f * pred_fast_tanh(c);
        }
    h = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(h)));
    hid[static_cast<uint64_t>(r) * kPredHidden + lane] = h;
    hid[static_cast<uint64_t>(r) * kPredHidden + 64u + lane] = h;
}

// A REAL LSTM cell (the reference's is degenerate, above; SURVEY 8f N1: "semantics must be defined by us"): the standard
// cell with PyTorch's nn.LSTM conventions -- per layer  gates = W_ih x + W_hh h + b  (4 x 128 rows, order i, f, g, o),
// c = sigmoid(f) c + sigmoid(i) tanh(g),  h = sigmoid(o) tanh(c),  h_0 = c_0 = 0, layer l > 0 fed with layer l-1's h of the
// same time step; 16-token history, embedding width 64, hidden width 128.  Output: the top layer's last h.
//   A prediction is a chain of 16 x layers dependent steps, so the kernel is written for the length of a step, layer by layer:
//   * one workgroup = one request, 512 threads (256 requests = one workgroup per CU);
//   * the layer's input projections W_ih x_t + b of ALL 16 steps have no dependency: computed first, into LDS;
//   * a thread keeps, in 128 registers for the 16 recurrent steps, the weights of EIGHT gate rows over an eighth of the
//     columns (lstm_arranged_index; the host arranged them so that the 512 threads read coalesced).  A step is 64
//     packed fused multiply-adds per thread (v_pk_fma_f32 over two neighbouring columns) against its 16 values of h -- four
//     16-byte LDS reads -- then a reduction over the eight threads that share the rows (7 exchanges: DPP inside a quad,
//     ds_swizzle across, after which thread tid owns gate row tid);
//   * the kernel numbers gate rows 4 * unit + gate, so the four gates of a hidden unit end in the four lanes of a quad: each
//     lane applies its gate's non-linearity (tanh as 2 sigmoid(2x) - 1: one code path), the quad exchanges the four results
//     with DPP, and all four lanes carry c (in a register) and h; lane 0 writes h -- to the layer's output sequence, which
//     is also where the next step reads it, so a step has ONE barrier and no buffer is ever rewritten while it is read.
//   The forms before this one: a thread owning ONE whole gate row read all of h, 64 16-byte LDS reads per step and wave; the
//   LDS returns 128 bytes per clock however many lanes ask for the same word, so a step was 8 waves x 64 reads x 8 clocks =
//   1.7 us of LDS time against 0.4 us of arithmetic (0.083 ms per prediction; with separate multiply and add,
//   -ffp-contract=off as the reference's cell needs, 0.110-0.117 ms).  Sliced rows with the non-linearities on 256 threads
//   between two barriers (libm tanhf, IEEE division): 0.070 ms.  First version (weights streamed from L2 in every step,
//   8 requests per workgroup): 0.7-0.8 ms per prediction of 256 requests.
struct LstmWeights { const float* w_ih_t[4]; const float* w_hh_t[4]; const float* bias[4]; uint32_t layers; };   // bias = b_ih + b_hh
constexpr uint32_t kLstmPitch = kPredHidden + 4u * (kPredHidden / 16u);      // a 16-column slice starts 20 floats after the one before: the eight slices a wave reads fall in different banks
__device__ __forceinline__ constexpr uint32_t lstm_pad(uint32_t j) { return j + 4u * (j >> 4); }
__device__ __forceinline__ f32x2 pk_fma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) { return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xf, 0xf, false)); }
__device__ __forceinline__ float lane_xor7(float v) { return dpp_mov<0x141>(v); }    // row_half_mirror: lane 7 - s of each 8 (a DPP move; lane ^ 4 would be a ds_swizzle)
__device__ __forceinline__ float lane_xor2(float v) { return dpp_mov<0x4E>(v); }     // quad_perm [2,3,0,1]
__device__ __forceinline__ float lane_xor1(float v) { return dpp_mov<0xB1>(v); }     // quad_perm [1,0,3,2]
// v[i] of slice-thread s holds a partial sum of gate row 8 * group + (i ^ s): after three exchanges with the threads s ^ 7,
// s ^ 2, s ^ 1 the return value is the whole sum of row 8 * group + s, i.e. of row threadIdx.x.  (First exchange: thread s keeps
// the rows (i ^ s), i < 4; its partner 7 - s = s ^ 7 holds its share of row i ^ s in v[(i ^ s) ^ (s ^ 7)] = v[7 - i].  All three are
// DPP moves: the step of the recurrence has no trip through the LDS crossbar left.)
__device__ __forceinline__ float lstm_reduce8(float (&v)[8])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] += lane_xor7(v[7 - i]);
#pragma unroll
    for (int i = 0; i < 2; ++i) v[i] += lane_xor2(v[i + 2]);
    return v[0] + lane_xor1(v[1]);
}
// sum over this thread's CS columns of  w[i][c] * x[c]  for its eight rows i; x: the thread's slice of the input vector
template <uint32_t CS>
__device__ __forceinline__ float lstm_slice_dot(const float (&w)[8u * CS], const float* x)
{
    f32x2 xv[CS / 2u];
#pragma unroll
    for (uint32_t k = 0; k < CS / 4u; ++k) {
        const float4 a = *reinterpret_cast<const float4*>(x + 4u * k);
        xv[2u * k] = f32x2{a.x, a.y}; xv[2u * k + 1u] = f32x2{a.z, a.w};
    }
    float red[8];
#pragma unroll
    for (uint32_t i = 0; i < 8u; ++i) {
        f32x2 a = {0.0f, 0.0f};                                         // (even columns, odd columns)
#pragma unroll
        for (uint32_t k = 0; k < CS / 2u; ++k) a = pk_fma(f32x2{w[i * CS + 2u * k], w[i * CS + 2u * k + 1u]}, xv[k], a);
        red[i] = a.x + a.y;
    }
    return lstm_reduce8(red);
}
template <uint32_t CS>
__device__ __forceinline__ void lstm_project(const float* __restrict__ wsrc, float b, const float (&seq)[kPredHist][kLstmPitch],
                                             float (&xp)[kPredHist][4 * kPredHidden])
{
    const uint32_t tid = threadIdx.x, s = tid & 7u;
    float w[8u * CS];
#pragma unroll
    for (uint32_t q = 0; q < 8u * CS; ++q) w[q] = wsrc[q * 512u + tid];
#pragma unroll 2
    for (uint32_t t = 0; t < kPredHist; ++t) xp[t][tid] = lstm_slice_dot<CS>(w, &seq[t][lstm_pad(CS * s)]) + b;
}
__device__ __forceinline__ float sigmoid_rcp(float x) { return __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(x * -1.4426950408889634f)); }     // the hardware's exp2 and reciprocal (1 ulp each; two of them on every step of the chain)
__global__ __launch_bounds__(512) void k_lstm_cell(const int32_t* __restrict__ hist, uint32_t n, const float* __restrict__ emb, uint32_t vocab,
                                                  LstmWeights w, float* __restrict__ hid)
{
    __shared__ __attribute__((aligned(16))) float seq[kPredHist][kLstmPitch];        // the layer's input sequence, then its own output (columns at lstm_pad)
    __shared__ float xp[kPredHist][4 * kPredHidden];                                // W_ih x_t + b of the current layer; [.][tid] is written and read by thread tid only
    const uint32_t tid = threadIdx.x, req = blockIdx.x, s = tid & 7u;
    const uint32_t unit = tid >> 2, gate = tid & 3u;                      // the gate row this thread owns after a reduction
    for (uint32_t i = tid; i < kPredHist * kPredEmb; i += 512u) {
        const uint32_t t = i / kPredEmb, j = i % kPredEmb;
        const uint32_t tok = static_cast<uint32_t>(hist[req * kPredHist + t]);
        seq[t][lstm_pad(j)] = tok < vocab ? emb[static_cast<uint64_t>(tok) * kPredEmb + j] : 0.0f;
    }
    __syncthreads();
    float h = 0.0f;
    for (uint32_t l = 0; l < w.layers; ++l) {
        const float b = w.bias[l][gate * kPredHidden + unit];
        if (l == 0) lstm_project<kPredEmb / 8u>(w.w_ih_t[l], b, seq, xp);
        else        lstm_project<kPredHidden / 8u>(w.w_ih_t[l], b, seq, xp);
        float wh[kPredHidden];                                            // eight rows x sixteen columns of W_hh
        {
            const float* whp = w.w_hh_t[l] + tid;
#pragma unroll
            for (uint32_t q = 0; q < kPredHidden; ++q) wh[q] = whp[q * 512u];
        }
        float c = 0.0f;
        __syncthreads();                                                  // everybody is done with seq as this layer's input
#pragma unroll 1
        for (uint32_t t = 0; t < kPredHist; ++t) {
            float g = xp[t][tid];
            if (t) g += lstm_slice_dot<kPredHidden / 8u>(wh, &seq[t - 1u][lstm_pad(16u * s)]);      // h_{-1} = 0
            const bool is_g = gate == 2u;
            const float sg = sigmoid_rcp(is_g ? g + g : g);
            const float act = is_g ? sg + sg - 1.0f : sg;                 // tanh(x) = 2 sigmoid(2x) - 1
            const float ai = dpp_mov<0x00>(act), af = dpp_mov<0x55>(act), ag = dpp_mov<0xAA>(act), ao = dpp_mov<0xFF>(act);   // quad_perm [k,k,k,k]
            c = af * c + ai * ag;
            const float sc = sigmoid_rcp(c + c);
            h = ao * (sc + sc - 1.0f);
            if (gate == 0u) seq[t][lstm_pad(unit)] = h;
            __syncthreads();
        }
    }
    if (gate == 0u) hid[static_cast<uint64_t>(req) * kPredHidden + unit] = h;
}

// logits[b][i] = sum_j hid[b][j] * wout[i][j] (+ bias[i]) on the fp32 matrix cores: a wave owns 32 output rows (16 KiB of
// weights, read once and kept in 64 registers) and walks the requests in tiles of 32 with v_mfma_f32_32x32x2_f32 -- the hidden
// vectors are the A operand (M = request), the weights the B operand (N = output row), so that an accumulator register holds
// 32 consecutive logits of one request per half-wave and every store instruction writes two whole 128-byte lines.
// The vector-ALU form this replaces (one quarter-row per lane, multiply and add per weight and request) needed ~80 VALU
// instructions per request and wave, 4 cycles each on a 16-lane SIMD: 0.115 ms for 256 requests against ~0.014 ms of matrix
// time (the instruction runs at 64 cycles back to back also on one accumulator: profiles/tools/probe/mfma_f32_rate.hip, 143-156
// TFLOP/s).  This kernel: 0.030 ms, of which 0.004 the stores and ~0.005 the weights' first read (one request: 0.0066 ms).
// The order of the 128 additions of one logit: k = 8j + 4*(lane/32) + e for j = 0..15, e = 0..3, the lower half-wave's k first
// inside each instruction (fused, unlike the oracle's mul + add: covered by the confidence tolerance of the parity tests).
typedef float f32x16 __attribute__((ext_vector_type(16)));
// tiles of 32 output rows, rounded up to the four waves of a workgroup of k_lstm_logits (every wave loads its tile unconditionally)
__host__ __device__ constexpr uint32_t logits_tiles_padded(uint32_t vocab) { return ((vocab + 31u) / 32u + 3u) & ~3u; }
// The output layer's weights in the order k_lstm_logits reads them: per 32 rows, float4 [j][lane] = row (lane % 32),
// columns 8j + 4 (lane / 32) .. + 3 -- a wave's load instruction is then one contiguous KiB (row-major, its 64 lanes touched
// 64 different lines 16 bytes at a time).  Once per predictor_load.
__global__ __launch_bounds__(256) void k_arrange_wout(const float* __restrict__ src, float4* __restrict__ dst, uint32_t vocab)
{
    const uint32_t lane = threadIdx.x & 63u, tile = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint32_t row = tile * 32u + (lane & 31u), kh = lane >> 5;
    if (tile >= logits_tiles_padded(vocab)) return;         // (tiles past the vocabulary, up to a whole workgroup of k_lstm_logits: zeros)
#pragma unroll
    for (uint32_t j = 0; j < 16u; ++j) {
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < vocab) v = *reinterpret_cast<const float4*>(src + static_cast<uint64_t>(row) * kPredHidden + 8u * j + 4u * kh);
        dst[(static_cast<uint64_t>(tile) * 16u + j) * 64u + lane] = v;
    }
}
constexpr uint32_t kLogitsTile = 32;        // requests per matrix tile
constexpr uint32_t kLogitsChunk = 128;      // requests per workgroup column (blockIdx.y): 2 waves per SIMD at 256 requests x 32 000 rows
constexpr uint32_t kLogitsPitch = kPredHidden + 4u;     // floats; 16 lanes x 16 B of one ds_read_b128 fall in 64 different banks
__global__ __launch_bounds__(256) void k_lstm_logits(const float* __restrict__ hid, uint32_t n,
        const float* __restrict__ wout, const float* __restrict__ out_bias, uint32_t vocab, float* __restrict__ logits)
{
    static_assert(kPredHidden == 128u, "16 float4 per lane and operand");
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t c = lane & 31u, kh = lane >> 5;
    const uint32_t row = (blockIdx.x * 4u + wave) * 32u + c;
    const bool live = row < vocab;
    // the weights arrive arranged (k_arrange_wout): the wave's 32 rows are 16 KiB in a row, [j][lane] float4, rows past the vocabulary zero
    float4 wq[16];
    const float4* wt = reinterpret_cast<const float4*>(wout) + static_cast<uint64_t>(blockIdx.x * 4u + wave) * (16u * 64u) + lane;
#pragma unroll
    for (int j = 0; j < 16; ++j) wq[j] = wt[j * 64];
    const float bias = (out_bias && live) ? out_bias[row] : 0.0f;
    const uint32_t b_begin = blockIdx.y * kLogitsChunk, b_end = min(n, b_begin + kLogitsChunk);
    // A tile of hidden vectors (32 requests, 16 KiB) goes through LDS, shared by the four waves; two buffers, so one barrier
    // per tile: a buffer is rewritten two tiles later, behind the barrier of the tile in between.
    __shared__ __attribute__((aligned(16))) float hs[2][kLogitsTile][kLogitsPitch];
    static_assert(kLogitsTile * kPredHidden / 4u == 4u * 256u, "four float4 per thread and tile");
    float4 nx[4];
    auto fetch = [&](uint32_t b0) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t e = threadIdx.x + 256u * static_cast<uint32_t>(q);
            const uint32_t r = e / (kPredHidden / 4u), c4 = e % (kPredHidden / 4u);
            nx[q] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (b0 + r < b_end) nx[q] = *reinterpret_cast<const float4*>(hid + static_cast<uint64_t>(b0 + r) * kPredHidden + 4u * c4);
        }
    };
    fetch(b_begin);
    uint32_t buf = 0;
    for (uint32_t b0 = b_begin; b0 < b_end; b0 += kLogitsTile, buf ^= 1u) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t e = threadIdx.x + 256u * static_cast<uint32_t>(q);
            *reinterpret_cast<float4*>(&hs[buf][e / (kPredHidden / 4u)][4u * (e % (kPredHidden / 4u))]) = nx[q];
        }
        __syncthreads();
        if (b0 + kLogitsTile < b_end) fetch(b0 + kLogitsTile);
        f32x16 acc;
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[v] = 0.0f;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float4 h4 = *reinterpret_cast<const float4*>(&hs[buf][c][8u * j + 4u * kh]);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(h4.x, wq[j].x, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(h4.y, wq[j].y, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(h4.z, wq[j].z, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(h4.w, wq[j].w, acc, 0, 0, 0);
        }
        // acc[v]: request b0 + 8*(v/4) + 4*(lane/32) + v%4, output row `row`
        if (live) {
            float* o = logits + static_cast<uint64_t>(b0 + 4u * kh) * vocab + row;
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const uint32_t m = 8u * (v >> 2) + (v & 3);
                if (b0 + 4u * kh + m < b_end) o[static_cast<uint64_t>(m) * vocab] = out_bias ? acc[v] + bias : acc[v];
            }
        }
    }
}

// softmax + top-k of one request per workgroup (k <= 8).  Ties: lower token id first.
constexpr uint32_t kSmThreads = 1024;
__global__ __launch_bounds__(1024) void k_softmax_topk(const float* __restrict__ logits, uint32_t vocab,
        uint32_t k, int32_t* __restrict__ out_tok, float* __restrict__ out_conf)
{
    __shared__ float red[kSmThreads];
    __shared__ uint32_t redi[kSmThreads];
    const uint32_t b = blockIdx.x, tid = threadIdx.x;
    const float* l = logits + static_cast<uint64_t>(b) * vocab;
    float val[8];
    uint32_t idx[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) { val[i] = -INFINITY; idx[i] = 0xFFFFFFFFu; }
    float mx = -INFINITY;
    for (uint32_t i = tid; i < vocab; i += kSmThreads) {
        const float v = l[i];
        mx = fmaxf(mx, v);
        // sorted insertion (descending value, ascending index); an absent logit (-inf, NaN) is no candidate
        if (v > -INFINITY && (v > val[7] || (v == val[7] && i < idx[7]))) {
            val[7] = v; idx[7] = i;
#pragma unroll
            for (int j = 7; j > 0; --j) {
                const bool sw = val[j] > val[j - 1] || (val[j] == val[j - 1] && idx[j] < idx[j - 1]);
                if (sw) { const float tv = val[j]; val[j] = val[j - 1]; val[j - 1] = tv;
                          const uint32_t ti = idx[j]; idx[j] = idx[j - 1]; idx[j - 1] = ti; }
            }
        }
    }
    red[tid] = mx; __syncthreads();
    for (uint32_t s = kSmThreads / 2; s > 0; s >>= 1) { if (tid < s) red[tid] = fmaxf(red[tid], red[tid + s]); __syncthreads(); }
    mx = red[0]; __syncthreads();
    float sum = 0.0f;
    for (uint32_t i = tid; i < vocab; i += kSmThreads) { const float v = l[i]; if (v > -INFINITY) sum += expf(v - mx); }     // absent logits add nothing
    red[tid] = sum; __syncthreads();
    for (uint32_t s = kSmThreads / 2; s > 0; s >>= 1) { if (tid < s) red[tid] += red[tid + s]; __syncthreads(); }
    sum = red[0]; __syncthreads();
    uint32_t head = 0;
    for (uint32_t r = 0; r < k; ++r) {
        float cv = -INFINITY; uint32_t ci = 0xFFFFFFFFu;
#pragma unroll
        for (int j = 0; j < 8; ++j) if (static_cast<uint32_t>(j) == head) { cv = val[j]; ci = idx[j]; }
        red[tid] = cv; redi[tid] = ci; __syncthreads();
        for (uint32_t s = kSmThreads / 2; s > 0; s >>= 1) {
            if (tid < s) {
                const float ov = red[tid + s]; const uint32_t oi = redi[tid + s];
                if (ov > red[tid] || (ov == red[tid] && oi < redi[tid])) { red[tid] = ov; redi[tid] = oi; }
            }
            __syncthreads();
        }
        const float bv = red[0]; const uint32_t bi = redi[0];
        __syncthreads();
        if (ci == bi && ci != 0xFFFFFFFFu) ++head;                 // the owner of the winner advances
        if (tid == 0) {
            out_tok[b * k + r] = static_cast<int32_t>(bi);             // no candidate left: 0xFFFFFFFF = -1
            out_conf[b * k + r] = bi != 0xFFFFFFFFu ? expf(bv - mx) / sum : 0.0f;
        }
    }
}

// The same for vocabularies of up to 262 144 tokens (kTkMaxParts parts), written for latency (one request per workgroup is a
// chain of dependent steps: the kernel above took 48-57 us per launch whatever the batch, a 1024-thread workgroup with 32
// logits per thread in registers 21-26 us).  A request is cut into parts of 4096 logits, one workgroup of 256 threads each, 16
// logits per thread:
//   * a wave finds ITS maximum, exp-sum (relative to its own maximum) and top k with shuffles only -- a candidate is one
//     64-bit key, the logit's bits made order-preserving above ~token id, so "value descending, token id ascending" (the
//     order of the sorted insertion above) is an unsigned maximum and a round is six exchange steps;
//   * one barrier, then wave 0 merges the four waves (maxima, rescaled sums, 4 k keys) and writes the part's result;
//   * a second kernel, one wave per request, merges the parts -- a lane holds one part's maximum, sum and k keys (already in
//     order: a round offers the lane's best key not yet taken) -- and writes tokens and confidences exp(logit - max) / sum.  (One kernel whose last-arriving workgroup merges was tried: 10 us for one request, but the
//     agent-scope release/acquire it needs writes back and invalidates the XCD's L2 once per workgroup -- 48 us for 256
//     requests against 26 us before.)
// A logit that is not greater than -inf (-inf or NaN) is ABSENT, in all three top-k forms and in k_predict_small: never chosen ("v > best"
// is false for it, its key is 0), dropped from the maximum (fmaxf) and from the exp-sum (it used to enter the sum, and one NaN logit made
// every confidence of its request NaN); a rank without a candidate reports token -1 and confidence 0.  +inf logits are not handled.
constexpr uint32_t kTkMaxParts = 64, kTkThreads = 256, kTkPer = 16, kTkSpan = kTkThreads * kTkPer;
static_assert(kTkSpan == kPredictTopkSpan && kTkMaxParts == kPredictTopkMaxParts, "predict_ws_bytes");
// workspace of one request: parts x (max, sum) | parts x 8 keys
__device__ __forceinline__ uint32_t tk_ws_stride(uint32_t parts) { return parts * kPredictWsPerPart; }
__device__ __forceinline__ uint64_t tk_key(float v, uint32_t i)
{
    if (!(v > -INFINITY)) return 0;
    uint32_t bits = __float_as_uint(v);
    bits ^= (bits >> 31) ? 0xFFFFFFFFu : 0x80000000u;
    return (static_cast<uint64_t>(bits) << 32) | (0xFFFFFFFFu - i);
}
__device__ __forceinline__ float tk_value(uint64_t key)
{
    uint32_t bits = static_cast<uint32_t>(key >> 32);
    bits ^= (bits >> 31) ? 0x80000000u : 0xFFFFFFFFu;
    return __uint_as_float(bits);
}
// merge of up to 64 (max, sum) pairs and 64 keys held one per lane; k rounds; lane 0 hands every round's winner to `put`
template <typename Put>
__device__ __forceinline__ void tk_merge(float m, float s, uint64_t key, uint32_t k, float& m_all, float& s_all, Put put)
{
    m_all = wave_max_f32(m);
    s_all = wave_sum_f32(m > -INFINITY ? s * pred_fast_exp(m - m_all) : 0.0f);
    for (uint32_t r = 0; r < k; ++r) {
        const uint64_t w = wave_max_u64(key);
        if (w == key) key = 0;                                          // keys are distinct (token ids are): one owner
        put(r, w);
    }
}
__global__ __launch_bounds__(256) void k_softmax_topk_small(const float* __restrict__ logits, uint32_t vocab,
        uint32_t k, uint8_t* __restrict__ ws)
{
    __shared__ float wm[4], wsum[4];
    __shared__ uint64_t wkey[4][8];
    const uint32_t b = blockIdx.x, part = blockIdx.y, tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;      // (requests on x: no 65 535 limit)
    const float* l = logits + static_cast<uint64_t>(b) * vocab;
    const uint32_t base = part * kTkSpan + tid;
    float v[kTkPer];
#pragma unroll
    for (uint32_t j = 0; j < kTkPer; ++j) {
        const uint32_t i = base + j * kTkThreads;
        v[j] = i < vocab ? l[i] : -INFINITY;
    }
    float m = v[0];
#pragma unroll
    for (uint32_t j = 1; j < kTkPer; ++j) m = fmaxf(m, v[j]);
    m = wave_max_f32(m);
    float sum = 0.0f;
#pragma unroll
    for (uint32_t j = 0; j < kTkPer; ++j)
        if (v[j] > -INFINITY) sum += pred_fast_exp(v[j] - m);           // an absent logit (-inf, NaN, past the vocabulary) adds nothing
    sum = wave_sum_f32(sum);
    for (uint32_t r = 0; r < k; ++r) {
        float bv = -INFINITY; int bj = -1;
#pragma unroll
        for (int j = 0; j < static_cast<int>(kTkPer); ++j)                // ascending token id: ">" keeps the lowest id among equals
            if (v[j] > bv) { bv = v[j]; bj = j; }
        const uint64_t key = bj >= 0 ? tk_key(bv, base + static_cast<uint32_t>(bj) * kTkThreads) : 0;
        const uint64_t w = wave_max_u64(key);
        if (w != 0 && w == key) {                                       // the owner retires the winner
#pragma unroll
            for (int j = 0; j < static_cast<int>(kTkPer); ++j) if (j == bj) v[j] = -INFINITY;
        }
        if (lane == 0u) wkey[wv][r] = w;
    }
    if (lane == 0u) { wm[wv] = m; wsum[wv] = sum; }
    __syncthreads();
    if (wv != 0u) return;
    const uint32_t parts = gridDim.y;
    uint8_t* mine = ws + static_cast<uint64_t>(b) * tk_ws_stride(parts);
    float* part_ms = reinterpret_cast<float*>(mine);                     // [part] (max, sum)
    uint64_t* part_key = reinterpret_cast<uint64_t*>(mine + parts * 8u);             // [part][8]
    float pm, ps;
    tk_merge(lane < 4u ? wm[lane] : -INFINITY, lane < 4u ? wsum[lane] : 0.0f, lane < 4u * k ? wkey[lane / k][lane % k] : 0, k, pm, ps,
             [&](uint32_t r, uint64_t w) { if (lane == 0u) part_key[part * 8u + r] = w; });
    if (lane == 0u) { part_ms[2u * part] = pm; part_ms[2u * part + 1u] = ps; }
}
__global__ __launch_bounds__(256) void k_softmax_topk_merge(const uint8_t* __restrict__ ws, uint32_t n, uint32_t k, uint32_t parts,
        int32_t* __restrict__ out_tok, float* __restrict__ out_conf)
{
    const uint32_t b = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (b >= n) return;
    const uint8_t* mine = ws + static_cast<uint64_t>(b) * tk_ws_stride(parts);
    const float* part_ms = reinterpret_cast<const float*>(mine);
    const uint64_t* part_key = reinterpret_cast<const uint64_t*>(mine + parts * 8u);
    const bool have = lane < parts;                                      // lane = part
    const float qm = have ? part_ms[2u * lane] : -INFINITY, qs = have ? part_ms[2u * lane + 1u] : 0.0f;
    uint64_t key[8];
#pragma unroll
    for (uint32_t r = 0; r < 8u; ++r) key[r] = (have && r < k) ? part_key[lane * 8u + r] : 0;       // descending: key[0] is the part's best not yet taken
    const float mx = wave_max_f32(qm);
    const float total = wave_sum_f32(qm > -INFINITY ? qs * pred_fast_exp(qm - mx) : 0.0f);
    float* conf = out_conf + static_cast<uint64_t>(b) * k;
    int32_t* tok = out_tok + static_cast<uint64_t>(b) * k;
    for (uint32_t r = 0; r < k; ++r) {
        const uint64_t w = wave_max_u64(key[0]);
        if (w != 0 && w == key[0]) {                                     // keys are distinct (token ids are): one owner, whose next key moves up
#pragma unroll
            for (uint32_t j = 0; j < 7u; ++j) key[j] = key[j + 1u];
            key[7] = 0;
        }
        if (lane == 0u) {
            tok[r] = w ? static_cast<int32_t>(0xFFFFFFFFu - static_cast<uint32_t>(w)) : -1;
            conf[r] = w ? pred_fast_exp(tk_value(w) - mx) / total : 0.0f;
        }
    }
}

// ---- a handful of requests (n <= kPredictSmallN): written for the length of the chain, not for throughput ----------------
// The batch path above is four launches (hidden state | logits on the matrix cores, 32 requests per tile | top-k of 4096-logit
// parts | merge) and writes n x vocab logits to memory in between: for ONE request that is four launch gaps around 16 MB of
// weights (23.7 us per prediction back to back, README's "< 10 us" claim of the reference's FPGA).  Here two launches:
//   k_predict_small:  a wave takes 32 output rows (its 16 KiB of arranged weights: the same k_arrange_wout layout), forms
//     their logits for every request with plain fused multiply-adds against the hidden vector in LDS -- which the workgroup
//     computes itself for the reference's degenerate cell (one wave per request: the loop of k_lstm_hidden) or reads from
//     k_lstm_cell's output for the real one -- and reduces them at once: maximum, exp-sum, top k of its 32 rows by wave
//     exchanges, then the four waves' results to one (max, sum, k keys) of the workgroup's 128 rows.  Logits never leave
//     the CU.
//   k_predict_small_merge:  one workgroup per request merges the workgroups' results (a lane per part, 64 parts per wave,
//     as k_softmax_topk_merge) and writes tokens and confidences.  (Merged by the workgroup that finishes last instead -- one
//     launch, write-through stores, arrival counter: 17.1 us per prediction against 15.7 with the second launch; the lone
//     workgroup's chain of counter, agent-scope loads and exchanges is longer than a launch gap.
//     profiles/experiments/r04_predict_small_last_arriver_merge.patch)
// Same arithmetic as the batch path up to the order of the dot product's additions (tests state 1e-4 on confidences, as for
// the batch path against the oracle); vocabularies up to kPredictSmallMaxParts x 128 rows, larger ones take the batch path.
__global__ __launch_bounds__(256) void k_predict_small(const int32_t* __restrict__ hist, uint32_t n, const float* __restrict__ emb,
        const float* __restrict__ hid_in, uint32_t layers, const float* __restrict__ wout, const float* __restrict__ out_bias,
        uint32_t vocab, uint32_t k, uint8_t* __restrict__ ws)
{
    __shared__ __attribute__((aligned(16))) float hs[kPredictSmallN][kPredHidden];
    __shared__ float wm[kPredictSmallN][4], wsum[kPredictSmallN][4];
    __shared__ uint64_t wkey[kPredictSmallN][4][8];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t c = lane & 31u, kh = lane >> 5;
    const uint32_t tile = blockIdx.x * 4u + wave;
    const uint32_t row = tile * 32u + c;
    const bool live = row < vocab && kh == 0u;                          // the two halves of the wave end with the same logit: one counts
    // the wave's weights first (they are the long pole: 16 KiB per wave from memory), then the hidden vectors under their flight
    float4 wq[16];
    const float4* wt = reinterpret_cast<const float4*>(wout) + static_cast<uint64_t>(tile) * (16u * 64u) + lane;
#pragma unroll
    for (int j = 0; j < 16; ++j) wq[j] = wt[j * 64];
    const float bias = (out_bias && row < vocab) ? out_bias[row] : 0.0f;
    if (hid_in) {                                                       // the real cell's output (k_lstm_cell)
        for (uint32_t e = threadIdx.x; e < n * kPredHidden; e += 256u) hs[e / kPredHidden][e % kPredHidden] = hid_in[e];
    } else if (wave < n) {                                              // the reference's degenerate cell: k_lstm_hidden's loop, request = wave
        float g[kPredHist];
#pragma unroll
        for (uint32_t t = 0; t < kPredHist; ++t) {
            const uint32_t tok = static_cast<uint32_t>(hist[wave * kPredHist + t]);
            g[t] = (tok < vocab) ? emb[static_cast<uint64_t>(tok) * kPredEmb + lane] * 0.1f : 0.0f;
        }
#pragma unroll
        for (uint32_t t = 0; t < kPredHist; ++t) g[t] = wave_sum_f32(g[t]);
        // (the recurrence: pred_fast_tanh, as k_lstm_hidden)
        float tg[kPredHist];
#pragma unroll
        for (uint32_t t = 0; t < kPredHist; ++t) tg[t] = 0.5f * pred_fast_tanh(g[t]);      // (independent of the chain)
        float h = 0.0f, cc = 0.0f;
#pragma unroll
        for (uint32_t t = 0; t < kPredHist; ++t)
            for (uint32_t l = 0; l < layers; ++l) {
                cc = 0.5f * cc + tg[t];
                h = 0.5f * pred_fast_tanh(cc);
            }
        h = __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(h)));
        hs[wave][lane] = h;
        hs[wave][64u + lane] = h;
    }
    __syncthreads();
    for (uint32_t b = 0; b < n; ++b) {                                  // (n <= 4: the weights stay in registers)
        float acc = 0.0f;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float4 h4 = *reinterpret_cast<const float4*>(&hs[b][8u * j + 4u * kh]);
            acc = __builtin_fmaf(h4.x, wq[j].x, acc);
            acc = __builtin_fmaf(h4.y, wq[j].y, acc);
            acc = __builtin_fmaf(h4.z, wq[j].z, acc);
            acc = __builtin_fmaf(h4.w, wq[j].w, acc);
        }
        { const TkPair h2 = tk_halves(__float_as_uint(acc)); acc = __uint_as_float(h2.a) + __uint_as_float(h2.b); }   // the other half of the columns
        const float v = live ? (out_bias ? acc + bias : acc) : -INFINITY;
        const float m = wave_max_f32(v);
        const float sum = wave_sum_f32(v > -INFINITY ? pred_fast_exp(v - m) : 0.0f);       // an absent logit (-inf, NaN, a dead lane) adds nothing
        uint64_t key = live ? tk_key(v, row) : 0;
        for (uint32_t r = 0; r < k; ++r) {
            const uint64_t w = wave_max_u64(key);
            if (w == key) key = 0;                                      // one row per lane: the owner retires it
            if (lane == 0u) wkey[b][wave][r] = w;
        }
        if (lane == 0u) { wm[b][wave] = m; wsum[b][wave] = sum; }
    }
    __syncthreads();
    if (wave >= n) return;                                              // wave b merges request b's four results
    const uint32_t b = wave, parts = gridDim.x, part = blockIdx.x;
    uint8_t* mine = ws + static_cast<uint64_t>(b) * tk_ws_stride(parts);
    float* part_ms = reinterpret_cast<float*>(mine);                     // [part] (max, sum)
    uint64_t* part_key = reinterpret_cast<uint64_t*>(mine + parts * 8u);             // [part][8]
    float pm, ps;
    tk_merge(lane < 4u ? wm[b][lane] : -INFINITY, lane < 4u ? wsum[b][lane] : 0.0f, lane < 4u * k ? wkey[b][lane / k][lane % k] : 0, k, pm, ps,
             [&](uint32_t r, uint64_t w) { if (lane == 0u) part_key[part * 8u + r] = w; });
    if (lane == 0u) { part_ms[2u * part] = pm; part_ms[2u * part + 1u] = ps; }
}
__global__ __launch_bounds__(256) void k_predict_small_merge(const uint8_t* __restrict__ ws, uint32_t k, uint32_t parts,
        int32_t* __restrict__ out_tok, float* __restrict__ out_conf)
{
    __shared__ float wm[4], wsum[4];
    __shared__ uint64_t wkey[4][8];
    const uint32_t b = blockIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint8_t* mine = ws + static_cast<uint64_t>(b) * tk_ws_stride(parts);
    const float* part_ms = reinterpret_cast<const float*>(mine);
    const uint64_t* part_key = reinterpret_cast<const uint64_t*>(mine + parts * 8u);
    const uint32_t part = wave * 64u + lane;                             // lane = part (up to 256 of them)
    const bool have = part < parts;
    const float qm = have ? part_ms[2u * part] : -INFINITY, qs = have ? part_ms[2u * part + 1u] : 0.0f;
    uint64_t key[8];
#pragma unroll
    for (uint32_t r = 0; r < 8u; ++r) key[r] = (have && r < k) ? part_key[part * 8u + r] : 0;       // descending: key[0] is the part's best not yet taken
    const float mx = wave_max_f32(qm);
    const float total = wave_sum_f32(qm > -INFINITY ? qs * pred_fast_exp(qm - mx) : 0.0f);
    for (uint32_t r = 0; r < k; ++r) {
        const uint64_t w = wave_max_u64(key[0]);
        if (w != 0 && w == key[0]) {                                     // keys are distinct (token ids are): one owner, whose next key moves up
#pragma unroll
            for (uint32_t j = 0; j < 7u; ++j) key[j] = key[j + 1u];
            key[7] = 0;
        }
        if (lane == 0u) wkey[wave][r] = w;
    }
    if (lane == 0u) { wm[wave] = mx; wsum[wave] = total; }
    __syncthreads();
    if (wave != 0u) return;
    float M, S;
    float* conf = out_conf + static_cast<uint64_t>(b) * k;
    int32_t* tok = out_tok + static_cast<uint64_t>(b) * k;
    tk_merge(lane < 4u ? wm[lane] : -INFINITY, lane < 4u ? wsum[lane] : 0.0f, lane < 4u * k ? wkey[lane / k][lane % k] : 0, k, M, S,
             [&](uint32_t r, uint64_t w) {
                 if (lane == 0u) {
                     tok[r] = w ? static_cast<int32_t>(0xFFFFFFFFu - static_cast<uint32_t>(w)) : -1;
                     conf[r] = w ? pred_fast_exp(tk_value(w) - M) / S : 0.0f;
                 }
             });
}

} // namespace

size_t arranged_wout_bytes(uint32_t vocab) { return static_cast<size_t>(logits_tiles_padded(vocab)) * 32u * kPredHidden * sizeof(float); }
hipError_t launch_arrange_wout(const float* d_src, float* d_dst, uint32_t vocab, hipStream_t s)
{
    const uint32_t tiles = logits_tiles_padded(vocab);
    hipLaunchKernelGGL(k_arrange_wout, dim3(tiles / 4u), dim3(256), 0, s, d_src, reinterpret_cast<float4*>(d_dst), vocab);
    return hipGetLastError();
}

hipError_t launch_predict(uint32_t n, const int32_t* d_hist, const float* d_emb, const float* d_wout, uint32_t vocab,
                          uint32_t layers, uint32_t k, float* d_hid, float* d_logits, void* d_ws, int32_t* d_tok, float* d_conf,
                          hipStream_t s, const LstmParams* lstm)
{
    if (n == 0) return hipSuccess;
    if (k == 0 || k > 8u || vocab < k) return hipErrorInvalidValue;
    const uint32_t small_parts = logits_tiles_padded(vocab) / 4u;       // workgroups of 128 rows
    if (n <= kPredictSmallN && small_parts <= kPredictSmallMaxParts && !tuning().predict_batch_path) {
        // a handful of requests: two launches (three with the real cell), no logits in memory (k_predict_small)
        const bool real = lstm && lstm->layers;
        if (real) {
            if (lstm->layers > 4u) return hipErrorInvalidValue;
            LstmWeights w{};
            w.layers = lstm->layers;
            for (uint32_t l = 0; l < lstm->layers; ++l) { w.w_ih_t[l] = lstm->w_ih_t[l]; w.w_hh_t[l] = lstm->w_hh_t[l]; w.bias[l] = lstm->bias[l]; }
            hipLaunchKernelGGL(k_lstm_cell, dim3(n), dim3(512), 0, s, d_hist, n, d_emb, vocab, w, d_hid);
        }
        hipLaunchKernelGGL(k_predict_small, dim3(small_parts), dim3(256), 0, s, d_hist, n, d_emb, real ? d_hid : nullptr, layers, d_wout,
                           lstm ? lstm->out_bias : nullptr, vocab, k, static_cast<uint8_t*>(d_ws));
        hipLaunchKernelGGL(k_predict_small_merge, dim3(n), dim3(256), 0, s, static_cast<const uint8_t*>(d_ws), k, small_parts, d_tok, d_conf);
        return hipGetLastError();
    }
    if (lstm && lstm->layers) {                       // the real cell (speckv_ext_predictor_load_lstm)
        if (lstm->layers > 4u) return hipErrorInvalidValue;
        LstmWeights w{};
        w.layers = lstm->layers;
        for (uint32_t l = 0; l < lstm->layers; ++l) { w.w_ih_t[l] = lstm->w_ih_t[l]; w.w_hh_t[l] = lstm->w_hh_t[l]; w.bias[l] = lstm->bias[l]; }
        hipLaunchKernelGGL(k_lstm_cell, dim3(n), dim3(512), 0, s, d_hist, n, d_emb, vocab, w, d_hid);
    } else {
        hipLaunchKernelGGL(k_lstm_hidden, dim3(n), dim3(64), 0, s, d_hist, n, d_emb, vocab, layers, d_hid);
    }
    const uint32_t waves = (vocab + 31u) / 32u;              // 32 output rows per wave (k_lstm_logits)
    hipLaunchKernelGGL(k_lstm_logits, dim3((waves + 3u) / 4u, (n + kLogitsChunk - 1u) / kLogitsChunk), dim3(256), 0, s, d_hid, n, d_wout, lstm ? lstm->out_bias : nullptr, vocab, d_logits);
    const uint32_t parts = predict_topk_parts(vocab);
    if (parts) {
        hipLaunchKernelGGL(k_softmax_topk_small, dim3(n, parts), dim3(kTkThreads), 0, s, d_logits, vocab, k, static_cast<uint8_t*>(d_ws));
        hipLaunchKernelGGL(k_softmax_topk_merge, dim3((n + 3u) / 4u), dim3(256), 0, s, static_cast<const uint8_t*>(d_ws), n, k, parts, d_tok, d_conf);
    }
    else                           hipLaunchKernelGGL(k_softmax_topk, dim3(n), dim3(1024), 0, s, d_logits, vocab, k, d_tok, d_conf);
    return hipGetLastError();
}
