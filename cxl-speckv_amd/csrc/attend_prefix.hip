// cxl-speckv_amd/csrc/attend_prefix.hip -- k_attend_prefix: the PREFIX form of the chunk walk (attend_chunk.hip).  The 64 query rows
// of a workgroup belong to DIFFERENT requests (the members of a group), see only stored positions of a THIRD allocation (the group's
// prefix), and FOLD their result into what each member attended on its own (Engine::attend_prefix, speckv_ext_attend_prefix_fold:
// parallel samples of one prompt, beams, a system prompt in front of many users -- the prefix is read once per 64 rows, not once
// per request).  A translation unit of its own: the chunk kernels keep their instruction streams; the record loaders, decoders and
// the LDS layout are chunk_device.hpp's.
//
// Semantics.  Group g = one prefix allocation and the members [first_member, first_member + n_pairs / C) of the call.  Member m
// brings n_q[m] <= C positions of rows_per_pos query rows per kv head (q, out, lse in the chunk entries' layout, indexed by MEMBER)
// and sees the stored positions [0, prefix_len[m]) of the prefix; prefix_len is even and per member.  Nothing is held: no tail
// rows, no new rows, no causal structure among rows.  THE QUERY STAYS fp16 in all three formats.  Both products, the rounding of the
// weights to fp16 and the fp32 running max / sum are the chunk kernel's.
//
// Execution model.  A work item is (group, block of 64 / rows_per_pos flat (member, position) pairs, [piece], kv head), head fast,
// found by the chunk kernel's binary search over the host's exclusive block / item prefixes.  Flat pair p of a group is member
// first_member + p / C, position p % C; a pair with p % C >= n_q[m] or prefix_len[m] == 0 is DEAD: its q is not loaded, out / lse
// are neither read nor written.  A block without a live row leaves at once.  A block walks the pool tiles [0, ceil(max_len / 32)),
// max_len = the largest prefix_len of the group; pages at or beyond max_len are staged as ZEROS, and a score is -inf at or beyond
// the ROW's own prefix_len -- one per-row compare where the chunk kernel has `limit`.  Between a row's prefix_len and max_len lie
// real, finite records weighed 0 (a non-finite V row the caller stored there gives NaN, 0 x NaN, like stale non-finite rows
// elsewhere).  A wave skips the products of tiles none of its rows sees.  Every live row sees position 0, so its sum is never 0.
//
// FOLD epilogue.  The launch runs on the stream behind the launches that wrote the members' own (out, lse).  With b = m + log2 l of
// the prefix part (finite) and a = lse log2 e of the own part: n = max(a, b) + log2(2^(a - max) + 2^(b - max)),
// out = out 2^(a - n) + (acc / l) 2^(b - n), lse = n ln 2.  A member without positions of its own arrives as out = 0, lse = -inf:
// a = -inf, max = b, the sum is 0 + 1, n = b, the weights are 2^-inf = 0 and 2^0 = 1 -- it leaves as exactly acc / l and b ln 2;
// -inf - (-inf) never occurs because b is finite.  Everything goes out through vector stores.
//
// Split form (SPLIT, PrefixArgs::part): the host cuts the group's tiles into n_pieces pieces of tiles_per_piece (chunk_split_plan,
// unchanged, with pos_end = max_len and n_q = members x C); piece p walks [p tpp, min((p + 1) tpp, n_pool)) and writes the chunk
// kernel's partial (kChunkPartBytes).  A piece beyond a row's prefix_len writes m = -inf, l = 0, zeros.  k_prefix_combine merges a
// row's pieces in ascending order exactly as k_chunk_combine does and then folds as above.
//
// Window form (WINDOW, PrefixArgs::window = W >= 1; speckv_ext_attend_prefix_fold_window: a local layer, decode steps, chunks and
// draft trees).  The member's own positions lie BEHIND the prefix, so a row sees of the prefix only [lo, prefix_len),
// lo = prefix_window_lo(prefix_len, own_seen[m], d, W) with d = depth[m * C + j] or, without a table, j (prefix_window.hpp).  A row
// with lo >= prefix_len sees nothing and is DEAD like a pair beyond n_q -- by the rule, in the piece kernel and in the merge alike.
// The group's walk starts at PrefixGroup::first_tile, the tile of the lowest depth-0 bound of its live members (the host's:
// prefix_window_group), so pages below it are never loaded; a score is -inf unless lo <= t < len; the ballot gains the lower test.
// SPLIT: the pieces cut the tiles that are left, piece p walks from first_tile + p tpp; a piece wholly below a row's lo or beyond
// its prefix_len writes m = -inf, l = 0, zeros, and the merge gives the unsplit weights (prefix_combine).  Every live row sees
// position lo, so its sum is never 0 and b stays finite.  The instances without WINDOW are the code above, untouched.
//
// Split pool (KS != VS, PrefixArgs::v_scheme; speckv_ext_attend_prefix_fold_kv: FP8 keys, MXFP4 values).  As in the chunk kernel: the
// scheme of the K side (load_pool, decode_pool<.., true>, pool_k_scale, k_scale) and of the V side (load_pool, decode_pool) are two
// template parameters, and the V pages are addressed through the table of an allocation of their own (PrefixGroup::v_table_row).  With
// KS == VS the V table IS the K table and the instances are the ones of one scheme, instruction for instruction.  (FP8, MXFP4) is the
// one mixed pair instantiated: four instances, SPLIT x WINDOW; the merge kernels read partials only and serve it as they are.
#include "chunk_device.hpp"
#include "prefix_window.hpp"

namespace speckv {
namespace {

// The group of a flat block (SPLIT: item) index: the last group whose prefix is <= fb (groups without blocks share their successor's
// prefix and are passed over)
template <bool ITEMS>
__device__ __forceinline__ uint32_t prefix_group_of(const PrefixArgs& a, uint32_t fb)
{
    uint32_t lo = 0, hi = a.n_groups;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(ITEMS ? a.groups[mid].first_item : a.groups[mid].first_block)) <= fb) lo = mid; else hi = mid;
    }
    return lo;
}

// Query row qr of block blk of a group: its member, its position, its own prefix_len (0: dead) and where its q / out / lse rows are.
// WINDOW: and its lower bound lo by the rule (prefix_window_lo); a row with lo >= prefix_len comes back dead (len = 0), so the piece
// kernel and the merge decide a row's life by the same rule and never by what the scratch holds.
struct PrefixRow { uint32_t len; uint64_t idx; uint32_t lo; };
template <bool WINDOW = false>
__device__ __forceinline__ PrefixRow prefix_row(const PrefixArgs& a, uint32_t first_member, uint32_t n_pairs, uint32_t blk, uint32_t qr, uint32_t h)
{
    const uint32_t rpp = a.rows_per_pos, p = blk * (64u / rpp) + qr / rpp, sub = qr % rpp;
    PrefixRow r{0u, 0u, 0u};
    if (p >= n_pairs) return r;
    const uint32_t m = first_member + p / a.C, j = p % a.C;
    if (j >= ck_ld<uint32_t>(a.n_q + m)) return r;
    const uint32_t len = ck_ld<uint32_t>(a.prefix_len + m);
    if (WINDOW) {
        const uint32_t d = a.depth ? ck_ld<uint32_t>(a.depth + static_cast<uint64_t>(m) * a.C + j) : j;
        r.lo = prefix_window_lo(len, ck_ld<uint32_t>(a.own_seen + m), d, a.window);
        if (r.lo >= len) return PrefixRow{0u, 0u, 0u};
    }
    r.len = len;
    r.idx = ((static_cast<uint64_t>(m) * a.C + j) * a.heads + h) * rpp + sub;
    return r;
}

// The fold's weights and the new lse: b = m + log2 l of the prefix part (finite), own = the row's lse so far (-inf: nothing of its own)
struct FoldW { float w_own, w_pre, lse; };
__device__ __forceinline__ FoldW fold_weights(float own, float b)
{
    const float a = own * kLog2e;                                   // -inf stays -inf
    const float mx = fmaxf(a, b);                                   // finite: b is
    const float n = mx + __builtin_amdgcn_logf(__builtin_amdgcn_exp2f(a - mx) + __builtin_amdgcn_exp2f(b - mx));
    return FoldW{__builtin_amdgcn_exp2f(a - n), __builtin_amdgcn_exp2f(b - n), n * kLn2};
}

template <int KS, int VS, bool SPLIT, bool WINDOW>
__global__ __launch_bounds__(kChunkThreads) void k_attend_prefix(PrefixArgs a)
{
    __shared__ __attribute__((aligned(16))) _Float16 lds[2 * kBufElems];
    __shared__ float k_scale[2][16];                          // FP8: the K block scale of the 16 pages of a staged tile (chunk_device.hpp)

    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t h = blockIdx.x % a.heads, fb = blockIdx.x / a.heads;          // SPLIT: fb = the flat work item (block, piece)
    const PrefixGroup* gp = a.groups + prefix_group_of<SPLIT>(a, fb);
    const uint32_t max_len = __builtin_amdgcn_readfirstlane(gp->max_len), n_pairs = __builtin_amdgcn_readfirstlane(gp->n_pairs);
    const uint32_t first_member = __builtin_amdgcn_readfirstlane(gp->first_member);
    uint32_t blk = fb - static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(SPLIT ? gp->first_item : gp->first_block));
    uint32_t piece = 0, tpp = 0;                              // (wave-uniform: they live in scalar registers)
    if (SPLIT) {
        const uint32_t n_pieces = __builtin_amdgcn_readfirstlane(gp->n_pieces);
        tpp = __builtin_amdgcn_readfirstlane(gp->tiles_per_piece);
        piece = blk % n_pieces;
        blk /= n_pieces;
    }
    const uint32_t n_pool = (max_len + 31u) >> 5, n_pages = max_len >> 1;
    const uint32_t t_first = WINDOW ? static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(gp->first_tile)) : 0u;
    const uint32_t t_begin = t_first + (SPLIT ? piece * tpp : 0u);
    const uint32_t t_end = SPLIT ? (t_begin + tpp < n_pool ? t_begin + tpp : n_pool) : n_pool;

    // compute role: query row qr of the block, contraction group g
    const uint32_t col = lane & 15u, g = lane >> 4;
    const uint32_t qr = 16u * wave + col;
    const PrefixRow row = prefix_row<WINDOW>(a, first_member, n_pairs, blk, qr, h);
    const bool row_live = row.len != 0u;                      // (WINDOW: and lo < len -- prefix_row)
    if (!__syncthreads_or(row_live)) return;                  // a block of dead pairs (workgroup-uniform)
    if (t_begin >= t_end) return;                             // (never: no piece of the plan is empty)

    const PageEntry* entries = reinterpret_cast<const PageEntry*>(ck_uniform(reinterpret_cast<uint64_t>(a.tab[gp->table_row].entries)));
    // the V pages' table: the same allocation's unless the schemes differ (the split pool: K and V in an allocation each)
    const PageEntry* v_entries = KS == VS ? entries : reinterpret_cast<const PageEntry*>(ck_uniform(reinterpret_cast<uint64_t>(a.tab[gp->v_table_row].entries)));
    const uint64_t k_first = ck_uniform(gp->k_first), v_first = ck_uniform(gp->v_first);

    // staging role: page pp of the tile, elements [8 c, 8 c + 8) of head h of both its positions
    const uint32_t pp = tid >> 4, c = tid & 15u;
    const uint32_t p0 = h * 128u + 8u * c;                    // element of the even position inside the page

    f16x8 qv[4];
#pragma unroll
    for (uint32_t s = 0; s < 4u; ++s) {
        u32x4 w = {0u, 0u, 0u, 0u};
        if (row_live) w = ck_ld<u32x4>(a.q + row.idx * 128u + 32u * s + 8u * g);
        qv[s] = __builtin_bit_cast(f16x8, w);
    }

    Raw rk, rv;
    const auto load_tile = [&](uint32_t tile) {
        const uint32_t page = 16u * tile + pp;
        const bool live = page < n_pages;
        rk = load_pool<KS>(entries + k_first + page, p0, live);
        rv = load_pool<VS>(v_entries + v_first + page, p0, live);
    };
    const auto store_tile = [&](_Float16* buf) {
        uint32_t ke[4], ko[4], ve[4], vo[4];
        if (KS == kFp8E4m3 && c == 0u) k_scale[buf != lds][pp] = pool_k_scale<KS>(rk);
        decode_pool<KS, true>(rk, p0, ke, ko);
        decode_pool<VS>(rv, p0, ve, vo);
        *reinterpret_cast<u32x4*>(buf + (2u * pp) * kKRow + 8u * c) = u32x4{ke[0], ke[1], ke[2], ke[3]};
        *reinterpret_cast<u32x4*>(buf + (2u * pp + 1u) * kKRow + 8u * c) = u32x4{ko[0], ko[1], ko[2], ko[3]};
        uint32_t* vt = reinterpret_cast<uint32_t*>(buf + kKTile);            // word (dim, page) = the dim's values at the page's two positions
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) {
            const uint32_t e = (ve[k >> 1] >> (16u * (k & 1u))) & 0xFFFFu, o = (vo[k >> 1] >> (16u * (k & 1u))) & 0xFFFFu;
            vt[(8u * c + k) * (kVRow / 2u) + pp] = e | (o << 16);
        }
    };

    f32x4 acc[8];
#pragma unroll
    for (uint32_t t = 0; t < 8u; ++t) acc[t] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float m_run = -__builtin_inff(), l_run = 0.0f;            // log2 domain
    const float scale2 = a.sm_scale * kLog2e;

    load_tile(t_begin);
    store_tile(lds);
    __syncthreads();
    for (uint32_t tile = t_begin; tile < t_end; ++tile) {
        _Float16* buf = lds + ((tile - t_begin) & 1u) * kBufElems;
        const bool more = tile + 1u < t_end;
        if (more) load_tile(tile + 1u);
        const uint32_t t_base = 32u * tile;
        // some row of the wave sees a position of this tile (a dead row has len 0)
        if (__builtin_amdgcn_ballot_w64(row.len > t_base && (!WINDOW || row.lo < t_base + 32u)) != 0ull) {
            // scores: rows = positions 16 hf + 4 g + r of the tile, column = the lane's query row
            f32x4 sc[2];
#pragma unroll
            for (uint32_t hf = 0; hf < 2u; ++hf) {
                f32x4 s4 = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
                for (uint32_t s = 0; s < 4u; ++s) {
                    const u32x4 kw = *reinterpret_cast<const u32x4*>(buf + (16u * hf + col) * kKRow + 32u * s + 8u * g);
                    s4 = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, kw), qv[s], s4, 0, 0, 0);
                }
                sc[hf] = s4;
            }
            const float* ks = k_scale[(tile - t_begin) & 1u];
            float sv[8], mx = -__builtin_inff();
#pragma unroll
            for (uint32_t i = 0; i < 8u; ++i) {
                const uint32_t t = t_base + 16u * (i >> 2) + 4u * g + (i & 3u);
                const float scale_i = KS == kFp8E4m3 ? scale2 * ks[8u * (i >> 2) + 2u * g + ((i & 3u) >> 1)] : scale2;       // the position's page
                sv[i] = t < row.len && (!WINDOW || t >= row.lo) ? sc[i >> 2][i & 3u] * scale_i : -__builtin_inff();   // the row's own range
                mx = fmaxf(mx, sv[i]);
            }
            mx = max_over_kb(mx);
            const float m_new = fmaxf(m_run, mx);
            const float m_use = m_new == -__builtin_inff() ? 0.0f : m_new;  // (a row that sees nothing: dead, or a piece outside its range)
            const float alpha = __builtin_amdgcn_exp2f(m_run - m_use);
            float p[8], sum = 0.0f;
#pragma unroll
            for (uint32_t i = 0; i < 8u; ++i) p[i] = __builtin_amdgcn_exp2f(sv[i] - m_use);
            uint32_t pw[4];
#pragma unroll
            for (uint32_t i = 0; i < 4u; ++i) {
                pw[i] = pack_half2(p[2 * i], p[2 * i + 1]);
                sum += half_bits_to_float(pw[i] & 0xFFFFu) + half_bits_to_float(pw[i] >> 16);
            }
            sum = sum_over_kb(sum);
            l_run = l_run * alpha + sum;
            m_run = m_new;
            const f16x8 P = __builtin_bit_cast(f16x8, u32x4{pw[0], pw[1], pw[2], pw[3]});
            const _Float16* vt = buf + kKTile;
#pragma unroll
            for (uint32_t t = 0; t < 8u; ++t) {
                const _Float16* vr = vt + (16u * t + col) * kVRow + 4u * g;
                const u32x2 v0 = *reinterpret_cast<const u32x2*>(vr), v1 = *reinterpret_cast<const u32x2*>(vr + 16);
                const f16x8 V = __builtin_bit_cast(f16x8, u32x4{v0.x, v0.y, v1.x, v1.y});
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(V, P, acc[t] * alpha, 0, 0, 0);
            }
        }
        if (more) store_tile(lds + ((tile + 1u - t_begin) & 1u) * kBufElems);
        __syncthreads();
    }

    if (!row_live) return;                                    // dead rows write nothing
    if (SPLIT) {
        // the partial of (item, head): the accumulator as it stands, (m_run, l_run) beside it
        uint8_t* pb = a.part + static_cast<uint64_t>(blockIdx.x) * kChunkPartBytes;
        float* o = reinterpret_cast<float*>(pb) + qr * 128u + 4u * g;
#pragma unroll
        for (uint32_t t = 0; t < 8u; ++t) ck_st<f32x4>(o + 16u * t, acc[t]);
        if (g == 0u) ck_st<u32x2>(pb + kChunkPartAccBytes + 8u * qr, u32x2{__float_as_uint(m_run), __float_as_uint(l_run)});
        return;
    }
    const FoldW f = fold_weights(ck_ld<float>(a.lse + row.idx), m_run + __builtin_amdgcn_logf(l_run));
    const float inv = 1.0f / l_run;
    float* o = a.out + row.idx * 128u + 4u * g;
#pragma unroll
    for (uint32_t t = 0; t < 8u; ++t) {
        const f32x4 own = __builtin_bit_cast(f32x4, ck_ld<u32x4>(o + 16u * t));
        ck_st<f32x4>(o + 16u * t, own * f.w_own + (acc[t] * inv) * f.w_pre);
    }
    // the row's four lanes have all read lse above: every lane's load precedes this store in program order of ONE wave
    if (g == 0u) ck_st<float>(a.lse + row.idx, f.lse);
}

// The merge of the split form: k_chunk_combine's thread roles and order -- one workgroup per (flat block, kv head), thread t = row
// t >> 2 of the block and the 16-byte columns (t & 3) + 4 k; a live row's n_pieces partials are read in ASCENDING piece order;
// a piece that saw nothing (m = -inf, l = 0, acc = 0) weighs 2^-inf = 0 exactly -- and then the fold of k_attend_prefix.  Whether a
// row is live is decided as the pieces decided it -- by prefix_row's rule -- never by what the scratch holds.  Without a window piece 0
// saw position 0 of every live row; under one (WINDOW) any number of a live row's pieces, the first ones included, lie wholly below
// its lo or beyond its prefix_len and saw nothing, but the piece that holds lo saw it: M is finite and is the max over the pieces
// that saw something (-inf never wins a max), the others weigh 2^(-inf - M) = 0 on l = 0 and zeros -- exactly the unsplit weights.
template <bool WINDOW>
__device__ __forceinline__ void prefix_combine(const PrefixArgs& a)
{
    const uint32_t tid = threadIdx.x;
    const uint32_t h = blockIdx.x % a.heads, fb = blockIdx.x / a.heads;
    const PrefixGroup* gp = a.groups + prefix_group_of<false>(a, fb);
    const uint32_t blk = fb - static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(gp->first_block));
    const uint32_t n_pieces = __builtin_amdgcn_readfirstlane(gp->n_pieces);
    const uint32_t item = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(gp->first_item)) + blk * n_pieces;
    const uint32_t qr = tid >> 2, c4 = tid & 3u;
    const PrefixRow row = prefix_row<WINDOW>(a, __builtin_amdgcn_readfirstlane(gp->first_member), __builtin_amdgcn_readfirstlane(gp->n_pairs), blk, qr, h);
    if (row.len == 0u) return;
    const uint64_t step = static_cast<uint64_t>(a.heads) * kChunkPartBytes;          // from a piece's partial to the next piece's
    const uint8_t* pb = a.part + (static_cast<uint64_t>(item) * a.heads + h) * kChunkPartBytes;
    const uint8_t* ml = pb + kChunkPartAccBytes + 8u * qr;
    float M = -__builtin_inff();
    for (uint32_t p = 0; p < n_pieces; ++p) M = fmaxf(M, ck_ld<float>(ml + p * step));
    const float m_use = M == -__builtin_inff() ? 0.0f : M;
    f32x4 acc[8];
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k) acc[k] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float l_sum = 0.0f;
    const float* ap = reinterpret_cast<const float*>(pb) + qr * 128u + 4u * c4;
    for (uint32_t p = 0; p < n_pieces; ++p) {
        const u32x2 w2 = ck_ld<u32x2>(ml + p * step);
        const float w = __builtin_amdgcn_exp2f(__uint_as_float(w2.x) - m_use);
        l_sum += __uint_as_float(w2.y) * w;
        const float* src = ap + p * (step / sizeof(float));
#pragma unroll
        for (uint32_t k = 0; k < 8u; ++k) acc[k] += __builtin_bit_cast(f32x4, ck_ld<u32x4>(src + 16u * k)) * w;
    }
    const FoldW f = fold_weights(ck_ld<float>(a.lse + row.idx), M + __builtin_amdgcn_logf(l_sum));
    const float inv = 1.0f / l_sum;
    float* o = a.out + row.idx * 128u + 4u * c4;
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k) {
        const f32x4 own = __builtin_bit_cast(f32x4, ck_ld<u32x4>(o + 16u * k));
        ck_st<f32x4>(o + 16u * k, own * f.w_own + (acc[k] * inv) * f.w_pre);
    }
    if (c4 == 0u) ck_st<float>(a.lse + row.idx, f.lse);
}
__global__ __launch_bounds__(kChunkThreads) void k_prefix_combine(PrefixArgs a) { prefix_combine<false>(a); }
__global__ __launch_bounds__(kChunkThreads) void k_prefix_combine_window(PrefixArgs a) { prefix_combine<true>(a); }

template <int KS, int VS, bool WINDOW>
hipError_t launch_prefix(const PrefixArgs& a, hipStream_t s)
{
    if (!a.part) {
        hipLaunchKernelGGL((k_attend_prefix<KS, VS, false, WINDOW>), dim3(a.n_blocks * a.heads), dim3(kChunkThreads), 0, s, a);
        return hipGetLastError();
    }
    hipLaunchKernelGGL((k_attend_prefix<KS, VS, true, WINDOW>), dim3(a.n_items * a.heads), dim3(kChunkThreads), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(WINDOW ? k_prefix_combine_window : k_prefix_combine, dim3(a.n_blocks * a.heads), dim3(kChunkThreads), 0, s, a);
    return hipGetLastError();
}

} // namespace

hipError_t launch_attend_prefix(const PrefixArgs& a, hipStream_t s)
{
    if (a.n_blocks == 0) return hipSuccess;
    if (!a.groups || !a.prefix_len || !a.n_q || !a.tab || !a.q || !a.out || !a.lse || a.n_groups == 0 || a.heads == 0 || a.C == 0 ||
        a.rows_per_pos == 0 || a.rows_per_pos > 16u || (a.rows_per_pos & (a.rows_per_pos - 1u)) ||
        static_cast<uint64_t>(a.n_blocks) * a.heads > 0x7FFFFFFFull ||
        (a.part && (a.n_items < a.n_blocks || static_cast<uint64_t>(a.n_items) * a.heads > 0x7FFFFFFFull || reinterpret_cast<uintptr_t>(a.part) % 16u)))
        return hipErrorInvalidValue;
    // the one mixed pair: K pages of an FP8 allocation, V pages of an MXFP4 one (the K8V4 split pool; PrefixGroup::v_table_row)
    if (a.v_scheme != a.scheme) {
        if (a.scheme != kFp8E4m3 || a.v_scheme != kMxFp4) return hipErrorInvalidValue;
        return a.window ? launch_prefix<kFp8E4m3, kMxFp4, true>(a, s) : launch_prefix<kFp8E4m3, kMxFp4, false>(a, s);
    }
    if (a.window) {                                           // (own_seen and depth are judged by Engine::attend_prefix)
        switch (a.scheme) {
        case kFp8E4m3: return launch_prefix<kFp8E4m3, kFp8E4m3, true>(a, s);
        case kInt4G32: return launch_prefix<kInt4G32, kInt4G32, true>(a, s);
        case kMxFp4: return launch_prefix<kMxFp4, kMxFp4, true>(a, s);
        default: return hipErrorInvalidValue;
        }
    }
    switch (a.scheme) {
    case kFp8E4m3: return launch_prefix<kFp8E4m3, kFp8E4m3, false>(a, s);
    case kInt4G32: return launch_prefix<kInt4G32, kInt4G32, false>(a, s);
    case kMxFp4: return launch_prefix<kMxFp4, kMxFp4, false>(a, s);
    default: return hipErrorInvalidValue;
    }
}

} // namespace speckv
