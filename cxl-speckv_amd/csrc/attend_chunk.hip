// cxl-speckv_amd/csrc/attend_chunk.hip -- k_attend_chunk: causal attention of a chunk of new positions per sequence over the
// positions the sequence has stored in the pool and the rows it holds outside it, in ONE launch (Engine::attend_chunk,
// speckv_ext_attend_chunk: chunked prefill, the suffix behind a fork, a prompt continued after a truncate).
//
// A translation unit of its own: the headline kernel of kernels.hip is pinned by the hash of its instructions and the three
// attention units stay as they are.  The three small decoders this kernel needs are restated for ONE head's 8 elements of both
// positions of a page (chunk_device.hpp, shared with attend_prefix.hip); they give the fp16 values speckv_ext_fetch_range gives (the
// fp32 product rounded once to fp16, pack_half2) -- except the K rows of an FP8 pool: those are staged as the E4M3 values
// themselves, exact in fp16, and the page's block scale multiplies the score in fp32 (k_scale below; chunk_device.hpp says why).
//
// Semantics.  Sequence i holds pos_end (even) stored positions, base in {0, 1} held odd last positions (the tail) and n_q <= C new
// positions.  Query position j < n_q sees the stored positions [0, pos_end) and the held positions 0 .. base + j: the tail, the new
// positions in front of it, itself.  out = softmax(q.K^T sm_scale).V per kv head, fp32, normalised; lse (natural log) on request.
// THE QUERY STAYS fp16 in all three formats -- the FP8 and MXFP4 decode kernels quantise q, this kernel does not.  Both products run
// on v_mfma_f32_16x16x32_f16; the weights are rounded to fp16; accumulation, running max and running sum are fp32.
//
// Execution model.  One workgroup of 4 waves owns (sequence, kv head, query block); a wave owns 16 query rows, a block is
// 64 / rows_per_pos positions.  The workgroup walks tiles of 32 positions with an online softmax: first the pool tiles, then the
// held tiles, up to the last held tile any live row of the block can see.  Staging: thread t takes page (t >> 4) of the tile's 16
// pages and elements [8 (t & 15), + 8) of head h of BOTH its positions -- 16 lanes read a head's contiguous slice of a record -- and
// the same piece of the V page; record addresses, lengths and scales come from PageEntry through the device allocation table, so
// linear, striped, migrated and sealed allocations are one body.  A held tile is staged by the same threads from the tail row
// (held position t < base) and from k_new / v_new where they lie (new row t - base), through strides; no gathered copy is made.
// After staging a tile is a tile.
//   LDS, two buffers of 17.5 KiB: K as [32 positions][128 + 8 pad] fp16 (a wave's 16-byte operand reads of 16 rows fall into 16
//   different 4-bank groups), V TRANSPOSED as [128 dims][32 + 4 pad] fp16 (the p.V operand wants 4 consecutive positions of one
//   dim: two 8-byte reads; rows 18 words apart spread 16 dims over the banks) -- a page's two positions go in as one 32-bit word.
//   The next tile's global loads are issued before the products of the current one and decoded into the other buffer behind them:
//   one workgroup barrier per tile.
//   S^T = K.Q^T (A = K rows from LDS, B = the wave's query rows, resident in 16 VGPRs), so a lane holds 8 scores of ONE query row
//   (row = lane & 15; positions 4 (lane >> 4) + r and 16 + 4 (lane >> 4) + r) -- exactly the 8 contraction slots of its P operand
//   in O^T = V^T.P^T once V^T is read in the same slot order.  Row max and sum go over the 4 lanes of a row by row/half swaps.
// No split over positions in this form (the split form is below): no merge kernel, no scratch, no atomics; a row's result does not
// depend on which other sequences share the launch.  Masks: stored positions >= pos_end and held positions beyond the sequence's count are staged as ZEROS (V) and scored
// -inf (truncate leaves stale records there, and 0 x inf would poison the product); held position t is -inf for rows with
// t > base + j; rows of positions >= n_q are neither loaded nor written.  Every live row sees itself, so its sum is never 0.
// Ragged chunks: the flat workgroup index is (block, kv head) with the head fast; the block maps to its sequence by binary search
// on the exclusive block prefixes the host computed.  Everything written goes out through vector stores.
//
// Tree form (MASKED, ChunkArgs::mask; speckv_ext_attend_chunk_masked: a step whose new positions form a tree of drafts of any size).
// The same body; a query row brings mask_words words, bit t of them = HELD position t is visible to it.  Held positions are numbered
// as above (the tail is 0, new position a is base + a), so word ht of a row is exactly the 32 positions of held tile ht: a lane loads
// the one word of its row in front of the tile's products and ANDs bit t & 31 into the causal test -- the causal bound stays, bits at
// or beyond base + j + 1 are ignored, and n_held, wave_t_last and the tile skipping by that bound hold unchanged.  Pool tiles take no
// mask work.  A row is live iff j < n_q AND its own bit base + j is set; a dead row is treated as rows >= n_q are (no query load, no
// mask load: its word reads 0; nothing written), so a live row still always sees itself.  A live row may see nothing for several
// tiles (empty pool, no tail, no ancestor in the first held tiles): m_new stays -inf, m_use = 0 gives alpha = exp2(-inf - 0) = 0,
// p = 0 and l_run = 0 until the tile with its first visible position, where alpha = 0 rescales an accumulator that is still 0.
//
// Split form (SPLIT, ChunkArgs::part; speckv_ext_attend_chunk_split: a short step or a small tree over a LONG context, where the
// query blocks alone leave most of the chip idle).  The same body; the host cuts sequence i's pool tiles into n_pieces pieces of
// tiles_per_piece tiles (chunk_split.hpp) and a work item is (sequence, query block, piece, kv head), head fast, found by the same
// binary search over the exclusive item prefixes.  Only the tile range changes: piece p walks pool tiles [p tpp, min((p + 1) tpp,
// n_pool)), the LAST piece also the held tiles exactly as the whole walk does (tail, new rows in place, causal bound, mask word,
// wave_t_last); the prologue stages tile t_begin and the buffer parity counts from it.  The epilogue writes the accumulator as it
// stands, [64 rows][128] fp32 in the row order of `out`, and (m_run, l_run) per row beside it, through vector stores; dead rows write
// nothing.  k_chunk_combine, launched behind it on the same stream, merges a row's partials in ascending piece order.  The piece
// bounds are wave-uniform (scalar registers): the SPLIT instances cost no vector registers worth mentioning.
//
// Window form (WINDOW, ChunkArgs::window = W >= 1; speckv_ext_attend_chunk_window: a local layer of a model that interleaves
// sliding-window and global layers).  The same body; with MASKED it is the form behind this one.  Query position j at the absolute position
// P = pos_end + base + j sees the absolute positions [lo(j), P], lo(j) = max(0, P + 1 - W) (chunk_window.hpp): a stored position t
// iff lo(j) <= t < pos_end, a held position t iff pos_end + t >= lo(j) and t <= base + j.  The block walks [t_first, n_tiles),
// t_first = the tile of lo(j_first): exactly the tiles that hold a position a live row of the block sees, never more than
// ceil((W + 64 / rows_per_pos - 1) / 32) + 2 of them; the prologue stages that tile and the buffer parity counts from it.  A score's
// test gains the row's lower bound, kept as ONE absolute position per row and re-based per part (two compares).  What NO row of the
// block sees -- positions below lo(j_first) inside the first tile -- is staged as ZEROS like the positions beyond the upper bounds,
// down to the one position of a page an odd bound cuts; what only some rows see is real, finite data weighed 0.  Rows of later
// positions see nothing in the block's first tile(s): the m_use path of the tree form.  A wave skips the products of tiles wholly
// below its first row's bound, the mirror of wave_t_last.  Split form: the pieces cut the pool tiles from ChunkSeq::first_tile (the
// first pool tile block 0 sees) on, clipped from below by the block's t_first; a piece that is not the last can be EMPTY for later
// blocks: it stages nothing and writes m = -inf, l = 0, zeros for its live rows, which k_chunk_combine weighs 0 exactly.
//
// Tree form under a window (MASKED and WINDOW, ChunkArgs::depth; speckv_ext_attend_chunk_tree_window: a draft tree on a local layer).
// Node j sits at the absolute position pos_end + base + depth(j), so its lower bound comes from its DEPTH, a device array [n_seq][C]
// a live row loads once beside its own mask bit: row_lo = chunk_window_lo(pos_end, base, depth[j], W).  Pool tiles: t >= row_lo and
// t < pos_end.  Held tiles: the mask words alone, as in the tree form -- the caller has folded the window into them, the kernel
// applies no lower bound there and stages no held zeros for the window.  Depths are not monotone in node order (a deep node may
// stand in front of a root inside one wave), so NOTHING is derived from a block's or a wave's first row: every block of a sequence
// walks from chunk_window_first_pool_tile, the tile of depth 0's bound (n_pool where depth 0 sees no stored position), positions
// below that bound are staged as zeros, and no wave skips a pool tile by a lower bound (the block-uniform bound, no per-wave skip).
// Split form: the pieces cut the pool tiles from ChunkSeq::first_tile on and every block shares that tile, so no piece is empty.
//
// Split pool (KS != VS, ChunkArgs::v_scheme; speckv_ext_attend_chunk_kv: FP8 keys, MXFP4 values).  The same body with the scheme of the K
// side (load_pool, decode_pool<.., true>, pool_k_scale, k_scale) and of the V side (load_pool, decode_pool) as two template parameters,
// and the V pages addressed through the table of an allocation of their own (ChunkSeq::v_table_row).  With KS == VS the V table IS the
// K table and the instances are the ones of one scheme, instruction for instruction.  (FP8, MXFP4) is the one mixed pair instantiated.
#include "chunk_device.hpp"          // the LDS layout, Raw, load_pool, decode_pool, load_held (shared with attend_prefix.hip)
#include "chunk_window.hpp"

namespace speckv {
namespace {

template <int KS, int VS, bool MASKED, bool SPLIT, bool WINDOW>
__global__ __launch_bounds__(kChunkThreads) void k_attend_chunk(ChunkArgs a)
{
    __shared__ __attribute__((aligned(16))) _Float16 lds[2 * kBufElems];
    __shared__ float k_scale[2][16];                          // FP8: the K block scale of the 16 pages of a staged tile (held tiles: 1)

    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const uint32_t h = blockIdx.x % a.heads, fb = blockIdx.x / a.heads;          // SPLIT: fb = the flat work item (block, piece)
    // the last sequence whose block prefix is <= fb (sequences without blocks share their successor's prefix and are passed over);
    // SPLIT: the same search over the item prefixes
    uint32_t lo = 0, hi = a.n_seq;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(SPLIT ? a.seqs[mid].first_item : a.seqs[mid].first_block)) <= fb) lo = mid; else hi = mid;
    }
    const ChunkSeq* sq = a.seqs + lo;
    const uint32_t seq = lo;
    const uint32_t pos_end = __builtin_amdgcn_readfirstlane(sq->pos_end), n_q = __builtin_amdgcn_readfirstlane(sq->n_q);
    const uint32_t base = __builtin_amdgcn_readfirstlane(sq->base);
    uint32_t blk = fb - static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(SPLIT ? sq->first_item : sq->first_block));
    uint32_t piece = 0, n_pieces = 1, tpp = 0;                // (wave-uniform: they live in scalar registers)
    if (SPLIT) {
        n_pieces = __builtin_amdgcn_readfirstlane(sq->n_pieces);
        tpp = __builtin_amdgcn_readfirstlane(sq->tiles_per_piece);
        piece = blk % n_pieces;
        blk /= n_pieces;
    }
    const uint32_t rpp = a.rows_per_pos, per_blk = 64u / rpp;
    const uint32_t j_first = blk * per_blk;
    if (j_first >= n_q) return;                               // (never: the host counts the blocks of live positions only)
    const uint32_t j_last = (j_first + per_blk < n_q ? j_first + per_blk : n_q) - 1u;     // the block's last live position
    const uint32_t n_pool = (pos_end + 31u) >> 5, n_held = ((base + j_last) >> 5) + 1u, n_tiles = n_pool + n_held;
    const uint32_t n_pages = pos_end >> 1, held_n = base + n_q;
    // SPLIT: piece p walks the pool tiles [p tpp, (p + 1) tpp); the LAST piece goes on through the held tiles, as the whole walk does
    // WINDOW: the block walks from the tile of its first row's lower bound (chunk_window.hpp); the pieces cut the pool tiles from the
    // sequence's first_tile on and are clipped from below by the block's first tile -- a piece that is not the last can be EMPTY
    // (t_begin >= t_end): it stages nothing and writes the partial of a piece that saw nothing
    const uint32_t piece_first = (SPLIT && WINDOW ? static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(sq->first_tile)) : 0u) + piece * tpp;
    // MASKED and WINDOW: a node's bound comes from its depth, which is not monotone in j: every block walks from depth 0's tile
    const uint32_t t_first = !WINDOW ? 0u : MASKED ? chunk_window_first_pool_tile(pos_end, base, a.window)
                                                   : chunk_window_first_tile(pos_end, base, j_first, a.window);
    const uint32_t t_begin = WINDOW ? (piece_first > t_first ? piece_first : t_first) : SPLIT ? piece * tpp : 0u;
    const uint32_t t_end = !SPLIT || piece + 1u == n_pieces ? n_tiles : (piece_first + tpp < n_pool ? piece_first + tpp : n_pool);
    // WINDOW: what no row of the block sees, as a stored position (lo_pool) and as a held one (lo_held): staged as zeros
    // (MASKED and WINDOW: below depth 0's bound, and no held zeros -- the held part is what the mask words say)
    const uint32_t lo_pool = WINDOW ? chunk_window_lo(pos_end, base, MASKED ? 0u : j_first, a.window) : 0u;
    const uint32_t lo_held = !MASKED && lo_pool > pos_end ? lo_pool - pos_end : 0u;

    const PageEntry* entries = reinterpret_cast<const PageEntry*>(ck_uniform(reinterpret_cast<uint64_t>(a.tab[sq->table_row].entries)));
    // the V pages' table: the same allocation's unless the schemes differ (the split pool: K and V in an allocation each)
    const PageEntry* v_entries = KS == VS ? entries : reinterpret_cast<const PageEntry*>(ck_uniform(reinterpret_cast<uint64_t>(a.tab[sq->v_table_row].entries)));
    const uint64_t k_first = ck_uniform(sq->k_first), v_first = ck_uniform(sq->v_first);
    const int32_t tail_idx = __builtin_amdgcn_readfirstlane(sq->tail_idx);
    const uint64_t head_off = static_cast<uint64_t>(h) * 128u;
    const _Float16* k_new = a.k_new + static_cast<uint64_t>(seq) * a.seq_stride + head_off;
    const _Float16* v_new = a.v_new + static_cast<uint64_t>(seq) * a.seq_stride + head_off;
    const _Float16* k_tail = base ? a.k_tail + static_cast<uint64_t>(tail_idx) * a.tail_stride + head_off : nullptr;
    const _Float16* v_tail = base ? a.v_tail + static_cast<uint64_t>(tail_idx) * a.tail_stride + head_off : nullptr;

    // staging role: page pp of the tile, elements [8 c, 8 c + 8) of head h of both its positions
    const uint32_t pp = tid >> 4, c = tid & 15u;
    const uint32_t p0 = h * 128u + 8u * c;                    // element of the even position inside the page

    // compute role: query row qr of the block, contraction group g
    const uint32_t col = lane & 15u, g = lane >> 4;
    const uint32_t qr = 16u * wave + col, j = j_first + qr / rpp, sub = qr % rpp;
    // tree form: the row's mask words (one per held tile), and whether its own bit is set
    const uint32_t* mrow = nullptr;
    bool row_live = j < n_q;
    uint32_t depth = 0u;                                      // MASKED and WINDOW: the node's depth, the j of its lower bound
    if (MASKED && row_live) {
        mrow = a.mask + (static_cast<uint64_t>(seq) * a.C + j) * a.mask_words;
        row_live = (ck_ld<uint32_t>(mrow + ((base + j) >> 5)) >> ((base + j) & 31u)) & 1u;
        if (WINDOW) depth = ck_ld<uint32_t>(a.depth + static_cast<uint64_t>(seq) * a.C + j);
        if (!row_live) mrow = nullptr;
    }
    const uint64_t row_idx = ((static_cast<uint64_t>(seq) * a.C + j) * a.heads + h) * rpp + sub;
    f16x8 qv[4];
#pragma unroll
    for (uint32_t s = 0; s < 4u; ++s) {
        u32x4 w = {0u, 0u, 0u, 0u};
        if (row_live) w = ck_ld<u32x4>(a.q + row_idx * 128u + 32u * s + 8u * g);
        qv[s] = __builtin_bit_cast(f16x8, w);
    }
    // the last held position the wave's rows see: tiles behind it are skipped by the wave (it still stages and meets the barriers)
    const uint32_t wave_j_last = j_first + (16u * wave + 15u) / rpp;
    const uint32_t wave_t_last = base + (wave_j_last < j_last ? wave_j_last : j_last);
    const bool wave_live = j_first + (16u * wave) / rpp < n_q;
    // WINDOW: the row's lower bound as an absolute position (re-based per part in front of the test), and the lowest bound of the
    // wave's rows, its first row's: tiles wholly below it are skipped by the wave as the tiles behind wave_t_last are
    // (MASKED and WINDOW: the bound of the row's depth; no wave bound -- a wave's first row need not be its shallowest)
    const uint32_t row_lo = WINDOW ? chunk_window_lo(pos_end, base, MASKED ? depth : j, a.window) : 0u;
    const uint32_t wave_lo = WINDOW && !MASKED ? chunk_window_lo(pos_end, base, j_first + (16u * wave) / rpp, a.window) : 0u;

    Raw rk, rv;
    const auto load_tile = [&](uint32_t tile) {
        if (tile < n_pool) {
            const uint32_t page = 16u * tile + pp;
            const bool live = page < n_pages && (!WINDOW || 2u * page + 1u >= lo_pool);
            rk = load_pool<KS>(entries + k_first + page, p0, live);
            rv = load_pool<VS>(v_entries + v_first + page, p0, live);
        } else {
            const uint32_t t0 = 32u * (tile - n_pool) + 2u * pp;
            const _Float16 *k0 = nullptr, *k1 = nullptr, *v0 = nullptr, *v1 = nullptr;
            if (t0 < held_n && (!WINDOW || t0 >= lo_held)) {
                if (t0 < base) { k0 = k_tail; v0 = v_tail; }
                else { const uint64_t o = static_cast<uint64_t>(t0 - base) * a.pos_stride; k0 = k_new + o; v0 = v_new + o; }
            }
            if (t0 + 1u < held_n && (!WINDOW || t0 + 1u >= lo_held)) { const uint64_t o = static_cast<uint64_t>(t0 + 1u - base) * a.pos_stride; k1 = k_new + o; v1 = v_new + o; }
            rk = load_held(k0 ? k0 + 8u * c : nullptr, k1 ? k1 + 8u * c : nullptr);
            rv = load_held(v0 ? v0 + 8u * c : nullptr, v1 ? v1 + 8u * c : nullptr);
        }
    };
    const auto store_tile = [&](uint32_t tile, _Float16* buf) {
        uint32_t ke[4], ko[4], ve[4], vo[4];
        if (KS == kFp8E4m3 && c == 0u) k_scale[buf != lds][pp] = tile < n_pool ? pool_k_scale<KS>(rk) : 1.0f;
        if (tile < n_pool) {
            decode_pool<KS, true>(rk, p0, ke, ko);
            decode_pool<VS>(rv, p0, ve, vo);
            if (WINDOW && 2u * (16u * tile + pp) < lo_pool) {               // the page the bound cuts: its even position is below it
#pragma unroll
                for (uint32_t k = 0; k < 4u; ++k) ke[k] = ve[k] = 0u;
            }
        } else {
            ke[0] = rk.a.x; ke[1] = rk.a.y; ke[2] = rk.a.z; ke[3] = rk.a.w;
            ko[0] = rk.b.x; ko[1] = rk.b.y; ko[2] = rk.b.z; ko[3] = rk.b.w;
            ve[0] = rv.a.x; ve[1] = rv.a.y; ve[2] = rv.a.z; ve[3] = rv.a.w;
            vo[0] = rv.b.x; vo[1] = rv.b.y; vo[2] = rv.b.z; vo[3] = rv.b.w;
        }
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

    if (!(SPLIT && WINDOW) || t_begin < t_end) {              // (workgroup-uniform)
        load_tile(t_begin);
        store_tile(t_begin, lds);
        __syncthreads();
    }
    for (uint32_t tile = t_begin; tile < t_end; ++tile) {
        _Float16* buf = lds + ((tile - t_begin) & 1u) * kBufElems;
        const bool more = tile + 1u < t_end;
        if (more) load_tile(tile + 1u);
        const bool held = tile >= n_pool;
        const uint32_t t_base = held ? 32u * (tile - n_pool) : 32u * tile;
        const uint32_t wave_lo_part = held ? (wave_lo > pos_end ? wave_lo - pos_end : 0u) : wave_lo;
        if (wave_live && (!held || t_base <= wave_t_last) && (!WINDOW || t_base + 31u >= wave_lo_part)) {
            // tree form: the row's word of this held tile (all lanes of a row read the same word), in flight under the products
            uint32_t mword = 0xFFFFFFFFu;
            if (MASKED && held) mword = mrow ? ck_ld<uint32_t>(mrow + (t_base >> 5)) : 0u;
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
            const uint32_t limit = held ? base + j + 1u : pos_end;           // positions of this part the row sees: [0, limit)
            const uint32_t lower = held ? (row_lo > pos_end ? row_lo - pos_end : 0u) : row_lo;     // WINDOW: [lower, limit) of this part
            uint32_t vis = 0u;
            if (MASKED) {
                const uint32_t n_seen = limit > t_base ? limit - t_base : 0u;
                vis = (mword & (n_seen >= 32u ? 0xFFFFFFFFu : (1u << n_seen) - 1u)) >> (4u * g);
            }
            const float* ks = k_scale[(tile - t_begin) & 1u];
            float sv[8], mx = -__builtin_inff();
#pragma unroll
            for (uint32_t i = 0; i < 8u; ++i) {
                const uint32_t t = t_base + 16u * (i >> 2) + 4u * g + (i & 3u);
                const float scale_i = KS == kFp8E4m3 ? scale2 * ks[8u * (i >> 2) + 2u * g + ((i & 3u) >> 1)] : scale2;       // the position's page
                // tree form: bit t & 31 of the word (t_base is a multiple of 32), the causal bound folded into the word
                // (under a window too: a stored position also needs t >= the bound of the row's depth, a held one its bit alone)
                const bool seen = MASKED ? ((vis >> (16u * (i >> 2) + (i & 3u))) & 1u) && (!WINDOW || held || t >= row_lo)
                                  : WINDOW ? t >= lower && t < limit : t < limit;
                sv[i] = seen ? sc[i >> 2][i & 3u] * scale_i : -__builtin_inff();
                mx = fmaxf(mx, sv[i]);
            }
            mx = max_over_kb(mx);
            const float m_new = fmaxf(m_run, mx);
            const float m_use = m_new == -__builtin_inff() ? 0.0f : m_new;  // (a dead row that sees nothing yet)
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
        if (more) store_tile(tile + 1u, lds + ((tile + 1u - t_begin) & 1u) * kBufElems);
        __syncthreads();
    }

    if (SPLIT) {
        // the partial of (item, head): the accumulator as it stands, (m_run, l_run) beside it; dead rows write nothing
        if (row_live) {
            uint8_t* pb = a.part + static_cast<uint64_t>(blockIdx.x) * kChunkPartBytes;
            float* o = reinterpret_cast<float*>(pb) + qr * 128u + 4u * g;
#pragma unroll
            for (uint32_t t = 0; t < 8u; ++t) ck_st<f32x4>(o + 16u * t, acc[t]);
            if (g == 0u) ck_st<u32x2>(pb + kChunkPartAccBytes + 8u * qr, u32x2{__float_as_uint(m_run), __float_as_uint(l_run)});
        }
        return;
    }
    if (row_live) {
        const float inv = 1.0f / l_run;
        float* o = a.out + row_idx * 128u + 4u * g;
#pragma unroll
        for (uint32_t t = 0; t < 8u; ++t) ck_st<f32x4>(o + 16u * t, acc[t] * inv);
        if (a.lse && g == 0u) ck_st<float>(a.lse + row_idx, (m_run + __builtin_amdgcn_logf(l_run)) * kLn2);
    }
}

// The merge of the split form: one workgroup per (flat query block, kv head), thread t = row t >> 2 of the block and the 16-byte
// columns (t & 3) + 4 k.  A live row's n_pieces partials are read in ASCENDING piece order (the result does not depend on how the
// pieces were scheduled): M = max m_p, out = sum acc_p 2^(m_p - M) / sum l_p 2^(m_p - M), lse = (M + log2 sum) ln 2.  A piece that
// saw nothing (m = -inf, l = 0, acc = 0) weighs 2^-inf = 0 exactly.  Whether a row is live is decided as the pieces decided it -- n_q
// and, in the tree form, the row's own mask bit -- never by what the scratch holds: a dead row's partials were not written and are
// not read, and out / lse keep what they held.  Every live row saw itself in the last piece, so its sum is never 0.
__global__ __launch_bounds__(kChunkThreads) void k_chunk_combine(ChunkArgs a)
{
    const uint32_t tid = threadIdx.x;
    const uint32_t h = blockIdx.x % a.heads, fb = blockIdx.x / a.heads;
    uint32_t lo = 0, hi = a.n_seq;
    while (hi - lo > 1u) {
        const uint32_t mid = (lo + hi) >> 1;
        if (static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(a.seqs[mid].first_block)) <= fb) lo = mid; else hi = mid;
    }
    const ChunkSeq* sq = a.seqs + lo;
    const uint32_t seq = lo;
    const uint32_t n_q = __builtin_amdgcn_readfirstlane(sq->n_q), base = __builtin_amdgcn_readfirstlane(sq->base);
    const uint32_t blk = fb - static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(sq->first_block));
    const uint32_t n_pieces = __builtin_amdgcn_readfirstlane(sq->n_pieces);
    const uint32_t item = static_cast<uint32_t>(__builtin_amdgcn_readfirstlane(sq->first_item)) + blk * n_pieces;
    const uint32_t rpp = a.rows_per_pos, per_blk = 64u / rpp;
    const uint32_t qr = tid >> 2, c4 = tid & 3u;
    const uint32_t j = blk * per_blk + qr / rpp, sub = qr % rpp;
    bool row_live = j < n_q;
    if (a.mask && row_live) {
        const uint32_t* mrow = a.mask + (static_cast<uint64_t>(seq) * a.C + j) * a.mask_words;
        row_live = (ck_ld<uint32_t>(mrow + ((base + j) >> 5)) >> ((base + j) & 31u)) & 1u;
    }
    if (!row_live) return;
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
    const uint64_t row_idx = ((static_cast<uint64_t>(seq) * a.C + j) * a.heads + h) * rpp + sub;
    const float inv = 1.0f / l_sum;
    float* o = a.out + row_idx * 128u + 4u * c4;
#pragma unroll
    for (uint32_t k = 0; k < 8u; ++k) ck_st<f32x4>(o + 16u * k, acc[k] * inv);
    if (a.lse && c4 == 0u) ck_st<float>(a.lse + row_idx, (M + __builtin_amdgcn_logf(l_sum)) * kLn2);
}

// The instance of a call, by what its arguments carry: a mask, a partial buffer (pieces: n_items work items and the merge behind
// them; otherwise n_blocks query blocks), a window.
template <int KS, int VS = KS>
hipError_t launch_chunk(const ChunkArgs& a, hipStream_t s)
{
    using Kernel = void (*)(ChunkArgs);
    static constexpr Kernel kInstance[2][2][2] = {                 // [MASKED][SPLIT][WINDOW]
        {{k_attend_chunk<KS, VS, false, false, false>, k_attend_chunk<KS, VS, false, false, true>},
         {k_attend_chunk<KS, VS, false, true, false>, k_attend_chunk<KS, VS, false, true, true>}},
        {{k_attend_chunk<KS, VS, true, false, false>, k_attend_chunk<KS, VS, true, false, true>},
         {k_attend_chunk<KS, VS, true, true, false>, k_attend_chunk<KS, VS, true, true, true>}}};
    hipLaunchKernelGGL(kInstance[a.mask != nullptr][a.part != nullptr][a.window != 0u], dim3((a.part ? a.n_items : a.n_blocks) * a.heads),
                       dim3(kChunkThreads), 0, s, a);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || !a.part) return e;
    hipLaunchKernelGGL(k_chunk_combine, dim3(a.n_blocks * a.heads), dim3(kChunkThreads), 0, s, a);
    return hipGetLastError();
}

} // namespace

hipError_t launch_attend_chunk(const ChunkArgs& a, hipStream_t s)
{
    if (a.n_blocks == 0) return hipSuccess;
    if (!a.seqs || !a.tab || !a.q || !a.k_new || !a.v_new || !a.out || a.n_seq == 0 || a.heads == 0 || a.rows_per_pos == 0 ||
        a.rows_per_pos > 16u || (a.rows_per_pos & (a.rows_per_pos - 1u)) || static_cast<uint64_t>(a.n_blocks) * a.heads > 0x7FFFFFFFull ||
        (a.mask && a.mask_words < (a.C + 32u) / 32u) || (a.mask && a.window && !a.depth) || (a.depth && reinterpret_cast<uintptr_t>(a.depth) % 4u) ||
        (a.part && (a.n_items < a.n_blocks || static_cast<uint64_t>(a.n_items) * a.heads > 0x7FFFFFFFull || reinterpret_cast<uintptr_t>(a.part) % 16u)))
        return hipErrorInvalidValue;
    // the one mixed pair: K pages of an FP8 allocation, V pages of an MXFP4 one (the K8V4 split pool; ChunkSeq::v_table_row)
    if (a.v_scheme != a.scheme) return a.scheme == kFp8E4m3 && a.v_scheme == kMxFp4 ? launch_chunk<kFp8E4m3, kMxFp4>(a, s) : hipErrorInvalidValue;
    switch (a.scheme) {
    case kFp8E4m3: return launch_chunk<kFp8E4m3>(a, s);
    case kInt4G32: return launch_chunk<kInt4G32>(a, s);
    case kMxFp4: return launch_chunk<kMxFp4>(a, s);
    default: return hipErrorInvalidValue;
    }
}

} // namespace speckv
