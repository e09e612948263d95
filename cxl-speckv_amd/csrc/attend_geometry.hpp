// cxl-speckv_amd/csrc/attend_geometry.hpp -- the launch decision of the fused attention as pure host functions.
// Batches: which kernel form runs (batch_form), the split length and the room for pieces (batch_geometry), the pieces of every member (assign_pieces)
// and the dispatch order (batch_dispatch_order).  Engine::attend_batch, attend_batch_plan and attend_planned (engine_attend.cpp) decide with these and
// with nothing else, so the three agree by construction.
// One sequence (Engine::qk_scores_fp8, attend_fp8, attend_int4, attend_mx4): seq_decide gives the placement form, the tiles, the splits, the stream
// form (int4_wg8_stream, mx4_stream), what runs in front of the launch and behind it, and for FP8 the kernel launch_attend_fp8 (attend.hip) runs.
// The CPU tests call the same functions (tests/csrc/host_rules_test.cpp) and replay recorded tables of decisions through them
// (tests/golden/attend_geometry.json, attend_seq_geometry.json).  Plain C++17, no HIP: the tuning keys the rules read come in as values.
#pragma once
#include "ring_rule.hpp"

#include <cmath>
#include <vector>

namespace speckv {

// the tuning keys (tuning.hpp) these rules read: attend_tiles_per_split, attend_order_as_given, attend_fp8_table_regs,
// attend_fp8_striped_table, attend_int4_striped_wg
struct BatchTuning { int32_t tiles_per_split, order_as_given, fp8_table_regs, fp8_striped_table, int4_striped_wg; };
// a batch: the format (neither fp8 nor mx4: INT4_G32), members, kv heads, the CUs of the engine's device, and what the members' placement
// allows: any_striped = a member whose records are not in one run (then the whole launch takes the striped kernels: a single run is
// "striped over 1"), any_table = a member without a regular placement (migrated pages: the launch reads addresses from the page tables)
struct BatchShape { bool fp8, mx4; uint32_t n_seq, heads, cus; bool any_striped, any_table; };
enum BatchEntry : uint32_t { kEntryBatch = 0, kEntryPlan = 1 };

// ---- the form ---------------------------------------------------------------------------------------------------------------
// table / striped: AttendArgs::table_form / stripe_bases; fp8_cls: AttendArgs::fp8_cls; by_class: the members' tiles are counted by residue
// class (ring_rule.hpp mx4_striped_tiles); wg8: AttendArgs::wg8 (0: not the whole-record INT4 kernel, 1: its 16-wave form, 2: one-run workgroups);
// order_round: sequences per round of the CUs for the kernel a batch of this format runs on (0: longest first), see batch_dispatch_order
struct BatchForm { bool table, striped, fp8_cls, int4_cls, by_class; uint32_t wg8, order_round; };

// INT4 batches on the whole-record kernel (k_attend_int4_wg8<2>: workgroups = sequences x splits, one 16-wave workgroup per
// CU resident, its two halves merged in LDS): one round of resident workgroups when the batch is smaller than that, whole
// sequences otherwise (a whole sequence is final: no partials, no merge launch); never under 8 tiles a split.
// More sequences than CUs: workgroups of one run (8 waves, two resident per CU) -- a finishing workgroup's successor starts
// under its neighbour's stream, where a second round of 16-wave workgroups would wait for the whole CU (512 x 1k 0.52 -> 0.54,
// 1024 x 1k 0.56 -> 0.595: profiles/r04_batch_short.txt); AttendArgs::wg8 = 2.
inline uint32_t int4_wg8_form(uint32_t n_seq, uint32_t cus) { return n_seq > cus ? 2u : 1u; }

inline BatchForm batch_form(const BatchShape& s, const BatchTuning& t)
{
    const bool int4 = !s.fp8 && !s.mx4;
    BatchForm f{};
    // FP8 over striped pools, every member placed regularly: the register-staged kernel by residue classes (k_attend_fp8_linear<.., CLS>);
    // on request (tests, A/B) the DMA pipeline with its addresses from the page tables (k_attend_fp8_dma<1>), in page order
    // (measured: batches of 256 x 8k over 7 runs 0.70-0.71 by residue classes against 0.71-0.73 through the page tables -- the table form
    //  stays the default for batches; attend_fp8_striped_table = -1 takes the class form: tests, A/B)
    f.fp8_cls = s.fp8 && s.any_striped && !s.any_table && t.fp8_table_regs == 0 && t.fp8_striped_table < 0;
    f.table = s.any_table || (s.fp8 && s.any_striped && t.fp8_table_regs == 0 && !f.fp8_cls);       // (AttendSeq::lin_base carries the page table in table launches)
    f.striped = s.any_striped && !f.table;
    // INT4_G32, 8 kv heads, every member placed regularly (one run = "striped over 1"): the whole-record kernel by residue classes
    f.int4_cls = int4 && f.striped && s.heads == 8u && t.int4_striped_wg == 0;
    // the striped forms of k_attend_mx4 / k_attend_int4_wg8 / k_attend_fp8_linear count their tiles by residue class
    f.by_class = (s.mx4 || f.int4_cls || f.fp8_cls) && f.striped;
    if (int4 && (!s.any_striped || f.int4_cls) && !f.table && s.heads == 8u) f.wg8 = int4_wg8_form(s.n_seq, s.cus);
    if (s.mx4) f.order_round = 0u;
    else if (int4 && s.heads == 8u) f.order_round = s.cus;                               // whole-record kernel (one column per sequence)
    else f.order_round = std::max(1u, s.cus / std::max(1u, s.heads / 4u));
    return f;
}

// Sequences of different lengths (round 6, profiles/r06_ragged_batches.txt): the order their workgroups are dispatched in decides how evenly the
// CUs are loaded -- a CU receives workgroups i, i + CUs, i + 2 CUs, ... of the launch.  Kernels that keep several workgroups resident per
// CU (FP8: 4; INT4 on one-run workgroups: 2) get the sequences sorted by length and laid out as a serpentine over rounds of `round`
// sequences (one round = the sequences whose workgroups cover the CUs once): a CU then holds a long one with a short one -- 256 sequences
// of 1k .. 16k, FP8: 0.54 of the HBM roofline as given, 0.63 sorted, 0.78 as a serpentine; 512: 0.535 -> 0.79, INT4 0.48 -> 0.67.
// round = 0 (MXFP4, one workgroup per CU): longest first, the short ones fill the tail (512 sequences 0.62 -> 0.84).
// Returns false (order as given, nothing written) when the lengths do not differ by more than a tile in eight.  pages[i] = pages of member i.
inline bool batch_dispatch_order(const BatchForm& f, const BatchTuning& t, const uint32_t* pages, uint32_t n_seq, uint32_t* order)
{
    return t.order_as_given == 0 && dispatch_order_by_length(pages, n_seq, f.order_round, order);           // ring_rule.hpp
}

// ---- the rules for members of equal length ---------------------------------------------------------------------------------------
// INT4 batch launches between half a machine and a whole one of workgroup columns: every long sequence in a long and a short
// piece, dispatched rows-first (ring_rule.hpp: int4_unequal_fraction / unequal_pieces).  The environment switches are for
// measurement runs.
using UnequalSplit = UnequalFraction;
inline UnequalSplit int4_unequal_split(uint32_t n_seq, uint32_t hq, uint32_t tiles_max, const BatchTuning& t)
{
    if (t.tiles_per_split > 0) return {false, 1.0};          // (a forced split length: plain even splits)
    return int4_unequal_fraction(n_seq * hq, tiles_max);
}

// Split length of a batch launch on the 4-head kernels (see the measurements quoted at batch_geometry).  tiles[i] = the tile count of
// sequence i (null: n_seq sequences of uniform_tiles each, the bound a plan is sized for).
inline uint32_t batch_tiles_per_split(bool fp8, uint32_t n_seq, uint32_t heads, const uint32_t* tiles, uint32_t uniform_tiles, const BatchTuning& t)
{
    if (t.tiles_per_split > 0) return static_cast<uint32_t>(t.tiles_per_split);
    const uint32_t hq = heads / 4u;
    // FP8: the busiest-CU cost rule of ring_rule.hpp (48 sequences x 16k: 288 workgroups 0.50 of HBM peak, 192: 0.64,
    // 768: 0.71; 32 x 32k: 256 workgroups 0.79, 512: 0.76, 384: 0.63; 128 x 2k: unsplit 0.73, two splits 0.56)
    if (fp8) return fp8_batch_tiles_per_split(tiles, n_seq, uniform_tiles, hq, 256u, 8u);
    uint64_t total_tiles = tiles ? 0u : static_cast<uint64_t>(uniform_tiles) * n_seq;
    if (tiles) for (uint32_t i = 0; i < n_seq; ++i) total_tiles += tiles[i];
    const uint64_t wg_target = 768u;
    uint32_t tps = static_cast<uint32_t>(std::max<uint64_t>(8, (total_tiles * hq + wg_target - 1u) / wg_target));
    tps = (static_cast<uint64_t>(n_seq) * hq >= 384u) ? 256u : std::min(tps, 256u);   // enough columns: whole sequences
    return tps;
}

// INT4 on the whole-record kernel (the forms: int4_wg8_form above)
inline uint32_t int4_wg8_batch_tps(uint32_t n_seq, uint32_t tiles_max, uint32_t cus, const BatchTuning& t)
{
    if (t.tiles_per_split > 0) return static_cast<uint32_t>(t.tiles_per_split);      // (tests, measurement runs)
    const uint32_t resident = cus;                                        // 16-wave workgroups (two halves each), one per CU
    const uint32_t splits = std::max(1u, resident / std::max(1u, n_seq));
    // more sequences than CUs: the pieces that balance the last round (ring_rule.hpp balanced_tiles_per_piece; 260 x 8k 0.45 -> 0.61
    // of the HBM roofline, 300 0.52 -> 0.67, 340 0.58 -> 0.70, 384 0.63 -> 0.71)
    if (n_seq > resident && tiles_max >= 64u) return balanced_tiles_per_piece(nullptr, n_seq, tiles_max, 1u, resident, kPiecesInt4Wg8);
    // between half a machine and a whole one (the 16-wave form): 130 x 8k 0.43 -> 0.57, 160 0.53 -> 0.64, 200 and up stay whole
    if (2u * n_seq > resident && tiles_max >= 64u) return balanced_tiles_per_piece(nullptr, n_seq, tiles_max, 1u, resident, kPiecesInt4Halves);
    // (the floor was 32 tiles until round 6: with few sequences that left most of the machine idle -- 8 x 8k: 64 workgroups 0.16 of the HBM
    //  roofline, 256 workgroups of 8 tiles 0.34; 16 x 8k 0.32 -> 0.49; 4 x 8k 0.08 -> 0.21)
    return std::max(8u, (tiles_max + splits - 1u) / splits);
}

// MXFP4 batches (k_attend_mx4: one workgroup of 4 waves = the 8 kv heads per (sequence, split), three tiles deep in LDS: ONE
// workgroup resident per CU): one round of resident workgroups -- measured at 256 sequences x 8k: whole sequences (256
// workgroups) 0.77 of the HBM roofline, two splits each 0.73 (profiles/r05_mx4.txt) -- never under 8 tiles a split; a whole
// sequence is final (no partials, no merge launch).
//
// More sequences than half the CUs (round 6): the pieces per sequence that balance the last round of workgroups (ring_rule.hpp
// balanced_tiles_per_piece: 260 x 8k 0.57 -> 0.69 of the HBM roofline, 300 0.65 -> 0.74, 340 0.72 -> 0.78; 360 and up stay whole).
inline uint32_t mx4_batch_tps(uint32_t n_seq, uint32_t tiles_max, uint32_t cus, const BatchTuning& t)
{
    if (t.tiles_per_split > 0) return static_cast<uint32_t>(t.tiles_per_split);      // (tests, measurement runs)
    const uint32_t resident = cus;
    const uint32_t splits = std::max(1u, resident / std::max(1u, n_seq));
    // (up to CUs sequences whole ones run on the 8-wave halves form: pieces pay from 8k context -- 130 x 8k 0.63 -> 0.65, 160 0.71 -> 0.76; 4k: 0.63 -> 0.61, 0.73 -> 0.70)
    if ((n_seq > resident && tiles_max >= 64u) || (2u * n_seq > resident && tiles_max >= 256u)) return balanced_tiles_per_piece(nullptr, n_seq, tiles_max, 1u, resident, kPiecesMx4);
    return std::max(8u, (tiles_max + splits - 1u) / splits);
}

// ---- split length and room ---------------------------------------------------------------------------------------------------------
// tps: AttendArgs::tiles_per_split; piece_tps: the length the members are cut by (assign_pieces); max_splits: AttendArgs::n_splits, the pieces a
// member has at most -- for a plan the ROOM its launches are sized for; rows_first: AttendArgs::rows_first; rule_tps / rule_splits: what the rule
// for equal lengths gives (a plan's room is kept per shape, and that rule is part of the shape: the tuning keys move it); fits: no member in
// more than 2048 pieces (the entries refuse otherwise)
struct BatchRoom { uint32_t max_splits; bool rows_first; };
struct BatchGeometry { uint32_t tps, piece_tps, max_splits; bool rows_first; UnequalSplit unequal; uint32_t rule_tps, rule_splits; bool fits; };

// the pieces of one member of n_tiles: {tiles of a piece (unequal: of the first), pieces}
inline EvenSplit member_pieces(const BatchGeometry& g, uint32_t n_tiles)
{
    // the sequence's tiles divided evenly over its splits (171 + 85 tiles instead of 128 + 128 cost 15 %)
    const EvenSplit es = g.unequal.on ? unequal_pieces(g.unequal, n_tiles) : even_split(n_tiles, (n_tiles + g.piece_tps - 1u) / g.piece_tps);
    return EvenSplit{n_tiles ? es.tiles_per_split : g.piece_tps, es.n_splits};
}

// (MXFP4 -- and INT4_G32 on the whole-record kernel, and FP8 by residue classes -- over striped pools count tiles by residue class: at most
//  ceil(pages / 16) + runs + 1 of them, whatever a member's run count; stripe_n_max is the largest run count of such a plan, 0 otherwise)
inline uint32_t plan_tiles_bound(uint32_t max_pos_end, uint32_t stripe_n_max)
{
    return (max_pos_end / 2u + 15u) / 16u + (stripe_n_max >= 2u ? stripe_n_max + 1u : 0u);
}

// One split length for the whole batch.  A batch brings its own parallelism: the fewer, longer splits the better, down
// to about one round of resident workgroups (256 sequences x 8k context, one layer, FP8: 8 tiles per split 0.50 of
// HBM peak, 32: 0.59, 64: 0.67, 128: 0.72, 256 = no split: 0.74; INT4: 64..128 best, 0.59; at 2k context both
// formats want no split at all).  INT4 target: 768 workgroups, never under 8 tiles per split; FP8: the cost rule of
// batch_tiles_per_split.
// INT4 (arithmetic-bound kernel): splits longer than 256 tiles stop paying (256 sequences x 32k: 256 tiles per split
// 0.67, 512: 0.65, 1024 = no split: 0.60), shorter sequences are best left whole (8k 0.63 against 0.59 in two
// splits, 4k 0.60 / 0.52, 2k 0.58 / 0.43: single-split rows are final, no partials and no merge).
//
// tiles[i] = the tiles of member i (by residue class where form.by_class); by_length = batch_dispatch_order gave an order.
// kEntryBatch (Engine::attend_batch): everything follows from the members' tiles; bound_tiles and kept are not read.
// kEntryPlan (Engine::attend_batch_plan, attend_planned): the launches of a plan may sit in a captured graph, so their grid (pieces per member at
// most) and the presence of the merge launch must not change under it, and so the plan differs from the batch entry in three places:
//  - the rule for equal lengths is taken on the plan's bound (bound_tiles = plan_tiles_bound) for every member -- it depends on the bound only, so
//    plan and launch agree -- and, for INT4 with 8 kv heads, it is the whole-record kernel's WHATEVER the placement (a striped / table launch runs
//    that geometry on the 4-head kernels): a page that migrates between two plans of a shape must not move the captured grid;
//  - the FIRST plan of a shape (members, format, bound) in a buffer fixes max_splits and rows_first -- from the lengths it sees: members of
//    different lengths get room for pieces (ragged_tiles_per_piece) and the rows-first grid -- and every later plan of that shape in that buffer
//    keeps them (kept != null; a later batch that wants more pieces than there is room for gets longer ones).  A new shape (the caller
//    captures anew for it anyway) decides anew;
//  - the room of a first plan is max(8, 32768 / (members x heads)) pieces at most, whatever the lengths ask for.
// attend_planned calls with tiles == null and the kept room of its plan: tps, max_splits and rows_first as the plan decided them.
inline BatchGeometry batch_geometry(BatchEntry entry, const BatchShape& s, const BatchForm& f, const BatchTuning& t, const uint32_t* tiles,
                                    uint32_t bound_tiles, bool by_length, const BatchRoom* kept)
{
    const bool int4 = !s.fp8 && !s.mx4, plan = entry == kEntryPlan;
    uint32_t n_max = 0;
    if (tiles) for (uint32_t i = 0; i < s.n_seq; ++i) n_max = std::max(n_max, tiles[i]);
    const uint32_t tiles_max = plan ? bound_tiles : n_max;
    const bool whole_record = int4 && (plan ? s.heads == 8u : f.wg8 != 0u);
    BatchGeometry g{};
    g.unequal = (s.fp8 || s.mx4 || whole_record) ? UnequalSplit{false, 1.0} : int4_unequal_split(s.n_seq, s.heads / 4u, tiles_max, t);
    g.tps = s.mx4 ? mx4_batch_tps(s.n_seq, tiles_max, s.cus, t) : whole_record ? int4_wg8_batch_tps(s.n_seq, tiles_max, s.cus, t)
          : plan && g.unequal.on ? tiles_max : batch_tiles_per_split(s.fp8, s.n_seq, s.heads, plan ? nullptr : tiles, tiles_max, t);
    g.rule_tps = g.piece_tps = g.tps;
    g.rule_splits = g.unequal.on ? 2u : std::max(1u, (tiles_max + g.tps - 1u) / g.tps);
    // members of different lengths: pieces on account of the lengths (ring_rule.hpp ragged_tiles_per_piece), dispatched by length and rows first
    // (INT4: on the whole-record kernel only)
    uint32_t r = 0;
    if (tiles && (s.fp8 || s.mx4 || f.wg8) && !g.unequal.on && t.tiles_per_split <= 0 && t.order_as_given == 0)
        r = ragged_tiles_per_piece(tiles, s.n_seq, s.cus, s.fp8 ? s.heads / 4u : 1u, s.fp8 ? 4u : 1u);
    if (!plan) {
        if (r && r < g.tps) g.tps = g.piece_tps = r;
        for (uint32_t i = 0; i < s.n_seq; ++i) g.max_splits = std::max(g.max_splits, member_pieces(g, tiles[i]).n_splits);
        // (members of different lengths with pieces: see launch_attend_fp8_batch)
        g.rows_first = (by_length && g.max_splits > 1u) || g.unequal.on;
        g.fits = (n_max + g.tps - 1u) / g.tps <= 2048u;
        return g;
    }
    g.fits = g.rule_splits <= 2048u;
    g.max_splits = g.rule_splits;
    g.rows_first = g.unequal.on;
    if (kept) {
        g.max_splits = kept->max_splits;
        g.rows_first = g.rows_first || kept->rows_first;
    } else if (r && r < g.tps) {
        // (the launches' scratch is sized for members x heads x room: 32 768 partials = 270 MB at most, 8 pieces at least)
        const uint32_t room = std::max(8u, 32768u / std::max(1u, s.n_seq * s.heads));
        g.max_splits = std::max(g.max_splits, std::min(room, (n_max + r - 1u) / r));
        g.rows_first = true;
    }
    if (r && r < g.tps && g.max_splits > 1u) g.piece_tps = std::max(r, (n_max + g.max_splits - 1u) / g.max_splits);      // (pieces on account of the lengths, as many as there is room for)
    // (a first plan whose members differ in length and have pieces -- by whichever rule -- takes the rows-first grid, as the batch entry does)
    if (!kept && by_length && g.max_splits > 1u) g.rows_first = true;
    return g;
}

// ---- pieces per member ------------------------------------------------------------------------------------------------------------
// seqs[i].n_splits holds the tiles of member i on entry; on return its pieces, with tiles_per_split and part_base (the member's first
// partial: heads x pieces partials each).  Returns the partials of the launch.  (Seq = AttendSeq, kernels.hpp)
template <class Seq> inline uint64_t assign_pieces(const BatchGeometry& g, uint32_t heads, Seq* seqs, uint32_t n_seq)
{
    uint64_t parts = 0;
    for (uint32_t i = 0; i < n_seq; ++i) {
        const EvenSplit es = member_pieces(g, seqs[i].n_splits);
        seqs[i].tiles_per_split = es.tiles_per_split;
        seqs[i].n_splits = es.n_splits;
        seqs[i].part_base = static_cast<uint32_t>(parts);
        parts += static_cast<uint64_t>(heads) * es.n_splits;
    }
    return parts;
}

// ---- several layers of one sequence: the stream form --------------------------------------------------------------------------------
// Engine::attend_int4 / attend_mx4 (k_attend_int4_wg8, k_attend_mx4): the launch's n_layers x n_tiles tiles, layer-major, in one contiguous
// piece per workgroup (ring_rule.hpp: the partition) -- one pipeline fill per workgroup, no partial last round, few partials per layer.
// Both decisions return the AttendArgs::stream fields, n_wgs == 0: the fixed grid.  They read two tuning keys as values: attend_splits > 0
// (a forced split count) always takes the fixed grid; attend_stream = N > 0 cuts the call into exactly N pieces whatever its size (tests reach
// the form, and every shape of its partition, with small calls), -1 never streams, 0 decides by size.  The placement (records in one run, or
// INT4_G32 by residue classes) is the caller's condition.
constexpr uint32_t kStreamMinTiles = 896;            // context (tiles of 32 positions) from which several layers of one sequence take the stream form

// the cut of n_layers x n_tiles tiles into n_wgs pieces; none when a piece would be empty or its length not fit 32 bits
inline AttendStream stream_cut(uint32_t n_layers, uint32_t n_tiles, uint64_t n_wgs)
{
    const uint64_t total = static_cast<uint64_t>(n_layers) * n_tiles;
    if (n_wgs == 0u || n_wgs > 0xFFFFFFFFull || total < n_wgs || total / n_wgs > 0xFFFFFFFFull) return AttendStream{};
    AttendStream s{static_cast<uint32_t>(total / n_wgs), static_cast<uint32_t>(total % n_wgs), static_cast<uint32_t>(n_wgs), 1u, 0u};
    for (uint32_t l = 0; l < n_layers; ++l) s.max_slots = std::max(s.max_slots, attend_stream_count(l, n_tiles, s.len, s.rem));
    return s;
}

// INT4_G32 on the whole-record kernel (512-thread workgroups, two resident per CU): as many pieces as workgroups are resident at once.
// Worth it when a piece is long enough to amortise its fill (>= 16 tiles) and from 28k context only (round 6: below it the fixed grid of
// ONE round -- layers x splits <= CUs, whole-layer rows final or merged -- is faster: 80 layers x 4k 0.515 (stream) against 0.567, 8k 0.60 /
// 0.63, 16k 0.64 / 0.66, 24k 0.667 / 0.66, 32k 0.70 / 0.67, 64k 0.71 / 0.69; 70 layers x 4k 0.46 / 0.55; profiles/r06_layers_by_context.txt).
// n_tiles: per layer, by residue class where cls (then also AttendStream::tiles: the merge counts a layer's partials from the same count).
// A ragged last tile (n_pages % 16 != 0) streams like any other: the kernel masks it by its index in the layer, in every layer.
// attend_stream = N > 0: N pieces, the size thresholds bypassed -- but the class form needs pieces of two tiles at least (a one-tile piece
// requests its tile twice, and the second request of a piece that ends a layer is addressed in the regions of the layer behind it, which the
// allocation may not have), and the merge takes 2048 partials a row at most: the fixed grid otherwise.
inline AttendStream int4_wg8_stream(uint32_t n_layers, uint32_t n_tiles, uint32_t cus, bool cls, int32_t attend_splits, int32_t attend_stream)
{
    if (n_layers < 2u || attend_splits > 0 || attend_stream < 0) return AttendStream{};
    const uint64_t total = static_cast<uint64_t>(n_layers) * n_tiles;
    AttendStream s{};
    if (attend_stream > 0) {
        s = stream_cut(n_layers, n_tiles, static_cast<uint64_t>(attend_stream));
        if ((cls && s.len < 2u) || s.max_slots > 2048u) return AttendStream{};
    } else {
        const uint64_t wgs = 2ull * static_cast<uint64_t>(cus);
        if (total < 16u * wgs || n_tiles < kStreamMinTiles) return AttendStream{};
        s = stream_cut(n_layers, n_tiles, wgs);
    }
    if (s.n_wgs && cls) s.tiles = n_tiles;
    return s;
}

// MXFP4, records in one run (k_attend_mx4 form 3; one workgroup per CU and group of eight query rows): one piece per CU, from 28k context
// (round 6: below it the fixed grid is ahead, 80 layers x 2k 0.48 (stream) against 0.55, 4k 0.61 / 0.66, 12k 0.77 / 0.83, 24k 0.81 / 0.82,
// 32k 0.83 / 0.80, 64k 0.84 / 0.75; 70 layers x 4k 0.56 / 0.66, 100 layers x 4k 0.65 / 0.72; profiles/r06_layers_by_context.txt), and only
// where the fixed grid would cut the layers (fixed_splits > 1: a fixed grid of whole layers writes final rows, no partials, no merge).
// Whole tiles only (n_pages % 16 == 0: the kernel's stream form has no ragged last tile).  zgroups = ceil(g / 8).
inline AttendStream mx4_stream(uint32_t n_layers, uint32_t n_tiles, uint32_t n_pages, uint32_t cus, uint32_t zgroups, uint32_t fixed_splits,
                               int32_t attend_splits, int32_t attend_stream)
{
    if (n_layers < 2u || (n_pages & 15u) != 0u || attend_splits > 0 || attend_stream < 0) return AttendStream{};
    const uint64_t total = static_cast<uint64_t>(n_layers) * n_tiles;
    const uint32_t wgs = attend_stream > 0 ? static_cast<uint32_t>(attend_stream) : cus / std::max(1u, zgroups);
    if (attend_stream == 0 && (total < 16ull * wgs || fixed_splits <= 1u || n_tiles < kStreamMinTiles)) return AttendStream{};
    return stream_cut(n_layers, n_tiles, wgs);
}

// ---- one sequence: the launch decision of qk_scores_fp8, attend_fp8, attend_int4 and attend_mx4 -------------------------------------------
// the tuning keys (tuning.hpp) these rules read: attend_general, attend_splits, attend_stream, attend_fp8_table_regs, attend_fp8_striped_table,
// attend_int4_striped_wg, attend_fp8_dma
struct SeqTuning { int32_t general, splits, stream, fp8_table_regs, fp8_striped_table, int4_striped_wg, fp8_dma; };
// a call: the format (neither fp8 nor mx4: INT4_G32), scores = the scores-only entry (qk_scores_fp8), layers, kv heads, query rows per head, the CUs of
// the engine's device, the layout's positions per layer, the range AS ATTENDED (Engine::attend_begin: FP8 over a scale table starts at the table's tile,
// the pages in front of the caller's begin are the skip_pages masked ones) and what the allocation offers: a scale table, its records in one run
// (Allocation::linear_base), the runs of its regular striping (Allocation::stripe_n; 0: no regular placement)
struct SeqShape { bool fp8, mx4, scores; uint32_t n_layers, heads, g, cus, num_tokens, pos_begin, n_pages, skip_pages; bool has_tab, one_run; uint32_t stripe_n; };
// where the record addresses come from -- AttendArgs::lin_base / stripe_bases / table_form; kSeqNone: the FP8 per-wave page-table kernels (k_attend_fp8,
// k_qk_scores_fp8), which take the query from a quantise launch of its own
enum SeqPlace : uint32_t { kSeqNone = 0, kSeqLinear = 1, kSeqStriped = 2, kSeqTable = 3 };
// the kernel launch_attend_fp8 (attend.hip) runs, in the order its branches had them (the class branch has two)
enum Fp8Kernel : uint32_t {
    kFp8NotFp8 = 0,
    kFp8DmaCls = 1,          // k_attend_fp8_dma<2>
    kFp8RegsCls = 2,         // k_attend_fp8_linear<false, false, true>
    kFp8DmaTable = 3,        // k_attend_fp8_dma<1>
    kFp8DmaLinear = 4,       // k_attend_fp8_dma<0>
    kFp8RegsLinear = 5,      // k_attend_fp8_linear<false>
    kFp8RegsStriped = 6,     // k_attend_fp8_linear<true>
    kFp8RegsTable = 7,       // k_attend_fp8_linear<false, true>
    kFp8PerWave = 8,         // k_attend_fp8
};
// place; cls = the tiles are counted by residue class (AttendArgs::fp8_cls, k_attend_int4_wg8<.., CLS>, k_attend_mx4<1>); wg8 = AttendArgs::wg8; n_tiles (by
// class where cls) in the fixed grid's n_splits x tiles_per_split; stream (n_wgs != 0: the stream form); slots = AttendArgs::n_splits, the partials a row
// has (the stream's max_slots, else n_splits); parts = rows x slots, what the scratch is sized for; direct_out = the kernel is handed the output rows
// (AttendArgs::direct_out), rows_final = ... and writes them: no merge launch; zero_page = Engine::ensure_zero_page in front of the launch; quantize_q =
// launch_quantize_q_e4m3 in front of it; kernel: FP8 only
struct SeqDecision {
    SeqPlace place; bool cls; uint32_t wg8, n_tiles, n_splits, tiles_per_split; AttendStream stream; uint32_t slots; uint64_t parts;
    bool direct_out, rows_final, zero_page, quantize_q; Fp8Kernel kernel;
};

// every 32-position tile of the range inside the layer's K / V region (the last one may be ragged)
inline bool seq_fits(const SeqShape& s)
{
    return static_cast<uint64_t>(s.pos_begin) + static_cast<uint64_t>((s.n_pages + 15u) / 16u) * 32u <= s.num_tokens;
}
// what the three formats end with.  seq_even_split: a forced split count, never more than 2048 pieces; seq_partials (once stream and kernel are known):
// the partials per row, and whether the rows are written directly
inline void seq_even_split(SeqDecision& d, uint32_t want, const SeqTuning& t)
{
    if (t.splits > 0) want = static_cast<uint32_t>(t.splits);
    const EvenSplit es = even_split(d.n_tiles, std::max(1u, std::min(want, 2048u)));
    d.n_splits = es.n_splits;
    d.tiles_per_split = es.tiles_per_split;
}
inline void seq_partials(SeqDecision& d, uint32_t rows)
{
    const bool stream = d.stream.n_wgs != 0u;
    d.slots = stream ? d.stream.max_slots : d.n_splits;      // (stream: slots per row)
    d.parts = static_cast<uint64_t>(rows) * d.slots;
    d.direct_out = d.slots == 1u && !stream;                 // no merge launch
    d.rows_final = d.direct_out && d.kernel != kFp8PerWave;  // (the page-table kernel always writes partials)
}

// qk_scores_fp8
inline SeqDecision seq_decide_scores(const SeqShape& s, const SeqTuning& t)
{
    // linear form (records in one run, scale table, tile-aligned range inside the layer's region): direct loads
    const bool fits = s.pos_begin % 32u == 0u && s.has_tab && s.one_run && !t.general && seq_fits(s);
    SeqDecision d{};
    d.place = fits ? kSeqLinear : kSeqNone;
    d.quantize_q = !fits;
    return d;
}

// attend_fp8 (attend.hip)
inline SeqDecision seq_decide_fp8(const SeqShape& s, const SeqTuning& t)
{
    SeqDecision d{};
    // splits: ~20 waves per CU over the launch (the LDS-DMA kernel keeps 8 resident; measured at 70B-shaped, 80 layers:
    // 8 splits/row 0.72 of HBM peak at 32k and 0.63 at 8k, 16 splits 0.705 / 0.61, 4 splits 0.71 / 0.63, 2: 0.63 / 0.58)
    // A launch that already has 128+ workgroup columns (layers x head quads) is best left unsplit: each workgroup then
    // streams one long run, the rows are final (no partials, no merge launch) -- 80 layers: 1 split 0.73 / 0.70 / 0.64 of
    // HBM peak at 32k / 8k / 2k context against 0.71 / 0.62 / 0.48 with 8 splits.
    uint32_t n_tiles = (s.n_pages + 15u) / 16u;
    const uint32_t rows = s.n_layers * s.heads;
    // linear form: records in one run, scale table present, tiles aligned with the table's (pos_begin a multiple of 32),
    // and the last (possibly ragged) 32-position tile must not read past the K / V region of its layer
    // (with the range aligned as above and num_tokens a multiple of 32 the tiles never leave the region)
    const bool fits = s.has_tab && seq_fits(s);
    const bool general_env = t.general != 0;
    const bool linear = !general_env && fits && s.one_run;
    // regular striping over several pools: the same kernel with computed record addresses (no page-table chase)
    const bool striped = !linear && fits && s.stripe_n >= 2 && !general_env;
    // no regular placement (pages migrated one by one), or SPECKV_ATTEND_GENERAL set (measurements, tests): the fast kernel
    // with its record addresses from the page table, looked up one request ahead
    const bool table = fits && !linear && !striped;
    // (the page-table form has nothing to gain from whole rows: it hides its look-ups behind other waves and always
    // goes through the merge -- 80 layers x 8k: one split 0.13 of HBM peak, eight 0.18+)
    // (striped / moved placements run the same DMA pipeline with their addresses from the page table, k_attend_fp8_dma<TABLE>: the
    //  same rule; the register-staged kernels of rounds 2-5 -- a range that starts inside a tile, or on request -- want the splits)
    const bool dma_table = (striped || table) && s.skip_pages == 0 && t.fp8_table_regs == 0;
    // striped regularly: the linear pipeline over the range's pages by residue class (k_attend_fp8_dma<2>): the tiles are then counted per class
    const bool cls = striped && dma_table && s.stripe_n <= 8 && t.fp8_striped_table <= 0;
    if (cls) n_tiles = mx4_striped_tiles(s.n_pages, s.stripe_n);
    uint32_t want = ((linear || dma_table) && rows / 4u >= 128u && n_tiles < 768u) ? 1u : (5120u + rows - 1u) / rows;     // (32k and beyond: 8 splits, below)
    // per-layer calls are latency-bound: short contexts want short splits (measured best: 2 tiles per split at 2k
    // context, 4 at 8k, 8 at 32k), long multi-layer launches are bounded by `want` above
    const uint32_t min_tiles = std::min(8u, std::max(2u, n_tiles / 64u));
    want = std::min(want, std::max(1u, n_tiles / min_tiles));
    // ... and never more than ONE round of workgroups (round 6, profiles/r06_layers_by_context.txt: one layer x 128k took 512 splits = 1024
    // workgroups 0.55 of the roofline, 128 splits = 256 workgroups 0.68; 4 layers x 32k 0.65 -> 0.74, 8 x 32k 0.59 -> 0.68, 12 x 16k 0.56 -> 0.65)
    if (linear || dma_table) want = std::min(want, std::max(1u, s.cus / std::max(1u, rows / 4u)));
    // Launches of many rows (several layers of one sequence): every workgroup resident at once and the CUs evenly loaded counts for
    // more than the split length -- 80 layers = 160 workgroup rows: 3 splits = 480 workgroups (15 of 16 CUs hold two) 0.777 of the
    // roofline at 32k and 0.738 at 8k, 5 splits = 800 (some CUs four, some three) 0.67, 8 = 1280 (a second round) 0.765, one split
    // (the DMA kernel, 160 of 256 CUs busy) 0.73 / 0.70; 32 layers x 32k: 4 splits = 256 workgroups 0.734, 20 splits 0.72.
    // So: the split count whose workgroups fill whole rounds of the CUs best, one round at most, splits of 64 tiles or more.
    // (A stream form as the INT4 / MXFP4 kernels have it -- the launch's rows x tiles in one equal piece per resident workgroup --
    //  was built for k_attend_fp8_linear and dropped: at the kernel's 128 registers the row-boundary path spilled, and the extra
    //  partials cost the short contexts more than the balance gave: 32k x 80 0.7635 against 0.7745, 8k 0.66 / 0.74, 128k 0.794 / 0.783.)
    if ((linear || cls) && rows / 4u >= 32u) {
        const uint32_t wg_rows = rows / 4u, n_cu = s.cus;
        uint32_t best_s = 1;
        double best = -1.0;
        for (uint32_t sp = 1; sp <= 16u; ++sp) {
            // (pieces under 64 tiles -- never under 16 -- only while the launch has not filled one round: 32 layers x 2k were 64 workgroups 0.36 of the
            //  roofline, 8 pieces 0.56; 4k: 128 workgroups 0.64, 8 pieces 0.685)
            if (sp > 1u && (n_tiles / sp < 16u || (n_tiles / sp < 64u && static_cast<uint64_t>(wg_rows) * (sp - 1u) >= n_cu))) break;
            const uint64_t wgs = static_cast<uint64_t>(wg_rows) * sp, cap = static_cast<uint64_t>(sp == 1u ? 2u : 4u) * n_cu;      // (resident: DMA kernel 2 per CU, register-staged 4)
            if (wgs > cap && sp > 1u) break;
            const double per_cu = static_cast<double>(wgs) / n_cu, score = per_cu / std::ceil(per_cu);
            if (score > best + 1e-9) { best = score; best_s = sp; }
        }
        want = best_s;
    }
    d.place = linear ? kSeqLinear : striped ? kSeqStriped : table ? kSeqTable : kSeqNone;
    d.cls = cls;
    d.n_tiles = n_tiles;
    seq_even_split(d, want, t);
    // one long split per row: the LDS-DMA kernel (two tiles deep per wave, 8 waves per CU); several shorter splits: the
    // register-staged one (16 waves per CU hide more) -- 80 layers x 32k: 8 splits 0.756 (register-staged) / 0.72 (DMA),
    // 1 split 0.58 / 0.73; 8k: 1 split DMA 0.69, 8 splits 0.63 / 0.62
    // (launches with few workgroup columns -- the per-layer calls of one sequence -- are latency-bound either way: DMA kernel,
    // 13.8 against 15.5 us at 8k context)
    const bool dma_shape = d.n_splits == 1u || s.n_layers * (s.heads / 4u) < 128u;
    if (cls) d.kernel = dma_shape ? kFp8DmaCls : kFp8RegsCls;         // striped regularly: the linear kernels over residue classes, by the linear forms' rule
    else if (dma_table) d.kernel = kFp8DmaTable;                       // moved page by page (or striped, on request): the DMA pipeline with addresses from the page table
    else if (linear && t.fp8_dma >= 0 && (dma_shape || t.fp8_dma > 0)) d.kernel = kFp8DmaLinear;
    else if (linear) d.kernel = kFp8RegsLinear;
    else if (striped) d.kernel = kFp8RegsStriped;
    else if (table) d.kernel = kFp8RegsTable;
    else d.kernel = kFp8PerWave;
    d.zero_page = true;                                                // (every form: the kernels are handed the page whether or not they read it)
    d.quantize_q = d.place == kSeqNone;                                // the linear / striped / table forms quantise the query in their own prologue
    seq_partials(d, rows);
    return d;
}

// Launch geometry of the whole-record INT4 kernel (k_attend_int4_wg8; 512-thread workgroups, two resident per CU); `cus` = the
// compute units of the ENGINE's device (Engine::cus()).  Its stream form for many layers of one sequence: int4_wg8_stream above.
// Fixed grid (per-layer calls, short launches): splits x layers workgroups, in whole rounds of the resident set when the
// launch is that long, else as many 8-tile pieces as there are.
inline uint32_t int4_wg8_splits(uint32_t n_layers, uint32_t n_tiles, uint32_t cus)
{
    const uint64_t resident = static_cast<uint64_t>(cus);                 // (16-wave workgroups, two halves each: one per CU)
    const uint64_t total = static_cast<uint64_t>(n_layers) * n_tiles;
    uint64_t wgs = std::max<uint64_t>(1, total / 64u);
    if (wgs >= resident && n_layers >= 2u) wgs = resident;                        // several layers: ONE round (80 layers x 16k: 3 splits 0.65, 6: 0.63, 10: 0.54)
    else if (wgs >= resident) wgs = (wgs + resident / 2u) / resident * resident;  // whole rounds
    else wgs = std::min<uint64_t>(resident, std::max<uint64_t>(wgs, total / 8u));
    const uint64_t per_layer = std::max<uint64_t>(1, n_layers >= 2u ? wgs / n_layers : (wgs + n_layers / 2u) / n_layers);
    return static_cast<uint32_t>(std::min<uint64_t>(per_layer, std::max<uint32_t>(1u, n_tiles / 4u)));
}

// attend_int4 (attend_int4.hip)
inline SeqDecision seq_decide_int4(const SeqShape& s, const SeqTuning& t)
{
    SeqDecision d{};
    uint32_t n_tiles = (s.n_pages + 15u) / 16u;
    // linear form: records in one local run and every 32-position tile inside the layer's K / V region; otherwise the
    // page-table form of the same kernel
    const bool fits = seq_fits(s);
    const bool general_env = t.general != 0;
    const bool linear = s.one_run && fits && !general_env;
    const bool striped = !linear && s.stripe_n >= 2 && fits && !general_env;
    // a pool striped over 2..8 runs, 8 kv heads: the whole-record kernel over the range's pages by residue class (every tile 16
    // consecutive records of one run: the linear form's fetch; k_attend_int4_wg8<.., CLS>)
    const bool cls = striped && s.heads == 8 && s.stripe_n <= 8 && t.int4_striped_wg == 0;
    if (cls) n_tiles = mx4_striped_tiles(s.n_pages, s.stripe_n);
    // everything else -- no regular placement, a last tile that would leave the region, SPECKV_ATTEND_GENERAL (measurements,
    // tests) -- takes the workgroup kernel with its record addresses from the page table: its look-ups are clamped to the
    // range, so a ragged last tile never reads a record it has no business with.  (The per-wave page-table kernel of rounds
    // 1-3, 0.37 of HBM peak, is gone.)
    d.place = linear ? kSeqLinear : striped ? kSeqStriped : kSeqTable;
    const uint32_t rows = s.n_layers * s.heads;
    uint32_t want = (5120u + rows - 1u) / rows;      // VALU-bound kernel: fewer, longer splits measured best
    const uint32_t min_tiles = std::min(8u, std::max(2u, n_tiles / 64u));      // per-layer calls: see seq_decide_fp8
    want = std::min(want, std::max(1u, n_tiles / min_tiles));
    // Workgroups go to the 8 XCDs round-robin by linear id = split + n_splits * (layer, head quad): with a split count that
    // is a multiple of 8 the two workgroups that share a page's scale line (head quads 0 and 1) run on the same XCD, next
    // to each other (measured at 32k x 80 layers: 8 splits 0.598, 10 or 12 splits 0.56, 16 splits 0.595)
    if (want > 8u) want &= ~7u;
    // whole-record kernel (8 waves = 8 heads, one workgroup per CU): workgroups = splits x layers, in whole rounds of the CUs
    const bool wg8 = (linear || cls) && s.heads == 8;
    if (wg8) want = int4_wg8_splits(s.n_layers, n_tiles, s.cus);
    d.cls = cls;
    d.wg8 = wg8 ? 1u : 0u;
    d.n_tiles = n_tiles;
    seq_even_split(d, want, t);
    if (!wg8 && d.n_splits > 8u && (d.n_splits & 7u) && t.splits <= 0) {      // the rounding can fall off a multiple of 8
        const EvenSplit es = even_split(n_tiles, d.n_splits & ~7u);
        d.n_splits = es.n_splits;
        d.tiles_per_split = es.tiles_per_split;
    }
    // several layers of one long sequence: the stream form (int4_wg8_stream above; SPECKV_ATTEND_STREAM cuts small calls for the tests)
    if (wg8) d.stream = int4_wg8_stream(s.n_layers, n_tiles, s.cus, cls, t.splits, t.stream);
    d.zero_page = !linear;
    seq_partials(d, rows);
    return d;
}

// attend_mx4 (attend_mx4.hip)
inline SeqDecision seq_decide_mx4(const SeqShape& s, const SeqTuning& t)
{
    SeqDecision d{};
    uint32_t n_tiles = (s.n_pages + 15u) / 16u;
    // arithmetic addresses need every 32-position tile inside the layer's K / V region (the last one may be ragged); otherwise,
    // or without a regular placement, the page-table form: its look-ups are clamped to the range
    const bool fits = seq_fits(s);
    const bool general_env = t.general != 0;
    const bool linear = s.one_run && fits && !general_env;
    // a pool striped over 2..8 runs: the range's pages by residue class of the page index (every tile 16 consecutive records of one
    // run: the linear form's fetch), whatever the range -- rows past a class's end are masked, nothing needs to "fit"
    const bool striped = !linear && s.stripe_n >= 2 && s.stripe_n <= 8 && !general_env;
    const bool table = !linear && !striped;
    if (striped) n_tiles = mx4_striped_tiles(s.n_pages, s.stripe_n);
    // workgroups = splits x layers x query-row groups (each covers the 8 kv heads; one resident per CU): one round of the CUs,
    // rounded down -- 80 layers at 32k: 3 splits (240 workgroups) 0.765 of the HBM roofline, 6 splits 0.72-0.75 (profiles/r05_mx4.txt)
    const uint32_t rows = s.n_layers * s.heads;
    const uint32_t columns = s.n_layers * ((s.g + 7u) / 8u);
    uint32_t want = std::max(1u, (table ? 2u : 1u) * s.cus / columns);          // (the page-table form: two workgroups per CU)
    const uint32_t min_tiles = std::min(8u, std::max(2u, n_tiles / 64u));      // per-layer calls: see seq_decide_fp8
    want = std::min(want, std::max(1u, n_tiles / min_tiles));
    d.place = linear ? kSeqLinear : striped ? kSeqStriped : kSeqTable;
    d.cls = striped;
    d.n_tiles = n_tiles;
    seq_even_split(d, want, t);
    // several layers of one long sequence: the stream form -- all tiles of the call in layer-major order cut into one equal piece
    // per CU (80 layers x 3 splits of the fixed grid occupy 240 CUs of 256; profiles/r05_mx4.txt); the decision: mx4_stream above
    if (linear) d.stream = mx4_stream(s.n_layers, n_tiles, s.n_pages, s.cus, (s.g + 7u) / 8u, d.n_splits, t.splits, t.stream);
    d.zero_page = table;
    seq_partials(d, rows);
    return d;
}

inline SeqDecision seq_decide(const SeqShape& s, const SeqTuning& t)
{
    return s.scores ? seq_decide_scores(s, t) : s.fp8 ? seq_decide_fp8(s, t) : s.mx4 ? seq_decide_mx4(s, t) : seq_decide_int4(s, t);
}

} // namespace speckv
