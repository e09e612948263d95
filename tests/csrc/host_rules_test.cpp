// tests/csrc/host_rules_test.cpp -- TEST-ONLY C wrappers around the header-only host/device rules of the engine
// (ring_rule.hpp: ring run / liveness arithmetic, even splits, the stream partition; attend_geometry.hpp: the launch decision of the batched attention and of
// the single-sequence entries, the stream decision of the INT4_G32 / MXFP4 attention among them), for the CPU property tests.
#include "../../cxl-speckv_amd/csrc/attend_geometry.hpp"

extern "C" {
void rules_ring_take(uint32_t seq, uint32_t m, uint32_t n, uint32_t* out3)
{
    const speckv::RingRun r = speckv::ring_take(seq, m, n);
    out3[0] = r.seq; out3[1] = r.slot; out3[2] = r.next;
}
int rules_ring_live(uint32_t seq, uint32_t q, uint32_t n) { return speckv::ring_live(seq, q, n) ? 1 : 0; }
void rules_even_split(uint32_t n_tiles, uint32_t want, uint32_t* out2)
{
    const speckv::EvenSplit e = speckv::even_split(n_tiles, want);
    out2[0] = e.tiles_per_split; out2[1] = e.n_splits;
}
uint32_t rules_fp8_batch_tiles_per_split(const uint32_t* tiles, uint32_t n_seq, uint32_t uniform_tiles, uint32_t columns_per_seq, uint32_t n_cus)
{
    return speckv::fp8_batch_tiles_per_split(tiles, n_seq, uniform_tiles, columns_per_seq, n_cus);
}
// model: 0 = MXFP4 (k_attend_mx4), 1 = FP8, 2 = INT4 on the whole-record kernel (one-run workgroups), 3 = the same, 16-wave form
uint32_t rules_balanced_tiles_per_piece(const uint32_t* tiles, uint32_t n_seq, uint32_t uniform_tiles, uint32_t columns_per_seq, uint32_t n_cus, uint32_t model)
{
    const speckv::PieceModel& m = model == 0u ? speckv::kPiecesMx4 : model == 1u ? speckv::kPiecesFp8 : model == 2u ? speckv::kPiecesInt4Wg8 : speckv::kPiecesInt4Halves;
    return speckv::balanced_tiles_per_piece(tiles, n_seq, uniform_tiles, columns_per_seq, n_cus, m);
}
uint32_t rules_ragged_tiles_per_piece(const uint32_t* tiles, uint32_t n_seq, uint32_t n_cus, uint32_t model)
{
    return speckv::ragged_tiles_per_piece(tiles, n_seq, n_cus, model == 1u ? 2u : 1u, model == 1u ? 4u : 1u);          // (model 1 = FP8 with 8 kv heads: two workgroup columns per member)
}
int rules_dispatch_order(const uint32_t* len, uint32_t n, uint32_t round, uint32_t* order) { return speckv::dispatch_order_by_length(len, n, round, order) ? 1 : 0; }
// {on, first piece, pieces} of a sequence of n_tiles in an INT4 batch of `columns` workgroup columns whose longest member has tiles_max
void rules_int4_unequal(uint32_t columns, uint32_t tiles_max, uint32_t n_tiles, uint32_t* out3)
{
    const speckv::UnequalFraction u = speckv::int4_unequal_fraction(columns, tiles_max);
    const speckv::EvenSplit e = u.on ? speckv::unequal_pieces(u, n_tiles) : speckv::EvenSplit{n_tiles ? n_tiles : 1u, n_tiles ? 1u : 0u};
    out3[0] = u.on ? 1u : 0u; out3[1] = e.tiles_per_split; out3[2] = e.n_splits;
}

// ---- attend_geometry.hpp: the functions Engine::attend_batch / attend_batch_plan / attend_planned decide with (tests/_rules.py drives them)
// shape7 = {fp8, mx4, n_seq, heads, cus, any_striped, any_table}; tun5 = {attend_tiles_per_split, attend_order_as_given, attend_fp8_table_regs,
// attend_fp8_striped_table, attend_int4_striped_wg}
static speckv::BatchShape shape_of(const uint32_t* s) { return speckv::BatchShape{s[0] != 0u, s[1] != 0u, s[2], s[3], s[4], s[5] != 0u, s[6] != 0u}; }
static speckv::BatchTuning tuning_of(const int32_t* t) { return speckv::BatchTuning{t[0], t[1], t[2], t[3], t[4]}; }
// out7 = {table, striped, fp8_cls, int4_cls, by_class, wg8, order_round}
void rules_batch_form(const uint32_t* shape7, const int32_t* tun5, uint32_t* out7)
{
    const speckv::BatchForm f = speckv::batch_form(shape_of(shape7), tuning_of(tun5));
    out7[0] = f.table; out7[1] = f.striped; out7[2] = f.fp8_cls; out7[3] = f.int4_cls; out7[4] = f.by_class; out7[5] = f.wg8; out7[6] = f.order_round;
}
int rules_batch_dispatch_order(const uint32_t* shape7, const int32_t* tun5, const uint32_t* pages, uint32_t* order)
{
    const speckv::BatchShape s = shape_of(shape7);
    return speckv::batch_dispatch_order(speckv::batch_form(s, tuning_of(tun5)), tuning_of(tun5), pages, s.n_seq, order) ? 1 : 0;
}
uint32_t rules_plan_tiles_bound(uint32_t max_pos_end, uint32_t stripe_n_max) { return speckv::plan_tiles_bound(max_pos_end, stripe_n_max); }
// entry 0: the batch entry, 1: a plan (kept_splits >= 0: the room its shape's first plan fixed; tiles null: as attend_planned asks).
// out8 = {tps, piece_tps, max_splits, rows_first, unequal, rule_tps, rule_splits, fits}; pieces (may be null, needs tiles) = {tiles_per_split, n_splits,
// part_base} per member; returns the partials of the launch (0 without pieces)
uint64_t rules_batch_geometry(uint32_t entry, const uint32_t* shape7, const int32_t* tun5, const uint32_t* tiles, uint32_t bound_tiles, uint32_t by_length,
                              int32_t kept_splits, int32_t kept_rows_first, uint32_t* out8, uint32_t* pieces)
{
    const speckv::BatchShape s = shape_of(shape7);
    const speckv::BatchTuning t = tuning_of(tun5);
    const speckv::BatchRoom kept{static_cast<uint32_t>(kept_splits), kept_rows_first != 0};
    const speckv::BatchGeometry g = speckv::batch_geometry(entry ? speckv::kEntryPlan : speckv::kEntryBatch, s, speckv::batch_form(s, t), t, tiles, bound_tiles,
                                                           by_length != 0u, kept_splits >= 0 ? &kept : nullptr);
    out8[0] = g.tps; out8[1] = g.piece_tps; out8[2] = g.max_splits; out8[3] = g.rows_first; out8[4] = g.unequal.on; out8[5] = g.rule_tps; out8[6] = g.rule_splits; out8[7] = g.fits;
    if (!pieces || !tiles || !g.fits) return 0;
    struct Seq { uint32_t n_splits, tiles_per_split, part_base; };
    std::vector<Seq> seqs(s.n_seq);
    for (uint32_t i = 0; i < s.n_seq; ++i) seqs[i].n_splits = tiles[i];
    const uint64_t parts = speckv::assign_pieces(g, s.heads, seqs.data(), s.n_seq);
    for (uint32_t i = 0; i < s.n_seq; ++i) { pieces[3 * i] = seqs[i].tiles_per_split; pieces[3 * i + 1] = seqs[i].n_splits; pieces[3 * i + 2] = seqs[i].part_base; }
    return parts;
}

// ---- the stream form of several layers of one sequence: the partition (ring_rule.hpp) and the two decisions (attend_geometry.hpp)
uint64_t rules_stream_begin(uint32_t w, uint32_t len, uint32_t rem) { return speckv::attend_stream_begin(w, len, rem); }
uint32_t rules_stream_wg_of(uint64_t G, uint32_t len, uint32_t rem) { return speckv::attend_stream_wg_of(G, len, rem); }
uint32_t rules_stream_count(uint32_t layer, uint32_t n_tiles, uint32_t len, uint32_t rem) { return speckv::attend_stream_count(layer, n_tiles, len, rem); }
static void stream_out(const speckv::AttendStream& s, uint32_t* out5) { out5[0] = s.n_wgs; out5[1] = s.len; out5[2] = s.rem; out5[3] = s.max_slots; out5[4] = s.tiles; }
// out5 = {n_wgs (0: the fixed grid), len, rem, max_slots, tiles}
void rules_int4_wg8_stream(uint32_t n_layers, uint32_t n_tiles, uint32_t cus, uint32_t cls, int32_t attend_splits, int32_t attend_stream, uint32_t* out5)
{
    stream_out(speckv::int4_wg8_stream(n_layers, n_tiles, cus, cls != 0u, attend_splits, attend_stream), out5);
}
void rules_mx4_stream(uint32_t n_layers, uint32_t n_tiles, uint32_t n_pages, uint32_t cus, uint32_t zgroups, uint32_t fixed_splits, int32_t attend_splits,
                      int32_t attend_stream, uint32_t* out5)
{
    stream_out(speckv::mx4_stream(n_layers, n_tiles, n_pages, cus, zgroups, fixed_splits, attend_splits, attend_stream), out5);
}
uint32_t rules_striped_tiles(uint32_t n_pages, uint32_t stripe_n) { return speckv::mx4_striped_tiles(n_pages, stripe_n); }
uint32_t rules_int4_wg8_splits(uint32_t n_layers, uint32_t n_tiles, uint32_t cus) { return speckv::int4_wg8_splits(n_layers, n_tiles, cus); }

// ---- attend_geometry.hpp: what Engine::qk_scores_fp8 / attend_fp8 / attend_int4 / attend_mx4 decide with (tests/_rules.py decide_seq)
// shape14 = {fp8, mx4, scores, n_layers, heads, g, cus, num_tokens, pos_begin, n_pages, skip_pages, has_tab, one_run, stripe_n}; tun7 = {attend_general,
// attend_splits, attend_stream, attend_fp8_table_regs, attend_fp8_striped_table, attend_int4_striped_wg, attend_fp8_dma}
// out17 = {place, cls, wg8, n_tiles, n_splits, tiles_per_split, stream len, rem, n_wgs, max_slots, tiles, slots, direct_out, rows_final, zero_page,
// quantize_q, kernel}; returns the partials
uint64_t rules_seq_decide(const uint32_t* s, const int32_t* t, uint32_t* out17)
{
    const speckv::SeqShape shape{s[0] != 0u, s[1] != 0u, s[2] != 0u, s[3], s[4], s[5], s[6], s[7], s[8], s[9], s[10], s[11] != 0u, s[12] != 0u, s[13]};
    const speckv::SeqDecision d = speckv::seq_decide(shape, speckv::SeqTuning{t[0], t[1], t[2], t[3], t[4], t[5], t[6]});
    const uint32_t out[17] = {d.place, d.cls, d.wg8, d.n_tiles, d.n_splits, d.tiles_per_split, d.stream.len, d.stream.rem, d.stream.n_wgs, d.stream.max_slots,
                              d.stream.tiles, d.slots, d.direct_out, d.rows_final, d.zero_page, d.quantize_q, d.kernel};
    std::copy(out, out + 17, out17);
    return d.parts;
}
}
