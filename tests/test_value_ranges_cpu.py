"""No GPU: the data sets of tests/_value_ranges.py are what they claim, the bound of the GPU test is decided here, and it would catch faults.

1. Conditions on every data set, in the float64 reference over the oracle's records (properties of the data and of the reference alone):
   the score error bound delta of HeadChecker <= 2e-3 (ramps: 4e-3) in the 8-bit formats; sum p|v| >= 1e-3 on >= 99 % of the checked elements
   (the absolute 1e-6 never carries the bound; ties-v0, whose V is zero, is the stated exception: its out must be exactly 0); and what the
   data set's dict claims -- the needle's weight, the tile maxima of a ramp and the distance of the two partial maxima, the ladder.
2. The tiers: model err / project bound per (profile, format), worst over the data sets, both ranges and every head; <= 0.5 is tier 1 (held to
   the project bound), anything else tier 2 (bound + 2 x term).  The table must be the one _value_ranges.TIERS and DESIGN.md state.  A tier-2
   profile keeps 2 x term <= 0.05 sum p|v| on >= 90 % of its elements: the wider bound is still a test.
3. Three deliberately wrong models each exceed their tier's bound by >= 10 x on a named data set."""
import os

import numpy as np
import pytest

from tests import _value_ranges as vr
from tests._gpu import H

FORMATS = (vr.FP8, vr.INT4, vr.MX4, vr.K8V4)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _layouts(fmt):
    return (256, 250) if fmt == vr.FP8 else (256,)                  # T = 250: the per-wave FP8 kernel's layout


@pytest.mark.parametrize("name", vr.DATASETS)
def test_every_data_set_meets_the_conditions(oracle, name):
    prof = vr.PROFILE_OF[name]
    for fmt in FORMATS:
        for T in _layouts(fmt):
            r = vr.ratios(oracle, name, fmt, T)
            assert r["delta"] <= vr.DELTA_MAX.get(prof, 2e-3), (name, vr.NAMES[fmt], T, r["delta"])
            if name != "ties-v0":
                assert r["mag_share"] >= 0.99, (name, vr.NAMES[fmt], T, r["mag_share"])
            if vr.TIERS[prof] == 2:
                assert r["term_share"] >= 0.90, (name, vr.NAMES[fmt], T, r["term_share"])
            assert r["ratio"] <= 0.5, (name, vr.NAMES[fmt], T, "the model itself must sit well inside the bound of its tier", r["ratio"])


def _weights(oracle, name, fmt, T, head, n):
    ds = vr.dataset(name, T)
    p, l, mx, V, vs = vr.checker(oracle, name, T, fmt).weight_rows(ds["q"][1, head], head, n, ds["sm"])
    return p, l, mx, V, vs


@pytest.mark.parametrize("name", vr.PROFILES["sink"])
def test_the_sink_takes_its_share_of_every_row(oracle, name):
    claims = vr.dataset(name)["claims"]
    for fmt in FORMATS:
        for T in _layouts(fmt):
            ds = vr.dataset(name, T)
            e, needle = ds["claims"]["ladder"], ds["claims"]["needle"]
            tile = slice(needle // 32 * 32, needle // 32 * 32 + 32)
            assert e[needle] == (e.min() if "tile" in name else e[tile].min())               # the smallest-V tile / page of its tile
            for n in vr.RANGES:
                if n > T or needle >= n:
                    continue
                for head in range(H):
                    p, l, _, _, _ = _weights(oracle, name, fmt, T, head, n)
                    assert np.all(p[:, needle] / l >= claims["weight"]), (name, vr.NAMES[fmt], T, n, head, float((p[:, needle] / l).min()))
                    rest = np.delete(p, needle, axis=1)
                    assert (rest < 2.0 ** -14).mean() >= 0.99, "the other weights sit in the fp16 subnormals"


@pytest.mark.parametrize("name", ["ramp-up", "ramp-down"])
def test_the_ramps_move_the_maximum_in_every_tile(oracle, name):
    claims = vr.dataset(name)["claims"]
    for fmt in FORMATS:
        for T in _layouts(fmt):
            for n in vr.RANGES:
                if n > T:
                    continue
                for head in range(H):
                    p, l, mx, _, _ = _weights(oracle, name, fmt, T, head, n)
                    with np.errstate(divide="ignore"):
                        s = np.log(p) + mx[:, None]
                    tmax = np.stack([s[:, t:t + 32].max(axis=1) for t in range(0, n, 32)], axis=1)            # [G][8]
                    steps = np.diff(tmax, axis=1) * claims["direction"]
                    assert np.all((steps >= claims["step"]).sum(axis=1) >= claims["steps"]) and np.all(steps > 0), (name, vr.NAMES[fmt], T, n, head)
                    gap = np.abs(tmax[:, :4].max(axis=1) - tmax[:, 4:].max(axis=1)) / np.log(2.0)             # two splits of 4 tiles
                    assert np.all(gap >= claims["split_gap_log2"]), (name, vr.NAMES[fmt], T, n, head, float(gap.min()))


def test_the_ladders_and_ties_are_in_the_records(oracle):
    for fmt in FORMATS:
        for name, span in (("v-tile-ladder", 14.0), ("v-page-ladder", 8.0)):
            e = vr.dataset(name)["claims"]["ladder"]
            assert e.max() - e.min() == span
            if name == "v-tile-ladder":
                assert all(len(set(e[t:t + 32])) == 1 for t in range(0, 256, 32)) and len(set(e)) == 8
            else:
                assert all(e[t:t + 32].max() - e[t:t + 32].min() == span for t in range(0, 256, 32))
            for head in range(H):
                V = vr.checker(oracle, name, 256, fmt).kv(head)[1]
                rms = np.sqrt((V * V).mean(axis=1))
                assert np.all(np.abs(np.log2(rms) - e) < 0.6), (name, vr.NAMES[fmt], head)                     # the records hold the ladder
                assert np.abs(V).max() <= 65504.0
        for head in range(H):
            for n in vr.RANGES:
                p, l, mx, V, _ = _weights(oracle, "ties-k0", fmt, 256, head, n)
                assert np.all(p == 1.0) and np.all(mx == 0.0)                                                   # every score exactly 0
                want, wlse, _, _ = vr.checker(oracle, "ties-k0", 256, fmt).want_rows(vr.dataset("ties-k0")["q"][1, head][None], head, [n], vr.SM)
                assert np.allclose(want[0], V.mean(axis=0)[None], rtol=1e-12, atol=1e-12) and np.all(wlse == np.log(n))
            assert not vr.checker(oracle, "ties-v0-tile", 256, fmt).kv(head)[1][:32].any()
            assert vr.checker(oracle, "ties-v0-tile", 256, fmt).kv(head)[1][32:].any()
            assert not vr.checker(oracle, "ties-v0", 256, fmt).kv(head)[1].any()
            out, lse = vr.model_rows(vr.checker(oracle, "ties-v0", 256, fmt), vr.dataset("ties-v0")["q"][1, head][None], head, [256], vr.SM)
            assert not out.any() and np.all(np.isfinite(lse))


def test_the_query_rows_are_what_they_claim():
    q = vr.dataset("queries")["q"][1].astype(np.float64)
    assert not q[:, 0].any()
    sig = np.sort(np.abs(q[:, 1]), axis=1)
    assert np.all(sig[:, -1] == 96.0) and np.all(sig[:, -2] < 8.0)
    assert np.all(np.abs(q[:, 2]).max(axis=1) < 2.0 ** -7) and np.all(np.abs(q[:, 2]).max(axis=1) > 0)
    huge = np.abs(vr.dataset("queries-huge")["q"][1].astype(np.float64))
    assert huge.min() >= 2.0 ** 14 and huge.max() <= 65504.0
    sub = np.abs(vr.dataset("queries-sub")["q"][1].astype(np.float64))
    assert sub.min() > 0.0 and sub.max() < 2.0 ** -14


# ----------------------------------------------------------------------------- the tiers
def test_the_tiers_are_decided_by_the_model_and_written_down(oracle):
    tab = vr.table(oracle)
    for prof in vr.PROFILES:
        worst = max(tab[prof, f] for f in FORMATS)
        assert vr.TIERS[prof] == (1 if worst <= 0.5 else 2), (prof, worst)
    with open(os.path.join(ROOT, "DESIGN.md")) as f:
        design = f.read()
    for line in vr.table_lines(tab):
        assert line in design, ("DESIGN.md, accuracy over value ranges: the table has moved; python -m tests._value_ranges prints it", line)


def test_the_term_is_half_an_fp16_ulp_of_every_weight(oracle):
    """h(w) against numpy's own fp16 rounding, and the model's error against the term: never above it"""
    w = np.concatenate([np.exp2(np.random.default_rng(1).uniform(-30, 0, 4000)), [0.0, 2.0 ** -14, 2.0 ** -24, 1.0]])
    err = np.abs(vr._f16(w) - w)
    assert np.all(err <= vr.half_ulp_f16(w))
    for name in ("sink-tile-0", "sink-page-128", "v-tile-ladder", "v-page-ladder"):
        for fmt in FORMATS:
            ds, hc = vr.dataset(name), vr.checker(oracle, name, 256, fmt)
            for head in range(H):
                q = ds["q"][1, head][None]
                want = hc.want_rows(q, head, [250], ds["sm"])[0]
                got = vr.model_rows(hc, q, head, [250], ds["sm"])[0]
                assert np.all(np.abs(got - want) <= vr.term_rows(hc, q, head, [250], ds["sm"]) * (1 + 1e-9) + 1e-300), (name, vr.NAMES[fmt], head)


# ----------------------------------------------------------------------------- wrong models
@pytest.mark.parametrize("fault,name,fmt", [("no-vref-carry", "v-tile-ladder", vr.FP8), ("no-vref-carry", "sink-tile-127", vr.FP8),
                                            ("no-rescale", "ramp-up", vr.FP8), ("no-rescale", "ramp-up", vr.INT4), ("no-rescale", "ramp-up", vr.MX4),
                                            ("no-rescale", "ramp-up", vr.K8V4), ("no-rescale", "sink-tile-249", vr.INT4),
                                            ("merge-without-maxima", "ramp-up", vr.FP8), ("merge-without-maxima", "ramp-down", vr.MX4),
                                            ("merge-without-maxima", "sink-page-128", vr.INT4), ("merge-without-maxima", "ramp-down", vr.K8V4)])
def test_a_wrong_model_is_caught_ten_times_over(oracle, fault, name, fmt):
    r = vr.ratios(oracle, name, fmt, fault=fault, ranges=(256,))
    assert r["ratio"] >= 10.0, f"{fault} on {name} ({vr.NAMES[fmt]}, tier {vr.TIERS[vr.PROFILE_OF[name]]}): err / bound {r['ratio']:.1f}"
