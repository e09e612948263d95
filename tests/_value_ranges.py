"""Value ranges INSIDE the attended span of the decode attention kernels: the data sets (profiles), a float64 model of the one rounding the
kernels declare (every softmax weight goes to fp16 once), and the bound term that rounding costs.  Pure numpy and the oracle; shared by
tests/test_value_ranges_cpu.py (the conditions on the data, the tiers, wrong models caught) and tests/test_gpu_decode_value_ranges.py.

Layout: that of tests/test_gpu_seq_geometry.py -- 8 kv heads x 128, G = 8 query rows a head, L = 2 layers of T positions (256: 8 tiles of 32;
250 for the per-wave FP8 kernel), a layer = T / 2 pages of K then T / 2 pages of V.  The profile lives in layer 1, layer 0 holds ordinary
rows (N(0, 1) x a per-page magnitude of U(0.2, 3), queries 1.5 x N(0, 1), rescaled where the call's sm_scale is not 1 / sqrt(128)).  Every seed is fixed here.

Profiles (DATASETS; what each claims is in its dict and asserted by the CPU test in the float64 reference over the oracle's records):
  v-tile-ladder   V magnitude constant inside a tile, the 8 tiles 2^{0, 2, .., 14} in a seeded permutation, clipped to +-60000
  v-page-ladder   the 16 V pages of every tile 2^(0 .. 8) (evenly spaced exponents) in a seeded permutation
  sink-*          a ladder and ONE key that takes >= 1 - 1e-3 of every row's weight, on the smallest-V page; needle at 0, 31, 127, 128, 249.
                  Narrowed ladders (the rounding term has to stay below 5 % of sum p|v|, see test_value_ranges_cpu.py): tiles 2^{0, 1.5, .., 10.5},
                  pages 2^(0 .. 6); the other keys N(0, 1) x U(0.2, 1), the queries c u + 0.5 N(0, 1) with the smallest c
                  that leaves the other keys 5e-4 of some row's weight (their weights then sit in the fp16 subnormals), the needle key 1.5 u (u = +-1 per head), the
                  needle's V row +-U(0.5, 1.5) x its page's magnitude (no element that a 4-bit format stores as 0)
  ramp-up / -down the largest score of a tile moves by >= 8 nats from tile to tile, one direction: key channels 0 .. 63 hold a_t u with a_t out
                  of +-{0.5, 0.75, 1, 1.5} (exact in every format), queries 8 u there; channels 64 .. 127 ordinary noise.  The maxima of
                  tiles 0 .. 3 and 4 .. 7 lie 90 nats (130 in the log2 domain) apart
  ties-k0         every K page zero: scores exactly 0, out = mean V, lse = ln n
  ties-v0-tile    the first tile's 16 V pages zero.  A page of zeros is stored with page scale 1 (the codec's rule), so the FP8 bodies elect 1.0 as
                  that tile's unit -- about 100 x the ordinary pages' scales: the carry vref / vref_t steps by that factor into tile 1, and in a tile by
                  residue classes the zero pages sit beside ordinary ones (the model's costliest tier-1 case, 0.36 of the bound).  The branch
                  "no candidate: keep the old unit" is reached only by a tile whose pages are all masked
  ties-v0         V zero everywhere: out exactly 0, lse finite
  queries         rows zero / one channel at 64 sigma / 2^-10 N(0, 1) / five ordinary; K magnitudes U(0.2, 1) (the spike row's score bound)
  queries-huge    every row +-U(2^14, 65504), sm_scale 2^-15 / sqrt(128)
  queries-sub     every row in the fp16 subnormals, sm_scale 2^12 / sqrt(128)"""
import functools

import numpy as np

from tests._gpu import D, H, HeadChecker

G, L = 8, 2
FP8, INT4, MX4, K8V4 = 4, 3, 5, 84                     # K8V4: K from the FP8 records, V from the MXFP4 records (not a scheme of the library)
NAMES = {FP8: "fp8", INT4: "int4", MX4: "mx4", K8V4: "k8v4"}
SM = 1.0 / np.sqrt(D)
RANGES = (256, 250)                                    # positions attended from 0: whole tiles, and a ragged last tile (13 pages)
NEEDLES = (0, 31, 127, 128, 249)


# ----------------------------------------------------------------------------- the data
def _ordinary(rng, T, lo=0.2, hi=3.0):
    """[T][H][D] float64: N(0, 1) x one magnitude per page"""
    x = rng.standard_normal((T // 2, 2, H, D)) * rng.uniform(lo, hi, (T // 2, 1, 1, 1))
    return x.reshape(T, H, D)


def _tile_exps(rng, T, exps):
    """exponent per position: one of `exps` per tile of 32, in a seeded permutation"""
    n_tiles = (T + 31) // 32
    e = np.asarray(exps, np.float64)[rng.permutation(len(exps))][:n_tiles]
    return np.repeat(e, 32)[:T]


def _page_exps(rng, T, top):
    """exponent per position: the 16 pages of every tile take 0 .. top evenly, a permutation per tile"""
    n_tiles = (T + 31) // 32
    e = np.concatenate([np.linspace(0.0, top, 16)[rng.permutation(16)] for _ in range(n_tiles)])
    return np.repeat(e, 2)[:T]


def _smallest_at(e, pos, tile_wide):
    """swap the exponents so that the page (tile_wide: the tile) of `pos` holds the smallest one of its tile (of the range)"""
    e = e.copy()
    if tile_wide:
        t, lo = pos // 32, int(np.argmin(e)) // 32
        a, b = e[32 * t:32 * t + 32].copy(), e[32 * lo:32 * lo + 32].copy()
        n = min(len(a), len(b))
        e[32 * t:32 * t + n], e[32 * lo:32 * lo + n] = b[:n], a[:n]
    else:
        t = pos // 32
        seg = e[32 * t:32 * t + 32]
        lo = 32 * t + (int(np.argmin(seg)) & ~1)
        p = pos & ~1
        e[[p, p + 1, lo, lo + 1]] = e[[lo, lo + 1, p, p + 1]]
    return e


def _ladder_v(rng, T, exps_per_pos):
    v = rng.standard_normal((T, H, D)) * np.exp2(exps_per_pos)[:, None, None]
    return np.clip(v, -60000.0, 60000.0)


@functools.lru_cache(maxsize=None)
def dataset(name, T=256):
    """-> dict(x: page images [L T][2048] fp16, q: [L][H][G][D] fp16, sm, claims: dict).  Read only."""
    seed = 9700 + 17 * sorted(DATASETS).index(name) + (T != 256)
    rng = np.random.default_rng(seed)
    k0, v0 = _ordinary(rng, T), _ordinary(rng, T)
    q = rng.standard_normal((L, H, G, D)) * 1.5
    k, v = _ordinary(rng, T), _ordinary(rng, T)
    sm, claims = SM, {}
    if name == "v-tile-ladder":
        e = _tile_exps(rng, T, np.arange(0, 16, 2))
        v = _ladder_v(rng, T, e)
        claims = dict(ladder=e)
    elif name == "v-page-ladder":
        e = _page_exps(rng, T, 8.0)
        v = _ladder_v(rng, T, e)
        claims = dict(ladder=e)
    elif name.startswith("sink-"):
        needle = int(name.split("-")[2])
        tile_wide = name.split("-")[1] == "tile"
        e = _tile_exps(rng, T, np.arange(8) * 1.5) if tile_wide else _page_exps(rng, T, 6.0)
        e = _smallest_at(e, needle, tile_wide)
        v = _ladder_v(rng, T, e)
        k = _ordinary(rng, T, 0.2, 1.0)
        u = np.where(rng.integers(0, 2, (H, D)) == 1, 1.0, -1.0)
        k[needle] = 1.5 * u
        v[needle] = rng.uniform(0.5, 1.5, (H, D)) * np.where(rng.integers(0, 2, (H, D)) == 1, 1.0, -1.0) * np.exp2(e[needle])   # no element that a 4-bit format rounds to 0
        noise = 0.5 * rng.standard_normal((H, G, D))
        lo_c, hi_c = 0.25, 4.0                                                        # the query's share of u: the smallest at which the other keys
        for _ in range(40):                                                           # keep 5e-4 of the weight in some row (fp16 data, float64 scores)
            c = 0.5 * (lo_c + hi_c)
            s = np.einsum("hgd,thd->hgt", (c * u[:, None, :] + noise).astype(np.float16).astype(np.float64), k.astype(np.float16).astype(np.float64)) * SM
            p = np.exp(s - s.max(axis=2, keepdims=True))
            rest = 1.0 - p[:, :, needle] / p.sum(axis=2)
            lo_c, hi_c = (c, hi_c) if rest.max() > 5e-4 else (lo_c, c)
        q[1] = hi_c * u[:, None, :] + noise
        claims = dict(ladder=e, needle=needle, weight=1.0 - 1e-3)
    elif name in ("ramp-up", "ramp-down"):
        a = np.array([-1.5, -1.0, -0.75, -0.5, 0.5, 0.75, 1.0, 1.5])
        a = a if name == "ramp-up" else a[::-1]
        u = np.where(rng.integers(0, 2, (H, 64)) == 1, 1.0, -1.0)
        k = np.concatenate([np.repeat(a, 32)[:T, None, None] * u[None], 0.5 * rng.standard_normal((T, H, 64))], axis=2)
        q[1] = np.concatenate([np.broadcast_to(8.0 * u[:, None, :], (H, G, 64)), rng.standard_normal((H, G, 64))], axis=2)
        claims = dict(step=8.0, steps=6, direction=1 if name == "ramp-up" else -1, split_gap_log2=126.0)
    elif name == "ties-k0":
        k = np.zeros((T, H, D))
        claims = dict(lse="ln n")
    elif name == "ties-v0-tile":
        v[:32] = 0.0
    elif name == "ties-v0":
        v = np.zeros((T, H, D))
        claims = dict(out=0.0)
    elif name == "queries":
        k = _ordinary(rng, T, 0.2, 1.0)
        q[1, :, 0] = 0.0
        q[1, np.arange(H), 1, rng.integers(0, D, H)] = 64 * 1.5 * np.where(rng.integers(0, 2, H) == 1, 1.0, -1.0)
        q[1, :, 2] = 2.0 ** -10 * rng.standard_normal((H, D))
        claims = dict(rows=("zero", "spike", "tiny"))
    elif name == "queries-huge":
        q[1] = rng.uniform(2.0 ** 14, 65504.0, (H, G, D)) * np.where(rng.integers(0, 2, (H, G, D)) == 1, 1.0, -1.0)
        sm = 2.0 ** -15 / np.sqrt(D)
        q[0] = 0.3 * 2.0 ** 15 * rng.standard_normal((H, G, D))                       # the ordinary layer under the call's sm_scale: 0.3 N(0, 1) in effect
        claims = dict(q_min=2.0 ** 14)
    elif name == "queries-sub":
        q[1] = rng.integers(1, 1024, (H, G, D)) * 2.0 ** -24 * np.where(rng.integers(0, 2, (H, G, D)) == 1, 1.0, -1.0)
        sm = 2.0 ** 12 / np.sqrt(D)
        q[0] *= 2.0 ** -12                                                            # the ordinary layer under the call's sm_scale: 1.5 N(0, 1) in effect
        claims = dict(q_max=1023 * 2.0 ** -24)
    else:
        raise KeyError(name)
    x = np.concatenate([region(k0, v0), region(k, v)]).astype(np.float16)
    q16 = q.astype(np.float16)
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(q16))
    x.setflags(write=False); q16.setflags(write=False)
    return dict(name=name, T=T, x=x, q=q16, sm=float(sm), claims=claims, kv16=(k.astype(np.float16), v.astype(np.float16)),
                kv16_layer0=(k0.astype(np.float16), v0.astype(np.float16)))


def region(k, v):
    """pages of one layer from positions k, v [T][H][D]: T / 2 pages of K, then T / 2 of V"""
    T = len(k)
    return np.concatenate([np.asarray(k).reshape(T // 2, 2 * H * D), np.asarray(v).reshape(T // 2, 2 * H * D)])


PROFILES = {
    "v-tile-ladder": ("v-tile-ladder",),
    "v-page-ladder": ("v-page-ladder",),
    "sink": tuple(f"sink-{'tile' if i % 2 == 0 else 'page'}-{n}" for i, n in enumerate(NEEDLES)),
    "ramp-up": ("ramp-up",),
    "ramp-down": ("ramp-down",),
    "ties": ("ties-k0", "ties-v0-tile", "ties-v0"),
    "queries": ("queries", "queries-huge", "queries-sub"),
}
DATASETS = tuple(n for names in PROFILES.values() for n in names)
PROFILE_OF = {n: p for p, names in PROFILES.items() for n in names}
# model err / project bound <= 0.5 on the CPU: tier 1, held to the project bound; else tier 2, held to the bound + 2 x term.  Decided by
# tests/test_value_ranges_cpu.py from the model alone (it asserts this table), never from a GPU result.
TIERS = {"v-tile-ladder": 1, "v-page-ladder": 1, "sink": 2, "ramp-up": 1, "ramp-down": 1, "ties": 1, "queries": 1}
DELTA_MAX = {"ramp-up": 4e-3, "ramp-down": 4e-3}       # everything else: 2e-3


# ----------------------------------------------------------------------------- checkers
class SplitChecker(HeadChecker):
    """the split pool: K and the E4M3 query of the FP8 checker, V of the MXFP4 checker over the same region"""

    def __init__(self, k8, v4):
        self.k8, self.v4, self.oracle, self.lut, self.T = k8, v4, k8.oracle, k8.lut, k8.T
        self.scheme, self.v_scheme = FP8, MX4

    def kv(self, head):
        return self.k8.kv(head)[0], self.v4.kv(head)[1]


_checkers = {}


def checker(oracle, name, T, fmt, layer=1):
    """the HeadChecker of a data set's layer in a format; built once"""
    key = (name, T, fmt, layer)
    if key not in _checkers:
        if fmt == K8V4:
            _checkers[key] = SplitChecker(checker(oracle, name, T, FP8, layer), checker(oracle, name, T, MX4, layer))
        else:
            _checkers[key] = HeadChecker(oracle, fmt, dataset(name, T)["x"][layer * T:(layer + 1) * T], T)
    return _checkers[key]


# ----------------------------------------------------------------------------- the model and the rounding term
def tile_ids(n, stripe_n=1):
    """the tile of every position of a range of n positions from 0, numbered in the order the kernels walk them: 32 consecutive positions, or --
    stripe_n > 1, the forms by residue class (ring_rule.hpp mx4_class_tiles) -- class-major, class c = the pages j with j % stripe_n == c, 16 to a tile"""
    pages = np.arange(n) // 2
    if stripe_n <= 1:
        return pages // 16
    cls_m = (((n + 1) // 2 + stripe_n - 1) // stripe_n + 15) // 16
    return (pages % stripe_n) * cls_m + (pages // stripe_n) // 16


def _tile_units(vs, tiles):
    """u [n]: per position, the largest V page scale among the kept positions of its tile; the previous tile's where that is 0 (1 before any)"""
    u = np.ones(len(tiles))
    prev = 1.0
    for t in np.unique(tiles):
        m = float(vs[tiles == t].max())
        prev = m if m > 0.0 else prev
        u[tiles == t] = prev
    return u


def _f16(w):
    return np.asarray(w, np.float64).astype(np.float32).astype(np.float16).astype(np.float64)


def _fp8_form(checker, fp8_ref):
    return (getattr(checker, "v_scheme", checker.scheme) == FP8) if fp8_ref is None else bool(fp8_ref)


def model_rows(checker, q16, head, npos, sm, fp8_ref=None, rounding=True, fault=None, stripe_n=1):
    """float64 attention over the records want_rows dequantises, every weight rounded to fp16 ONCE: fp16(p) (INT4_G32, MXFP4, K8V4), or --
    fp8_ref, None = by the checker's V format -- fp16(p x vs_j / u_t), u_t the tile's unit (_tile_units; stripe_n: tile_ids).  q16 [M][G][D], npos [M] -> out
    [M][G][D], lse [M][G].  It models neither the kernels' schedule nor their fp32 steps.  rounding=False: want_rows itself.
    fault: a deliberately WRONG model -- "no-vref-carry" (the accumulator keeps its number when the tile unit changes), "no-rescale" (the
    accumulator is not brought to a risen maximum), "merge-without-maxima" (two partials of 4 tiles added as they are)."""
    q16 = np.asarray(q16, np.float16)
    M, Gq = q16.shape[:2]
    out, lse = np.zeros((M, Gq, D)), np.full((M, Gq), -np.inf)
    fp8 = _fp8_form(checker, fp8_ref)
    for m in range(M):
        n = int(np.asarray(npos)[m])
        if n == 0:
            continue
        p, l, mx, V, vs = checker.weight_rows(q16[m], head, n, sm)
        tile = tile_ids(n, stripe_n)
        u = _tile_units(vs, tile) if fp8 else np.ones(n)
        vs_ = vs if fp8 else np.ones(n)
        ok = vs_ > 0
        vq = np.where(ok[:, None], V / np.where(ok, vs_, 1.0)[:, None], 0.0)           # V in units of its page scale
        with np.errstate(divide="ignore"):
            s = np.log(p) + mx[:, None]
        if fault == "no-rescale":                                                     # weights against the running maximum of their tile, never brought on
            run = np.maximum.accumulate(np.stack([s[:, tile == t].max(axis=1) for t in range(tile.max() + 1)], axis=1), axis=1)
            pw = np.exp(s - run[:, tile])
        elif fault == "merge-without-maxima":
            first = tile < 4
            own = np.where(first, s[:, first].max(axis=1, keepdims=True), s[:, ~first].max(axis=1, keepdims=True, initial=-np.inf))
            pw = np.exp(s - own)                                                      # each partial against its own maximum, sums and rows added
            l = pw.sum(axis=1)
        else:
            pw = p
        w = pw * (vs_ / u)[None]
        if rounding:
            w = _f16(w)
        unit = np.full(n, u[np.argmax(tile)]) if fault == "no-vref-carry" else u
        out[m] = ((w * unit[None]) @ vq) / l[:, None]
        lse[m] = mx + np.log(p.sum(axis=1))
    return out, lse


def half_ulp_f16(w):
    """h(w): half an fp16 ulp at w -- 2^(floor(log2 w) - 11) for w >= 2^-14, 2^-25 below (the subnormals, 0 included)"""
    w = np.asarray(w, np.float64)
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.maximum(w, 2.0 ** -14)))
    return np.where(w >= 2.0 ** -14, np.exp2(e - 11), 2.0 ** -25)


def term_rows(checker, q16, head, npos, sm, fp8_ref=None, stripe_n=1):
    """term [M][G][D] = (1 / l) sum_j h(w_j) u_t(j) |V_jd| / s_j: what rounding every weight to fp16 can cost at most.  w_j is the weight the
    format rounds, taken against the row's FINAL maximum; u_t = s_j = 1 outside FP8."""
    q16 = np.asarray(q16, np.float16)
    M, Gq = q16.shape[:2]
    term = np.zeros((M, Gq, D))
    fp8 = _fp8_form(checker, fp8_ref)
    for m in range(M):
        n = int(np.asarray(npos)[m])
        if n == 0:
            continue
        p, l, mx, V, vs = checker.weight_rows(q16[m], head, n, sm)
        u = _tile_units(vs, tile_ids(n, stripe_n)) if fp8 else np.ones(n)
        vs_ = vs if fp8 else np.ones(n)
        ok = vs_ > 0
        vq = np.where(ok[:, None], np.abs(V) / np.where(ok, vs_, 1.0)[:, None], 0.0)
        term[m] = ((half_ulp_f16(p * (vs_ / u)[None]) * u[None]) @ vq) / l[:, None]
    return term


def bound_rows(checker, q16, head, npos, sm):
    """(want, lse, mag, delta, the project bound (2e-3 + 2 delta) sum p|v| + 1e-6) of want_rows"""
    want, wlse, mag, delta = checker.want_rows(q16, head, npos, sm)
    return want, wlse, mag, delta, (2e-3 + 2 * delta)[:, None, None] * mag + 1e-6


def extra_tol(oracle, name, T, fmt, head, npos, layer=1, stripe_n=1):
    """what check_rows adds to the bound for the data set's profile: None in tier 1 (and in the ordinary layer), 2 x term in tier 2"""
    if layer != 1 or TIERS[PROFILE_OF[name]] == 1:
        return None
    ds = dataset(name, T)
    return 2.0 * term_rows(checker(oracle, name, T, fmt), ds["q"][1, head][None].repeat(len(npos), axis=0), head, npos, ds["sm"], stripe_n=stripe_n)


def tile_maps(fmt):
    """the tile maps the bodies of a format round in: FP8 walks 32 consecutive positions, or (k_attend_fp8_dma<2> on two pools) two residue classes"""
    return (1, 2) if fmt == FP8 else (1,)


def ratios(oracle, name, fmt, T=256, fault=None, ranges=RANGES):
    """the worst |model - float64| / bound of a data set in a format over the ranges (each a position count from 0) and heads, the bound that of the
    data set's tier; plus the worst delta, the share of elements with sum p|v| >= 1e-3 and the share with 2 x term <= 0.05 sum p|v|"""
    ds, hc = dataset(name, T), checker(oracle, name, T, fmt)
    tier = TIERS[PROFILE_OF[name]]
    worst, dmax, big, small_term, count = 0.0, 0.0, 0, 0, 0
    for n, stripe_n in ((n, st) for n in ranges if n <= T for st in tile_maps(fmt)):
        for head in range(H):
            q = ds["q"][1, head][None]
            want, wlse, mag, delta, tol = bound_rows(hc, q, head, [n], ds["sm"])
            term = term_rows(hc, q, head, [n], ds["sm"], stripe_n=stripe_n)
            if tier == 2:
                tol = tol + 2.0 * term
            got, _ = model_rows(hc, q, head, [n], ds["sm"], fault=fault, stripe_n=stripe_n)
            worst = max(worst, float((np.abs(got - want) / tol).max()))
            dmax = max(dmax, float(delta.max()))
            big += int((mag >= 1e-3).sum()); small_term += int((2.0 * term <= 0.05 * mag).sum()); count += mag.size
    return dict(ratio=worst, delta=dmax, mag_share=big / count, term_share=small_term / count)


def table(oracle):
    """{(profile, format): worst model err / PROJECT bound over the profile's data sets, both ranges, every head and row, and -- FP8 -- both layouts
    (T = 250: the per-wave kernel's) and both tile maps} -- what decides the tiers"""
    out = {}
    for prof, names in PROFILES.items():
        for fmt in (FP8, INT4, MX4, K8V4):
            worst = 0.0
            for name in names:
                for T in ((256, 250) if fmt == FP8 else (256,)):
                    ds, hc = dataset(name, T), checker(oracle, name, T, fmt)
                    for n in (n for n in RANGES if n <= T):
                        for head in range(H):
                            q = ds["q"][1, head][None]
                            want, _, _, _, tol = bound_rows(hc, q, head, [n], ds["sm"])
                            for stripe_n in tile_maps(fmt):
                                worst = max(worst, float((np.abs(model_rows(hc, q, head, [n], ds["sm"], stripe_n=stripe_n)[0] - want) / tol).max()))
            out[prof, fmt] = worst
    return out


def table_lines(tab):
    """the rows of DESIGN.md's table"""
    lines = ["| profile | fp8 | int4 | mx4 | k8v4 | tier |", "|---|---|---|---|---|---|"]
    for prof in PROFILES:
        lines.append(f"| {prof} | " + " | ".join(f"{tab[prof, f]:.2f}" for f in (FP8, INT4, MX4, K8V4)) + f" | {TIERS[prof]} |")
    return lines


if __name__ == "__main__":
    from oracle.bindings import Oracle, build_oracle
    build_oracle()
    print("\n".join(table_lines(table(Oracle()))))
