"""-m "not gpu": the stream form of several layers of one sequence (Engine::attend_int4 / attend_mx4) on the host.

  * the partition the kernels, the merge and the engine share (ring_rule.hpp attend_stream_begin / _wg_of / _count) against a brute-force count;
  * the two decisions (attend_geometry.hpp int4_wg8_stream / mx4_stream) pinned at the shapes the full-size tests run (80 layers x 32k on 256 CUs)
    -- with the tuning keys at 0 they are the rules the engine had inline -- and what the keys attend_stream / attend_splits do to them.

All through the wrappers of tests/csrc/host_rules_test.cpp (tests/_rules.py)."""
import numpy as np
import pytest

from tests._rules import MX4, decide_seq, int4_stream, load_rules, mx4_stream


@pytest.fixture(scope="module")
def rules():
    return load_rules()


def test_stream_partition_against_brute_force(rules):
    """Every n_layers in 1..6, n_tiles in 1..20, n_wgs in 1..n_layers x n_tiles (len = total / n_wgs, rem = total % n_wgs): the pieces
    [begin(w), begin(w + 1)) tile [0, total) exactly, the first rem of them len + 1 long and the others len; wg_of(G) is the piece that
    holds G; attend_stream_count(l) is the number of pieces that meet layer l; and the slot a piece has in a layer it meets,
    w - wg_of(l x n_tiles), is below count(l) and no two pieces of a layer share one."""
    for n_layers in range(1, 7):
        for n_tiles in range(1, 21):
            total = n_layers * n_tiles
            for n_wgs in range(1, total + 1):
                ln, rem = divmod(total, n_wgs)
                what = (n_layers, n_tiles, n_wgs)
                begin = np.array([rules.rules_stream_begin(w, ln, rem) for w in range(n_wgs + 1)], np.int64)
                assert begin[0] == 0 and begin[-1] == total, what
                assert np.array_equal(np.diff(begin), np.where(np.arange(n_wgs) < rem, ln + 1, ln)), what
                owner = np.repeat(np.arange(n_wgs), np.diff(begin))                       # brute force: the piece of every tile
                assert [rules.rules_stream_wg_of(G, ln, rem) for G in range(total)] == owner.tolist(), what
                for layer in range(n_layers):
                    pieces = np.unique(owner[layer * n_tiles:(layer + 1) * n_tiles])        # the pieces that meet the layer
                    count = rules.rules_stream_count(layer, n_tiles, ln, rem)
                    assert count == len(pieces), (what, layer)
                    slots = pieces - rules.rules_stream_wg_of(layer * n_tiles, ln, rem)
                    assert slots.min() >= 0 and slots.max() < count and len(set(slots.tolist())) == len(slots), (what, layer)


def _model_begin(w, ln, rem):
    return w * ln + min(w, rem)


@pytest.mark.parametrize("n_layers,n_tiles,n_wgs", [
    (4, (1 << 30) - 1, 512),                       # total = 2^32 - 4: long pieces, rem = 508
    (3, 1431655763, 2147483645),                   # total = 2^32 - 7, len = 1, rem = n_wgs - 1
    (80, 53687091, 4294967280),                    # total = n_wgs: every piece one tile, rem = 0
    (5, 858993459, 7),                             # total = 2^32 - 1, rem = 3
])
def test_stream_partition_at_32_bit_sizes(rules, n_layers, n_tiles, n_wgs):
    """The same near 2^32 tiles, against Python integers: piece boundaries, the piece of the tiles on either side of them, and the count of
    every layer from a bisection over the model's boundaries."""
    total = n_layers * n_tiles
    assert total < (1 << 32) and n_wgs <= total
    ln, rem = divmod(total, n_wgs)
    if (n_layers, n_wgs) == (3, 2147483645):
        assert ln == 1 and rem == n_wgs - 1
    rng = np.random.default_rng(5)
    ws = sorted({0, 1, rem - 1, rem, rem + 1, n_wgs - 2, n_wgs - 1} | set(int(v) for v in rng.integers(0, n_wgs, 200)))
    for w in (w for w in ws if 0 <= w < n_wgs):
        b, e = _model_begin(w, ln, rem), _model_begin(w + 1, ln, rem)
        assert e - b == ln + (1 if w < rem else 0)
        assert rules.rules_stream_begin(w, ln, rem) == b and rules.rules_stream_begin(w + 1, ln, rem) == e, w
        assert rules.rules_stream_wg_of(b, ln, rem) == w and rules.rules_stream_wg_of(e - 1, ln, rem) == w, w
    assert _model_begin(n_wgs, ln, rem) == total

    def piece_of(G):                               # bisection over the model's boundaries: the w with begin(w) <= G < begin(w + 1)
        lo, hi = 0, n_wgs - 1
        while lo < hi:
            mid = (lo + hi + 1) // 2
            if _model_begin(mid, ln, rem) <= G: lo = mid
            else: hi = mid - 1
        return lo

    for layer in sorted({0, 1, n_layers // 2, n_layers - 1}):
        first, last = piece_of(layer * n_tiles), piece_of((layer + 1) * n_tiles - 1)
        assert rules.rules_stream_count(layer, n_tiles, ln, rem) == last - first + 1, layer
        assert rules.rules_stream_wg_of(layer * n_tiles, ln, rem) == first


def _max_slots(n_layers, n_tiles, n_wgs):
    """most pieces any layer meets, by brute force over the piece boundaries"""
    total = n_layers * n_tiles
    ln, rem = divmod(total, n_wgs)
    begin = np.arange(n_wgs + 1, dtype=np.int64) * ln + np.minimum(np.arange(n_wgs + 1), rem)
    first = np.searchsorted(begin, np.arange(n_layers) * n_tiles, side="right") - 1
    last = np.searchsorted(begin, (np.arange(n_layers) + 1) * n_tiles - 1, side="right") - 1
    return int((last - first + 1).max())


def test_stream_decisions_at_the_full_size_shapes_are_the_inline_rules(rules):
    """Tuning keys at 0, 256 CUs: the shapes tests/test_gpu_full_size.py runs decide as they did when the rules stood inline in
    engine_attend.cpp.  INT4_G32: 2 x CUs pieces from 896 tiles and 16 tiles a piece, several layers only; MXFP4: CUs / ceil(g / 8)
    pieces under the same thresholds, whole tiles only, and only where the fixed grid would cut the layers."""
    cus = 256
    # INT4_G32, 80 layers x 32k in one run: 81 920 tiles in 512 pieces of 160
    assert int4_stream(rules, 80, 1024, cus) == dict(n_wgs=512, len=160, rem=0, max_slots=_max_slots(80, 1024, 512), tiles=0)
    # ... striped over 7 runs: 7 x ceil(ceil(16384 / 7) / 16) = 1029 class tiles a layer, 82 320 = 512 x 160 + 400
    assert int4_stream(rules, 80, 1029, cus, cls=True) == dict(n_wgs=512, len=160, rem=400, max_slots=_max_slots(80, 1029, 512), tiles=1029)
    assert int4_stream(rules, 80, 895, cus) is None                       # under 28k context: the fixed grid
    assert int4_stream(rules, 80, 896, cus) == dict(n_wgs=512, len=140, rem=0, max_slots=_max_slots(80, 896, 512), tiles=0)
    assert int4_stream(rules, 1, 1024, cus) is None and int4_stream(rules, 1, 1 << 20, cus) is None      # one layer never streams
    assert int4_stream(rules, 8, 1023, cus) is None                       # 8184 tiles < 16 x 512
    assert int4_stream(rules, 8, 1024, cus)["len"] == 16
    assert int4_stream(rules, 80, 1024, 304) == dict(n_wgs=608, len=134, rem=448, max_slots=_max_slots(80, 1024, 608), tiles=0)
    # MXFP4, 80 layers x 32k, g = 8: 256 pieces of 320 (the fixed grid: 256 / 80 = 3 splits a layer)
    assert mx4_stream(rules, 80, 16384, cus, g=8) == dict(n_wgs=256, len=320, rem=0, max_slots=_max_slots(80, 1024, 256), tiles=0)
    # g = 16, two row groups: 128 pieces -- the rule alone under three splits; the entry's fixed grid has 256 / 160 = 1 split at 80 layers, whole layers, and
    # does not stream; 40 layers (80 columns, three splits) do
    assert mx4_stream(rules, 80, 16384, cus, g=16, fixed_splits=3) == dict(n_wgs=128, len=640, rem=0, max_slots=_max_slots(80, 1024, 128), tiles=0)
    assert decide_seq(rules, MX4, 80, 16384, cus, g=16)["n_splits"] == 1 and mx4_stream(rules, 80, 16384, cus, g=16) is None
    assert mx4_stream(rules, 40, 16384, cus, g=16) == dict(n_wgs=128, len=320, rem=0, max_slots=_max_slots(40, 1024, 128), tiles=0)
    assert mx4_stream(rules, 80, 895 * 16, cus) is None
    assert mx4_stream(rules, 1, 16384, cus) is None
    assert decide_seq(rules, MX4, 80, 16384, cus)["n_splits"] == 3         # (the fixed-grid split count: Engine::attend_mx4's own, asked by mx4_stream)
    assert mx4_stream(rules, 80, 16384, cus, fixed_splits=1) is None      # whole layers are final rows: no partials, no merge (the rule alone) ...
    assert decide_seq(rules, MX4, 80, 16384, 128)["n_splits"] == 1 and mx4_stream(rules, 80, 16384, 128) is None      # ... and where the entry gets there: 128 CUs
    assert mx4_stream(rules, 80, 16384 - 15, cus) is None  # a ragged last tile
    assert mx4_stream(rules, 2, 1024 * 16, cus) is None    # 2048 tiles < 16 x 256
    assert mx4_stream(rules, 4, 1024 * 16, cus) == dict(n_wgs=256, len=16, rem=0, max_slots=_max_slots(4, 1024, 256), tiles=0)


def test_stream_tuning_keys(rules):
    """attend_stream = N > 0: exactly N pieces whatever the size, for both formats; N beyond layers x tiles, one layer, -1 and a forced
    attend_splits: the fixed grid.  INT4_G32 by residue classes: pieces of two tiles at least; and never more than 2048 partials a row."""
    for n_layers, n_tiles in ((5, 4), (5, 16), (3, 18), (2, 1)):
        total = n_layers * n_tiles
        for n in range(1, total + 1):
            want = dict(n_wgs=n, len=total // n, rem=total % n, max_slots=_max_slots(n_layers, n_tiles, n), tiles=0)
            assert int4_stream(rules, n_layers, n_tiles, 256, attend_stream=n) == want
            assert mx4_stream(rules, n_layers, n_tiles * 16, 256, fixed_splits=1, attend_stream=n) == want
            cls = int4_stream(rules, n_layers, n_tiles, 256, cls=True, attend_stream=n)
            assert cls == (dict(want, tiles=n_tiles) if total // n >= 2 else None)
        assert int4_stream(rules, n_layers, n_tiles, 256, attend_stream=total + 1) is None
        assert mx4_stream(rules, n_layers, n_tiles * 16, 256, attend_stream=total + 1) is None
        assert int4_stream(rules, n_layers, n_tiles, 256, attend_splits=2, attend_stream=2) is None
        assert mx4_stream(rules, n_layers, n_tiles * 16, 256, attend_splits=2, attend_stream=2) is None
        assert mx4_stream(rules, n_layers, n_tiles * 16 - 1, 256, attend_stream=2) is None          # MXFP4: whole tiles only, also on request
    assert int4_stream(rules, 1, 16, 256, attend_stream=4) is None and mx4_stream(rules, 1, 256, 256, attend_stream=4) is None
    # never, and a forced split count, at the sizes that stream by themselves
    assert int4_stream(rules, 80, 1024, 256, attend_stream=-1) is None and mx4_stream(rules, 80, 16384, 256, attend_stream=-1) is None
    assert int4_stream(rules, 80, 1024, 256, attend_splits=8) is None and mx4_stream(rules, 80, 16384, 256, attend_splits=8) is None
    # the merge takes 2048 partials a row: 2 layers x 4096 tiles in one-tile pieces would be 4096
    assert int4_stream(rules, 2, 4096, 256, attend_stream=8192) is None
    assert int4_stream(rules, 2, 4096, 256, attend_stream=4096)["max_slots"] == 2048
