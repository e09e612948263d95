"""-m gpu: the token predictor's nine kernels (csrc/predictor_kernels.inl) against float64 where random fp32 weights never reach -- exact
ties on every seam of the five places that implement "value descending, token id ascending", absent logits (-inf, NaN) and ranks
without a candidate, the request-count seams of the batch route, the merge fan-in of the small route, 1 / 3 / 4 layers of the real
cell, and a softmax so peaked that every fp32 probability but one underflows.

The reference, the case builders and the tolerance are tests/_predictor_ref.py (its header states the pinned rules, how the bound is
derived from fp32 numpy in two orders of addition, the factor 4 and the derived values); tests/test_predictor_ref_cpu.py shows without a
GPU that the reference is right and the cases are what they claim.  Tokens are compared exactly everywhere: no case here has a near-tie
(every gap among a request's best k + 1 logits is either exactly 0 between identical rows or at least 100 x the fp32 logit error).
Outputs are prefilled with -7 / NaN, so a rank that is not written is caught.  +inf logits are out of scope."""
import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd.speckv_ctypes import SpeckvError, SpeckvLib
from tests import _predictor_ref as R
from tests._gpu import set_tuning, torch_mod

pytestmark = pytest.mark.gpu
INVAL = -4                                                          # include/speckv.h: SPECKV_ERR_INVAL
CELLS = ["degenerate", "real"]


def open_lib():
    return SpeckvLib(pkg.library_path(), "hip:0")


def load(lib, case):
    p = lambda a: a.ctypes.data
    if case["lstm"] is None:
        lib.predictor_load(p(case["emb"]), p(case["wout"]), case["vocab"], False)
    else:
        w_ih, w_hh, b_ih, b_hh = case["lstm"]
        lib.predictor_load_lstm(p(case["emb"]), case["vocab"], [p(a) for a in w_ih], [p(a) for a in w_hh], [p(a) for a in b_ih],
                                [p(a) for a in b_hh], p(case["wout"]), p(case["bias"]) if case["bias"] is not None else 0, False)


def run(lib, case, batch):
    """predict_batch on the route asked for (batch: predict_batch_path forces the four-launch route for n <= 4)"""
    torch = torch_mod()
    n, k = case["n"], case["k"]
    d_h = torch.from_numpy(case["hist"]).cuda()
    d_tok = torch.full((n, k), -7, dtype=torch.int32, device="cuda")
    d_conf = torch.full((n, k), float("nan"), dtype=torch.float32, device="cuda")
    if batch:
        set_tuning("predict_batch_path", 1)
    try:
        lib.predict_batch(n, d_h.data_ptr(), k, d_tok.data_ptr(), d_conf.data_ptr())
        torch.cuda.synchronize()
    finally:
        if batch:
            set_tuning("predict_batch_path", 0)
    return d_tok.cpu().numpy(), d_conf.cpu().numpy().astype(np.float64)


def check(case, got, what):
    """tokens exactly the float64 ranking, confidences within conf_tolerance; prints the worst err / tol before it asserts"""
    tok, conf = got
    want_tok, want_conf, _ = R.reference(case)
    tol = R.conf_tolerance(case)
    err = np.abs(conf - want_conf)
    with np.errstate(invalid="ignore"):
        worst = float(np.nan_to_num(err / tol, nan=np.inf).max())
    e_logit, e_conf, _ = R.fp32_errors(case)
    print(f"predictor-edges {what} cell={case['cell']} vocab={case['vocab']} n={case['n']} k={case['k']}: E_logit {e_logit:.3g} E_conf {e_conf:.3g} "
          f"worst err/tol {worst:.3f}")
    assert np.array_equal(tok, want_tok), (what, np.argwhere(tok != want_tok)[0].tolist(), tok[tok != want_tok][:4], want_tok[tok != want_tok][:4])
    assert not np.isnan(conf).any(), (what, "NaN confidence", np.argwhere(np.isnan(conf))[0].tolist())
    assert np.all(conf[want_tok < 0] == 0.0), (what, "a rank without a candidate reports confidence 0")
    assert np.all(err <= tol), (what, worst, np.argwhere(err > tol)[0].tolist())
    return worst


def run_and_check(case, routes, what):
    """one engine, the case's weights loaded once, every route asked for; returns {route: (tok, conf)}"""
    lib = open_lib()
    out = {}
    try:
        load(lib, case)
        for route in routes:
            batch = route != "small"
            assert R.route(case["vocab"], case["n"], batch) == route, (what, route)
            out[route] = run(lib, case, batch and case["n"] <= R.CONSTANTS["kPredictSmallN"])
            check(case, out[route], f"{what} route={route}")
    finally:
        lib.finalize()
    return out


# ---- ties ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("name", [n for n, t in R.TIE_CASES.items() if t["form"] == "split"])
def test_ties_in_the_split_topk_of_the_batch_route(name, cell):
    """k_softmax_topk_small + k_softmax_topk_merge, vocab 8200 = 3 parts, n = 5, k = 8: tied logits across the thread stride, two waves, two
    parts, nine in one thread's registers, the first and the last part, and a group boundary inside k"""
    case = R.tie(name, cell)
    out = run_and_check(case, ["split"], f"tie {name}")
    assert np.array_equal(out["split"][0], case["expect"])


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("name", [n for n, t in R.TIE_CASES.items() if t["form"] == "small"])
def test_ties_on_the_small_route(name, cell):
    """k_predict_small + k_predict_small_merge with more than one merge wave live (vocab 8320: 65 parts; 32768: 256): tied rows across a
    wave's 32 rows, two workgroups and two merge waves; n = 4 and n = 1"""
    case = R.tie(name, cell)
    full = R.sub_case(case, list(range(case["n"])))
    for sub in ([full] if case["n"] == 1 else [full, R.sub_case(case, [case["n"] - 1])]):
        out = run_and_check(sub, ["small"], f"tie {name}")
        assert np.array_equal(out["small"][0], sub["expect"])


@pytest.mark.parametrize("name", [n for n, t in R.TIE_CASES.items() if t["form"] == "one"])
def test_ties_in_the_one_workgroup_topk(name):
    """k_softmax_topk (vocab 262145 is past the 64 parts of the split form): the sorted insertion and the 1024-thread reduction"""
    case = R.tie(name, "degenerate")
    out = run_and_check(case, ["one"], f"tie {name}")
    assert np.array_equal(out["one"][0], case["expect"])


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("route,vocab,n", [("split", 8200, 5), ("small", 8200, 2), ("one", 262145, 2)])
def test_uniform_logits_report_the_first_k_tokens(route, vocab, n, cell):
    """every logit the same (hidden = 0, or identical rows under a constant out_bias): tokens 0 .. 7, every confidence 1 / vocab"""
    case = R.uniform(cell, vocab, n)
    tok, conf = run_and_check(case, [route], "uniform")[route]
    assert np.array_equal(tok, np.tile(np.arange(8, dtype=np.int32), (n, 1)))
    assert np.all(np.abs(conf * vocab - 1.0) <= R.ULP)


# ---- absent logits --------------------------------------------------------------------------------------------------------------------------
ABSENT = [(route, vocab, n, kind) for route, vocab, n in (("small", 136, 3), ("split", 136, 3), ("split", 8200, 5)) for kind in ("three", "none", "tied", "nan")]
ABSENT += [("one", 262145, 2, "three"), ("one", 262145, 2, "nan")]


@pytest.mark.parametrize("route,vocab,n,kind", ABSENT)
def test_absent_logits_are_never_chosen_and_never_summed(route, vocab, n, kind):
    """-inf and NaN logits through out_bias: never reported, not in the softmax; a rank without a candidate is (-1, 0.0).  Kinds: all rows
    -inf but three; every row -inf; -inf rows inside tied groups; a NaN row in the tied top group and one outside.  (Before the kernels
    left absent logits out of the exp-sum, a NaN logit made every confidence of its request NaN.)"""
    case = R.absent(kind, vocab, n)
    tok, conf = run_and_check(case, [route], f"absent {kind}")[route]
    assert np.array_equal(tok, case["expect"])
    gone = np.nonzero(~(case["bias"] > -np.inf))[0]
    assert not set(gone.tolist()) & set(tok.reshape(-1).tolist())
    if kind == "three":
        assert np.all(tok[:, 3:] == -1) and np.all(conf[:, 3:] == 0.0)
        assert np.all(np.abs(conf.sum(-1) - 1.0) <= R.conf_tolerance(case).sum(-1))
    if kind == "none":
        assert np.all(tok == -1) and np.all(conf == 0.0)


# ---- launch seams ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in R.RANDOM_CASES if n.startswith("seam-")])
def test_request_count_seams_of_the_batch_route(name):
    """k_lstm_logits cuts the requests into columns of 128 (blockIdx.y) and tiles of 32, k_softmax_topk_merge packs four requests a
    workgroup: n on both sides of each, every request checked, k in {2, 3, 6, 7}"""
    case = R.random_case(name)
    run_and_check(case, ["small", "split"] if case["n"] <= 4 else ["split"], name)


# ---- merge fan-in ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in R.RANDOM_CASES if n.startswith("fan-")])
def test_merge_fan_in_of_the_small_route(name):
    """65, 157 and 256 parts with k in {3, 7, 8}: waves 1 - 3 of k_predict_small_merge live and the lane < 4 k packing of their keys; one
    row past 256 parts the request takes the batch route.  Both routes against float64 and against each other."""
    case = R.random_case(name)
    small_ok = case["vocab"] <= R.CONSTANTS["kPredictSmallMaxParts"] * R.SMALL_ROWS
    assert small_ok == (name != "fan-32769")
    out = run_and_check(case, ["small", "split"] if small_ok else ["split"], name)
    if small_ok:
        assert np.array_equal(out["small"][0], out["split"][0])
        assert np.all(np.abs(out["small"][1] - out["split"][1]) <= 2 * R.conf_tolerance(case))


# ---- cell depth -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("layers", [1, 3, 4])
def test_real_cell_of_one_three_and_four_layers(layers):
    """k_lstm_cell: with one layer the 16-column projection never runs, three and four reuse the sequence buffer more often; n = 6 on the
    batch route, the same requests as 4 + 2 on the small route"""
    case = R.random_case(f"depth-{layers}")
    assert len(case["lstm"][0]) == layers
    run_and_check(case, ["split"], f"depth {layers}")
    for rows in ([0, 1, 2, 3], [4, 5]):
        sub = R.sub_case(case, rows)
        sub["_ref"] = tuple(a[rows] for a in R.reference(case))
        sub["_err"] = R.fp32_errors(case)                                  # the bound of the six requests holds for any of them
        run_and_check(sub, ["small"], f"depth {layers}")


def test_a_fifth_layer_is_refused_and_nothing_is_written():
    torch = torch_mod()
    case = R.random_case("depth-4")
    five = dict(case, lstm=tuple(list(a) + [a[-1]] for a in case["lstm"]))
    n, k = case["n"], case["k"]
    d_h = torch.from_numpy(case["hist"]).cuda()
    d_tok = torch.full((n, k), -7, dtype=torch.int32, device="cuda")
    d_conf = torch.full((n, k), float("nan"), dtype=torch.float32, device="cuda")
    lib = open_lib()
    try:
        with pytest.raises(SpeckvError) as e:
            load(lib, five)
        assert e.value.status == INVAL
        with pytest.raises(SpeckvError) as e:                               # no predictor was loaded: the prediction is refused as well
            lib.predict_batch(n, d_h.data_ptr(), k, d_tok.data_ptr(), d_conf.data_ptr())
        assert e.value.status == INVAL
        torch.cuda.synchronize()
        assert bool((d_tok == -7).all()) and bool(torch.isnan(d_conf).all())
        load(lib, case)                                                     # four layers load; a refused fifth leaves them in place
        with pytest.raises(SpeckvError) as e:
            load(lib, five)
        assert e.value.status == INVAL
        check(case, run(lib, case, False), "depth 4 after a refused load")
    finally:
        lib.finalize()


# ---- peaked softmax -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["small", "split"])
def test_peaked_softmax_ranks_by_logit_where_probabilities_underflow(route):
    """float64 logit gaps above 100: every confidence but the first is below fp32's range, where a ranking by fp32 probability sees ties;
    the device ranks by logit and must follow the float64 order through all k ranks.  Confidences: 1 and (absolutely, within the flush
    threshold) 0."""
    case = R.peaked()
    tok, conf = run_and_check(case, [route], "peaked")[route]
    assert np.all(conf[:, 1:] <= R.FLUSH) and np.all(np.abs(conf[:, 0] - 1.0) <= R.ULP)
