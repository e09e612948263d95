"""The float64 reference of the token predictor (tests/_predictor_ref.py) is right, and the cases it builds for
tests/test_gpu_predictor_edges.py are what they claim: runs without a GPU.

  * the reference against two implementations that are not it: the oracle's fp32 restatement of the reference's predictor, and
    torch.nn.LSTM(...).double() on the CPU for 1 .. 4 layers;
  * every random case leaves at least 100 x the measured fp32 logit error between neighbours among its best k + 1 logits, so the GPU file
    compares rankings exactly, without exemptions;
  * every tie case straddles the seam it is named for, computed from the launch constants restated in _predictor_ref.CONSTANTS, which the
    sources must still state;
  * every tie, uniform and absent-logit case yields its expected ranking in an fp32 numpy emulation added left to right and added
    pairwise: the expectation does not rest on an order of additions."""
import os
import re

import numpy as np
import pytest

from tests import _predictor_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIE_RUNS = [(name, cell) for name, t in R.TIE_CASES.items() for cell in (("degenerate",) if t["form"] == "one" else ("degenerate", "real"))]
ABSENT_RUNS = [(kind, vocab, n) for kind in ("three", "none", "tied", "nan") for vocab, n in ((136, 3), (8200, 5))] + [("three", 262145, 2), ("nan", 262145, 2)]


def test_reference_agrees_with_the_oracle(oracle):
    rng = np.random.default_rng(0)                                  # (a seed at which the gap condition below holds)
    vocab, n, k = 777, 9, 8
    emb = (rng.standard_normal((vocab, R.EMB)) * 0.5).astype(np.float32)
    wout = (rng.standard_normal((vocab, R.HID)) * 0.5).astype(np.float32)
    hist = rng.integers(0, vocab, (n, R.HIST))
    hist[2, :4] = vocab + 9
    case = R._case("degenerate", vocab, n, k, emb, wout, hist)
    tok, conf, _ = R.reference(case)
    e_logit, e_conf, _ = R.fp32_errors(case)
    assert min(g.min() for g in R.top_gaps(case)) >= 100 * e_logit
    for i in range(n):
        o_tok, o_conf = oracle.lstm_predict(emb, wout, hist[i].astype(np.uint32), k)
        assert o_tok.astype(np.int32).tolist() == tok[i].tolist(), i
        assert np.all(np.abs(o_conf - conf[i]) <= max(4 * e_conf, R.ULP) * conf[i]), (i, np.abs(o_conf / conf[i] - 1).max(), e_conf)


@pytest.mark.parametrize("layers", [1, 2, 3, 4])
def test_reference_agrees_with_torch_lstm_in_float64(layers):
    import torch
    rng = np.random.default_rng(layers)
    vocab, n, k = 300, 7, 8
    emb = (rng.standard_normal((vocab, R.EMB)) * 0.5).astype(np.float32)
    wout = (rng.standard_normal((vocab, R.HID)) * 0.5).astype(np.float32)
    bias = (rng.standard_normal(vocab) * 0.3).astype(np.float32)
    hist = rng.integers(0, vocab, (n, R.HIST))
    hist[1, 3:6] = vocab
    hist[4, 0] = -1
    w = R.lstm_weights(rng, layers)
    lstm = torch.nn.LSTM(R.EMB, R.HID, num_layers=layers, batch_first=True).double()
    with torch.no_grad():
        for l in range(layers):
            for name, arr in zip(("weight_ih", "weight_hh", "bias_ih", "bias_hh"), w):
                getattr(lstm, f"{name}_l{l}").copy_(torch.from_numpy(arr[l].astype(np.float64)))
        ok = torch.from_numpy((hist >= 0) & (hist < vocab))
        x = torch.from_numpy(emb.astype(np.float64))[torch.from_numpy(hist).clamp(0, vocab - 1)] * ok.unsqueeze(-1)
        out, _ = lstm(x)
        probs = torch.softmax(out[:, -1] @ torch.from_numpy(wout.astype(np.float64)).T + torch.from_numpy(bias.astype(np.float64)), -1)
        want_p, want_t = probs.topk(k, dim=-1)
    hidden = R.hidden_lstm(emb, hist, *w)
    assert np.abs(hidden - out[:, -1].numpy()).max() <= 1e-13
    tok, conf = R.predict(hidden, wout, bias, k)
    assert tok.tolist() == want_t.numpy().tolist()
    assert np.abs(conf - want_p.numpy()).max() <= 1e-13


def test_sources_still_state_the_constants_the_seams_are_computed_from():
    text = ""
    for name in ("kernels.hpp", "predictor_kernels.inl"):
        with open(os.path.join(ROOT, "cxl-speckv_amd", "csrc", name)) as f:
            text += f.read()
    for name, value in R.CONSTANTS.items():
        m = re.search(r"\b%s\s*=\s*([^,;]+)[,;]" % name, text)
        assert m, name
        assert m.group(1).strip().rstrip("u") == str(value), (name, m.group(1))
    # k_predict_small: a workgroup of four waves, 32 output rows a wave; the merge holds one part per lane
    assert "tile * 32u + c" in text and "blockIdx.x * 4u + wave" in text and "wave * 64u + lane" in text
    assert R.SMALL_ROWS == 4 * R.WAVE_ROWS


@pytest.mark.parametrize("name", sorted(R.RANDOM_CASES) + ["peaked"])
def test_random_cases_keep_a_gap_of_100_logit_errors(name):
    case = R.peaked() if name == "peaked" else R.random_case(name)
    e_logit, e_conf, ranks = R.fp32_errors(case)
    gap = min(float(g.min()) for g in R.top_gaps(case))
    print(f"{name}: E_logit {e_logit:.3g} E_conf {e_conf:.3g} smallest gap {gap:.3g} = {gap / e_logit:.0f} E_logit")
    assert all(len(g) == case["k"] for g in R.top_gaps(case))
    assert gap >= 100 * e_logit
    if name == "peaked":
        assert gap > 100
        conf = R.reference(case)[1]
        assert np.all(conf[:, 0] == 1.0) and np.all(conf[:, 1:] < R.FLUSH)          # every confidence but the first underflows in fp32
    for r in ranks:
        assert np.array_equal(r, R.reference(case)[0])


def test_tie_cases_straddle_the_seams_they_are_named_for():
    c = R.CONSTANTS
    for name, t in R.TIE_CASES.items():
        assert R.route(t["vocab"], t["n"], t["form"] == "split") == t["form"], name
    top = lambda name: R.TIE_CASES[name]["top"]
    split = lambda name: [R.place_split(i) for i in top(name)]          # (part, wave, thread, register)
    small = lambda name: [R.place_small(i) for i in top(name)]          # (merge wave, workgroup, wave, lane)
    one = lambda name: [R.place_one(i) for i in top(name)]              # (thread, iteration)
    parts = (8200 + c["kPredictTopkSpan"] - 1) // c["kPredictTopkSpan"]
    assert parts == 3
    assert split("split-thread-stride") == [(0, 3, c["kTkThreads"] - 1, 0), (0, 0, 0, 1)]       # last thread's first register, first thread's second
    assert split("split-wave") == [(0, 0, 63, 0), (0, 1, 64, 0)]
    assert split("split-part") == [(0, 3, 255, 15), (1, 0, 0, 0)]
    nine = split("split-one-thread-nine")
    assert len(nine) == 9 > 8 and {p[:3] for p in nine} == {(0, 0, 7)} and [p[3] for p in nine] == list(range(9))
    assert split("split-first-last") == [(0, 0, 5, 0), (parts - 1, 0, 7, 0)] and top("split-first-last")[1] == 8200 - 1
    gb = R.TIE_CASES["split-group-boundary"]
    assert len(gb["top"]) < 8 < len(gb["top"]) + len(gb["second"])
    assert {R.place_split(i)[0] for i in gb["top"]} == {0, 1, 2} == {R.place_split(i)[0] for i in gb["second"]}
    assert (8320 + R.SMALL_ROWS - 1) // R.SMALL_ROWS == R.MERGE_LANES + 1                         # 65 workgroups: the second merge wave has one part
    assert small("small-wave-rows") == [(0, 0, 0, 31), (0, 0, 1, 0)]
    assert small("small-workgroup") == [(0, 0, 3, 31), (0, 1, 0, 0)]
    assert small("small-merge-wave") == [(0, 63, 3, 31), (1, 64, 0, 0)]
    assert 32768 // R.SMALL_ROWS == c["kPredictSmallMaxParts"] == 4 * R.MERGE_LANES
    assert small("small-first-last") == [(0, 0, 0, 0), (3, 255, 3, 31)]
    assert small("small-merge-wave-1-2") == [(1, 127, 3, 31), (2, 128, 0, 0)]
    assert 262145 > c["kPredictTopkMaxParts"] * c["kPredictTopkSpan"]
    assert one("one-thread-stride") == [(c["kSmThreads"] - 1, 0), (0, 1)]
    assert one("one-same-thread") == [(9, 0), (9, 1), (9, 2)]
    assert one("one-last-token") == [(1023, 255), (0, 256)] and top("one-last-token")[1] == 262145 - 1


def _check_designed(case, what):
    tok, conf, l64 = R.reference(case)
    e_logit, e_conf, ranks = R.fp32_errors(case)
    assert np.array_equal(tok, case["expect"]), what
    for order, r in zip(("left to right", "pairwise"), ranks):
        assert np.array_equal(r, case["expect"]), (what, order)
    gaps = np.concatenate(R.top_gaps(case)) if case["n"] else np.zeros(0)
    assert np.all((gaps == 0.0) | (gaps >= 100 * e_logit)), (what, gaps[gaps > 0].min(), e_logit)      # an exact tie or a forced rank, nothing between
    return tok, conf, gaps


@pytest.mark.parametrize("name,cell", TIE_RUNS)
def test_tie_cases_rank_as_expected_in_fp32_in_both_orders(name, cell):
    case = R.tie(name, cell)
    tok, conf, gaps = _check_designed(case, (name, cell))
    top, second = case["groups"]
    assert (gaps == 0.0).sum() >= case["n"] * (len(top) - 1), "the tied ids have bit-equal float64 logits"
    assert np.array_equal(case["wout"][top], np.repeat(case["wout"][top[:1]], len(top), 0))
    if cell == "real":
        assert np.abs(R.reference(case)[2] - case["bias"].astype(np.float64)).max() < 3.0      # |h . w| < 3 under biases 30 / 20 / 0
    else:
        assert np.all(R.hidden_of(case) > 0.0)


@pytest.mark.parametrize("cell", ["degenerate", "real"])
@pytest.mark.parametrize("vocab", [8200, 262145])
def test_uniform_cases_are_uniform(cell, vocab):
    case = R.uniform(cell, vocab)
    tok, conf, _ = _check_designed(case, (cell, vocab))
    assert np.all(np.abs(conf * vocab - 1.0) <= 1e-12)
    if cell == "degenerate":
        assert np.all(R.hidden_of(case) == 0.0)


@pytest.mark.parametrize("kind,vocab,n", ABSENT_RUNS)
def test_absent_logit_cases_rank_as_expected(kind, vocab, n):
    case = R.absent(kind, vocab, n)
    tok, conf, _ = _check_designed(case, (kind, vocab))
    bias = case["bias"]
    assert not np.isnan(conf).any()
    if kind == "three":
        assert np.all(tok[:, 3:] == -1) and np.all(tok[:, :3] >= 0) and np.all(conf[:, 3:] == 0.0)
        assert np.all(np.abs(conf.sum(-1) - 1.0) <= 1e-12) and np.isneginf(bias).sum() == vocab - 3
        assert tok[0, :3].tolist() != sorted(tok[0, :3].tolist()), "the order is not the ids'"
    elif kind == "none":
        assert np.all(tok == -1) and np.all(conf == 0.0) and np.isneginf(bias).all()
    else:
        top, second = case["groups"]
        gone = np.nonzero(~(bias > -np.inf))[0]
        assert len(gone) and not set(gone) & set(tok.reshape(-1).tolist())
        assert set(gone) & set(top), "an absent row inside the tied top group"
        assert np.isnan(bias).sum() == (2 if kind == "nan" else 0)
        # the softmax is over the present logits only
        l = R.reference(case)[2][0]
        p = np.exp(l[l > -np.inf] - l[l > -np.inf].max())
        assert abs(conf[0, 0] - p.max() / p.sum()) <= 1e-15
