"""The token predictor in float64, and the cases of tests/test_predictor_ref_cpu.py (which checks the reference and the cases) and
tests/test_gpu_predictor_edges.py (which runs them on the device).  numpy only.

The operation (csrc/predictor_kernels.inl): a 16-token history -> a hidden vector of 128 (the reference's degenerate cell, or a real LSTM
cell in nn.LSTM's conventions) -> logits = wout h (+ out_bias) -> softmax -> the k best tokens with their probabilities.  The rules pinned
here: rank by (logit descending, token id ascending); a logit that is not greater than -inf (-inf or NaN) is ABSENT -- never chosen, not
in the softmax; a rank without a candidate is (-1, 0.0).  +inf logits are out of scope.

Tolerances come from the reference, not from the kernels: fp32_errors() evaluates the same maths in fp32 numpy in two orders of addition
(left to right, as the oracle adds, and pairwise) and takes the larger error against float64 -- E_logit absolute over the logits, E_conf
relative over the reported confidences.  conf_tolerance() is the device's bound: 4 x E_conf, not below one fp32 ulp (2^-23: the
result is stored in fp32) and not above the ceiling of the older tests (5e-4 relative with the degenerate cell, 2e-5 absolute with the real
one), plus the fp32 flush threshold 1.2e-38 as the absolute term for confidences that underflow.  The factor 4 is a chosen margin for
the hardware's exp2 and reciprocal (about 1 ulp each, chained 16 x layers x 2 times in the cell, once per softmax term); nobody has measured
it.  Values derived on the cases below (E_logit / E_conf, the larger of the two orders):
    random, degenerate cell, vocab 200 .. 32769     1.2e-6 .. 3.3e-6 / 1.3e-6 .. 6.2e-6
    random, real cell, 1 .. 4 layers                1.6e-6 .. 1.9e-6 / 1.4e-6 .. 1.7e-6
    ties, degenerate cell, vocab 8200 .. 32768      1.9e-6 .. 4.8e-6 / 2.7e-6 .. 4.6e-5
    ties, degenerate cell, vocab 262145             1.9e-6 .. 2.7e-6 / 8.5e-5 .. 5.8e-4 (262 145 terms added left to right; 4 x that is
                                                    above the 5e-4 ceiling, which holds)
    ties and absent logits, real cell (bias 30)     4.1e-7 .. 9.5e-7 / up to 1.7e-6
    uniform                                         0 .. 6.6e-7 / < 1e-9 (the bound is the fp32 ulp)
    peaked (logits ~ 1e6, gaps > 100)               0.6 / 0 (the confidences are 1 and 0)
"""
import functools

import numpy as np

HIST, EMB, HID = 16, 64, 128
# the launch constants the seams are computed from (test_predictor_ref_cpu.py asserts that the sources still state them)
CONSTANTS = {
    "kPredictTopkSpan": 4096, "kPredictTopkMaxParts": 64, "kPredictSmallN": 4, "kPredictSmallMaxParts": 256,      # kernels.hpp
    "kTkThreads": 256, "kSmThreads": 1024, "kLogitsTile": 32, "kLogitsChunk": 128,                             # predictor_kernels.inl
}
SMALL_ROWS, WAVE_ROWS, MERGE_LANES = 128, 32, 64        # k_predict_small: rows of a workgroup and of a wave; parts of one merge wave
FLUSH = 1.2e-38                                        # fp32's denormal-flush threshold
ULP = 2.0 ** -23
CEILING = {"degenerate": ("rel", 5e-4), "real": ("abs", 2e-5)}


# ---- where a token id lands in each top-k form ------------------------------------------------------------------------------------------
def place_split(i):
    """k_softmax_topk_small: (part, wave, thread, register) of logit i"""
    c = CONSTANTS
    part, r = divmod(i, c["kPredictTopkSpan"])
    j, tid = divmod(r, c["kTkThreads"])
    return part, tid // 64, tid, j


def place_small(i):
    """k_predict_small + k_predict_small_merge: (merge wave, workgroup, wave, lane) of output row i"""
    wg, r = divmod(i, SMALL_ROWS)
    return wg // MERGE_LANES, wg, r // WAVE_ROWS, r % WAVE_ROWS


def place_one(i):
    """k_softmax_topk: (thread, iteration) of logit i"""
    it, tid = divmod(i, CONSTANTS["kSmThreads"])
    return tid, it


def route(vocab, n, force_batch):
    """the kernels launch_predict takes: 'small', 'split' (k_softmax_topk_small + merge) or 'one' (k_softmax_topk)"""
    c = CONSTANTS
    if n <= c["kPredictSmallN"] and (vocab + SMALL_ROWS - 1) // SMALL_ROWS <= c["kPredictSmallMaxParts"] and not force_batch:
        return "small"
    return "split" if (vocab + c["kPredictTopkSpan"] - 1) // c["kPredictTopkSpan"] <= c["kPredictTopkMaxParts"] else "one"


# ---- the maths, in a chosen precision and order of addition ------------------------------------------------------------------------------
def _sum_last(a, order):
    """sum over the last axis in a's own precision: 'seq' left to right, 'pair' by halves"""
    if order == "seq":
        acc = a[..., 0].copy()
        for j in range(1, a.shape[-1]):
            acc = acc + a[..., j]
        return acc
    n = a.shape[-1]
    while n > 1:
        if n & 1:
            a = np.concatenate([a, np.zeros_like(a[..., :1])], -1)
            n += 1
        a = a[..., : n // 2] + a[..., n // 2:]
        n //= 2
    return a[..., 0]


def _matvec(h, w, order):
    """[n][C] x [R][C] -> [n][R] in the operands' precision; order None: numpy's own (float64 reference)"""
    if order is None:
        return h @ w.T
    if order == "seq":
        acc = np.zeros((h.shape[0], w.shape[0]), h.dtype)
        for j in range(h.shape[1]):
            acc = acc + h[:, j:j + 1] * w[None, :, j]
        return acc
    out = np.empty((h.shape[0], w.shape[0]), h.dtype)
    step = max(1, (1 << 22) // (h.shape[0] * h.shape[1]))
    for r0 in range(0, w.shape[0], step):
        out[:, r0:r0 + step] = _sum_last(h[:, None, :] * w[None, r0:r0 + step, :], "pair")
    return out


def _embed(emb, hist, dtype):
    hist = np.asarray(hist, np.int64).reshape(-1, HIST)
    ok = (hist >= 0) & (hist < emb.shape[0])                      # out-of-vocabulary and negative ids embed as zeros
    x = np.asarray(emb)[np.where(ok, hist, 0)].astype(dtype)
    x[~ok] = 0
    return x


def hidden_degenerate(emb, hist, layers=2, dtype=np.float64, order=None):
    """the reference's cell: gates fixed at 0.5, candidate g_t = sum_j 0.1 emb[token_t][j]; every one of the 128 hidden values is the same"""
    x = _embed(emb, hist, dtype) * dtype(0.1)
    g = x.sum(-1) if order is None else _sum_last(x, order)
    half = dtype(0.5)
    c = np.zeros(g.shape[0], dtype)
    h = np.zeros(g.shape[0], dtype)
    for t in range(HIST):
        for _ in range(layers):
            c = half * c + half * np.tanh(g[:, t])
            h = half * np.tanh(c)
    return np.repeat(h[:, None], HID, axis=1)


def hidden_lstm(emb, hist, w_ih, w_hh, b_ih, b_hh, dtype=np.float64, order=None):
    """nn.LSTM: per layer gates = W_ih x + W_hh h + b_ih + b_hh (rows i, f, g, o), c = s(f) c + s(i) tanh(g), h = s(o) tanh(c), h_0 = c_0 = 0"""
    one = dtype(1.0)
    sig = lambda v: one / (one + np.exp(-v))
    seq = _embed(emb, hist, dtype)
    n = seq.shape[0]
    h = np.zeros((n, HID), dtype)
    for l in range(len(w_ih)):
        wi, wh = np.asarray(w_ih[l]).astype(dtype), np.asarray(w_hh[l]).astype(dtype)
        b = np.asarray(b_ih[l]).astype(dtype) + np.asarray(b_hh[l]).astype(dtype)
        h = np.zeros((n, HID), dtype)
        c = np.zeros((n, HID), dtype)
        out = []
        for t in range(HIST):
            gates = _matvec(seq[:, t], wi, order) + _matvec(h, wh, order) + b
            i, f, g, o = (gates[:, q * HID:(q + 1) * HID] for q in range(4))
            c = sig(f) * c + sig(i) * np.tanh(g)
            h = sig(o) * np.tanh(c)
            out.append(h)
        seq = np.stack(out, 1)
    return h


def logits_of(hidden, wout, bias=None, order=None):
    """float64 (order None) or the operands' fp32 in the given order.  The float64 logits are added pairwise with elementwise operations
    only, so that identical rows give identical logits (a BLAS product lets the last bit depend on where a row stands)."""
    dtype = hidden.dtype
    order = order or "pair"
    wout = np.asarray(wout)
    out = np.empty((hidden.shape[0], wout.shape[0]), dtype)
    for r0 in range(0, wout.shape[0], 65536):
        out[:, r0:r0 + 65536] = _matvec(hidden, wout[r0:r0 + 65536].astype(dtype), order)
    if bias is not None:
        with np.errstate(invalid="ignore"):
            out = out + np.asarray(bias).astype(dtype)[None, :]
    return out


def rank(logits, k):
    """tokens [n][k] int32 and confidences [n][k] float64 by the pinned rules, from logits of any precision (softmax in float64)"""
    n = logits.shape[0]
    tok = np.full((n, k), -1, np.int32)
    conf = np.zeros((n, k), np.float64)
    for b in range(n):
        l = logits[b].astype(np.float64)
        with np.errstate(invalid="ignore"):
            ids = np.nonzero(l > -np.inf)[0]                      # -inf and NaN are absent
        if not len(ids):
            continue
        lp = l[ids]
        best = np.lexsort((ids, -lp))[:k]
        p = np.exp(lp - lp.max())
        tok[b, :len(best)] = ids[best]
        conf[b, :len(best)] = p[best] / p.sum()
    return tok, conf


def predict(hidden, wout, bias, k):
    return rank(logits_of(np.asarray(hidden, np.float64), wout, bias), k)


def hidden_of(case, dtype=np.float64, order=None):
    if case["lstm"] is None:
        return hidden_degenerate(case["emb"], case["hist"], 2, dtype, order)
    return hidden_lstm(case["emb"], case["hist"], *case["lstm"], dtype=dtype, order=order)


def reference(case):
    """(tokens, confidences, logits) of a case in float64; computed once per case"""
    if "_ref" not in case:
        l = logits_of(hidden_of(case), case["wout"], case["bias"])
        case["_ref"] = rank(l, case["k"]) + (l,)
    return case["_ref"]


def _conf32(l32, tok, order):
    """the confidences of tokens `tok` from fp32 logits, every step in fp32"""
    out = np.zeros(tok.shape, np.float32)
    for b in range(l32.shape[0]):
        with np.errstate(invalid="ignore"):
            lp = l32[b][l32[b] > -np.inf]
        if not len(lp):
            continue
        p = np.exp(lp - lp.max())
        s = _sum_last(p, order)
        live = tok[b] >= 0
        out[b, live] = np.exp(l32[b][tok[b][live]] - lp.max()) / s
    return out


def fp32_errors(case):
    """(E_logit, E_conf, rankings): the case's maths in fp32 numpy, added left to right and pairwise, against float64 -- the larger absolute
    error of a logit, the larger relative error of a reported confidence (those above the flush threshold), and the two fp32 rankings"""
    if "_err" not in case:
        tok, conf, l64 = reference(case)
        e_logit = e_conf = 0.0
        ranks = []
        with np.errstate(invalid="ignore"):
            present = l64 > -np.inf
        for order in ("seq", "pair"):
            l32 = logits_of(hidden_of(case, np.float32, order), case["wout"], case["bias"], order)
            assert l32.dtype == np.float32
            if present.any():
                e_logit = max(e_logit, float(np.abs(l32.astype(np.float64)[present] - l64[present]).max()))
            c32 = _conf32(l32, tok, order).astype(np.float64)
            big = conf > FLUSH
            if big.any():
                e_conf = max(e_conf, float((np.abs(c32 - conf)[big] / conf[big]).max()))
            ranks.append(rank(l32, case["k"])[0])
        case["_err"] = (e_logit, e_conf, ranks)
    return case["_err"]


def conf_tolerance(case):
    """the device's bound on |confidence - float64|, per reported rank"""
    conf = reference(case)[1]
    tol = max(4.0 * fp32_errors(case)[1], ULP) * conf
    kind, ceil = CEILING[case["cell"]]
    return np.minimum(tol, ceil * conf if kind == "rel" else ceil) + FLUSH


def top_gaps(case):
    """float64 logit gaps between neighbours among each request's best k + 1 present logits: [n][<= k]"""
    l64 = reference(case)[2]
    out = []
    for b in range(l64.shape[0]):
        with np.errstate(invalid="ignore"):
            lp = np.sort(l64[b][l64[b] > -np.inf])[::-1][:case["k"] + 1]
        out.append(-np.diff(lp))
    return out


# ---- weights ----------------------------------------------------------------------------------------------------------------------------
def _tiled(block, rows):
    """`rows` rows by repeating a small block (the 262 145-token cases are built in well under a second)"""
    reps = (rows + len(block) - 1) // len(block)
    return np.ascontiguousarray(np.tile(block, (reps, 1))[:rows])


def lstm_weights(rng, layers, scale=0.15):
    u = lambda *shape: (rng.standard_normal(shape) * scale).astype(np.float32)
    w_ih = [u(4 * HID, EMB if l == 0 else HID) for l in range(layers)]
    w_hh = [u(4 * HID, HID) for _ in range(layers)]
    return w_ih, w_hh, [u(4 * HID) for _ in range(layers)], [u(4 * HID) for _ in range(layers)]


def _case(cell, vocab, n, k, emb, wout, hist, lstm=None, bias=None, **more):
    assert (cell == "real") == (lstm is not None)
    d = dict(cell=cell, vocab=vocab, n=n, k=k, emb=np.ascontiguousarray(emb, np.float32), wout=np.ascontiguousarray(wout, np.float32),
             hist=np.ascontiguousarray(hist, np.int32), lstm=lstm, bias=None if bias is None else np.ascontiguousarray(bias, np.float32))
    d.update(more)
    return d


# ---- ties -------------------------------------------------------------------------------------------------------------------------------
# A tie must be bit-equal on the device whatever the order of its additions: tied tokens have IDENTICAL wout rows (and out_bias), and the
# rank between groups is forced from outside the dot product.  Degenerate cell: every element of a row is one constant, a multiple of
# 1/1024 -- 1/16 for the top group, 3/64 for the second, (id mod 33)/1024 <= 1/32 for everybody else -- and embeddings are positive, so the
# hidden value h is > 0 and the logit 128 h c grows with c.  Real cell: out_bias 30 / 20 / 0 with |h . w| < 3 (|h| < 1, a row's absolute
# sum < 3).  The groups together hold at least k + 1 ids, so no rank and no neighbour of a rank is left to a chance gap.
def filler(vocab, avoid, count=7):
    """a second group for the cases that name only the tied pair: ids spread over the vocabulary"""
    out = []
    for j in range(1, 64):
        i = (vocab * j) // (count + 1) + 3
        while i in avoid or i in out:
            i += 1
        if i < vocab:
            out.append(i)
        if len(out) == count:
            break
    return out


def tie_case(cell, vocab, groups, n, k=8, seed=0, absent=(), nan=()):
    """groups = [top ids, second ids]; absent / nan (real cell): ids whose out_bias is -inf / NaN.  Returns the case with case["expect"]:
    the ranking every request must report (the groups' present ids in ascending order, top group first)."""
    top, second = (sorted(int(i) for i in g) for g in groups)
    assert not set(top) & set(second) and max(top + second) < vocab
    gone = set(absent) | set(nan)
    expect = [i for i in top + second if i not in gone]
    assert len(expect) >= k + 1, "the groups' present ids cover every rank and its neighbour"
    rng = np.random.default_rng(seed)
    blk = min(vocab, 4096)
    hist = rng.integers(0, vocab, (n, HIST))
    if cell == "degenerate":
        assert not gone, "the degenerate cell has no out_bias"
        emb = _tiled(rng.uniform(0.02, 0.3, (blk, EMB)).astype(np.float32), vocab)
        c = (np.arange(vocab) % 33).astype(np.float32) / 1024
        c[top] = 1.0 / 16
        c[second] = 3.0 / 64
        wout = np.empty((vocab, HID), np.float32)
        wout[:] = c[:, None]
        case = _case(cell, vocab, n, k, emb, wout, hist)
    else:
        emb = _tiled((rng.standard_normal((blk, EMB)) * 0.5).astype(np.float32), vocab)
        wout = _tiled((rng.uniform(-1, 1, (blk, HID)) * (3.0 / HID)).astype(np.float32), vocab)
        wout[top] = wout[top[0]]
        if second:
            wout[second] = wout[second[0]]
        assert float(np.abs(wout).sum(-1).max()) < 3.0
        bias = np.zeros(vocab, np.float32)
        bias[top] = 30.0
        bias[second] = 20.0
        bias[list(absent)] = -np.inf
        bias[list(nan)] = np.nan
        case = _case(cell, vocab, n, k, emb, wout, hist, lstm_weights(rng, 2), bias)
    want = (expect + [-1] * k)[:k]
    case["expect"] = np.tile(np.array(want, np.int32), (n, 1))
    case["groups"] = (top, second)
    return case


def _seam(name, vocab, n, form, top, second=None):
    return dict(name=name, vocab=vocab, n=n, form=form, top=list(top), second=second)


# name -> (vocab, n, the top-k form whose seam it straddles, top group, second group or None = filler)
TIE_CASES = {c["name"]: c for c in [
    # batch route, split top-k: 3 parts of 4096 logits, 256 threads x 16 registers a part
    _seam("split-thread-stride", 8200, 5, "split", [255, 256]),
    _seam("split-wave", 8200, 5, "split", [63, 64]),
    _seam("split-part", 8200, 5, "split", [4095, 4096]),
    _seam("split-one-thread-nine", 8200, 5, "split", [7 + 256 * j for j in range(9)], []),
    _seam("split-first-last", 8200, 5, "split", [5, 8199]),
    _seam("split-group-boundary", 8200, 5, "split", [300, 4396, 8198], [2, 66, 258, 4095, 4096, 4098, 6000, 8192, 8199]),
    # small route: 65 workgroups of 128 rows -> the second merge wave; 256 workgroups -> all four
    _seam("small-wave-rows", 8320, 4, "small", [31, 32]),
    _seam("small-workgroup", 8320, 1, "small", [127, 128]),
    _seam("small-merge-wave", 8320, 4, "small", [8191, 8192]),
    _seam("small-first-last", 32768, 1, "small", [0, 32767]),
    _seam("small-merge-wave-1-2", 32768, 4, "small", [16383, 16384]),
    # one workgroup of 1024 threads
    _seam("one-thread-stride", 262145, 2, "one", [1023, 1024]),
    _seam("one-same-thread", 262145, 2, "one", [9, 1033, 2057]),
    _seam("one-last-token", 262145, 2, "one", [262143, 262144]),
]}


@functools.lru_cache(maxsize=None)
def tie(name, cell):
    t = TIE_CASES[name]
    second = t["second"] if t["second"] is not None else filler(t["vocab"], set(t["top"]))
    case = tie_case(cell, t["vocab"], [t["top"], second], t["n"], 8, seed=len(name) + t["vocab"])
    case["form"] = t["form"]
    return case


@functools.lru_cache(maxsize=None)
def uniform(cell, vocab, n=2, k=8):
    """every logit the same: tokens 0 .. k-1, every confidence 1/vocab.  Degenerate cell: a history that is entirely out of vocabulary gives
    hidden = 0.  Real cell: the same history, every wout row the same, a constant out_bias."""
    rng = np.random.default_rng(vocab)
    blk = min(vocab, 4096)
    hist = np.full((n, HIST), vocab + 5)
    hist[0, ::2] = -3
    emb = _tiled((rng.standard_normal((blk, EMB)) * 0.5).astype(np.float32), vocab)
    if cell == "degenerate":
        case = _case(cell, vocab, n, k, emb, _tiled((rng.standard_normal((blk, HID)) * 0.5).astype(np.float32), vocab), hist)
    else:
        row = (rng.standard_normal((1, HID)) * 0.5).astype(np.float32)
        case = _case(cell, vocab, n, k, emb, _tiled(row, vocab), hist, lstm_weights(rng, 2), np.full(vocab, 1.5, np.float32))
    case["expect"] = np.tile(np.arange(k, dtype=np.int32), (n, 1))
    return case


# ---- absent logits (real cell, out_bias) ------------------------------------------------------------------------------------------------
def _spread(vocab):
    """three ids in three different places of every form: (late, early, middle)"""
    return [vocab - 1, 5, vocab // 2 + 2]


@functools.lru_cache(maxsize=None)
def absent(kind, vocab, n):
    """kind 'three': all rows -inf but three (biases 20 / 10 / 0, so the order is not the ids'); 'none': every row -inf; 'tied': -inf rows
    inside tied groups; 'nan': a NaN row in the top group and one outside the groups"""
    k = 8
    if kind in ("three", "none"):
        rng = np.random.default_rng(vocab + n)
        blk = min(vocab, 4096)
        emb = _tiled((rng.standard_normal((blk, EMB)) * 0.5).astype(np.float32), vocab)
        wout = _tiled((rng.uniform(-1, 1, (blk, HID)) * (3.0 / HID)).astype(np.float32), vocab)
        bias = np.full(vocab, -np.inf, np.float32)
        keep = _spread(vocab) if kind == "three" else []
        bias[keep] = [20.0, 10.0, 0.0][:len(keep)]
        case = _case("real", vocab, n, k, emb, wout, rng.integers(0, vocab, (n, HIST)), lstm_weights(rng, 2), bias)
        case["expect"] = np.tile(np.array((keep + [-1] * k)[:k], np.int32), (n, 1))
        return case
    a, b, c = _spread(vocab)
    top = [b, b + 1, 40, 41, c, a - 1, a]
    second = [i for i in filler(vocab, set(top), 9)]
    if kind == "tied":
        return tie_case("real", vocab, [top, second], n, k, seed=vocab + 1, absent=[b + 1, c, a, second[0], second[4]])
    assert kind == "nan"
    other = next(i for i in range(vocab // 3, vocab) if i not in top and i not in second)
    return tie_case("real", vocab, [top, second], n, k, seed=vocab + 2, nan=[41, other])


# ---- random weights ---------------------------------------------------------------------------------------------------------------------
# Every random case has float64 logit gaps among each request's best k + 1 of at least 100 x E_logit (test_predictor_ref_cpu.py asserts it;
# the seeds were chosen until it held), so the device must report the float64 ranking exactly: no comparison here is free of order.
RANDOM_CASES = {
    # launch seams of the batch route: columns of kLogitsChunk = 128 requests, tiles of 32, four requests a merge workgroup
    "seam-4": ("degenerate", 200, 4, 6, 2, 1), "seam-5": ("degenerate", 200, 5, 7, 2, 0), "seam-127": ("degenerate", 200, 127, 6, 2, 13),
    "seam-128": ("degenerate", 200, 128, 7, 2, 7), "seam-129": ("degenerate", 200, 129, 2, 2, 1), "seam-161": ("degenerate", 200, 161, 3, 2, 2),
    "seam-257": ("degenerate", 200, 257, 2, 2, 4), "seam-129-real": ("real", 200, 129, 3, 2, 2),
    # merge fan-in of the small route: 65, 65, 157 and 256 workgroups; one row past 256 workgroups: the batch route
    "fan-8193": ("degenerate", 8193, 4, 8, 2, 0), "fan-8320": ("degenerate", 8320, 2, 3, 2, 0), "fan-20000": ("degenerate", 20000, 3, 7, 2, 1),
    "fan-32768": ("degenerate", 32768, 4, 8, 2, 1), "fan-32769": ("degenerate", 32769, 4, 8, 2, 1),
    # depth of the real cell
    "depth-1": ("real", 1000, 6, 8, 1, 0), "depth-3": ("real", 1000, 6, 8, 3, 0), "depth-4": ("real", 1000, 6, 8, 4, 0),
}


def _random(cell, vocab, n, k, layers, seed, scale=0.5):
    rng = np.random.default_rng([seed, vocab, n, layers])
    emb = (rng.standard_normal((vocab, EMB)) * 0.5).astype(np.float32)
    wout = (rng.standard_normal((vocab, HID)) * scale).astype(np.float32)
    hist = rng.integers(0, vocab, (n, HIST))
    hist[0, :3] = vocab + 1                                          # out-of-vocabulary ids embed as zeros
    hist[n - 1, 5] = -2
    if cell == "degenerate":
        return _case(cell, vocab, n, k, emb, wout, hist)
    return _case(cell, vocab, n, k, emb, wout, hist, lstm_weights(rng, layers), (rng.standard_normal(vocab) * 0.3).astype(np.float32))


@functools.lru_cache(maxsize=None)
def random_case(name):
    return _random(*RANDOM_CASES[name])


PEAKED = dict(vocab=300, n=3, k=8, seed=0, scale=3.0e5)


@functools.lru_cache(maxsize=None)
def peaked():
    """wout scaled until the float64 logit gaps among the best k + 1 exceed 100: every confidence but the first underflows in fp32, so a
    ranking by fp32 probability (the oracle's) sees ties where the logits, and float64, see an order"""
    p = PEAKED
    return _random("degenerate", p["vocab"], p["n"], p["k"], 2, p["seed"], p["scale"])


def sub_case(case, rows):
    """the same weights with a subset of the requests (a route that takes at most four)"""
    d = {key: val for key, val in case.items() if not key.startswith("_")}
    d["hist"] = np.ascontiguousarray(case["hist"][rows])
    d["n"] = len(d["hist"])
    if "expect" in d:
        d["expect"] = case["expect"][rows]
    return d
