"""Not -m gpu: SpeckvKVConnector.attend_spec(window=W) on an FP8 pool -- the ValueErrors of the argument, window=None / 0 issuing exactly today's library
calls (a recording stand-in), and a numpy restatement of the entry's documented arithmetic against float64 softmax inside the GPU test's bound."""
import numpy as np
import pytest

from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from tests._gpu import D, H, HeadChecker
from tests.test_gpu_decode_window import content
from tests.test_k8v4_spec_cpu import _step
from tests.test_paged_io_cpu import _cpu_torch

L, T, SM, PTR = 4, 256, 1.0 / np.sqrt(D), "address"              # (L: the layers of tests.test_k8v4_spec_cpu._step)


class _Recording:                  # every library call by name and arguments, the addresses among them (anything from 2^32 on) as PTR; all answer 0
    def __getattr__(self, name):
        plain = lambda x: PTR if isinstance(x, int) and x >= 2 ** 32 else x if isinstance(x, (int, float)) else [int(v) for v in x]
        return lambda *a: (self.__dict__.setdefault("calls", []).append((name,) + tuple(plain(x) for x in a)), 0)[1]


def _calls(torch, scheme, st, q, k_new, v_new, layer, lengths=(0, 1, 37, 36), n_layers=None, **how):
    conn = SpeckvKVConnector(_Recording(), L, H, D, T, scheme)
    for b, n in enumerate(lengths):
        conn.add_request(10 + b)
        conn.requests[10 + b].length = n
        if n & 1:
            conn.requests[10 + b].set_tail(torch.randn((L, H, D)).to(torch.float16), torch.randn((L, H, D)).to(torch.float16))
    del conn.lib.calls[:]
    if n_layers is None:
        conn.attend_spec(layer, [10 + b for b in range(len(lengths))], q, k_new, v_new, 0.125, stream=st, **how)
    else:                                                        # attend_spec_layers from `layer` on, the same query rows on every layer
        conn.attend_spec_layers(layer, n_layers, [10 + b for b in range(len(lengths))], torch.stack([q] * n_layers), k_new, v_new, 0.125, stream=st, **how)
    return conn.lib.calls


def test_the_window_argument(monkeypatch):
    torch, st = _cpu_torch(monkeypatch)
    monkeypatch.setattr(torch, "zeros", lambda *a, device=None, _zeros=torch.zeros, **k: _zeros(*a, **k))      # (the plan buffer of the unwindowed route)
    step = _step(torch, 4, 4, 4)
    for scheme, bad, names in (("int4", 33, r"attend_chunk\(window=W\)"), ("mxfp4", 33, r"attend_chunk\(window=W\)"), ("fp8", -1, None), ("fp8", 1.5, None), ("fp8", 2 ** 32, None)):
        with pytest.raises(ValueError, match=names):
            _calls(torch, scheme, st, *step, 1, window=bad)
    today = [("attend_plan_bytes", 4), ("attend_batch_plan", [0, 0, 0, 0], [0, 0, 36, 36], T, 0, 0, 7),
             ("attend_planned", 4, 0, 4, 1, PTR, 16, T, 0.125, PTR, PTR, 7),
             ("attend_fold_held", 4, 0, H, 16, 4, PTR, PTR, PTR, 5 * H * D, H * D, PTR, 0, 0.125, PTR, PTR, 7)]
    for how in ({}, dict(window=None), dict(window=0)):
        assert _calls(torch, "fp8", st, *step, 1, **how) == today, how
    (name, handles, layer, _, g, R, pos_end, lengths, _, window, *rest), = _calls(torch, "fp8", st, *step, 1, window=33)
    assert (name, layer, g, R, pos_end, lengths, window) == ("attend_spec_window", 1, 16, 4, [0, 0, 36, 36], [0, 1, 37, 36], 33)
    # attend_spec_layers over layers 1 and 2: one call per layer and nothing else
    assert _calls(torch, "fp8", st, *step, 1, n_layers=2, window=33) == [
        ("attend_spec_window", [0, 0, 0, 0], layer, PTR, 16, 4, [0, 0, 36, 36], [0, 1, 37, 36], PTR, 33, PTR, PTR, 5 * H * D, H * D, PTR, 4, 0.125, PTR, 0, 7)
        for layer in (1, 2)]


@pytest.mark.parametrize("length,window", [(97, 33), (61, 33), (200, 100)])
def test_the_documented_arithmetic_stays_inside_the_bound(oracle, length, window):
    """16 chain rows as k_attend_fp8_spec computes them: E4M3 query on the pool positions [lo(d), stored), fp16 query on the held 0..d; a pool weight is
    fp16(p x vs / vref) -- vs the V page scale, vref the largest of the tile of 32 behind every window's front, the page cut by lo(0) at 2^-10 --, sums exact"""
    rng, stored, lo0, pos = np.random.default_rng(length), length & ~1, max(0, length + 1 - window), np.arange(T)
    c = HeadChecker(oracle, 4, content(lo0, stored)[:T], T)
    q, kh, vh = (rng.standard_normal((16, D)).astype(np.float16).astype(np.float64) for _ in range(3))      # (fp16 values)
    (K, V), qe, qf = c.kv(3), c.q_rows(q.astype(np.float16)), q
    vs = np.repeat(np.asarray(c.scales[T // 2:T], np.float64), 2)                              # the V page scale of every position
    cand = np.where((pos < (lo0 & ~1)) | (pos >= stored), 0.0, np.where((pos | 1) == lo0, vs * 2.0 ** -10, vs))
    vref = np.repeat(np.maximum(cand.reshape(-1, 32).max(axis=1), 1e-30), 32)
    worst = 0.0
    for d in range(16):
        lo = min(max(0, length + d + 1 - window), stored)
        s = np.concatenate([(K[lo:stored] @ qe[d]) * SM, (kh[:d + 1] @ qf[d]) * SM])
        vals = np.concatenate([V[lo:stored], vh[:d + 1]])
        p = np.exp(s - s.max())
        w = (p[:stored - lo] * vs[lo:stored] / vref[lo:stored]).astype(np.float16).astype(np.float64) * vref[lo:stored]
        got = ((w / vs[lo:stored]) @ V[lo:stored] + p[stored - lo:] @ vh[:d + 1]) / p.sum()
        delta = 3e-5 * max(float((np.abs(qe[d]) @ np.abs(K[lo:stored]).T).max(initial=0.0)), float((np.abs(qf[d]) @ np.abs(kh[:d + 1]).T).max())) * SM
        tol = (2e-3 + 2 * delta) * ((p @ np.abs(vals)) / p.sum()) + 1e-6
        worst = max(worst, float((np.abs(got - (p @ vals) / p.sum()) / tol).max()))
    print(f"fp8 spec window arithmetic, length {length} W {window}: worst err / tol {worst:.3f}")
    assert worst <= 1.0
