"""Not -m gpu: what tests/test_gpu_k8v4_decode_geometry.py rests on, checked without a GPU -- every regime of tests/_k8v4_cases.py
reaches its branch of the launch decision at 256 and at 304 CUs; the contents that file writes are sharp where k_attend_k8v4's addressing
is risky (the one E8M0 code byte per page and lane, the scale quadruple of a tile) while the rows of tests/test_gpu_k8v4_decode.py are
not; and the project's bound is met on such a content by the arithmetic the kernel is documented to do."""
import numpy as np
import pytest

from cxl_speckv_amd import kv_accuracy
from tests import _k8v4_cases as cases
from tests._rules import load_rules

H, D = cases.H, cases.D
SM = 1.0 / np.sqrt(D)


@pytest.fixture(scope="module")
def rules():
    return load_rules()


@pytest.mark.parametrize("n_cus", [256, 304])
@pytest.mark.parametrize("name", cases.REGIMES)
def test_every_regime_reaches_its_branch(rules, name, n_cus):
    d = cases.assert_branch(rules, name, cases.regime(name, n_cus), n_cus)
    print(f"{name} at {n_cus} CUs: {d['tps']} tiles a piece, {d['max_splits']} pieces at most, by length {d['by_length']}, "
          f"rows first {d['rows_first']}, {d['parts']} partials")


def _assert_sharp(k, v, what):
    (along_blocks, along_pages, distinct), k_step, positions = cases.content_is_sharp(k, v)
    print(f"{what}: equal codes {along_blocks:.3f} along blocks, {along_pages:.3f} along pages, {distinct} distinct; "
          f"K scale step {k_step:.3f}; effective positions {positions:.1f}")
    assert along_blocks <= 0.25 and along_pages <= 0.25 and distinct >= 9, what
    assert k_step >= 0.25 and positions >= 8.0, what


@pytest.mark.parametrize("name", cases.REGIMES)
def test_the_contents_of_every_regime_are_sharp(name):
    T = cases.layout_tokens(cases.regime(name, 256))
    assert T == cases.layout_tokens(cases.regime(name, 304))                    # the same contents on either machine
    contents = cases.case_contents(name, T)
    for c, (k, v) in enumerate(contents):
        assert k.shape == v.shape == (2, T, H, D) and k.dtype == v.dtype == np.float16
        assert not np.array_equal(k[0], k[1]) and not np.array_equal(v[0], v[1])     # the layers differ
        _assert_sharp(k, v, (name, c))
    for a in range(len(contents)):
        for b in range(a):
            assert not np.array_equal(contents[a][0], contents[b][0]) and not np.array_equal(contents[a][1], contents[b][1])


def test_the_contents_of_the_other_cases_are_sharp():
    for T in (256, 1024):
        for c, (k, v) in enumerate(cases.mixed_contents(T)):
            _assert_sharp(k, v, ("mixed", T, c))
    _assert_sharp(*cases.bound_content(), "the 2048-piece case")


def test_the_rows_of_the_existing_suite_are_not():
    """tests/test_gpu_k8v4_decode.py _prompt(): standard-normal rows -- most neighbouring blocks share their code (measured: 0.65 along
    either axis, 3 distinct codes, K scale steps of 0.085), which is why the geometry file writes contents of its own"""
    from tests.test_gpu_k8v4_decode import _prompt                              # (importing that module touches no GPU)
    k, v = _prompt()
    (along_blocks, along_pages, distinct), k_step, _ = cases.content_is_sharp(k, v)
    print(f"standard-normal rows: equal codes {along_blocks:.3f} / {along_pages:.3f}, {distinct} distinct, K scale step {k_step:.3f}")
    assert along_blocks >= 0.5 and along_pages >= 0.5


def emulate_kernel(q16, K, V, sm, tile=32):
    """k_attend_k8v4's documented arithmetic for one kv head in numpy: q16 [G][D] fp16 -> the E4M3 query x its row scale
    (kv_accuracy.quantize_query_e4m3), scores in float64, then per tile of 32 positions the online softmax -- the running maximum, the
    row sum from the unrounded p, the weights p ROUNDED TO FP16 against the running maximum into p.V, V exact; the fp32 accumulators
    are float64 here (their summation order is not modelled).  -> out [G][D], lse [G]"""
    qe = kv_accuracy.quantize_query_e4m3(q16)
    s = (qe @ K.T) * sm
    G, n = s.shape
    m, l, acc = np.full(G, -np.inf), np.zeros(G), np.zeros((G, V.shape[1]))
    for t in range(0, n, tile):
        st = s[:, t:t + tile]
        m_new = np.maximum(m, st.max(axis=1))
        f, p = np.exp(m - m_new), np.exp(st - m_new[:, None])
        l = l * f + p.sum(axis=1)
        acc = acc * f[:, None] + p.astype(np.float16).astype(np.float64) @ V[t:t + tile]
        m = m_new
    return acc / l[:, None], m + np.log(l)


def test_the_bound_is_meetable_on_a_sharp_content_by_the_documented_arithmetic():
    """512 positions of E3's first content, G = 8, every head of both layers: emulate_kernel against the plain float64 attention with the
    same E4M3 query, K as the FP8 pool holds it and V as the MXFP4 pool holds it (kv_accuracy.quantize_fp8_e4m3 / quantize_mxfp4), held to
    the project's bound |err| <= (2e-3 + 2 delta) sum p|v| + 1e-6, |lse err| <= 2e-3 + delta, delta = 3e-5 max sum |q||k| sm.
    Measured: worst err / tol 0.071 -- the fp16 weights cost 2^-11 of sum p|v| at most, a quarter of the 2e-3: the GPU file keeps the
    project's bound as it stands on these contents."""
    k, v = cases.case_contents("E3", 2048)[0]
    n, G = 512, 8
    q = np.random.default_rng(8500).standard_normal((2, H, G, D)).astype(np.float16)
    worst = 0.0
    for layer in range(2):
        Kq, Vq = kv_accuracy.quantize_fp8_e4m3(k[layer, :n]), kv_accuracy.quantize_mxfp4(v[layer, :n])
        for head in range(H):
            K, V = Kq[:, head], Vq[:, head]
            out, lse = emulate_kernel(q[layer, head], K, V, SM)
            qe = kv_accuracy.quantize_query_e4m3(q[layer, head])
            s = (qe @ K.T) * SM
            delta = 3e-5 * float((np.abs(qe) @ np.abs(K).T).max()) * SM
            mx = s.max(axis=1)
            p = np.exp(s - mx[:, None])
            tot = p.sum(axis=1)
            want, mag, wlse = (p @ V) / tot[:, None], (p @ np.abs(V)) / tot[:, None], mx + np.log(tot)
            ratio = max(float((np.abs(out - want) / ((2e-3 + 2 * delta) * mag + 1e-6)).max()), float((np.abs(lse - wlse) / (2e-3 + delta)).max()))
            worst = max(worst, ratio)
            assert (np.abs(out - want) > 0).any()                                # the rounding of p is in the emulation
    print(f"the documented arithmetic on a sharp content: worst err / tol {worst:.3f}")
    assert worst <= 1.0
