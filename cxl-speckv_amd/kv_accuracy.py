"""What the pool formats cost in attention accuracy, on data shaped like real KV (VERDICT r5 missing #2; the reference's claims:
docs/ARCHITECTURE.md:246 "Accuracy: 99.5 % preservation", README.md:18 "3-4x compression ratio with minimal accuracy loss" -- it
publishes no measurement and its codec is INT8, so these are figures for OUR pool formats).

N(0,1) blocks flatter every block format.  Real K / V have structure that block scaling reacts to:
  * K: a few channels per head carry values 10-50 x the rest (a bias that survives RoPE in the slow-rotating pairs), RoPE pairs
    (i, i + D/2) rotate with the position, per-channel magnitudes spread log-normally;
  * V: heavy tails (Student t, 4 degrees of freedom) on log-normal channel scales;
  * q: the same outlier channels as K (the model learns them together); softmax either PEAKY (one key takes most of the mass: a
    retrieval head) or FLAT (hundreds of keys share it: an averaging head), or in between (a decode-like query).
The reference result is float64 attention over the ORIGINAL fp16 K / V with the UNQUANTISED fp16 query -- nothing of the pool
format or of the kernel's own query quantisation is in it.  Measured per format: relative L2 error and cosine of the fused
attention's output rows, top-1 agreement of the attention weights (the position with the largest score, from the format's
dequantised K and the exact query), and the error split in two: `format_rel_l2` = float64 attention over the DEQUANTISED K / V
with the exact query against the reference (what 8 or 4 bits of K and V cost, whatever the kernel), `kernel_rel_l2` = the fused
kernel against that same float64 attention over the dequantised values (what the kernel adds: its query quantisation --
e4m3 per row for FP8, MXFP8 blocks for MXFP4, none for INT4_G32 -- f16 weights, fp32 accumulation).

`kv_format_accuracy(kv)` runs it on a CxlSpeckvKVAllocator over the HIP engine: bench.py prints the table (`kv_format_accuracy`),
tests/test_gpu_accuracy.py holds thresholds on it.  numpy float64 is the checker here; no oracle, no reference involved.
"""
import numpy as np

H, D, PAGE, N = 8, 128, 4096, 2048
SCHEMES = {"fp8_e4m3": 4, "int4_g32": 3, "mxfp4": 5}
REGIMES = ("peaky", "decode", "flat")


def synth_kv(T=2048, g=8, seed=7001, outlier_channels=2, outlier_lo=10.0, outlier_hi=50.0):
    """K, V fp16 [T][H][D] and fp16 queries {regime: [H][g][D]} with the structure described in the module text (seeded)."""
    rng = np.random.default_rng(seed)
    half = D // 2
    theta = 10000.0 ** (-np.arange(half) / half)                               # RoPE frequencies of the pairs (i, i + D/2)
    pos = np.arange(T)[:, None]
    ch_scale = np.exp(rng.normal(0.0, 0.5, (H, D)))                            # log-normal channel magnitudes
    bias = np.zeros((H, D))
    out_ch = np.zeros((H, outlier_channels), np.int64)
    for h in range(H):
        # outliers sit in slow pairs (high pair index): the rotation over T positions is a small angle, the bias survives
        pairs = rng.choice(np.arange(half * 3 // 4, half), outlier_channels, replace=False)
        out_ch[h] = pairs + half * rng.integers(0, 2, outlier_channels)
        bias[h, out_ch[h]] = rng.uniform(outlier_lo, outlier_hi, outlier_channels) * rng.choice([-1.0, 1.0], outlier_channels)
    k0 = rng.standard_normal((T, H, D)) * ch_scale + bias                      # content before the rotation
    ang = pos * theta                                                          # [T][half]
    c, s = np.cos(ang)[:, None, :], np.sin(ang)[:, None, :]
    K = np.concatenate([k0[..., :half] * c - k0[..., half:] * s, k0[..., :half] * s + k0[..., half:] * c], axis=-1)
    v_scale = np.exp(rng.normal(0.0, 0.3, (H, D)))
    V = rng.standard_t(4, (T, H, D)) * v_scale
    q = {}
    # decode-like: content with the same outlier channels (at 1-3 x the bulk: with K's 10-50 x that is a common score term of up to
    # 13 nats that moves slowly with the position), rotated to position T
    q0 = rng.standard_normal((H, g, D)) * ch_scale[:, None, :]
    for h in range(H):
        q0[h][:, out_ch[h]] += np.sign(bias[h, out_ch[h]]) * rng.uniform(1.0, 3.0, (g, outlier_channels))
    aT = T * theta
    q["decode"] = np.concatenate([q0[..., :half] * np.cos(aT) - q0[..., half:] * np.sin(aT), q0[..., :half] * np.sin(aT) + q0[..., half:] * np.cos(aT)], axis=-1)
    # peaky: each query row points at one key of its head (minus the head's mean key: the common bias does not pick a position)
    tgt = rng.integers(0, T, (H, g))
    kmean = K.mean(axis=0)
    qp = np.stack([np.stack([K[tgt[h, r], h] - kmean[h] for r in range(g)]) for h in range(H)])
    qp *= (14.0 * np.sqrt(D) / np.maximum((qp * qp).sum(-1, keepdims=True), 1e-9))      # margin of ~14 nats over an average key
    q["peaky"] = qp + rng.standard_normal((H, g, D)) * 0.05
    q["flat"] = rng.standard_normal((H, g, D)) * 0.15
    f16 = lambda a: np.ascontiguousarray(a.astype(np.float16))
    return f16(K), f16(V), {k: f16(v) for k, v in q.items()}, {"targets": tgt, "outlier_channels": out_ch}


def attention_f64(K, V, q, sm_scale):
    """float64 softmax(q.K^T * sm_scale).V per kv head: out [H][g][D], weights' argmax [H][g]"""
    Kd, Vd, qd = K.astype(np.float64), V.astype(np.float64), q.astype(np.float64)
    s = np.einsum("hgd,thd->hgt", qd, Kd) * sm_scale
    top1 = s.argmax(-1)
    p = np.exp(s - s.max(-1, keepdims=True))
    p /= p.sum(-1, keepdims=True)
    return np.einsum("hgt,thd->hgd", p, Vd), top1, p.max(-1)


def pow2_channel_scales(K):
    """Per-(head, channel) power-of-two pre-scale for K: the channel's max|k| relative to the head's median channel, rounded to a
    power of two (exact in fp16 both ways).  K / s is what goes into the pool, q * s is what meets it: q.k is unchanged, and an
    outlier channel no longer sets the block scale for the 15 channels that share its MX block."""
    amax = np.abs(K.astype(np.float32)).max(axis=0)                            # [H][D]
    med = np.median(amax, axis=-1, keepdims=True)
    return np.exp2(np.round(np.log2(np.maximum(amax / np.maximum(med, 1e-9), 1e-9)))).astype(np.float32)


def _rel(a, b):
    return float(np.sqrt(((a.astype(np.float64) - b.astype(np.float64)) ** 2).sum() / (b.astype(np.float64) ** 2).sum()))


def _metrics(got, ref, top1_fmt, top1_ref):
    g64, r64 = got.astype(np.float64), ref.astype(np.float64)
    num = np.sqrt(((g64 - r64) ** 2).sum(-1))
    den = np.sqrt((r64 ** 2).sum(-1))
    cos = (g64 * r64).sum(-1) / np.maximum(np.sqrt((g64 ** 2).sum(-1)) * den, 1e-300)
    return {"rel_l2": float(np.sqrt(((g64 - r64) ** 2).sum() / (r64 ** 2).sum())), "rel_l2_worst_row": float((num / np.maximum(den, 1e-300)).max()),
            "cosine_mean": float(cos.mean()), "cosine_min": float(cos.min()), "top1_agreement": float((top1_fmt == top1_ref).mean())}


def kv_format_accuracy(kv, T=2048, g=8, seed=7001, schemes=None, k_prescale=("mxfp4", "int4_g32")):
    """{format: {regime: metrics}} on the HIP engine behind `kv` (a CxlSpeckvKVAllocator); formats in `k_prescale` are also
    measured with the power-of-two per-channel pre-scale of K folded into the query ("<format>+kscale")."""
    import torch
    lib = kv.lib
    K, V, qs, info = synth_kv(T, g, seed)
    sm = 1.0 / np.sqrt(D)
    ref = {r: attention_f64(K, V, qs[r], sm) for r in REGIMES}
    n_pages = 2 * T * H * D * 2 // PAGE
    out = {"_data": {"T": T, "g": g, "seed": seed, "outlier_channels_per_head": int(info["outlier_channels"].shape[1]),
                     "reference": "float64 attention over the original fp16 K / V, unquantised fp16 query",
                     "softmax_top_weight_mean": {r: round(float(ref[r][2].mean()), 4) for r in REGIMES}}}
    scale = pow2_channel_scales(K)
    variants = []
    for name, scheme in (schemes or SCHEMES).items():
        variants.append((name, scheme, None))
        if name in k_prescale: variants.append((name + "+kscale", scheme, scale))
    st = torch.cuda.current_stream().cuda_stream
    for name, scheme, ks in variants:
        lib.set_compression_scheme(scheme)
        h = kv.allocate(T, 1, H, D, 2)
        Kw = K if ks is None else (K.astype(np.float32) / ks[None]).astype(np.float16)       # (a power of two: exact)
        buf = np.concatenate([Kw.reshape(-1), V.reshape(-1)])
        lib.write(h, 0, buf.ctypes.data, buf.nbytes, False)
        deq = torch.empty((n_pages, N), dtype=torch.float16, device="cuda")
        lib.fetch_range(h, 0, n_pages, deq.data_ptr(), False, st)
        torch.cuda.synchronize()
        flat = deq.cpu().numpy().reshape(-1)
        Kq, Vq = flat[:T * H * D].reshape(T, H, D), flat[T * H * D:].reshape(T, H, D)
        res = {}
        for r in REGIMES:
            qv = qs[r] if ks is None else (qs[r].astype(np.float32) * ks[:, None, :]).astype(np.float16)
            dq = torch.from_numpy(qv.view(np.int16)).cuda()
            o = torch.full((H, g, D), float("nan"), dtype=torch.float32, device="cuda")
            lse = torch.empty((H, g), dtype=torch.float32, device="cuda")
            {4: lib.attend_fp8, 3: lib.attend_int4, 5: lib.attend_mx4}[scheme](h, 0, 1, dq.data_ptr(), g, 0, T, sm, o.data_ptr(), lse.data_ptr(), st)
            torch.cuda.synchronize()
            of, top1_fmt, _ = attention_f64(Kq, Vq, qv, sm)              # the format alone: exact arithmetic over the dequantised values
            m = _metrics(o.cpu().numpy(), ref[r][0], top1_fmt, ref[r][1])
            m["format_rel_l2"] = _rel(of, ref[r][0])
            m["kernel_rel_l2"] = _rel(o.cpu().numpy(), of)
            res[r] = {k: round(v, 5) for k, v in m.items()}
        out[name] = res
        lib.free(h)
    return out


def format_table(acc):
    """markdown rows of kv_format_accuracy's result"""
    rows = ["| format | regime | rel. L2 error (format alone + kernel) | worst row | cosine (mean / min) | top-1 agreement |", "|---|---|---|---|---|---|"]
    for name, res in acc.items():
        if name.startswith("_"): continue
        for r in REGIMES:
            m = res[r]
            rows.append(f"| {name} | {r} | {m['rel_l2']:.4f} ({m['format_rel_l2']:.4f} + {m['kernel_rel_l2']:.4f}) | {m['rel_l2_worst_row']:.4f} | {m['cosine_mean']:.5f} / {m['cosine_min']:.5f} | {m['top1_agreement']:.3f} |")
    return "\n".join(rows)


# ------------------------------------------------------------------------------------------------------------------------------
# The pool formats restated in numpy, and the split pool ("K8V4": FP8 keys, MXFP4 values).  No GPU in the first half: the formats'
# own cost on the data above, for any pair of K and V formats (DESIGN section 4's table of the routes to a denser pool).
# ------------------------------------------------------------------------------------------------------------------------------
def _pages(x):
    """[T][H][D] fp16 (T even, H * D = 1024) -> the pool's blocks in page order, fp32 [T / 2][2048]: a page is two positions"""
    x = np.asarray(x)
    if x.ndim != 3 or x.shape[0] % 2 or x.shape[1] * x.shape[2] != N // 2:
        raise ValueError("a tensor of [T][H][D] with T even and H * D = 1024: whole pages of two positions")
    return np.ascontiguousarray(x.astype(np.float16)).astype(np.float32).reshape(-1, N)


def _held(y32, shape):
    """what fetch_range gives for fp32 decoded values: rounded once to fp16; as float64 in the tensor's shape"""
    with np.errstate(over="ignore"):
        return y32.astype(np.float16).astype(np.float64).reshape(shape)


def quantize_fp8_e4m3(x):
    """The values an FP8_E4M3 pool holds for x ([T][H][D] fp16), float64: per page scale = max|x| / 448 (1 for a page of zeros),
    x / scale rounded to nearest-even E4M3 (saturating at 448), times the scale in fp32, rounded to fp16 as fetch_range does."""
    b = _pages(x)
    mx = np.abs(b).max(axis=1, keepdims=True)
    s = np.where(mx > 0, mx / np.float32(448.0), np.float32(1.0)).astype(np.float32)
    v = np.clip((b / s).astype(np.float32), -448.0, 448.0)
    _, ex = np.frexp(np.abs(v))                                                  # |v| = m 2^ex, m in [0.5, 1): floor(log2) = ex - 1
    quantum = np.exp2(np.maximum(ex - 1, -6) - 3.0)                              # three mantissa bits; subnormals below 2^-6: 2^-9
    e4m3 = (np.rint(v.astype(np.float64) / quantum) * quantum).astype(np.float32)    # (exact: a power of two; rint is ties-to-even, -0 stays -0)
    return _held(e4m3 * s, np.shape(x))


def quantize_query_e4m3(q):
    """The query rows the FP8-score kernels multiply (k_attend_fp8_linear, k_attend_k8v4), float64 in q's shape: per row ([..., D] fp16)
    scale = max|q| / 448 in fp32 (1 for a row of zeros), q / scale in fp32 rounded to nearest-even E4M3 (saturating at 448) as
    quantize_fp8_e4m3 rounds, times the scale -- NOT rounded to fp16: the row scale multiplies the score in fp32."""
    x = np.asarray(q).astype(np.float16).astype(np.float32)
    mx = np.abs(x).max(axis=-1, keepdims=True)
    s = np.where(mx > 0, mx / np.float32(448.0), np.float32(1.0)).astype(np.float32)
    v = np.clip((x / s).astype(np.float32), -448.0, 448.0)
    _, ex = np.frexp(np.abs(v))
    quantum = np.exp2(np.maximum(ex - 1, -6) - 3.0)
    e4m3 = np.rint(v.astype(np.float64) / quantum) * quantum
    return e4m3 * s.astype(np.float64)


def mxfp4_codes(x):
    """The E8M0 codes an MXFP4 pool holds for x ([T][H][D] fp16), int64 [T / 2][H * D / 16]: one per page and block of 16 channels (of
    BOTH positions of the page), floor(log2 max|x|) - 2 + 127 clipped to 0 .. 254, 0 for a block of zeros."""
    b = _pages(x).astype(np.float64).reshape(-1, 2, N // 32, 16)                 # [page][position][group][16 channels]
    amax = np.abs(b).max(axis=(1, 3))
    _, ex = np.frexp(amax)
    return np.where(amax > 0, np.clip(ex - 1 - 2 + 127, 0, 254), 0).astype(np.int64)


def quantize_mxfp4(x):
    """The values an MXFP4 pool holds for x, float64: an MX block is 16 channels of BOTH positions of a page, its E8M0 scale
    2^(floor(log2 max|x|) - 2) (mxfp4_codes), the elements E2M1 (0, .5, 1, 1.5, 2, 3, 4, 6; ties to the even code, saturating at 6)."""
    b = _pages(x).astype(np.float64).reshape(-1, 2, N // 32, 16)                 # [page][position][group][16 channels]
    code = mxfp4_codes(x)[:, None, :, None]
    a = np.abs(np.ldexp(b, 127 - code))
    idx = sum((a > m).astype(np.int64) for m in (0.25, 1.25, 2.5, 5.0)) + sum((a >= m).astype(np.int64) for m in (0.75, 1.75, 3.5))
    mag = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])[idx]
    y = np.copysign(np.ldexp(mag, code - 127), b)
    return _held(y.astype(np.float32), np.shape(x))


def quantize_int4_g32(x):
    """The values an INT4_G32 pool holds for x, float64: groups of 32 consecutive channels of one position, scale = fp16(max|x| / 7),
    elements round(x / scale) (halves away from zero) in -7 .. 7."""
    b = _pages(x).reshape(-1, 32)
    s = (np.abs(b).max(axis=1, keepdims=True) / np.float32(7.0)).astype(np.float16).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (b / s).astype(np.float32).astype(np.float64)
    r = np.where(s != 0, np.clip(np.copysign(np.floor(np.abs(r) + 0.5), r), -7.0, 7.0), 0.0)
    return _held((r + 0.0).astype(np.float32) * s, np.shape(x))                 # (an integer has no sign of zero: -0 + 0 = +0)


def quantize_mxfp4_tile_mean(x):
    """A route that was weighed and NOT built (route a): MXFP4 of x minus an fp16 offset per (32-position tile,
    channel) -- the tile's mean -- with the offset added back.  T a multiple of 32."""
    x32 = np.asarray(x).astype(np.float32)
    tiles = x32.reshape(-1, 32, *x32.shape[1:])
    mean = tiles.mean(axis=1, keepdims=True).astype(np.float16).astype(np.float32)
    rest = (tiles - mean).astype(np.float16).reshape(x32.shape)
    return (quantize_mxfp4(rest).reshape(tiles.shape) + mean.astype(np.float64)).reshape(x32.shape)


def quantize_mxfp4_top4_fp8(x):
    """A route that was weighed and NOT built (route b): per head the 4 channels of the largest max|x| kept in an FP8_E4M3 side plane
    (here: their values out of the FP8 pool's blocks), the other channels MXFP4 with those four zeroed, so that they set no block scale."""
    x16 = np.asarray(x).astype(np.float16)
    top = np.argsort(np.abs(x16.astype(np.float32)).max(axis=0), axis=-1)[:, -4:]                     # [H][4]
    side = np.zeros(x16.shape[1:], bool)
    np.put_along_axis(side, top, True, axis=-1)
    return np.where(side[None], quantize_fp8_e4m3(x16), quantize_mxfp4(np.where(side[None], np.float16(0), x16)))


QUANTIZERS = {"fp8_e4m3": quantize_fp8_e4m3, "mxfp4": quantize_mxfp4, "int4_g32": quantize_int4_g32, "exact": lambda x: np.asarray(x, np.float64),
              "mxfp4_tile_mean": quantize_mxfp4_tile_mean, "mxfp4_top4_fp8": quantize_mxfp4_top4_fp8}


def format_accuracy_cpu(k_format, v_format, T=2048, g=8, seed=7001, query="fp16"):
    """{regime: rel. L2 error} of float64 attention over K as `k_format` and V as `v_format` hold them (names of QUANTIZERS) with the
    exact fp16 query, against float64 attention over the original rows: the "format alone" column of kv_format_accuracy for any pair
    of formats, without a GPU.  query="e4m3": the formats' side takes the query as the FP8-score decode kernels restate it
    (quantize_query_e4m3) -- what a route through those kernels costs, the query's share included; the reference keeps the fp16 query."""
    if query not in ("fp16", "e4m3"):
        raise ValueError('query: "fp16" or "e4m3"')
    K, V, qs, _ = synth_kv(T, g, seed)
    Kq, Vq = QUANTIZERS[k_format](K), QUANTIZERS[v_format](V)
    sm = 1.0 / np.sqrt(D)
    seen = (lambda q: q) if query == "fp16" else quantize_query_e4m3
    return {r: _rel(attention_f64(Kq, Vq, seen(qs[r]), sm)[0], attention_f64(K, V, qs[r], sm)[0]) for r in REGIMES}


def kv_split_accuracy(lib, T=2048, g=8, seed=7001):
    """kv_format_accuracy's figures for the split pool on the HIP engine behind `lib` (a SpeckvLib): the data goes through
    SpeckvSplitKVConnector -- T - 2 positions as a prompt, the last two as a chunk whose last row carries the regime's queries, so the
    call walks pool tiles and a held tile -- and {regime: metrics} comes back, with format_rel_l2 (float64 over the numpy restatement
    of what the two allocations hold; the two held rows are exact) and kernel_rel_l2 (the launch against that) per regime."""
    import torch
    from .kv_split_connector import SpeckvSplitKVConnector
    K, V, qs, _ = synth_kv(T, g, seed)
    sm = 1.0 / np.sqrt(D)
    Kq, Vq = quantize_fp8_e4m3(K[:T - 2]), quantize_mxfp4(V[:T - 2])
    Kq, Vq = np.concatenate([Kq, K[T - 2:].astype(np.float64)]), np.concatenate([Vq, V[T - 2:].astype(np.float64)])
    conn = SpeckvSplitKVConnector(lib, 2, H, D, (T + 31) // 32 * 32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    two = lambda a: np.stack([a, a])                                            # the same rows in both layers
    conn.add_request(0)
    res = {}
    try:
        keep = conn.write_prefill(0, dev(two(K[:T - 2])), dev(two(V[:T - 2])))
        k_new, v_new = dev(two(K[T - 2:]).transpose(1, 0, 2, 3)[None]), dev(two(V[T - 2:]).transpose(1, 0, 2, 3)[None])    # [1][2][L][H][D]
        for r in REGIMES:
            q = np.zeros((1, 2, H, g, D), np.float16)
            q[0, 1] = qs[r]
            o = conn.attend_chunk(1, [0], dev(q), k_new, v_new, sm)
            torch.cuda.synchronize()
            got = o.cpu().numpy()[0, 1]
            ref, top1_ref, _ = attention_f64(K, V, qs[r], sm)
            of, top1_fmt, _ = attention_f64(Kq, Vq, qs[r], sm)
            m = _metrics(got, ref, top1_fmt, top1_ref)
            m["format_rel_l2"] = _rel(of, ref)
            m["kernel_rel_l2"] = _rel(got, of)
            res[r] = {k: round(v, 5) for k, v in m.items()}
        del keep
    finally:
        conn.free_request(0)
    return res


def kv_split_decode_accuracy(lib, T=2048, g=8, seed=7001):
    """kv_split_accuracy's figures for the split pool's DECODE route on the HIP engine behind `lib`: all T positions (even) go in as a
    prompt through SpeckvSplitKVConnector and are attended through conn.attend -- speckv_ext_attend_kv_batch, the batch kernel over FP8
    keys and MXFP4 values.  {regime: metrics}: rel_l2 and its kin against float64 over the original rows with the fp16 query;
    format_rel_l2 = float64 over the numpy restatement of what the two allocations hold, with the fp16 query; kernel_rel_l2 = the launch
    against float64 over those values with the query as the kernel restates it (quantize_query_e4m3), so the query's share is in rel_l2
    and not in kernel_rel_l2."""
    import torch
    from .kv_split_connector import SpeckvSplitKVConnector
    if T % 2:
        raise ValueError("T even: every position is stored")
    K, V, qs, _ = synth_kv(T, g, seed)
    sm = 1.0 / np.sqrt(D)
    Kq, Vq = quantize_fp8_e4m3(K), quantize_mxfp4(V)
    conn = SpeckvSplitKVConnector(lib, 2, H, D, (T + 31) // 32 * 32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    two = lambda a: np.stack([a, a])                                            # the same rows in both layers
    conn.add_request(0)
    res = {}
    try:
        keep = conn.write_prefill(0, dev(two(K)), dev(two(V)))
        for r in REGIMES:
            o = conn.attend(1, [0], dev(qs[r][None]), sm)
            torch.cuda.synchronize()
            got = o.cpu().numpy()[0]
            ref, top1_ref, _ = attention_f64(K, V, qs[r], sm)
            of, top1_fmt, _ = attention_f64(Kq, Vq, qs[r], sm)
            oq = attention_f64(Kq, Vq, quantize_query_e4m3(qs[r]), sm)[0]
            m = _metrics(got, ref, top1_fmt, top1_ref)
            m["format_rel_l2"] = _rel(of, ref)
            m["kernel_rel_l2"] = _rel(got, oq)
            res[r] = {k: round(v, 5) for k, v in m.items()}
        del keep
    finally:
        conn.free_request(0)
    return res
