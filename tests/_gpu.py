"""Helpers for the -m gpu tests: drive libcxlspeckv.so through its C ABI with
torch tensors as plain device buffers (torch is plumbing only)."""
import contextlib
import ctypes as C
import gc

import numpy as np

import cxl_speckv_amd as pkg
from cxl_speckv_amd.speckv_ctypes import bind_ext

N = 2048
H, D = 8, 128                              # the page layout of the attention entries: 8 kv heads x 128, two positions a page


def load_raw_lib():
    """The library without speckv_init: raw codec / verify operators only."""
    lib = pkg.load_library()
    bind_ext(lib)
    return lib


def load_debug_lib():
    """tests/_build/libspeckv_debug.so: TEST-ONLY self-check kernels over the product's device helpers
    (tests/csrc/debug_kernels.hip); built on demand, never part of libcxlspeckv.so."""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.check_call(["make", "-s", "-C", os.path.join(root, "tests", "csrc")])
    pkg.load_library()                      # one HIP runtime in the process (torch's), mapped first
    return C.CDLL(os.path.join(root, "tests", "_build", "libspeckv_debug.so"))


_TUNE_WORDS = {"wg": 1, "serial": 2, "kernel": 1, "copy": 2}


def set_tuning(key, value):
    """speckv_ext_set_tuning: the library reads its environment once; tests that flip a launch form between two calls say so
    through the C ABI (include/speckv_ext.h).  Words of the old environment values ("wg", "serial", ...) are accepted."""
    lib = pkg.load_library()
    lib.speckv_ext_set_tuning.argtypes = [C.c_char_p, C.c_longlong]
    lib.speckv_ext_set_tuning.restype = C.c_int
    rc = lib.speckv_ext_set_tuning(key.encode(), int(_TUNE_WORDS.get(value, value)))
    assert rc == 0, (key, value, rc)


def torch_mod():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@contextlib.contextmanager
def graph_capture(graph, stream):
    """torch.cuda.graph with the cyclic garbage collector held off: a collection that runs inside the capture may
    destroy a graph or stream left in a reference cycle by an EARLIER test (pytest.raises keeps frames alive), and HIP
    calls of that kind abort a global-mode capture."""
    torch = torch_mod()
    gc.collect()
    was_enabled = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph, stream=stream):
            yield
    finally:
        if was_enabled:
            gc.enable()


def stream_ptr():
    torch = torch_mod()
    return torch.cuda.current_stream().cuda_stream


def gpu_compress(lib, x16, scheme, mode, rec_stride=4096):
    """x16: (B, 2048) float16 numpy.  Returns scales f32[B], lens u32[B], recs u8[B, stride]."""
    torch = torch_mod()
    x16 = np.ascontiguousarray(x16, dtype=np.float16).reshape(-1, N)
    B = x16.shape[0]
    d_x = torch.from_numpy(x16.view(np.int16)).cuda()
    d_recs = torch.full((B, rec_stride), 0xA5, dtype=torch.uint8, device="cuda")
    d_len = torch.zeros(B, dtype=torch.int32, device="cuda")
    d_scale = torch.zeros(B, dtype=torch.float32, device="cuda")
    rc = lib.speckv_ext_codec_compress(d_x.data_ptr(), B, d_recs.data_ptr(), rec_stride, d_len.data_ptr(),
                                       d_scale.data_ptr(), scheme, mode, stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return (d_scale.cpu().numpy(), d_len.cpu().numpy().view(np.uint32), d_recs.cpu().numpy())


def gpu_decompress(lib, recs, lens, scales, scheme, mode, out_f32=False):
    torch = torch_mod()
    recs = np.ascontiguousarray(recs, dtype=np.uint8)
    B, stride = recs.shape
    d_recs = torch.from_numpy(recs).cuda()
    d_len = torch.from_numpy(np.ascontiguousarray(lens, dtype=np.uint32).view(np.int32)).cuda()
    d_scale = torch.from_numpy(np.ascontiguousarray(scales, dtype=np.float32)).cuda()
    if out_f32:
        d_y = torch.full((B, N), float("nan"), dtype=torch.float32, device="cuda")
    else:
        d_y = torch.full((B, N), 0x7E00, dtype=torch.int16, device="cuda")
    rc = lib.speckv_ext_codec_decompress(d_recs.data_ptr(), stride, d_len.data_ptr(), d_scale.data_ptr(), B,
                                         d_y.data_ptr(), int(out_f32), scheme, mode, stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    y = d_y.cpu().numpy()
    return y if out_f32 else y.view(np.float16)


def assert_same_float_bits(a, b, what=""):
    """Bit-exact except that NaNs only have to be NaNs on both sides."""
    a = np.asarray(a); b = np.asarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), f"{what}: NaN positions differ"
    ua = a.view(np.uint16 if a.dtype == np.float16 else np.uint32)
    ub = b.view(np.uint16 if b.dtype == np.float16 else np.uint32)
    bad = (ua != ub) & ~na
    assert not bad.any(), f"{what}: {int(bad.sum())} elements differ, first at {np.argwhere(bad)[0]}"


def _hip_runtime():
    """The one HIP runtime already mapped in this process (torch's bundled copy)."""
    import os
    torch = torch_mod()
    path = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    rt = C.CDLL(path if os.path.exists(path) else "libamdhip64.so")
    rt.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    rt.hipMemcpy.restype = C.c_int
    return rt


def dev_to_host(ptr, nbytes):
    """Copy nbytes from a raw device address (as returned by speckv_access)."""
    torch_mod().cuda.synchronize()
    buf = np.empty(nbytes, np.uint8)
    rc = _hip_runtime().hipMemcpy(buf.ctypes.data, C.c_void_p(ptr), nbytes, 2)   # hipMemcpyDeviceToHost
    assert rc == 0, rc
    return buf


def stored_record(info, nbytes):
    """The first nbytes of a page's pool record as speckv_ext_translate describes it: contiguous at pool_addr, or -- tile-planar
    MXFP4, aux_offset != 0 -- bytes 0..1023 there and the 64 codes aux_offset further on (include/speckv_ext.h)."""
    nbytes = int(nbytes)
    if not info.aux_offset or nbytes <= 1024:
        return dev_to_host(info.pool_addr, nbytes)
    return np.concatenate([dev_to_host(info.pool_addr, 1024), dev_to_host(info.pool_addr + info.aux_offset, nbytes - 1024)])


class HeadChecker:
    """The oracle's attention of one kv head over the K / V regions of one layer, from the HOST copy of that layer's
    pages (region = T/2 pages of K followed by T/2 pages of V), through the oracle's own compress -> records."""

    def __init__(self, oracle, scheme, region_pages16, T):
        self.oracle, self.scheme, self.T = oracle, scheme, T
        self.scales, self.lens, self.recs = oracle.compress_blocks_f16(region_pages16, scheme, 0)
        self._kv = {}
        if scheme == 3:
            self.dec = oracle.decompress_blocks_f16(self.recs, self.lens, self.scales, 3, 0).reshape(-1, 2, H, D)
        elif scheme == 5:
            self.lut = np.array([oracle.lib.orc_e4m3_to_f32(b) for b in range(256)], np.float64)
            self.lut[np.isnan(self.lut)] = 0.0
        else:
            self.lut = np.array([oracle.lib.orc_e4m3_to_f32(b) for b in range(256)], np.float32)
            self.lut[np.isnan(self.lut)] = 0.0

    def want(self, q_head, head, npos, sm):
        """q_head [G][D] fp16 -> out [G][D], lse [G], mag [G][D], delta (FP8: score error bound of the fp8 MFMA)."""
        from oracle.bindings import _ptr, u8p, u16p, f32p
        L = self.oracle.lib
        G = len(q_head)
        hp = self.T // 2                                               # pages per K / V region
        o = np.zeros((G, D), np.float32); l = np.zeros(G, np.float32); m = np.zeros((G, D), np.float32)
        if npos == 0:
            return o, np.full(G, -np.inf, np.float32), m, 0.0
        if self.scheme == 3:
            k16 = np.ascontiguousarray(self.dec[:hp, :, head, :].reshape(-1, D)[:npos]).view(np.uint16)
            v16 = np.ascontiguousarray(self.dec[hp:2 * hp, :, head, :].reshape(-1, D)[:npos]).view(np.uint16)
            L.orc_attend_f16(_ptr(np.ascontiguousarray(q_head).view(np.uint16).reshape(-1), u16p), G, _ptr(k16.reshape(-1), u16p),
                             _ptr(v16.reshape(-1), u16p), npos, D, float(sm), _ptr(o, f32p), _ptr(l, f32p), _ptr(m, f32p))
            return o, l, m, 0.0
        if self.scheme == 5:                                         # MXFP4: page rows of one head + their codes (tests/test_gpu_mx4.py)
            from tests.test_gpu_mx4 import head_rows, dequant_rows
            kr, kc = head_rows(self.recs, 0, npos, head)
            vr, vc = head_rows(self.recs, hp, npos, head)
            q8 = np.zeros((G, D), np.uint8); qc = np.zeros((G, D // 16), np.uint8)
            L.orc_quantize_rows_mxfp8(_ptr(np.ascontiguousarray(q_head).view(np.uint16).reshape(-1), u16p), G, D, 16, _ptr(q8, u8p), _ptr(qc, u8p))
            qd = self.lut[q8] * np.repeat(np.exp2(qc.astype(np.float64) - 127.0), 16, axis=1)
            delta = 3e-5 * float((np.abs(qd) @ np.abs(dequant_rows(kr, kc, npos)).T).max()) * sm
            L.orc_attend_mx4(_ptr(q8, u8p), _ptr(qc, u8p), 16, G, _ptr(kr, u8p), _ptr(kc, u8p), _ptr(vr, u8p), _ptr(vc, u8p), npos, D,
                             float(sm), _ptr(o, f32p), _ptr(l, f32p), _ptr(m, f32p))
            return o, l, m, delta
        r4 = self.recs[:, :N].reshape(-1, 2, H, D)
        krows = np.ascontiguousarray(r4[:hp, :, head, :].reshape(-1, D)[:npos])
        vrows = np.ascontiguousarray(r4[hp:2 * hp, :, head, :].reshape(-1, D)[:npos])
        ksc = np.ascontiguousarray(np.repeat(self.scales[:hp], 2)[:npos]); vsc = np.ascontiguousarray(np.repeat(self.scales[hp:2 * hp], 2)[:npos])
        q8 = np.zeros((G, D), np.uint8); qs = np.zeros(G, np.float32)
        L.orc_quantize_rows_e4m3(_ptr(np.ascontiguousarray(q_head).view(np.uint16).reshape(-1), u16p), G, D, _ptr(q8, u8p), _ptr(qs, f32p))
        smag = (np.abs(self.lut[q8]) @ np.abs(self.lut[krows]).T) * ksc[None, :] * qs[:, None] * sm
        delta = 3e-5 * float(smag.max())
        L.orc_attend_fp8(_ptr(q8, u8p), _ptr(qs, f32p), G, _ptr(krows, u8p), _ptr(ksc, f32p), _ptr(vrows, u8p), _ptr(vsc, f32p),
                         npos, D, float(sm), _ptr(o, f32p), _ptr(l, f32p), _ptr(m, f32p))
        return o, l, m, delta

    def check(self, got, got_lse, q_head, head, npos, sm, what):
        want, wlse, mag, delta = self.want(q_head, head, npos, sm)
        err = np.abs(np.asarray(got, np.float32) - want)
        tol = (2e-3 + 2 * delta) * mag + 1e-6
        assert np.all(err <= tol), (what, float((err / (mag + 1e-9)).max()), delta)
        if got_lse is not None and npos:
            assert np.all(np.abs(np.asarray(got_lse, np.float32) - wlse) <= 2e-3 + delta), (what, float(np.abs(got_lse - wlse).max()))

    # ---- the same float64 attention for many query rows at once (every member of a batch that shares this region's content), in numpy:
    # the region's K / V rows of a head dequantised once, the query quantised as the kernel takes it (tests/test_host_units.py pins these
    # rows to want() above, which calls the oracle's own attention)
    def kv(self, head):
        """float64 K and V rows [T][D] of kv head `head` over the whole region, as the records hold them"""
        if head not in self._kv:
            hp = self.T // 2
            if self.scheme == 3:
                k = self.dec[:hp, :, head, :].reshape(-1, D); v = self.dec[hp:2 * hp, :, head, :].reshape(-1, D)
            elif self.scheme == 5:
                from tests.test_gpu_mx4 import head_rows, dequant_rows
                k = dequant_rows(*head_rows(self.recs, 0, self.T, head), self.T); v = dequant_rows(*head_rows(self.recs, hp, self.T, head), self.T)
            else:
                r4 = self.recs[:, :N].reshape(-1, 2, H, D)
                lut = self.lut.astype(np.float64)
                k = lut[r4[:hp, :, head, :].reshape(-1, D)] * np.repeat(self.scales[:hp].astype(np.float64), 2)[:, None]
                v = lut[r4[hp:2 * hp, :, head, :].reshape(-1, D)] * np.repeat(self.scales[hp:2 * hp].astype(np.float64), 2)[:, None]
            self._kv[head] = (np.asarray(k, np.float64), np.asarray(v, np.float64))
        return self._kv[head]

    def q_rows(self, q16):
        """float64 query rows [R][D] as the format's kernel multiplies them: fp16 (INT4_G32), E4M3 x a row scale (FP8), MXFP8 (MXFP4)"""
        from oracle.bindings import _ptr, u8p, u16p, f32p
        q16 = np.ascontiguousarray(q16, np.float16).reshape(-1, D)
        R = len(q16)
        if self.scheme == 3:
            return q16.astype(np.float64)
        lut = self.lut.astype(np.float64)
        q8 = np.zeros((R, D), np.uint8)
        if self.scheme == 5:
            qc = np.zeros((R, D // 16), np.uint8)
            self.oracle.lib.orc_quantize_rows_mxfp8(_ptr(q16.view(np.uint16).reshape(-1), u16p), R, D, 16, _ptr(q8, u8p), _ptr(qc, u8p))
            return lut[q8] * np.repeat(np.exp2(qc.astype(np.float64) - 127.0), 16, axis=1)
        qs = np.zeros(R, np.float32)
        self.oracle.lib.orc_quantize_rows_e4m3(_ptr(q16.view(np.uint16).reshape(-1), u16p), R, D, _ptr(q8, u8p), _ptr(qs, f32p))
        return lut[q8] * qs.astype(np.float64)[:, None]

    def want_rows(self, q16, head, npos, sm, tail=None, pos_begin=0):
        """q16 [M][G][D] fp16 of M members over this content, npos [M] -> out [M][G][D], lse [M][G], mag [M][G][D] (sum p|v|), delta [M]
        (as want(): the score error bound of the 8-bit formats, per member and head).  tail = (k [M][D], v [M][D]) fp16: one more
        position per member, outside the pool (the kernel takes its score from the fp16 query).  pos_begin: the members attend positions
        [pos_begin, pos_begin + npos) of the region instead of its first npos."""
        q16 = np.asarray(q16, np.float16)
        M, G = q16.shape[:2]
        npos = np.asarray(npos, np.int64)
        K, V = self.kv(head)
        K, V = K[pos_begin:], V[pos_begin:]
        qe = self.q_rows(q16).reshape(M, G, D)
        out = np.zeros((M, G, D)); mag = np.zeros((M, G, D)); lse = np.full((M, G), -np.inf); delta = np.zeros(M)
        for n in np.unique(npos):
            idx = np.nonzero(npos == n)[0]
            m = len(idx)
            s = (qe[idx].reshape(-1, D) @ K[:n].T) * sm                                  # [m G][n]
            if self.scheme != 3 and n:
                delta[idx] = 3e-5 * ((np.abs(qe[idx].reshape(-1, D)) @ np.abs(K[:n]).T).reshape(m, -1).max(axis=1)) * sm
            st = np.full(m * G, -np.inf)
            if tail is not None:
                st = np.einsum("mgd,md->mg", q16[idx].astype(np.float64), np.asarray(tail[0], np.float16)[idx].astype(np.float64)).reshape(-1) * sm
            if n == 0 and tail is None:
                continue
            mx = np.maximum(s.max(axis=1) if n else -np.inf, st)
            p = np.exp(s - mx[:, None]); pt = np.exp(st - mx)
            l = p.sum(axis=1) + pt
            o = p @ V[:n]; a = p @ np.abs(V[:n])
            if tail is not None:
                vt = np.repeat(np.asarray(tail[1], np.float16)[idx].astype(np.float64), G, axis=0)
                o += pt[:, None] * vt; a += pt[:, None] * np.abs(vt)
            out[idx] = (o / l[:, None]).reshape(m, G, D); mag[idx] = (a / l[:, None]).reshape(m, G, D)
            lse[idx] = (mx + np.log(l)).reshape(m, G)
        return out, lse, mag, delta

    def weight_rows(self, q16, head, n, sm, pos_begin=0, v_from=None):
        """What a model of the kernels' weight rounding needs (tests/_value_ranges.py), from the dequantisation want_rows uses: q16 [R][D] fp16 over
        the positions [pos_begin, pos_begin + n) -> (p [R][n]: the float64 weights exp(s - max s) against the row's final maximum, l [R] their sums,
        mx [R] the maxima (natural log domain), V [n][D] float64, vs [n]: the V page scale of every position -- FP8 only, ones elsewhere).
        v_from: the checker whose V rows (and V format) are attended instead of this one's -- the split pool, K here and V there."""
        K = self.kv(head)[0][pos_begin:pos_begin + n]
        vc = self if v_from is None else v_from
        V = vc.kv(head)[1][pos_begin:pos_begin + n]
        s = (self.q_rows(q16) @ K.T) * sm
        mx = s.max(axis=1)
        p = np.exp(s - mx[:, None])
        hp = vc.T // 2
        fp8_v = getattr(vc, "v_scheme", vc.scheme) == 4
        vs = np.repeat(vc.scales[hp:2 * hp].astype(np.float64), 2)[pos_begin:pos_begin + n] if fp8_v else np.ones(n)
        return p, p.sum(axis=1), mx, V, vs

    def check_rows(self, got, got_lse, q16, head, npos, sm, what, tail=None, pos_begin=0, worst=None, extra_tol=None):
        """every row of M members' head `head` against want_rows, with check()'s bound: |err| <= (2e-3 + 2 delta) sum p|v| + 1e-6,
        |lse err| <= 2e-3 + delta; a member with no position (and no tail) exactly 0.  got_lse None: a call without a log-sum-exp, out only.
        worst: a list that receives the largest err / tol of out and of lse (0.0 where nothing was compared) BEFORE anything is asserted.
        extra_tol [M][G][D]: added to the bound of out (None: nothing) -- what a declared rounding of the format costs, worked out by the caller."""
        want, wlse, mag, delta = self.want_rows(q16, head, npos, sm, tail, pos_begin)
        got = np.asarray(got, np.float64)
        npos = np.asarray(npos)
        empty = (npos == 0) if tail is None else np.zeros(len(npos), bool)
        assert np.all(got[empty] == 0.0), (what, "empty member not 0", np.nonzero(empty)[0].tolist())
        live = ~empty
        err = np.abs(got[live] - want[live])
        tol = (2e-3 + 2 * delta[live])[:, None, None] * mag[live] + 1e-6
        if extra_tol is not None:
            tol = tol + np.asarray(extra_tol, np.float64)[live]
        if worst is not None:
            lerr = np.abs(np.asarray(got_lse, np.float64)[live] - wlse[live]) / (2e-3 + delta[live])[:, None] if got_lse is not None else np.zeros(0)
            with np.errstate(invalid="ignore"):
                worst.append(max(float(np.nan_to_num(err / tol, nan=np.inf).max(initial=0.0)), float(np.nan_to_num(lerr, nan=np.inf).max(initial=0.0))))
        bad = ~(err <= tol)
        assert not bad.any(), (what, "out", [int(i) for i in np.nonzero(live)[0][np.argwhere(bad)[0][:1]]], int(bad.sum()),
                               float((err / (mag[live] + 1e-9)).max()))
        if got_lse is None:
            return
        got_lse = np.asarray(got_lse, np.float64)
        lerr = np.abs(got_lse[live] - wlse[live])
        lbad = ~(lerr <= (2e-3 + delta[live])[:, None])
        assert not lbad.any(), (what, "lse", [int(i) for i in np.nonzero(live)[0][np.argwhere(lbad)[0][:1]]], float(np.nanmax(lerr)))

