"""-m gpu: the one-launch commit of a multi-position step.  speckv_ext_write_pairs (the encoder gathers a page's two rows itself)
against speckv_ext_write_strided_batch from torch-built page images of the same rows, and SpeckvKVConnector.commit against
append_tokens / append_path: records, scales, decoded pages, lengths, tails and a following attention agree bit for bit."""
import numpy as np
import pytest

import cxl_speckv_amd as pkg
from cxl_speckv_amd.kv_connector import SpeckvKVConnector
from cxl_speckv_amd.speckv_ctypes import SpeckvError
from tests._gpu import N, torch_mod

pytestmark = pytest.mark.gpu
PAGE = 4096
H, D = 8, 128
ERR_GENERAL, ERR_INVAL = -1, -4


def open_lib():
    return pkg.SpeckvLib(pkg.library_path(), "hip:0")


@pytest.mark.parametrize("scheme", [2, 3, 4, 5])
def test_write_pairs_equals_write_strided_batch(scheme):
    """Four allocations written by ONE write_pairs call, their twins by write_strided_batch from contiguous images of the same rows.
    The rows lie in a padded [B][S][L][H][D] step tensor (layer stride 2304 bytes) at scattered (b, s) and in a tail tensor; the pairs
    cover two pairs of one allocation on region pages 15 and 16 (across the MXFP4 tile), halves from different tensors, a row with inf
    and one with NaN, constant and all-zero rows (long runs), N(0, 3) noise, and a target page that was resident."""
    torch = torch_mod()
    lib = open_lib()
    try:
        lib.set_compression_scheme(scheme)
        T, L, bpe = 64, 3, 2
        region, n_pages = T // 2, 2 * T * L * H * D * bpe // PAGE
        st = torch.cuda.Stream()
        gen = torch.Generator(device="cuda"); gen.manual_seed(50 + scheme)
        noise = lambda *s: (torch.randn(s, generator=gen, device="cuda") * 3).to(torch.float16)
        pair_h, twin_h = [], []
        for _ in range(4):
            for lst in (pair_h, twin_h):
                h = lib.alloc(n_pages * PAGE); lib.set_layout(h, T, L, H, D, bpe); lst.append(h)
        # sources with padding between the layers: one more head than a row has
        k_step, v_step = noise(3, 4, L, H + 1, D), noise(3, 4, L, H + 1, D)
        k_tail, v_tail = noise(2, L, H + 1, D), noise(2, L, H + 1, D)
        stride = (H + 1) * D * 2
        k_step[1, 2, 1, 3, 17] = float("inf"); k_step[1, 2, 0, 0, 0] = float("-inf")
        v_step[1, 3, 2, 7, 127] = float("nan")
        k_tail[1] = 1.5; k_step[2, 0] = 1.5; v_tail[1] = 0.0; v_step[2, 0] = -0.25; v_step[2, 0, 1] = 0.0   # (layer 1's V page: all zero)
        # (allocation, first page, K even, K odd, V even, V odd): rows as (tensor, index)
        ks, vs, kt, vt = k_step, v_step, k_tail, v_tail
        pairs = [
            (0, 15, ks[2, 3], ks[0, 1], vs[2, 3], vs[0, 1]),           # two pairs of allocation 0: pages 15 and 16 of every region
            (0, 16, kt[0], ks[1, 0], vt[0], vs[1, 0]),                 # halves from different tensors, as a tail and a new row are
            (1, 3, ks[1, 2], ks[1, 3], vs[1, 2], vs[1, 3]),            # inf in K, NaN in V
            (2, 31, kt[1], ks[2, 0], vt[1], vs[2, 0]),                 # constant / all-zero rows: long runs
            (3, 0, ks[0, 0], ks[2, 1], vs[0, 0], vs[2, 1]),            # page 0 of allocation 3 is resident before the call
        ]
        image = lambda p: torch.stack([torch.stack((torch.cat((p[2][l, :H].reshape(-1), p[3][l, :H].reshape(-1))),
                                                    torch.cat((p[4][l, :H].reshape(-1), p[5][l, :H].reshape(-1))))) for l in range(L)]).contiguous()
        images = [image(p) for p in pairs]                              # [L][kind][2048] = 2 * L pages each
        assert all(im.numel() == 2 * L * N for im in images)
        lib.access(pair_h[3], 0, 8)
        assert lib.translate(pair_h[3], 0).flags & 3
        torch.cuda.synchronize()
        handles = np.asarray([pair_h[p[0]] for p in pairs], dtype=np.uint64)
        firsts = np.asarray([p[1] for p in pairs], dtype=np.uint64)
        rows = np.asarray([[r.data_ptr() for r in p[2:]] for p in pairs], dtype=np.uint64)
        before = lib.stats().total_compressions
        lib.write_pairs(handles, firsts, rows, region, L, stride, st.cuda_stream)
        assert lib.stats().total_compressions - before == len(pairs) * 2 * L
        twins = [1, 2, 3, 4]                                            # one descriptor per allocation: allocation 0's first pair on its own
        lib.write_strided(twin_h[0], 15, region, 2 * L, images[0].data_ptr(), st.cuda_stream)
        lib.write_strided_batch([twin_h[pairs[i][0]] for i in twins], [pairs[i][1] for i in twins], [images[i].data_ptr() for i in twins],
                                region, 2 * L, st.cuda_stream)
        st.synchronize()
        assert not (lib.translate(pair_h[3], 0).flags & 3)
        got = torch.empty((n_pages, N), dtype=torch.float16, device="cuda")
        want = torch.empty((n_pages, N), dtype=torch.float16, device="cuda")
        for a, b in zip(pair_h, twin_h):
            lib.fetch_range(a, 0, n_pages, got.data_ptr(), False, st.cuda_stream)
            lib.fetch_range(b, 0, n_pages, want.data_ptr(), False, st.cuda_stream)
            st.synchronize()
            assert torch.equal(got.view(torch.int16), want.view(torch.int16))
        for p in pairs:
            for j in range(2 * L):
                a, b = lib.translate(pair_h[p[0]], (p[1] + j * region) * PAGE), lib.translate(twin_h[p[0]], (p[1] + j * region) * PAGE)
                assert (a.rec_bytes, np.float32(a.scale).tobytes()) == (b.rec_bytes, np.float32(b.scale).tobytes()), (p[:2], j)
                assert a.rec_bytes > 0
        # refusals
        def refused(status, handles=handles, firsts=firsts, rows=rows, step=region, layers=L, stride=stride, stream=st.cuda_stream):
            with pytest.raises(SpeckvError) as e:
                lib.write_pairs(handles, firsts, rows, step, layers, stride, stream)
            assert e.value.status == status
        refused(ERR_INVAL, stream=0)                                                            # NULL stream
        bad = rows.copy(); bad[2, 1] += 8
        refused(ERR_INVAL, rows=bad)                                                            # a row that is not 16-byte aligned
        bad = rows.copy(); bad[4, 3] = 0
        refused(ERR_INVAL, rows=bad)                                                            # a NULL row
        refused(ERR_INVAL, stride=stride + 8)                                                   # stride not a multiple of 16
        refused(ERR_INVAL, step=0)
        same = firsts.copy(); same[1] = 15
        refused(ERR_INVAL, firsts=same)                                                         # the same (allocation, page) twice
        same[1] = 15 + region
        refused(ERR_INVAL, firsts=same, layers=1)                                               # ... and pairs one region apart share a page
        off = firsts.copy(); off[3] = region + 5
        refused(ERR_GENERAL, firsts=off)                                                        # the last pages leave the allocation
        unknown = handles.copy(); unknown[2] = 0xDEAD0000
        refused(ERR_GENERAL, handles=unknown)
        lib.set_compression_scheme(1)
        other = lib.alloc(n_pages * PAGE)
        mixed = handles.copy(); mixed[4] = other
        refused(ERR_INVAL, handles=mixed)                                                       # mixed schemes
        lib.write_pairs(handles, firsts, rows, region, 0, stride, st.cuda_stream)                # no layers: nothing to do, fine
        st.synchronize()
        for h in pair_h + twin_h + [other]:
            lib.free(h)
    finally:
        lib.finalize()


def _same_pool_and_tails(torch, a, b, ids_a, ids_b, L, G, gen):
    torch.cuda.synchronize()
    for ra, rb in zip(ids_a, ids_b):
        assert a.length(ra) == b.length(rb)
        qa, qb = a.requests[ra], b.requests[rb]
        assert (qa.tail_k is None) == (qb.tail_k is None) == (a.length(ra) % 2 == 0)
        if qa.tail_k is not None:
            assert torch.equal(qa.tail_k.view(torch.int16), qb.tail_k.view(torch.int16)) and torch.equal(qa.tail_v.view(torch.int16), qb.tail_v.view(torch.int16))
        for layer in range(L):
            for kind in (0, 1):
                assert torch.equal(a.kv_rows(ra, layer, kind).view(torch.int16), b.kv_rows(rb, layer, kind).view(torch.int16)), (ra, layer, kind)
    q = torch.randn((len(ids_a), H, G, D), generator=gen, device="cuda").to(torch.float16)
    for layer in range(L):
        assert torch.equal(a.attend(layer, ids_a, q, 1.0 / np.sqrt(D)), b.attend(layer, ids_b, q, 1.0 / np.sqrt(D))), layer


@pytest.mark.parametrize("scheme", ["fp8", "int4", "mxfp4"])
def test_commit_equals_append_tokens_and_append_path(scheme):
    """Two connectors over the same seeded data from starting lengths 0, 1, 31, 32: one commits with commit(), the other with
    append_tokens (four steps of accept counts 0..S) and append_path (a tree step).  After every step the rows of every (request,
    layer, kind), the lengths, the tails and an attention over both agree bit for bit.  INT4: once more with the K pre-scale on."""
    torch = torch_mod()
    lib = open_lib()
    try:
        L, T, B, S, G = 2, 128, 4, 4, 4
        gen = torch.Generator(device="cuda"); gen.manual_seed(61)
        rnd = lambda *s: torch.randn(s, generator=gen, device="cuda", dtype=torch.float32).to(torch.float16)
        rng = np.random.default_rng(61)
        next_id = [1]
        for kscale in ([False, True] if scheme == "int4" else [False]):
            a, b = SpeckvKVConnector(lib, L, H, D, T, scheme), SpeckvKVConnector(lib, L, H, D, T, scheme)
            if kscale:
                scale = torch.exp2(torch.randint(-2, 3, (L, H, D), generator=gen, device="cuda").to(torch.float32))
                a.set_k_channel_scale(scale); b.set_k_channel_scale(scale)
            ids_a = list(range(next_id[0], next_id[0] + B)); ids_b = [i + B for i in ids_a]; next_id[0] += 2 * B
            keep = []
            for ra, rb, n in zip(ids_a, ids_b, [0, 1, 31, 32]):
                a.add_request(ra); b.add_request(rb)
                if n:
                    k, v = rnd(L, n, H, D), rnd(L, n, H, D)
                    keep += a.write_prefill(ra, k, v) + b.write_prefill(rb, k, v)
            steps = [[1, 4, 3, 2]] + ([] if kscale else [[int(x) for x in rng.integers(0, S + 1, B)] for _ in range(3)])
            for n_accept in steps:
                k_new, v_new = rnd(B, S, L, H, D), rnd(B, S, L, H, D)
                keep += a.commit(ids_a, k_new, v_new, [list(range(n)) for n in n_accept])
                keep += b.append_tokens(ids_b, k_new, v_new, n_accept)
                _same_pool_and_tails(torch, a, b, ids_a, ids_b, L, G, gen)
            # a tree step: node 0 <- 1 <- 2, 1 <- 3; each request accepts another path
            tree, paths = [-1, 0, 1, 1], [[0, 1, 3], [0, 1, 2], [], [0]]
            k_new, v_new = rnd(B, S, L, H, D), rnd(B, S, L, H, D)
            keep += a.commit(ids_a, k_new, v_new, paths, parents=tree)
            keep += b.append_path(ids_b, k_new, v_new, paths, parents=tree)
            _same_pool_and_tails(torch, a, b, ids_a, ids_b, L, G, gen)
            lengths = [a.length(r) for r in ids_a]
            with pytest.raises(ValueError):
                a.commit(ids_a, k_new, v_new, [[0, 2, 3], [], [], []], parents=tree)         # 2 and 3 are siblings
            assert [a.length(r) for r in ids_a] == lengths
            torch.cuda.synchronize()
    finally:
        lib.finalize()
