"""A vLLM-shaped KV connector on top of libcxlspeckv.so.

The reference stops at a sketch of the decode loop (reference host/python/vllm_speckv_backend.py:104-129: per token,
``prefetch_step`` per layer, ``get_kv_ptr`` per entry) around a single-request allocator.  This class is the piece a
paged-attention layer would talk to for a BATCH of requests:

  add_request / free_request   one allocation per request (the shim layout of ``CxlSpeckvKVAllocator.allocate``:
                               ``[layer][kind][pos][head]``), its geometry and its request id bound in the engine
  write_prefill                the prompt's K / V of every layer, compressed into the pool
  append                       one decode step's new K / V rows of every layer for every request of the batch; rows
                               are stored page-wise (one 4 KiB page = 2 positions x 8 kv heads x 128), so an odd last
                               position lives in a small fp16 tail on the compute GPU until its partner arrives
  begin_step                   one batched speculative look-ahead for the whole batch (one device-side flush)
  block_table                  device addresses of the decompressed pages of a request (paged-attention consumers)
  attend                       the attention of one layer for the whole batch straight from the compressed records
                               (FP8 / INT4 pools: ``speckv_ext_attend_*_batch``), the tail position folded in with
                               the returned log-sum-exp
  attend_spec / append_tokens  a step of SEVERAL positions per request (speculative decoding, chunked prefill, ragged
                               batches): the S new positions ride through the same pass over the records as extra query
                               rows, the rows held outside the pool are folded in causally by one launch
                               (``speckv_ext_attend_fold_held``); then the accepted prefix is committed
  commit / truncate            the commit in one launch (``speckv_ext_write_pairs``), and its undo: roll requests back to shorter
                               lengths, the new odd last positions read back out of their pairs by one launch
                               (``speckv_ext_read_pairs``)
  attend_chunk                 the same attention for a CHUNK of any length (chunked prefill, the suffix behind a fork, a prompt continued
                               after a truncate): one launch, a workgroup per 64 query rows of a kv head (``speckv_ext_attend_chunk``)
  fork                         new requests started from positions other requests hold (parallel sampling, beam search, a shared
                               prefix): the stored records copied by one launch (``speckv_ext_copy_runs``), nothing decoded
  tree_masks / append_path     the same step with drafts that form a TREE (``attend_spec(parents=...)``): a node sees its
                               ancestors only, the held rows are folded in by ``speckv_ext_attend_fold_masked`` with one mask
                               word per (request, node); then the accepted root-to-node path is committed
  chunk_tree_masks             trees of ANY size (``attend_chunk(parents=...)``, ``speckv_ext_attend_chunk_masked``): mask rows of several
                               words per node, one launch; ``commit(nodes=path)`` stores the accepted path
  attend_tree                  the tree step of a layer, global or LOCAL (sliding window): a node's window goes by its DEPTH
                               (``chunk_tree_depths``, ``chunk_tree_masks(window=W)``, ``speckv_ext_attend_chunk_tree_window``)
  attend_shared                requests that SHARE A PREFIX without copies of it (parallel samples, beams, a system prompt): the members
                               hold only what is their own, the prefix is a request the call names; the own step as attend / attend_chunk
                               issue it, then ONE ``speckv_ext_attend_prefix_fold`` launch that reads the prefix once per 64 query rows
                               and folds it in (``attend_chunk_shared`` for a member's own chunk; ``shared_groups``)
  load_paged / store_paged     the route in and out of the pool for vLLM-style paged caches (one tensor per layer, rows addressed by a
                               slot mapping on the device): spans of positions of a batch of requests decoded into their slots, or encoded
                               from them, by one launch each way (``speckv_ext_read_slots`` / ``speckv_ext_write_slots``; ``paged_spans``);
                               ``fused=True``: bf16 caches and odd lengths in the same launch, the tail as a held row
                               (``speckv_ext_read_slots_ex`` / ``speckv_ext_write_slots_ex``); ``kscale=True`` on top: a connector with a K
                               pre-scale takes that launch too, the factor applied inside it (``speckv_ext_read_slots_kmul`` /
                               ``speckv_ext_write_slots_kmul``)

Only plain device pointers cross into the library; torch is used for device buffers and the tail fold.
"""
import numbers
from typing import Dict, List, Optional, Sequence

from .kv_shared import PARENTS_RULE, SPLITS_RULE, SharedPrefixSteps, _is_int, paged_cache_geometry, tail_index
from .speckv_ctypes import HELD_MAX, SpeckvLib

PAGE = 4096
SCHEMES = {"fp16": 0, "int8": 1, "int8_delta_rle": 2, "int4": 3, "fp8": 4, "mxfp4": 5}
FUSED = (3, 4, 5)              # schemes whose records the fused attention reads directly (speckv_ext_attend_{int4,fp8,mx4}_*)


class _Request:
    """handle, length, and the fp16 K / V rows of an odd last position ([layers][heads][dim]).  The tail is kept as a
    reference into the batch tensor it arrived in (tensor pair + row) and only sliced when somebody asks for it: creating
    512 tensor views per decode step of a 256-sequence batch cost 0.3 ms of host time that the lockstep path never used."""
    __slots__ = ("handle", "length", "_tail")

    def __init__(self, handle):
        self.handle = handle
        self.length = 0            # positions stored or held in the tail
        self._tail = None          # (k rows, v rows, row index) or (k, v, None) for tensors of this request alone

    def set_tail(self, k, v, row=None):
        self._tail = (k, v, row)

    def clear_tail(self):
        self._tail = None

    @property
    def tail_k(self):
        t = self._tail
        return None if t is None else (t[0] if t[2] is None else t[0][t[2]])

    @property
    def tail_v(self):
        t = self._tail
        return None if t is None else (t[1] if t[2] is None else t[1][t[2]])


def _device_index(values):
    """int32 index tensor on the device without a blocking copy (torch.tensor(list, device="cuda") waits for the stream)."""
    import torch
    return torch.tensor(values, dtype=torch.int32).pin_memory().to("cuda", non_blocking=True)


class SpeckvKVConnector(SharedPrefixSteps):
    def __init__(self, lib: SpeckvLib, num_layers: int, num_kv_heads: int = 8, head_dim: int = 128, max_tokens: int = 4096,
                 scheme: str = "fp8"):
        if num_kv_heads * head_dim * 2 != 2048:
            raise ValueError("the page-wise layout needs num_kv_heads * head_dim == 1024 fp16 elements per position "
                             "(8 kv heads x 128: Llama-3 8B / 70B)")
        if max_tokens % 32:
            raise ValueError("max_tokens must be a multiple of 32 (tile size of the fused attention)")
        self.lib = lib
        self.L, self.H, self.D, self.T = num_layers, num_kv_heads, head_dim, max_tokens
        self.scheme = SCHEMES[scheme] if isinstance(scheme, str) else int(scheme)
        self.requests: Dict[int, _Request] = {}
        self.region_pages = max_tokens // 2                   # pages of one (layer, kind) region
        self._side = None
        # the tails of the last append as ONE tensor per kind ([n][layers][heads][dim]) and the request ids they belong to:
        # a batch that decodes in lockstep folds / pairs its tails without touching 256 per-request views
        self._tail_ids = ()
        self._tail_k = self._tail_v = None
        self._fold_key = self._arg_key = None
        self._plan = None                                     # device buffer of the step's attention plan
        self._plan_bound = 0
        self._wplans = {}                                     # window -> [plan buffer, bound, arg key]: one plan per window value beside the global one
        self._fold_rows = self._fold_idx = self._fold_k = self._fold_v = None
        self._fold_n = 0
        # host-side bookkeeping of a decode loop is per STEP, not per layer: `_epoch` moves whenever a length or the set of
        # requests changes, and everything derived from (batch, lengths) -- the attention plan, the fold rows, the ctypes
        # arrays of a batched append -- is keyed by (the caller's id sequence, epoch) instead of rebuilding 256-element tuples
        # for every layer (that alone was ~20 us per attend() call)
        self._epoch = 0
        self._batch_cache = {}
        self._step_cols = {}
        self._plan_stream = None
        self._kscale = self._kscale_inv = None               # set_k_channel_scale
        self._spec_key = self._spec_idx = self._spec_base = None     # attend_spec: where the held rows of a step come from
        self._tree_key = self._tree_masks = None                     # attend_spec(parents=...): the mask words of a step, [n_layers * batch][S]
        self._chunk_tree_key = self._chunk_tree_masks = None         # attend_chunk(parents=...): the mask rows of a step, [batch][S][W]
        self._chunk_tree_wtabs = {}                                  # attend_tree(window=W): W -> (key, mask rows, depths [batch][S])
        self._shared_key = self._shared_plan = None                  # attend_shared / attend_chunk_shared: the judged arguments of a step

    def set_k_channel_scale(self, scale):
        """Per-(layer, kv head, channel) pre-scale of K, folded into the query: K / scale goes into the pool, q * scale meets it, q.k is
        unchanged.  `scale`: [layers][heads][dim] tensor of POWERS OF TWO (exact in fp16 both ways; kv_accuracy.pow2_channel_scales
        calibrates them from a prompt's K: the channel's max|k| over the head's median channel), or None to switch it off.  What it buys:
        an outlier channel of K no longer sets the block scale of the channels that share its quantisation group -- on KV-like data
        INT4_G32 loses 0.33-0.42 of the attention output instead of 0.57-0.71 when the query weighs those channels (MXFP4, whose limit
        there is the element's one mantissa bit, gains little): profiles/r06d_kv_format_accuracy.txt, tests/test_gpu_accuracy.py.
        Set it before the first write; rows read back through kv_rows() are scaled back."""
        import torch
        if any(r.length for r in self.requests.values()):
            raise ValueError("set_k_channel_scale after positions were written: the pool would hold K in two scalings")
        if scale is None:
            self._kscale = self._kscale_inv = None
            return
        scale = torch.as_tensor(scale, dtype=torch.float32, device="cuda")
        if tuple(scale.shape) != (self.L, self.H, self.D):
            raise ValueError(f"k channel scale must be [layers][heads][dim] = {(self.L, self.H, self.D)}")
        if not bool(torch.all(scale == torch.exp2(torch.round(torch.log2(scale))))):
            raise ValueError("k channel scales must be powers of two (anything else rounds K and q a second time)")
        self._kscale = scale.to(torch.float16).contiguous()
        self._kscale_inv = (1.0 / scale).to(torch.float16).contiguous()

    def calibrate_k_channel_scale(self, k):
        """set_k_channel_scale from a sample of K ([layers][tokens][heads][dim], e.g. a first prompt): per (layer, head, channel) the
        channel's max|k| over the head's median channel, rounded to a power of two (kv_accuracy.pow2_channel_scales, here on the device).
        Returns the scales it set."""
        import torch
        k = torch.as_tensor(k, device="cuda")
        if k.dim() != 4 or tuple(k.shape[0:1] + k.shape[2:]) != (self.L, self.H, self.D) or k.shape[1] == 0:
            raise ValueError(f"k sample must be [layers][tokens][heads][dim] = ({self.L}, n, {self.H}, {self.D})")
        amax = k.abs().to(torch.float32).amax(dim=1)                                 # [layers][heads][dim]
        med = torch.quantile(amax, 0.5, dim=-1, keepdim=True).clamp_min(1e-9)        # (the mean of the two middle channels, as numpy's median)
        scale = torch.exp2(torch.round(torch.log2((amax / med).clamp_min(1e-9)))).clamp(2.0 ** -14, 2.0 ** 14)      # (exact in fp16 both ways)
        self.set_k_channel_scale(scale)
        return scale

    # The library takes a hipStream_t and reads NULL as "the engine's own stream".  torch's default stream IS the NULL
    # stream, so work issued from it goes through a side stream that is ordered after it and that it then waits for.
    class _On:
        def __init__(self, conn, stream):
            import torch
            self.cur = stream if stream is not None else torch.cuda.current_stream()
            self.side = None
            if self.cur.cuda_stream == 0:
                if conn._side is None:
                    conn._side = torch.cuda.Stream()
                self.side = conn._side

        def __enter__(self):
            import torch
            if self.side is not None:
                self.side.wait_stream(self.cur)
                return self.side
            # an explicit stream that is not torch's current one: tensors the caller (or this class) produced on the
            # current stream -- q.contiguous(), the gathered page images -- must be complete before the library reads them
            now = torch.cuda.current_stream()
            if now.cuda_stream != self.cur.cuda_stream:
                self.cur.wait_stream(now)
            return self.cur

        def __exit__(self, *exc):
            if self.side is not None:
                self.cur.wait_stream(self.side)
            return False

    # ------------------------------------------------------------------ requests
    def add_request(self, req_id: int) -> int:
        if req_id in self.requests:
            raise KeyError(f"request {req_id} already exists")
        self.lib.set_compression_scheme(self.scheme)
        h = self.lib.alloc(2 * self.T * self.L * self.H * self.D * 2)
        self.lib.set_layout(h, self.T, self.L, self.H, self.D, 2)
        self.lib.bind_request(req_id, h, 0)
        self.requests[req_id] = _Request(h)
        self._epoch += 1
        self._batch_cache.clear()
        self._step_cols.clear()
        return h

    def free_request(self, req_id: int):
        r = self.requests.pop(req_id)
        self._epoch += 1
        self._batch_cache.clear()
        self._step_cols.clear()
        if req_id in self._tail_ids:
            self._tail_ids, self._tail_k, self._tail_v = (), None, None
        self._arg_key = self._fold_key = None                 # a plan names record addresses: plan again
        self._plan_stream = None                              # (and no early plan on a stream the caller may be done with)
        self.lib.free(r.handle)                               # the binding goes with the handle

    def length(self, req_id: int) -> int:
        return self.requests[req_id].length

    def _page(self, layer: int, kind: int, pos: int) -> int:
        return ((layer * 2 + kind) * self.T + pos) // 2

    def _batch(self, req_ids):
        """Per-batch constants (the request objects, their handles as a ctypes array), cached by the id sequence."""
        import ctypes
        key = tuple(req_ids)
        b = self._batch_cache.get(key)
        if b is None:
            if len(self._batch_cache) > 16:
                self._batch_cache.clear()
            reqs = [self.requests[r] for r in req_ids]
            b = self._batch_cache[key] = (key, reqs, (ctypes.c_uint64 * len(reqs))(*[r.handle for r in reqs]))
        return b

    # ------------------------------------------------------------------ writes
    def write_prefill(self, req_id: int, k, v, stream=None):
        """k, v: [layers][tokens][heads][dim] fp16 CUDA tensors of the prompt.  ONE asynchronous launch for the request
        (speckv_ext_write_runs: the 2 * layers K / V regions are page runs of the allocation, read in place from k and v);
        returns the tensors the launch reads -- hold them until the stream has passed it."""
        r = self.requests[req_id]
        n = k.shape[1]
        if r.length:
            raise ValueError("write_prefill on a request that already has positions")
        even = n & ~1
        if self._kscale_inv is not None:
            k = k * self._kscale_inv[:, None]                  # [layers][tokens][heads][dim] / [layers][1][heads][dim]
        k = k.contiguous(); v = v.contiguous()
        if even:
            layer_bytes = n * self.H * self.D * 2
            firsts = [self._page(layer, kind, 0) for kind in (0, 1) for layer in range(self.L)]
            srcs = [t.data_ptr() + layer * layer_bytes for t in (k, v) for layer in range(self.L)]
            with self._On(self, stream) as st:
                self.lib.write_runs(r.handle, firsts, srcs, even // 2, st.cuda_stream)
        if n & 1:
            r.set_tail(k[:, n - 1].contiguous().clone(), v[:, n - 1].contiguous().clone())
        r.length = n
        self._epoch += 1
        return [k, v]

    def append(self, req_ids: Sequence[int], k_new, v_new, stream=None):
        """One decode step: k_new, v_new [batch][layers][heads][dim] fp16.  A position that completes a pair is written
        together with its partner -- 2 * layers pages per request, ONE asynchronous launch for the whole batch
        (speckv_ext_write_strided_batch); an odd one waits in the tail.  A handful of torch kernels per call, whatever
        the batch size: the tails of a step are kept as views of one gathered tensor."""
        import torch
        if self._kscale_inv is not None:
            k_new = k_new * self._kscale_inv[None]              # [batch][layers][heads][dim]
        pair_b, tail_b = [], []
        for b, rid in enumerate(req_ids):
            r = self.requests[rid]
            if r.length >= self.T:
                raise ValueError(f"request {rid} is full")
            (pair_b if r.length % 2 else tail_b).append(b)
        keep = []
        if pair_b:
            reqs = [self.requests[req_ids[b]] for b in pair_b]
            whole = len(pair_b) == len(req_ids)
            idx = None if whole else _device_index(pair_b)
            if tuple(req_ids[b] for b in pair_b) == self._tail_ids:
                kt, vt = self._tail_k, self._tail_v                                                    # [n][layers][heads][dim]
            else:
                kt = torch.stack([r.tail_k for r in reqs]); vt = torch.stack([r.tail_v for r in reqs])
            with self._On(self, stream) as st:
                # the page images are built ON the stream the write runs on (ordered after the producers of k_new / the
                # tails by _On): a compress kernel must never see a half-built image
                with torch.cuda.stream(st):
                    kn, vn = (k_new, v_new) if whole else (k_new.index_select(0, idx), v_new.index_select(0, idx))
                    # page image of the pair for every (layer, kind): [n][layer][kind][2 positions][heads][dim]
                    pair = torch.stack((torch.stack((kt, kn), dim=2), torch.stack((vt, vn), dim=2)), dim=2).contiguous()
                keep.append(pair)
                step_bytes = pair[0].numel() * 2
                if len(reqs) == 1:
                    self.lib.write_strided(reqs[0].handle, self._page(0, 0, reqs[0].length - 1), self.region_pages, 2 * self.L,
                                           pair.data_ptr(), st.cuda_stream)
                else:
                    import ctypes
                    import numpy as np
                    n_ = len(reqs)
                    handles = self._batch(req_ids)[2] if whole else [r.handle for r in reqs]
                    firsts = np.fromiter((r.length - 1 for r in reqs), dtype=np.uint64, count=n_) // 2       # _page(0, 0, pos) = pos // 2
                    srcs = np.arange(n_, dtype=np.uint64) * np.uint64(step_bytes) + np.uint64(pair.data_ptr())
                    self.lib.write_strided_batch(handles, firsts, srcs, self.region_pages, 2 * self.L, st.cuda_stream)
            for r in reqs:
                r.clear_tail()
            self._tail_ids, self._tail_k, self._tail_v = (), None, None
        if tail_b:
            if len(tail_b) == len(req_ids):                                                             # copies: the caller may reuse k_new
                tk, tv = k_new.clone(memory_format=torch.contiguous_format), v_new.clone(memory_format=torch.contiguous_format)
            else:
                idx = _device_index(tail_b)
                tk = k_new.index_select(0, idx); tv = v_new.index_select(0, idx)
            for i, b in enumerate(tail_b):
                r = self.requests[req_ids[b]]
                r.set_tail(tk, tv, i)
            self._tail_ids, self._tail_k, self._tail_v = tuple(req_ids[b] for b in tail_b), tk, tv
        for rid in req_ids:
            self.requests[rid].length += 1
        self._epoch += 1
        # The next step's attention plan, now: the host is ahead of the GPU here (the step's attention launches are still
        # running), so its handle look-ups and the upload of its descriptors cost the next step nothing.  On the stream the
        # step's attention ran on: the upload is ordered behind the launches that still read the current plan.
        st = self._plan_stream
        if st is not None and self._arg_key is not None and self._arg_key[0][0] == tuple(req_ids) and self.scheme in FUSED:
            # best effort: the append itself has taken effect (lengths, tails, pool write) -- a plan that cannot be made now (the
            # stream is capturing, or was destroyed by its owner) must not make the caller retry it; attend() plans again instead
            # (only those two cases are swallowed -- the capture status is asked of the stream the plan would go to, not
            # of torch's current one -- a real failure of the plan, a bad layout or an exhausted pool, is the caller's to see)
            from .speckv_ctypes import SpeckvError
            try:
                if not self.lib.stream_is_capturing(st.cuda_stream):
                    self.plan_step(req_ids, st)
                    key, reqs, _ = self._batch(req_ids)
                    self._prepare_tails(req_ids, key, reqs, st)   # (and which rows carry a tail into the next step: 40 us of host time off its start)
                else:
                    self._arg_key = self._plan_stream = None
            except SpeckvError as e:
                self._arg_key = self._plan_stream = None
                if e.status != -4:                             # SPECKV_ERR_INVAL: the stream refuses the plan now (capturing / destroyed): attend() plans again
                    raise
        return keep                                            # sources of the asynchronous writes: hold until the stream passed them

    # ------------------------------------------------------------------ reads
    def begin_step(self, req_ids: Sequence[int], depth_k: int = 0, force: bool = False) -> Optional[int]:
        """Speculative look-ahead of the next positions of every (request, layer): one prefetch batch, one flush.
        For pools whose pages are consumed decompressed (fp16 / int8 schemes).  The fused attention of the FP8 / INT4 / MXFP4
        pools reads the records themselves and never looks into the ring of decoded pages, so for those pools the call does
        nothing (it used to decode 4 positions x layers x requests per step that nobody read: 0.09 ms of a 1 ms decode step,
        profiles/r06_connector_step.txt) unless `force` says that block_table() / access() consumers exist beside it."""
        import numpy as np
        if self.scheme in FUSED and not force:
            return None
        key, robjs, _ = self._batch(req_ids)
        cols = self._step_cols.get((key, depth_k))            # request / layer / depth columns: constants of the batch
        if cols is None:
            if len(self._step_cols) > 16:
                self._step_cols.clear()
            n = len(req_ids) * self.L
            cols = self._step_cols[(key, depth_k)] = (np.repeat(np.asarray(req_ids, dtype=np.uint32), self.L),
                                                      np.tile(np.arange(self.L, dtype=np.uint16), len(req_ids)),
                                                      np.full(n, depth_k, np.uint32))
        reqs, layers, depth = cols
        pos = np.repeat(np.fromiter((max(r.length - 1, 0) for r in robjs), dtype=np.uint32, count=len(robjs)), self.L)
        self.lib.prefetch_batch(reqs, layers, pos, depth)
        return self.lib.prefetch_flush(want_count=False)

    def block_table(self, req_id: int, layer: int, kind: int, pos_begin: int, pos_end: int) -> List[int]:
        """Device addresses of the decompressed rows [pos_begin, pos_end) (stored positions only)."""
        r = self.requests[req_id]
        row = self.H * self.D * 2
        base = ((layer * 2 + kind) * self.T) * row
        return self.lib.access_batch(r.handle, [base + p * row for p in range(pos_begin, min(pos_end, r.length & ~1))])

    def kv_rows(self, req_id: int, layer: int, kind: int, pos_begin: int = 0, pos_end: Optional[int] = None):
        """The stored rows [pos_begin, pos_end) of one layer (default: all of them) as an fp16 tensor [positions][heads][dim]
        (fetch + decompress of the pages that hold them), tail included.  Only those pages are read."""
        import torch
        r = self.requests[req_id]
        pos_end = r.length if pos_end is None else pos_end
        if not 0 <= pos_begin <= pos_end <= r.length:
            raise ValueError(f"rows [{pos_begin}, {pos_end}) of a request with {r.length} positions")
        even = r.length & ~1
        lo, hi = pos_begin & ~1, min((pos_end + 1) & ~1, even)          # whole pages (2 positions each) of the stored part
        out = torch.empty((max(hi, pos_end) - lo, self.H, self.D), dtype=torch.float16, device="cuda")
        if hi > lo:
            with self._On(self, None) as st:
                self.lib.fetch_range(r.handle, self._page(layer, kind, lo), (hi - lo) // 2, out.data_ptr(), False, st.cuda_stream)
        if pos_end > even:                                               # the odd last position lives in the tail
            out[even - lo] = (r.tail_k if kind == 0 else r.tail_v)[layer]
        if kind == 0 and self._kscale is not None:
            out = out * self._kscale[layer][None]                        # back to the caller's scaling (exact: powers of two)
        return out[pos_begin - lo:pos_end - lo]

    # ------------------------------------------------------------------ paged caches (vLLM's blocks)
    @staticmethod
    def paged_spans(firsts: Sequence[int], counts: Sequence[int]):
        """The position pairs a paged transfer touches, per span [firsts[i], firsts[i] + counts[i]): (first pair, pair count, pairs of
        the spans in front of it).  A span covers the pairs [first // 2, (first + count + 1) // 2) -- a pair it only half covers
        included -- and an empty span none; the exclusive prefix is what the kernels search to find the span of a flat pair index
        (speckv_ext_read_slots / _write_slots compute the same on the host).  Pure: no connector state."""
        if len(firsts) != len(counts):
            raise ValueError("paged_spans: one count per first position")
        out, prefix = [], 0
        for f, c in zip(firsts, counts):
            f, c = int(f), int(c)
            if f < 0 or c < 0:
                raise ValueError(f"paged_spans: span [{f}, {f} + {c})")
            n = (f + c + 1) // 2 - f // 2 if c else 0
            out.append((f // 2, n, prefix))
            prefix += n
        return out

    def _paged_geometry(self, caches, bf16=False, kscale=False):
        """(slots per cache, bytes between the K and the V plane) if the one-launch route can address `caches` -- per layer a
        [2, blocks, block_size, heads, dim] fp16 tensor whose slots are 2048-byte rows one after the other -- else None.
        bf16=True (the fused route): the caches may all be bfloat16 instead, and the element type (SLOT_ELEM_*) comes third.
        kscale=True (the fused route with the factor inside the launch): a K pre-scale does not shut the route."""
        if self._kscale is not None and not kscale:
            return None
        return paged_cache_geometry(caches, self.L, bf16)[0]          # (kv_shared.py: the split connector judges its caches by the same)

    def _held_tail(self, r):
        """(K address, V address) of request r's tail for a fused paged call -- fp16, 16-byte aligned, a layer every H * D elements;
        a tail that does not lie like that (never one this class made) is laid out again first."""
        k, v, row = r._tail
        ok = lambda t: t.is_contiguous() and t.data_ptr() % 16 == 0
        if row is not None:
            if ok(k) and ok(v):                                               # a row of the batched tails: no view is made
                step = k.stride(0) * 2
                return k.data_ptr() + row * step, v.data_ptr() + row * step, (k, v)
            k, v = k[row], v[row]
        if not (ok(k) and ok(v)):
            k, v = k.contiguous().clone(), v.contiguous().clone()
            r.set_tail(k, v)
        return k.data_ptr(), v.data_ptr(), (k, v)

    def _paged_args(self, req_ids, counts, slot_mapping, caches):
        import torch
        reqs = [self.requests[rid] for rid in req_ids]
        counts = [int(c) for c in counts]
        if len(counts) != len(reqs) or any(c < 0 for c in counts):
            raise ValueError("one non-negative count per request")
        if len(caches) != self.L:
            raise ValueError(f"{len(caches)} caches for {self.L} layers")
        if slot_mapping.dtype != torch.int64 or slot_mapping.dim() != 1 or not slot_mapping.is_contiguous() \
                or slot_mapping.numel() != sum(counts):
            raise ValueError("slot_mapping: one contiguous int64 device tensor, the spans concatenated")
        begins, at = [], 0
        for c in counts:
            begins.append(at)
            at += c
        return reqs, counts, begins

    def load_paged(self, req_ids: Sequence[int], firsts: Sequence[int], counts: Sequence[int], slot_mapping, caches, stream=None, fused=False,
                   kscale=False):
        """Pool -> paged caches: positions [firsts[i], firsts[i] + counts[i]) of request req_ids[i] go into the slots
        slot_mapping[b_i : b_i + counts[i]] (b_i = the counts in front: ONE int64 device tensor for the call, the spans concatenated) of
        `caches`, the per-layer [2, blocks, block_size, 8, 128] fp16 tensors.  ONE speckv_ext_read_slots call decodes every stored row
        of every layer where its slot is; a span that reaches a request's odd last position gets that row from the held tail by a
        torch copy, as kv_rows does.  A slot < 0 or beyond the cache is skipped.
        Fall-back to the row route (kv_rows + index_copy_ per request, layer and kind) when a K pre-scale is set, a cache is not
        fp16, not contiguous in its last three dimensions, or does not have 2048-byte rows one block after the other (without fused=True
        that includes bf16 caches).
        fused=True: bf16 caches of that geometry take the one-launch route as well (the decoded fp16 value rounded once to bf16:
        kv_rows(...).to(bfloat16)), and the tail is handed to the launch as a held row: exactly ONE speckv_ext_read_slots_ex call,
        no torch copy per request.  The K pre-scale, other dtypes and other strides still go the row route.
        kscale=True on top of fused=True: a connector with a K pre-scale takes the one launch as well -- ONE
        speckv_ext_read_slots_kmul call, every K element multiplied by its channel's scale inside the kernel (the exact product
        rounded once to the caches' element type: with fp16 caches the row route's bits), the tail as a held row.  Without a
        pre-scale the keyword changes nothing."""
        import numpy as np
        import torch
        reqs, counts, begins = self._paged_args(req_ids, counts, slot_mapping, caches)
        firsts = [int(f) for f in firsts]
        if len(firsts) != len(reqs):
            raise ValueError("one first position per request")
        for r, f, c in zip(reqs, firsts, counts):
            if not 0 <= f <= f + c <= r.length:
                raise ValueError(f"rows [{f}, {f + c}) of a request with {r.length} positions")
        geo = self._paged_geometry(caches, bf16=True, kscale=bool(kscale)) if fused else None
        if geo is not None:
            n_slots, kind_stride, elem = geo
            held, any_held = np.zeros(2 * len(reqs), dtype=np.uint64), False
            read, factor = self.lib.read_slots_ex, {}
            if self._kscale is not None:                                      # back to the caller's scaling inside the launch
                read, factor = self.lib.read_slots_kmul, dict(k_mul=self._kscale.data_ptr(), k_mul_stride=self.H * self.D * 2)
            for i, (r, f, c) in enumerate(zip(reqs, firsts, counts)):
                if c and (r.length & 1) and f + c == r.length:                # the span ends on the tail: a held row
                    held[2 * i], held[2 * i + 1], _ = self._held_tail(r)
                    any_held = True
            if any(counts):
                with self._On(self, stream) as st:
                    read(np.asarray([r.handle for r in reqs], dtype=np.uint64), np.asarray(firsts, dtype=np.uint64),
                         np.asarray(counts, dtype=np.uint64), np.asarray(begins, dtype=np.uint64), slot_mapping.data_ptr(),
                         n_slots, np.asarray([c.data_ptr() for c in caches], dtype=np.uint64), 0, kind_stride,
                         self.region_pages, st.cuda_stream, elem=elem, held_in=held if any_held else None,
                         held_stride=self.H * self.D * 2, **factor)
            return
        geo = self._paged_geometry(caches)
        if geo is None:
            with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
                for rid, f, c, b in zip(req_ids, firsts, counts, begins):
                    if not c:
                        continue
                    slots = slot_mapping[b:b + c]
                    for layer, cache in enumerate(caches):
                        flat = cache.reshape(2, cache.shape[1] * cache.shape[2], cache.shape[3], cache.shape[4])
                        for kind in (0, 1):
                            flat[kind].index_copy_(0, slots, self.kv_rows(rid, layer, kind, f, f + c).to(flat.dtype))
            return
        n_slots, kind_stride = geo
        stored = [max(min(f + c, r.length & ~1) - f, 0) for r, f, c in zip(reqs, firsts, counts)]
        with self._On(self, stream) as st:
            if any(stored):
                self.lib.read_slots(np.asarray([r.handle for r in reqs], dtype=np.uint64), np.asarray(firsts, dtype=np.uint64),
                                    np.asarray(stored, dtype=np.uint64), np.asarray(begins, dtype=np.uint64), slot_mapping.data_ptr(), n_slots,
                                    np.asarray([c.data_ptr() for c in caches], dtype=np.uint64), 0, kind_stride, self.region_pages, st.cuda_stream)
            with torch.cuda.stream(st):
                for r, f, c, b, n in zip(reqs, firsts, counts, begins, stored):
                    if c > n:                                                 # the odd last position lives in the tail
                        at = slot_mapping[b + n:b + n + 1]
                        for layer, cache in enumerate(caches):
                            cache[0].view(n_slots, self.H, self.D).index_copy_(0, at, r.tail_k[layer][None])
                            cache[1].view(n_slots, self.H, self.D).index_copy_(0, at, r.tail_v[layer][None])

    def store_paged(self, req_ids: Sequence[int], counts: Sequence[int], slot_mapping, caches, stream=None, fused=False, kscale=False):
        """Paged caches -> pool: request req_ids[i], whose current length is even (an odd one raises ValueError: not built), gets
        counts[i] more positions, read from the slots slot_mapping[b_i : b_i + counts[i]] of `caches` (as load_paged).  ONE
        speckv_ext_write_slots call encodes the whole pairs of every layer straight from the caches -- no gathered copy exists, so
        the caller holds nothing, but the caches and the mapping stay unchanged until the stream has passed the call; an odd last
        position becomes the tail, gathered with torch.  Lengths and the step bookkeeping move as in write_prefill.  A slot < 0 or
        beyond the cache is stored as a row of zeros.
        Fall-back to the row route (index_select per layer, torch.stack, write_prefill per request -- for requests that are still
        empty) under the conditions load_paged names.  Returns the tensors the row route's launches read (hold them until the
        stream has passed), an empty list on the one-launch route.
        fused=True: bf16 caches of that geometry take the one-launch route too (a bf16 element rounded once to fp16, and that is
        stored: the records of row.to(float16)), and a request of odd length is accepted: its tail goes into the launch as the held
        row that completes its pair, a new odd last position comes back through held rows -- one [tails][layers][heads][dim] fp16
        tensor per kind for the call, installed as the batched tails a lockstep append pairs without per-request views.  Exactly
        ONE speckv_ext_write_slots_ex call and no torch copy per request; returns the tails the launch read.  On the row route (K
        pre-scale, other dtypes or strides) an odd length still raises.
        kscale=True on top of fused=True: a connector with a K pre-scale takes the one launch too -- ONE speckv_ext_write_slots_kmul
        call, every K element of a cache row divided by its channel's scale inside the kernel (times the power-of-two inverse, the
        exact product rounded once to fp16: from a bf16 cache ONE rounding where the row route rounds twice), tails as held rows,
        which hold pre-scaled K like every tail.  Without a pre-scale the keyword changes nothing."""
        import numpy as np
        import torch
        reqs, counts, begins = self._paged_args(req_ids, counts, slot_mapping, caches)
        if len(set(req_ids)) != len(reqs):
            raise ValueError("store_paged: a request named twice")
        geo = self._paged_geometry(caches, bf16=True, kscale=bool(kscale)) if fused else None
        for r, c in zip(reqs, counts):
            if r.length & 1 and geo is None:
                raise ValueError("store_paged on a request of odd length")
            if r.length + c > self.T:
                raise ValueError(f"{r.length} + {c} positions in a request built for {self.T}")
        if geo is not None:
            n_slots, kind_stride, elem = geo
            n = len(reqs)
            h_in, h_out, read, tails = np.zeros(2 * n, dtype=np.uint64), np.zeros(2 * n, dtype=np.uint64), [], []
            first = [r.length if c else r.length & ~1 for r, c in zip(reqs, counts)]      # (an empty span names an even position)
            write, factor = self.lib.write_slots_ex, {}
            if self._kscale_inv is not None:                                  # into the pool's scaling inside the launch
                write, factor = self.lib.write_slots_kmul, dict(k_mul=self._kscale_inv.data_ptr(), k_mul_stride=self.H * self.D * 2)
            for i, (r, c) in enumerate(zip(reqs, counts)):
                if c and r.length & 1:
                    h_in[2 * i], h_in[2 * i + 1], keep = self._held_tail(r)
                    read += keep
                if c and (r.length + c) & 1:
                    tails.append(i)
            with self._On(self, stream) as st:
                tk = tv = None
                if tails:
                    with torch.cuda.stream(st):
                        tk = torch.empty((len(tails), self.L, self.H, self.D), dtype=torch.float16, device=slot_mapping.device)
                        tv = torch.empty_like(tk)
                    row = tk[0].numel() * 2
                    for j, i in enumerate(tails):
                        h_out[2 * i], h_out[2 * i + 1] = tk.data_ptr() + j * row, tv.data_ptr() + j * row
                if any(counts):
                    write(np.asarray([r.handle for r in reqs], dtype=np.uint64), np.asarray(first, dtype=np.uint64),
                          np.asarray(counts, dtype=np.uint64), np.asarray(begins, dtype=np.uint64), slot_mapping.data_ptr(),
                          n_slots, np.asarray([c.data_ptr() for c in caches], dtype=np.uint64), 0, kind_stride,
                          self.region_pages, st.cuda_stream, elem=elem, held_in=h_in if read else None,
                          held_stride=self.H * self.D * 2, held_out=h_out if tails else None, **factor)
            touched = [rid for rid, c in zip(req_ids, counts) if c]
            for r, c in zip(reqs, counts):
                if c:
                    r.clear_tail()
                    r.length += c
            for j, i in enumerate(tails):
                reqs[i].set_tail(tk, tv, j)
            if tails:
                self._tail_ids, self._tail_k, self._tail_v = tuple(req_ids[i] for i in tails), tk, tv
            elif any(rid in self._tail_ids for rid in touched):
                self._tail_ids, self._tail_k, self._tail_v = (), None, None
            self._epoch += 1
            return read
        geo = self._paged_geometry(caches)
        if geo is None:
            held = []
            if any(r.length for r, c in zip(reqs, counts) if c):
                raise ValueError("store_paged: the row route writes whole prompts (write_prefill) and these requests hold positions")
            for rid, c, b in zip(req_ids, counts, begins):
                if not c:
                    continue
                slots = slot_mapping[b:b + c]
                flats = [cache.reshape(2, cache.shape[1] * cache.shape[2], cache.shape[3], cache.shape[4]) for cache in caches]
                k = torch.stack([f[0].index_select(0, slots) for f in flats]).to(torch.float16)      # [layers][tokens][heads][dim]
                v = torch.stack([f[1].index_select(0, slots) for f in flats]).to(torch.float16)
                held += self.write_prefill(rid, k, v, stream)
            return held
        n_slots, kind_stride = geo
        whole = [c & ~1 for c in counts]
        with self._On(self, stream) as st:
            if any(whole):
                self.lib.write_slots(np.asarray([r.handle for r in reqs], dtype=np.uint64), np.asarray([r.length for r in reqs], dtype=np.uint64),
                                     np.asarray(whole, dtype=np.uint64), np.asarray(begins, dtype=np.uint64), slot_mapping.data_ptr(), n_slots,
                                     np.asarray([c.data_ptr() for c in caches], dtype=np.uint64), 0, kind_stride, self.region_pages, st.cuda_stream)
            with torch.cuda.stream(st):
                for r, c, b in zip(reqs, counts, begins):
                    if c & 1:
                        at = slot_mapping[b + c - 1:b + c]
                        r.set_tail(torch.cat([cache[0].view(n_slots, self.H, self.D).index_select(0, at) for cache in caches]),
                                   torch.cat([cache[1].view(n_slots, self.H, self.D).index_select(0, at) for cache in caches]))
        if any(rid in self._tail_ids for rid in req_ids):
            self._tail_ids, self._tail_k, self._tail_v = (), None, None
        for r, c in zip(reqs, counts):
            r.length += c
        self._epoch += 1
        return []

    PLAN_BUCKET = 512
    WINDOW_PLANS_MAX = 8                 # plan buffers kept for window values (plan_step(window=W)) beside the global one

    @staticmethod
    def _decode_window(window):
        """window=None or 0: none; else an int >= 1"""
        if window is None or window == 0:
            return 0
        if int(window) != window or not 1 <= int(window) < 2 ** 32:
            raise ValueError("window must be None or an integer >= 1")
        return int(window)

    @staticmethod
    def decode_window_range(length: int, window):
        """The walk rule of attend(window=W) (csrc/decode_window.hpp, speckv_ext_decode_window_range), restated: a request of `length`
        positions -- the step's own included, i.e. its length when attend() runs -- has stored = length & ~1 of them in the pool and its
        query at length - 1 sees [lo, length - 1], lo = max(0, length - W).  Returns (begin, skip, n_pages): the launch walks the pool from
        the tile of lo, begin = lo & ~31, with the first skip = lo - begin positions masked, over n_pages = (stored - begin) / 2 pages;
        n_pages = 0 where lo == stored (W = 1 with an odd length, a length below 2): no pool position, the tail at most."""
        W = SpeckvKVConnector._decode_window(window)
        length = int(length)
        stored = length & ~1
        lo = length - W if W and length > W else 0
        begin = lo & ~31
        return begin, lo - begin, (stored - begin) // 2 if lo < stored else 0

    def plan_step(self, req_ids: Sequence[int], stream, window=None):
        """The attention plan of this decode step for the batch `req_ids` at their current lengths, on `stream` (a torch
        stream, not the default one).  attend() calls it by itself when the batch or the lengths changed; a caller that
        replays captured per-layer calls runs it before every replay.  Returns the length bound the launches are sized for.
        window=W: the plan of the step's sliding-window layers of that window (speckv_ext_attend_batch_plan_window) -- ONE PLAN PER
        WINDOW VALUE is kept beside the global one, so a step over interleaved local and global layers plans once per kind and
        launches as before; the bound is bucketed in the same way."""
        import ctypes
        import torch
        key, reqs, handles = self._batch(req_ids)
        B = len(reqs)
        lens = [r.length & ~1 for r in reqs]
        bound = min(self.T, max(self.PLAN_BUCKET, (max(lens) + self.PLAN_BUCKET - 1) // self.PLAN_BUCKET * self.PLAN_BUCKET))
        W = self._decode_window(window)
        if W:
            need = self.lib.attend_plan_window_bytes(B)
            if W not in self._wplans and len(self._wplans) >= self.WINDOW_PLANS_MAX:      # (a model has one or two window values: the oldest goes)
                del self._wplans[next(iter(self._wplans))]
            slot = self._wplans.setdefault(W, [None, 0, None])
            if slot[0] is None or slot[0].numel() < need:
                slot[0] = torch.zeros(need, dtype=torch.uint8, device="cuda")
            q_pos = [max(r.length, 1) - 1 for r in reqs]
            self.lib.attend_batch_plan_window(handles, (ctypes.c_uint32 * B)(*lens), (ctypes.c_uint32 * B)(*q_pos), W, bound, slot[0].data_ptr(), need,
                                              stream.cuda_stream)
            slot[1], slot[2] = bound, ((key, self._epoch), stream.cuda_stream)
            return bound
        need = self.lib.attend_plan_bytes(B)
        if self._plan is None or self._plan.numel() < need:
            self._plan = torch.zeros(need, dtype=torch.uint8, device="cuda")
        self.lib.attend_batch_plan(handles, (ctypes.c_uint32 * B)(*lens), bound, self._plan.data_ptr(), need, stream.cuda_stream)
        self._arg_key = ((key, self._epoch), stream.cuda_stream)
        self._plan_bound = bound
        return bound

    def _prepare_tails(self, req_ids, key, reqs, st):
        """Which sequences of the batch keep a position outside the pool, and their fp16 rows as one tensor per kind: the same for every
        layer of a step, so it is set up once per (batch, epoch) -- by append(), while the host is ahead of the GPU, for the step that
        follows; by the first attend() otherwise."""
        import torch
        akey = (key, self._epoch)
        if self._fold_key == akey:
            return
        B = len(reqs)
        odd = [b for b, r in enumerate(reqs) if r.length & 1]
        self._fold_key, self._fold_n = akey, len(odd)
        self._fold_rows = self._fold_idx = self._fold_k = self._fold_v = None
        if odd:
            with torch.cuda.stream(st):
                if len(odd) != B:
                    self._fold_rows = _device_index(odd)
                    inv = [-1] * B
                    for i, b in enumerate(odd):
                        inv[b] = i
                    self._fold_idx = _device_index(inv)
                if tuple(req_ids[b] for b in odd) == self._tail_ids:
                    self._fold_k, self._fold_v = self._tail_k, self._tail_v                 # [n][layers][heads][dim]
                else:
                    self._fold_k = torch.stack([reqs[b].tail_k for b in odd]).contiguous()
                    self._fold_v = torch.stack([reqs[b].tail_v for b in odd]).contiguous()

    def attend(self, layer: int, req_ids: Sequence[int], q, sm_scale: float, stream=None, window=None):
        """softmax(q.K^T * sm_scale).V of one layer for the batch.  q: [batch][heads][g][dim] fp16 (g query rows per kv
        head, GQA); returns [batch][heads][g][dim] fp32.  Stored positions come straight from the compressed records
        (one launch pair for the batch); the position still waiting for its partner goes along in the same call
        (speckv_ext_attend_planned_tail: folded in by the MXFP4 kernel itself, by one launch inside the call otherwise).
        window=W: a sliding-window (local) layer -- every request's query sees its last W positions, its own included
        (decode_window_range), and the launch walks the window's tiles only."""
        return self.attend_layers(layer, 1, req_ids, q[None], sm_scale, stream, window)[0]

    def attend_layers(self, layer_begin: int, n_layers: int, req_ids: Sequence[int], q, sm_scale: float, stream=None, window=None):
        """The same for n_layers consecutive layers whose query rows exist at once (speckv_ext_attend_planned_layers): q
        [n_layers][batch][heads][g][dim] fp16, returns [n_layers][batch][heads][g][dim] fp32.  One library call; over an MXFP4 pool
        with a batch that fills the chip, one launch.  window=W: the layers are sliding-window layers of that window (attend)."""
        return self._attend_layers_lse(layer_begin, n_layers, req_ids, q, sm_scale, stream, window)[0]

    def _attend_layers_lse(self, layer_begin, n_layers, req_ids, q, sm_scale, stream, window):
        """attend_layers' body: (out, lse [n_layers][batch][heads][g] fp32, the query as the launches read it -- contiguous, the K
        pre-scale applied)"""
        import torch
        W = self._decode_window(window)
        if self.scheme not in FUSED:
            raise ValueError("attend() needs an FP8, INT4 or MXFP4 pool; use block_table() / kv_rows() with the other schemes")
        NL, B, H, G, D = q.shape
        if NL != n_layers:
            raise ValueError("q must be [n_layers][batch][heads][g][dim]")
        key, reqs, _ = self._batch(req_ids)
        if self._kscale is not None:
            q = q * self._kscale[layer_begin:layer_begin + n_layers][:, None, :, None, :]
        q = q.contiguous()
        out = torch.empty((NL, B, H, G, D), dtype=torch.float32, device="cuda")
        lse = torch.empty((NL, B, H, G), dtype=torch.float32, device="cuda")
        # One plan per decode step (speckv_ext_attend_batch_plan: handle look-ups and descriptors once, resident on the
        # device), then launch-only calls (speckv_ext_attend_*_planned*).  The length bound moves in steps of
        # PLAN_BUCKET positions, so a caller that captures its per-layer calls into a HIP graph can replay that graph for
        # PLAN_BUCKET decode steps (plan_step() outside the graph, then the replay).
        akey = (key, self._epoch)
        with self._On(self, stream) as st:
            if W:                                                 # the plan of this window value, kept beside the global one
                if W not in self._wplans or self._wplans[W][2] != (akey, st.cuda_stream):
                    self.plan_step(req_ids, st, W)
                plan, bound = self._wplans[W][0], self._wplans[W][1]
            else:
                if self._arg_key != (akey, st.cuda_stream):
                    self.plan_step(req_ids, st)
                plan, bound = self._plan, self._plan_bound
            self._plan_stream = st
            self._prepare_tails(req_ids, key, reqs, st)
            n_tail = self._fold_n
            rows = self._fold_rows.data_ptr() if n_tail and self._fold_rows is not None else 0
            idx = self._fold_idx.data_ptr() if n_tail and self._fold_idx is not None else 0
            kt = self._fold_k.data_ptr() if n_tail else 0
            vt = self._fold_v.data_ptr() if n_tail else 0
            if n_layers == 1 and not n_tail:
                self.lib.attend_planned(self.scheme, plan.data_ptr(), B, layer_begin, q.data_ptr(), G, bound, sm_scale,
                                        out.data_ptr(), lse.data_ptr(), st.cuda_stream)
            elif n_layers == 1:
                self.lib.attend_planned_tail(self.scheme, plan.data_ptr(), B, layer_begin, q.data_ptr(), G, bound, sm_scale,
                                             out.data_ptr(), lse.data_ptr(), n_tail, rows, idx, kt, vt, self.L * self.H * self.D, st.cuda_stream)
            else:
                self.lib.attend_planned_layers(self.scheme, plan.data_ptr(), B, layer_begin, n_layers, q.data_ptr(), G, bound, sm_scale,
                                               out.data_ptr(), lse.data_ptr(), st.cuda_stream, n_tail, rows, idx, kt, vt, self.L * self.H * self.D)
        return out, lse, q

    # ------------------------------------------------------------------ steps of several positions
    @staticmethod
    def spec_groups(S: int, rows_per_pos: int):
        """How a step of S new positions with rows_per_pos query rows per kv head and position goes through the attention kernels,
        which take at most 16 query rows per kv head in one pass over the records: [(first position, positions)] -- groups of
        16 // rows_per_pos positions, the last one possibly shorter.  One group = one pass; every further group reads the records again."""
        if not 1 <= rows_per_pos <= 16:
            raise ValueError("rows_per_pos must be 1..16 (query rows per kv head of one position)")
        if not 1 <= S <= HELD_MAX - 1:
            raise ValueError(f"a step carries 1..{HELD_MAX - 1} new positions per request")
        per = 16 // rows_per_pos
        return [(j0, min(per, S - j0)) for j0 in range(0, S, per)]

    @staticmethod
    def commit_plan(lengths: Sequence[int], n_accept: Sequence[int]):
        """The pool writes and tails that committing the first n_accept[b] new positions of request b (current length lengths[b])
        comes to -- what that many single append() calls would do.  A source is the index of a new position, or -1 for the odd
        position the request holds already.  Returns (pairs, tails): pairs[p] = [(b, page of the K region of layer 0, source of the
        pair's first position, source of its second)] for the p-th pair of every request that has one; tails = [(b, source)] for the
        requests that end on an odd length (requests with n_accept 0 appear in neither)."""
        pairs, tails = [], []
        for b, (ln, n) in enumerate(zip(lengths, n_accept)):
            if n == 0:
                continue
            held = ([-1] if ln & 1 else []) + list(range(n))           # the positions outside the pool, oldest first
            for p in range(len(held) // 2):
                while len(pairs) <= p:
                    pairs.append([])
                pairs[p].append((b, (ln & ~1) // 2 + p, held[2 * p], held[2 * p + 1]))
            if len(held) & 1:
                tails.append((b, held[-1]))
        return pairs, tails

    @staticmethod
    def _tree_parents(parents, batch):
        """parents as one list per request: [S] is the same tree for every request, [batch][S] one tree each.  Every entry an int in
        -1 .. j-1 (a parent precedes its children), 1 .. SPECKV_HELD_MAX - 1 nodes, the same count for every request."""
        parents = list(parents)
        if parents and not isinstance(parents[0], numbers.Integral):
            trees = [list(p) for p in parents]
            if len(trees) != batch:
                raise ValueError(PARENTS_RULE)
        else:
            trees = [parents] * batch
        S = len(trees[0]) if trees else 0
        for tree in trees:
            if len(tree) != S or not 1 <= S <= HELD_MAX - 1:
                raise ValueError(f"parents: 1..{HELD_MAX - 1} nodes, the same count for every request")
            for j, p in enumerate(tree):
                if not isinstance(p, numbers.Integral) or isinstance(p, bool) or not -1 <= p < j:
                    raise ValueError(f"parents[{j}] = {p!r}: a node's parent is -1 (the committed context) or a node in front of it")
        return [[int(p) for p in tree] for tree in trees]

    @staticmethod
    def tree_masks(parents, base, n_new=None, window=None):
        """The mask words of a step whose S new positions form a tree, as speckv_ext_attend_fold_masked takes them: [batch][S] ints.
        parents: [S], or [batch][S] for one tree per request; parents[j] in -1 .. j-1, -1 = a child of the committed context, nodes in
        an order where a parent precedes its children.  base[b]: the held positions in front of node 0 (a request's odd last position:
        0 or 1), all visible to every node.  Node j's word = the low base[b] bits, and the bits base[b] + a of its ancestors a and of j
        itself.  Nodes >= n_new[b] (a ragged step) are dead: word 0, and so is every node below a dead one.  A chain (parents[j] = j - 1)
        gives (1 << (base + j + 1)) - 1, the rule of speckv_ext_attend_fold_held.
        window (None or 0: none, the words above; W >= 1 as speckv_ext_attend_kv_spec_window takes them): node j of depth d sits at the
        absolute position length + d and sees [length + d + 1 - W, length + d], so its word keeps the bit of ancestor a iff depth(a) >=
        d + 1 - W, its own bit always, and the bit of a held position in front of node 0 iff it lies inside that range -- the odd last
        position, one in front of depth 0, iff d + 2 <= W.  Which nodes are dead does not depend on the window; W >= 17 changes no word
        (no node is deeper than 15).  Pure python, no device."""
        W = SpeckvKVConnector._decode_window(window)
        base = [int(x) for x in base]
        trees = SpeckvKVConnector._tree_parents(parents, len(base))
        if not trees:
            return []
        S = len(trees[0])
        if n_new is None:
            n_new = [S] * len(base)
        n_new = [int(n) for n in n_new]
        if len(n_new) != len(base) or not all(0 <= n <= S for n in n_new):
            raise ValueError("n_new: one count 0..S per request")
        if not all(0 <= x and x + S <= HELD_MAX for x in base):
            raise ValueError(f"base: 0 .. {HELD_MAX} - S held positions in front of the new ones")
        words = []
        for tree, x, n in zip(trees, base, n_new):
            row = []
            for j, p in enumerate(tree):
                up = ((1 << x) - 1) if p < 0 else row[p]                  # what the parent sees (0: the parent is dead)
                row.append(up | 1 << (x + j) if j < n and (p < 0 or up) else 0)
            if W:                                                          # the window, on the finished words: liveness is decided above
                depth = []
                for p in tree:
                    depth.append(0 if p < 0 else depth[p] + 1)
                for j, d in enumerate(depth):
                    keep = sum(1 << t for t in range(x) if d + 1 + (x - t) <= W) | sum(1 << (x + a) for a in range(j + 1) if depth[a] >= d + 1 - W)
                    row[j] &= keep
            words.append(row)
        return words

    @staticmethod
    def spec_window_range(length: int, window):
        """The walk rule of attend_spec(window=W) on a split pool (csrc/spec_window.hpp, speckv_ext_spec_window_range), restated: a
        request of `length` committed positions has stored = length & ~1 of them in the pool; a draft node of depth d sits at length + d
        and sees the absolute positions from lo(d) = max(0, length + d + 1 - W) on.  Returns (begin, rel, n_pages): the launch walks the
        pool from the tile of depth 0's bound, begin = lo(0) & ~31, over n_pages = (stored - begin) / 2 pages (0 where lo(0) >= stored: no
        node sees a pool position), and a row of depth d does not see the leading spec_window_skip(rel, d) positions of that walk; rel =
        length + 1 - W - begin is signed."""
        W = SpeckvKVConnector._decode_window(window)
        if not W:
            raise ValueError("window must be an integer >= 1")
        length = int(length)
        stored = length & ~1
        lo = max(0, length + 1 - W)
        begin = lo & ~31
        return begin, length + 1 - W - begin, (stored - begin) // 2 if lo < stored else 0

    @staticmethod
    def spec_window_skip(rel: int, depth: int):
        """max(0, rel + min(depth, 15)): the leading positions of a request's walk (spec_window_range) that a node of `depth` does not see"""
        return max(0, int(rel) + min(int(depth), 15))

    def _held_rows(self, req_ids, key, reqs, k_new, v_new, layer_begin, n_layers, st):
        """The rows a step holds outside the pool as speckv_ext_attend_fold_held takes them: fp16 [n_layers][batch][1 + S][heads][dim]
        per kind -- the request's odd last position (if any) followed by its new positions -- and the count of positions in front of
        the first new one, int32 [n_layers * batch].  Two torch kernels per kind; the gather indices are per (batch, lengths, S)."""
        import torch
        B, S = k_new.shape[0], k_new.shape[1]
        self._prepare_tails(req_ids, key, reqs, st)                     # the odd positions of the batch as one tensor per kind
        skey = (key, self._epoch, S, n_layers)
        if self._spec_key != skey:
            idx, base, rank = [], [], 0
            for b, r in enumerate(reqs):
                if r.length & 1:
                    idx += [B * S + rank] + [b * S + t for t in range(S)]
                    rank += 1
                else:
                    idx += [b * S + t for t in range(S)] + [b * S + S - 1]      # (the last slot is never visible)
                base.append(r.length & 1)
            self._spec_key, self._spec_idx, self._spec_base = skey, _device_index(idx), _device_index(base * n_layers)
        held = []
        for new, tails in ((k_new, self._fold_k), (v_new, self._fold_v)):
            flat = new[:, :, layer_begin:layer_begin + n_layers].permute(2, 0, 1, 3, 4).reshape(n_layers, B * S, self.H, self.D)
            if self._fold_n:
                flat = torch.cat((flat, tails[:, layer_begin:layer_begin + n_layers].permute(1, 0, 2, 3)), dim=1)
            held.append(flat.index_select(1, self._spec_idx))
        return held[0], held[1], self._spec_base

    def attend_spec(self, layer: int, req_ids: Sequence[int], q, k_new, v_new, sm_scale: float, n_new=None, stream=None, parents=None):
        """One layer of a step that carries S new positions per request -- draft tokens to verify, a chunk of a prompt: query position
        j of a request sees everything the request holds (pool and odd last position) and the new positions 0..j.
        q [batch][S][heads][rows_per_pos][dim] fp16; k_new / v_new [batch][S][layers][heads][dim] fp16, the positions that would follow
        each request's current length; n_new: optional per-request counts <= S of positions that are live (a ragged step).  Returns
        [batch][S][heads][rows_per_pos][dim] fp32; rows of positions >= n_new[b] are unspecified but finite.
        Changes no state: lengths, tails and pool stay as they are -- append_tokens() commits what was accepted.
        The stored positions are read ONCE for up to 16 query rows per kv head: S * rows_per_pos <= 16 is one pass over the records,
        more goes in groups of 16 // rows_per_pos positions (spec_groups) with one pass each.  The held rows are folded in by one launch
        per group (speckv_ext_attend_fold_held).
        parents (see tree_masks): the new positions form a tree instead of a chain -- node j sees what the request holds, its ancestors
        and itself, not its siblings.  The pass over the records is the same; the held rows are folded in by
        speckv_ext_attend_fold_masked, one launch per group, with the group's columns of the step's mask table (a node's ancestors in
        earlier groups are held positions like any other).  Rows of dead nodes (>= n_new[b], or below one) are unspecified but finite."""
        return self.attend_spec_layers(layer, 1, req_ids, q[None], k_new, v_new, sm_scale, n_new, stream, parents)[0]

    def attend_spec_layers(self, layer_begin: int, n_layers: int, req_ids: Sequence[int], q, k_new, v_new, sm_scale: float, n_new=None,
                           stream=None, parents=None):
        """attend_spec for n_layers consecutive layers whose query rows exist at once: q [n_layers][batch][S][heads][rows_per_pos][dim],
        returns the same shape in fp32.  Per group of positions one speckv_ext_attend_planned_layers call and one fold launch over all
        the layers."""
        import torch
        if self.scheme not in FUSED:
            raise ValueError("attend_spec() needs an FP8, INT4 or MXFP4 pool")
        NL, B, S, H, R, D = q.shape
        if NL != n_layers or tuple(k_new.shape) != (B, S, self.L, H, D) or tuple(v_new.shape) != (B, S, self.L, H, D):
            raise ValueError("q must be [n_layers][batch][S][heads][rows_per_pos][dim], k_new / v_new [batch][S][layers][heads][dim]")
        groups = self.spec_groups(S, R)
        if n_new is not None:
            n_new = [int(n) for n in n_new]
            if len(n_new) != B or not all(0 <= n <= S for n in n_new):
                raise ValueError("n_new: one count 0..S per request")
        key, reqs, _ = self._batch(req_ids)
        if self._kscale is not None:
            q = q * self._kscale[layer_begin:layer_begin + n_layers][:, None, None, :, None, :]
            k_new = k_new * self._kscale_inv[None, None]
        out = torch.empty((NL, B, S, H, R, D), dtype=torch.float32, device="cuda")
        akey = (key, self._epoch)
        with self._On(self, stream) as st:
            if self._arg_key != (akey, st.cuda_stream):
                self.plan_step(req_ids, st)
            self._plan_stream = st
            with torch.cuda.stream(st):
                kh, vh, base = self._held_rows(req_ids, key, reqs, k_new, v_new, layer_begin, n_layers, st)
                live = None if n_new is None or parents is not None else _device_index(n_new * NL)
                masks = None if parents is None else self._tree_table(key, reqs, parents, n_new, NL, S)
                for j0, n in groups:
                    g = n * R
                    qg = q[:, :, j0:j0 + n].permute(0, 1, 3, 2, 4, 5).reshape(NL, B, H, g, D).contiguous()
                    og = torch.empty((NL, B, H, g, D), dtype=torch.float32, device="cuda")
                    lse = torch.empty((NL, B, H, g), dtype=torch.float32, device="cuda")
                    if NL == 1:
                        self.lib.attend_planned(self.scheme, self._plan.data_ptr(), B, layer_begin, qg.data_ptr(), g, self._plan_bound, sm_scale,
                                                og.data_ptr(), lse.data_ptr(), st.cuda_stream)
                    else:
                        self.lib.attend_planned_layers(self.scheme, self._plan.data_ptr(), B, layer_begin, NL, qg.data_ptr(), g, self._plan_bound,
                                                       sm_scale, og.data_ptr(), lse.data_ptr(), st.cuda_stream)
                    if masks is not None:
                        self.lib.attend_fold_masked(NL * B, 0, H, g, R, qg.data_ptr(), kh.data_ptr(), vh.data_ptr(), (1 + S) * H * D, H * D,
                                                    masks.data_ptr() + 4 * j0, S, sm_scale, og.data_ptr(), lse.data_ptr(), st.cuda_stream)
                        out[:, :, j0:j0 + n] = og.view(NL, B, H, n, R, D).permute(0, 1, 3, 2, 4, 5)
                        continue
                    d_base = base + j0 if j0 else base
                    d_live = None if live is None else (live - j0).clamp_(0, n)
                    self.lib.attend_fold_held(NL * B, 0, H, g, R, qg.data_ptr(), kh.data_ptr(), vh.data_ptr(), (1 + S) * H * D, H * D,
                                              d_base.data_ptr(), 0 if d_live is None else d_live.data_ptr(), sm_scale, og.data_ptr(),
                                              lse.data_ptr(), st.cuda_stream)
                    out[:, :, j0:j0 + n] = og.view(NL, B, H, n, R, D).permute(0, 1, 3, 2, 4, 5)
        return out

    # ------------------------------------------------------------------ chunks of any length
    @staticmethod
    def chunk_blocks(n_new: Sequence[int], rows_per_pos: int):
        """How a chunk step is cut into the workgroups of speckv_ext_attend_chunk: a query block is 64 // rows_per_pos positions of one
        request (64 query rows per kv head: 16 per wave), request b with n_new[b] live positions has ceil(n_new[b] / that) blocks, none
        for 0.  Returns (counts, firsts): the per-request block counts and their exclusive prefix -- the rule by which the kernel finds
        the request of a flat block index (the last request whose prefix is <= the index; requests without blocks share their
        successor's prefix and are passed over).  Pure python, no device."""
        if not _is_int(rows_per_pos) or rows_per_pos not in (1, 2, 4, 8, 16):
            raise ValueError("rows_per_pos must be 1, 2, 4, 8 or 16 (query rows per kv head of one position)")
        per = 64 // int(rows_per_pos)
        counts, firsts, total = [], [], 0
        for n in n_new:
            if not _is_int(n) or n < 0:
                raise ValueError(f"n_new: counts of positions >= 0, not {n!r}")
            counts.append((int(n) + per - 1) // per)
            firsts.append(total)
            total += counts[-1]
        return counts, firsts

    @staticmethod
    def chunk_pieces(n_new: Sequence[int], stored: Sequence[int], rows_per_pos: int, splits: int = 0, n_cus: int = 256, window=None):
        """How attend_chunk(splits=...) cuts the stored positions of every request into pieces (speckv_ext_chunk_split_plan restated):
        request b with stored[b] positions (its length; an odd last position is held, not stored) has n_pool = ceil((stored[b] & ~1)
        / 32) pool tiles of 32 positions.  splits 1: one piece each.  splits N in 2..64 (forced): min(N, max(1, n_pool)) pieces -- from
        the request alone.  splits 0 (the library's rule, from the whole step): with G0 = 8 x the step's query blocks (chunk_blocks)
        and target = 3 x n_cus, one piece each while G0 > target / 2, otherwise clamp(n_pool // 32, 1, min(target // G0, 64)).
        Then tiles_per_piece = ceil(n_pool / pieces) and pieces = ceil(n_pool / tiles_per_piece), so no piece is empty; piece p walks
        pool tiles [p * tpp, min((p + 1) * tpp, n_pool)) and the last piece also the held positions; a request without pool tiles
        has one piece of 0 tiles.  Returns (pieces, tiles_per_piece, firsts): firsts = the exclusive prefix of blocks x pieces, the
        rule by which the kernel finds (request, block, piece) of a flat work item -- the last request whose prefix is <= the item,
        block = rest // pieces, piece = rest % pieces.  Pure python, no device.
        window (None or 0: none; W >= 1 as attend_chunk(window=W) cuts when some row of the step loses a position): a fourth list is
        returned, first_tiles, and the rule runs over the pool tiles that are LEFT -- first_tiles[b] = the first pool tile position 0
        of the request sees, lo(0) // 32 with lo(0) = max(0, stored[b] + 1 - W), or n_pool where it sees none; n_pool - first_tiles[b]
        takes n_pool's place above.  Piece p then covers pool tiles [first + p * tpp, min(first + (p + 1) * tpp, n_pool)), clipped
        from below by the block's first tile (chunk_window_walk), and the last piece goes on through the held tiles from the later
        of its start and that tile; a piece that is not the last can be empty for later blocks."""
        if not _is_int(splits) or not 0 <= splits <= 64:
            raise ValueError(SPLITS_RULE)
        if not _is_int(n_cus) or n_cus < 0:
            raise ValueError("n_cus: the compute units of the device (0: 256)")
        counts, _ = SpeckvKVConnector.chunk_blocks(n_new, rows_per_pos)
        stored = SpeckvKVConnector._chunk_stored(stored, len(counts))
        most = int(splits)
        if splits == 0:
            g0, target = 8 * sum(counts), 3 * (int(n_cus) or 256)
            most = 1 if g0 == 0 or g0 >= target else min(target // g0, 64)
        window = SpeckvKVConnector._chunk_window(window)
        pieces, tiles, firsts, first_tiles, total = [], [], [], [], 0
        for blocks, s in zip(counts, stored):
            n_pool = ((int(s) & ~1) + 31) // 32
            if window:
                lo = max(0, int(s) + 1 - window)
                first_tiles.append(lo // 32 if lo < (int(s) & ~1) else n_pool)
                n_pool -= first_tiles[-1]
            p = min(max(n_pool // 32 if splits == 0 else n_pool, 1), most)
            tpp = -(-n_pool // p)
            pieces.append(-(-n_pool // tpp) if tpp else 1)
            tiles.append(tpp)
            firsts.append(total)
            total += blocks * pieces[-1]
        if window:
            return pieces, tiles, firsts, first_tiles
        return pieces, tiles, firsts

    @staticmethod
    def _chunk_window(window):
        """window as attend_chunk takes it: None or 0 -> 0 (none), an int >= 1 -> itself; anything else is a ValueError"""
        if window is None:
            return 0
        if not _is_int(window) or not 0 <= window <= 0xFFFFFFFF:
            raise ValueError("window must be None or 0 (no window) or a count of positions >= 1")
        return int(window)

    @staticmethod
    def _chunk_stored(stored, n):
        """stored as chunk_pieces and chunk_window_walk take it, as a list: n counts of positions >= 0; anything else is a ValueError"""
        stored = list(stored)
        if len(stored) != n or not all(_is_int(s) and s >= 0 for s in stored):
            raise ValueError("stored: one count of positions >= 0 per request")
        return stored

    @staticmethod
    def chunk_window_walk(n_new: Sequence[int], stored: Sequence[int], rows_per_pos: int, window):
        """Which tiles attend_chunk(window=W) walks (speckv_ext_chunk_window_walk restated): request b with stored[b] positions (its
        length: pos_end = stored[b] & ~1 of them in the pool, base = stored[b] & 1 held) and n_new[b] new ones has n_pool =
        ceil(pos_end / 32) pool tiles of 32 positions, counted first, then the held tiles (held position t = base + new position).
        Query position j sits at the absolute position P = stored[b] + j and sees [lo(j), P], lo(j) = max(0, P + 1 - W) (W None or
        0: lo = 0).  Query block blk = positions j_first = blk * (64 // rows_per_pos) .. j_last (the last live one of the block)
        walks the tiles [t_first, n_tiles): n_tiles = n_pool + ((base + j_last) >> 5) + 1, t_first = lo(j_first) >> 5 while
        lo(j_first) < pos_end, otherwise n_pool + ((lo(j_first) - pos_end) >> 5) -- exactly the tiles that hold a position a live row
        of the block sees, never more than ceil((W + 64 // rows_per_pos - 1) / 32) + 2.  Returns one list per request of
        (t_first, tile count) per block.  Pure python, no device."""
        window = SpeckvKVConnector._chunk_window(window)
        counts, _ = SpeckvKVConnector.chunk_blocks(n_new, rows_per_pos)
        stored = SpeckvKVConnector._chunk_stored(stored, len(counts))
        per, walks = 64 // int(rows_per_pos), []
        for n, blocks, s in zip(n_new, counts, stored):
            pos_end, base = int(s) & ~1, int(s) & 1
            n_pool, walk = (pos_end + 31) // 32, []
            for blk in range(blocks):
                j_first, j_last = blk * per, min(blk * per + per, int(n)) - 1
                lo = max(0, int(s) + j_first + 1 - window) if window else 0
                t_first = lo >> 5 if lo < pos_end else n_pool + ((lo - pos_end) >> 5)
                walk.append((t_first, n_pool + ((base + j_last) >> 5) + 1 - t_first))
            walks.append(walk)
        return walks

    @staticmethod
    def _chunk_tree_parents(parents, batch):
        """_tree_parents without its bound on the node count: parents as one list per request ([S] is the same tree for every request,
        [batch][S] one tree each), every entry an int in -1 .. j-1, S >= 1 nodes, the same count for every request."""
        parents = list(parents)
        if parents and not isinstance(parents[0], numbers.Integral):
            try:
                trees = [list(p) for p in parents]
            except TypeError:
                raise ValueError("parents: ints, or one list of ints per request") from None
            if len(trees) != batch:
                raise ValueError(PARENTS_RULE)
        else:
            trees = [parents] * batch
        S = len(trees[0]) if trees else 0
        for tree in trees:
            if len(tree) != S or S < 1:
                raise ValueError("parents: at least one node, the same count for every request")
            for j, p in enumerate(tree):
                # spelled out, not _is_int: this runs per node of every tree at every layer's call, where a function call per node shows
                if not isinstance(p, numbers.Integral) or isinstance(p, bool) or not -1 <= p < j:
                    raise ValueError(f"parents[{j}] = {p!r}: a node's parent is -1 (the committed context) or a node in front of it")
        return [[int(p) for p in tree] for tree in trees]

    @staticmethod
    def chunk_tree_depths(parents, batch=1):
        """The depth of every node of a tree step, as speckv_ext_attend_chunk_tree_window takes it: [batch][S] ints, 0 for a child of
        the committed context (parents[j] < 0), otherwise the parent's depth + 1 -- node j of a request of `length` positions sits at
        the absolute position length + depth.  parents [S] (one tree for all `batch` requests) or [batch][S], judged as
        chunk_tree_masks judges them.  Dead nodes have depths like any other.  Pure python, no device."""
        depths = []
        for tree in SpeckvKVConnector._chunk_tree_parents(parents, int(batch)):
            d = []
            for p in tree:
                d.append(0 if p < 0 else d[p] + 1)
            depths.append(d)
        return depths

    @staticmethod
    def chunk_tree_masks(parents, base, n_new=None, window=None):
        """The mask rows of a step whose S new positions form a tree of ANY size, as speckv_ext_attend_chunk_masked takes them:
        [batch][S][W] ints, W = (S + 1 + 31) // 32 words of 32 bits per node.  parents, base, n_new as tree_masks: parents [S] or
        [batch][S] with parents[j] in -1 .. j-1; base[b] in {0, 1}: the request's odd last position, visible to every node.  Bit t of a
        row (bit t & 31 of word t >> 5) = held position t: node j's row = the low base[b] bits, and the bits base[b] + a of its
        ancestors a and of j itself.  Nodes >= n_new[b] and every node below a dead one get all-zero rows (the kernel neither computes
        nor writes them).  For S <= 16 the single word is tree_masks' word; a chain gives (1 << (base + j + 1)) - 1 across the words.
        window (None or 0: none, the rows above; W >= 1 as speckv_ext_attend_chunk_tree_window takes them, the window folded in): node j
        of depth d sits at the absolute position P = length + d and sees [max(0, P + 1 - W), P] on its root path, so its row keeps the
        tail's bit iff d + 2 <= W (the tail is the position in front of depth 0), the bit of ancestor a iff depth(a) > d - W, and its
        own bit always; which rows are dead does not depend on the window.  None of it depends on the request's length.
        Pure python, no device."""
        window = SpeckvKVConnector._chunk_window(window)
        base = [int(x) for x in base]
        trees = SpeckvKVConnector._chunk_tree_parents(parents, len(base))
        if not trees:
            return []
        S = len(trees[0])
        if n_new is None:
            n_new = [S] * len(base)
        n_new = [int(n) for n in n_new]
        if len(n_new) != len(base) or not all(0 <= n <= S for n in n_new):
            raise ValueError("n_new: one count 0..S per request")
        if not all(x in (0, 1) for x in base):
            raise ValueError("base: 0 or 1 held positions in front of the new ones")
        W = (S + 1 + 31) // 32
        rows = []
        for tree, x, n in zip(trees, base, n_new):
            bits = []                                                     # a node's row as one python int
            for j, p in enumerate(tree):
                up = ((1 << x) - 1) if p < 0 else bits[p]                 # what the parent sees (0: the parent is dead)
                bits.append(up | 1 << (x + j) if j < n and (p < 0 or bits[p]) else 0)
            if window:                                                    # a live row keeps itself and W - 1 positions up its path
                depth, cut = [], []
                for j, p in enumerate(tree):
                    depth.append(0 if p < 0 else depth[p] + 1)
                    v, a = 0, j
                    for _ in range(min(depth[j] + 1, window)):
                        v |= 1 << (x + a)
                        a = tree[a]
                    if x and depth[j] + 2 <= window:
                        v |= 1
                    cut.append(v if bits[j] else 0)
                bits = cut
            rows.append([[(v >> (32 * w)) & 0xFFFFFFFF for w in range(W)] for v in bits])
        return rows

    def _chunk_tree_table(self, key, reqs, parents, live, S):
        """The mask rows of a tree chunk step on the device, int32 [batch][S][W] (bit patterns of the uint32 words), kept per (batch,
        epoch, S, tree, live counts) the way _tree_table keeps its words: every layer's call of a step finds the same table."""
        import numpy as np
        import torch
        one = len(parents) > 0 and isinstance(parents[0], numbers.Integral)      # one tree for every request
        tkey = (key, self._epoch, S, tuple(parents) if one else tuple(map(tuple, parents)), tuple(live))
        if self._chunk_tree_key != tkey:
            rows = self.chunk_tree_masks(parents, [r.length & 1 for r in reqs], live)
            if len(rows[0]) != S:
                raise ValueError("parents: one entry per new position")
            words = np.asarray(rows, dtype=np.uint32).view(np.int32)
            self._chunk_tree_key, self._chunk_tree_masks = tkey, torch.from_numpy(words).pin_memory().to("cuda", non_blocking=True)
        return self._chunk_tree_masks

    def _chunk_tree_window_table(self, key, reqs, parents, live, S, window):
        """(mask rows with the window folded in, depths) of a tree step on a local layer on the device, int32 [batch][S][W] and
        [batch][S], kept per (batch, epoch, S, tree, live counts, window) as _chunk_tree_table keeps its rows: one table per window
        value beside the global layers' one, so a model's local and global layers each find theirs at every layer of a step."""
        import numpy as np
        import torch
        one = len(parents) > 0 and isinstance(parents[0], numbers.Integral)
        tkey = (key, self._epoch, S, tuple(parents) if one else tuple(map(tuple, parents)), tuple(live), window)
        held = self._chunk_tree_wtabs.get(window)
        if held is None or held[0] != tkey:
            rows = self.chunk_tree_masks(parents, [r.length & 1 for r in reqs], live, window=window)
            if len(rows[0]) != S:
                raise ValueError("parents: one entry per new position")
            on_device = lambda a: torch.from_numpy(a).pin_memory().to("cuda", non_blocking=True)
            words = np.asarray(rows, dtype=np.uint32).view(np.int32)
            depths = np.asarray(self.chunk_tree_depths(parents, len(reqs)), dtype=np.uint32).view(np.int32)
            if len(self._chunk_tree_wtabs) >= 4:                          # window values of layers long gone
                self._chunk_tree_wtabs.clear()
            held = self._chunk_tree_wtabs[window] = (tkey, on_device(words), on_device(depths))
        return held[1], held[2]

    def attend_tree(self, layer: int, req_ids: Sequence[int], q, k_new, v_new, sm_scale: float, parents, n_new=None, stream=None, splits=1,
                    window=None):
        """The TREE step of one layer, global or local: attend_chunk(parents=...) with a window that goes by a node's DEPTH.  Shapes,
        n_new, splits, stream, the K pre-scale and the result (zeros for dead nodes) are attend_chunk's; `parents` is required.
        window None or 0 (a global layer): exactly attend_chunk(layer, ..., parents=parents, splits=splits) -- the same call, the
        same bits.  window W >= 1 (a local layer): node j of depth d (chunk_tree_depths) sits at the absolute position P = length + d
        and sees the positions [max(0, P + 1 - W), P] ON ITS ROOT PATH: the stored positions from that bound on, the odd last
        position iff d + 2 <= W, ancestor a iff depth(a) > d - W, itself always (W = 1: its own V row).  ONE call
        (speckv_ext_attend_chunk_tree_window): the library bounds the stored positions by the depth table, the held part is the mask
        rows with the window folded in (chunk_tree_masks(window=W)); both tables are built once per (batch, lengths, tree, n_new, W)
        and shared by the layers of a step, next to the global layers' table.  The cost follows W, not the context: every query block
        walks the pool tiles from depth 0's bound on.  A window no node can lose a position under (length + S <= W) runs the
        unwindowed launch, bit for bit.  A chain given as a tree agrees with attend_chunk(window=W) within the error bound, not bit
        for bit.  Afterwards commit(req_ids, k_new, v_new, nodes=accepted path), as for any tree step.  Anything attend_chunk
        refuses is a ValueError here, with its message, before any library call."""
        if not self._chunk_window(window):
            if parents is None:
                raise ValueError("parents: ints, or one list of ints per request")
            return self.attend_chunk(layer, req_ids, q, k_new, v_new, sm_scale, n_new, stream, parents=parents, splits=splits)
        return self._chunk_step(layer, req_ids, q, k_new, v_new, sm_scale, n_new, stream, parents, splits, window, True)

    def attend_chunk(self, layer: int, req_ids: Sequence[int], q, k_new, v_new, sm_scale: float, n_new=None, stream=None, parents=None,
                     splits=1, window=None):
        """One layer of a step that carries a CHUNK of S new positions per request, S >= 1 with no bound but max_tokens -- chunked prefill
        of a long prompt, the differing suffix behind fork(), a prompt continued after truncate().  Shapes and meaning are those of
        attend_spec without `parents`: q [batch][S][heads][rows_per_pos][dim] fp16 (rows_per_pos 1, 2, 4, 8 or 16), k_new / v_new
        [batch][S][layers][heads][dim] fp16, n_new optional per-request counts <= S of live positions; query position j of a request
        sees everything the request holds (pool and odd last position) and the new positions 0..j.  Returns [batch][S][heads]
        [rows_per_pos][dim] fp32; rows of positions >= n_new[b] are zeros.  Changes no state -- commit(nodes=range(n)) or
        append_tokens() stores the chunk afterwards.
        ONE launch (speckv_ext_attend_chunk): a workgroup takes 64 // rows_per_pos positions of one kv head and walks the request's
        records once for them (chunk_blocks), k_new / v_new are read in place through their strides.  The query stays fp16 in every
        pool format (attend() and attend_spec() over FP8 and MXFP4 pools quantise it).
        splits: 1 (the default) = no split over the stored positions: exactly the launch and the bits described above.  0 = the
        library's rule (chunk_pieces): the stored positions of a request are cut into pieces that run side by side, and a second
        launch merges them, whenever the step's query blocks alone would leave most of the chip idle; a step that fills the chip is
        issued as with splits=1, bit for bit.  N in 2..64 forces min(N, pool tiles) pieces per request.  With pieces a row's bits
        depend on its request's piece count (within the same error bound); under 0 that count depends on the whole step, under a
        forced N on the request alone.  Works with and without `parents` (speckv_ext_attend_chunk_split).  Anything else is a
        ValueError before any library call.
        When to use which: few positions, or a tree, over a LONG context -- a fork's short suffix, the last short chunk of a prompt, a
        draft tree of more than 16 nodes -- should pass splits=0: without pieces such a step leaves most of the chip idle.  A chunk
        that fills the chip with query blocks is not split by the rule, so splits=0 costs it nothing.  attend_spec remains the route
        for chains of S <= 16 positions (it quantises the query for FP8 and MXFP4 pools and splits the stored positions itself);
        profiles/tools/chunk_split_bench.py times the routes side by side.
        parents (see chunk_tree_masks): the S new positions form a TREE of drafts of any size instead of a chain -- node j sees what the
        request holds, its ancestors and itself, not its siblings.  Still ONE launch (speckv_ext_attend_chunk_masked) with a mask table
        built once per (batch, lengths, tree, n_new) and shared by the layers' calls; attend_spec(parents=...) stops at 16 nodes and
        reads the records once per 16 // rows_per_pos of them.  Rows of dead nodes (>= n_new[b], or below one) are zeros.  Afterwards
        commit(req_ids, k_new, v_new, nodes=accepted path) stores a root-to-node path of a tree of any size.
        window: None or 0 (the default) = every row sees everything its request holds: the path above, untouched.  An int W >= 1 is
        the call of a LOCAL (sliding-window) layer of a model that interleaves local and global layers: query position j at the
        absolute position P = length + j sees the positions (P - W, P] only -- itself and the W - 1 in front of it, stored, held or
        new (speckv_ext_attend_chunk_window, with `splits` passed through).  It serves prefill chunks and multi-position steps alike,
        and S = 1 is the windowed DECODE step for a request of any length, odd or even -- attend() has no window.  A query block
        walks only the tiles its rows see (chunk_window_walk), so the cost follows W, not the context; a window no row of the step
        loses a position under issues the unwindowed launch, bit for bit.  The query stays fp16 in all pool formats; the K
        pre-scale, the tails and the strides are those of the path above.  Not with `parents` (a node's position in a tree is its
        depth, not its index: attend_tree is the tree step of a local layer): ValueError, as for a bool, a negative or a
        non-integer, before any library call.  Records below a window stay in the pool: nothing is freed."""
        return self._chunk_step(layer, req_ids, q, k_new, v_new, sm_scale, n_new, stream, parents, splits, window, False)

    def _chunk_step(self, layer, req_ids, q, k_new, v_new, sm_scale, n_new, stream, parents, splits, window, by_depth, keep_lse=False):
        """attend_chunk's body; by_depth: attend_tree's call under a window -- `parents` is required and the window goes by depth.
        keep_lse (attend_chunk_shared): the same calls with d_lse given; returns (out, lse [batch][S][heads][rows_per_pos] fp32 with
        -inf where nothing was written, the query as the launch read it)"""
        import numpy as np
        import torch
        window = self._chunk_window(window)
        if window and parents is not None and not by_depth:
            raise ValueError("window does not combine with parents: a windowed layer takes a chain of new positions, not a tree")
        if by_depth and parents is None:
            raise ValueError("parents: ints, or one list of ints per request")
        reqs, live, (S, R), out, lse, some = self._chunk_judge(layer, req_ids, q, k_new, v_new, n_new, splits, parents, keep_lse)
        if not some:
            return (out, lse, q.contiguous()) if keep_lse else out
        key, _, handles = self._batch(req_ids)
        splits, row = int(splits), self.H * self.D
        with self._On(self, stream) as st:
            with torch.cuda.stream(st):
                if self._kscale is not None:
                    q = q * self._kscale[layer][None, None, :, None, :]
                    k_new = k_new * self._kscale_inv[None, None]
                q = q.contiguous()
                k_new, v_new = self._chunk_rows(k_new, v_new)
                self._prepare_tails(req_ids, key, reqs, st)
                tail_idx, rank = tail_index(reqs)
                kt = self._fold_k.data_ptr() + 2 * layer * row if rank else 0
                vt = self._fold_v.data_ptr() + 2 * layer * row if rank else 0
                if window and by_depth:
                    masks, depths = self._chunk_tree_window_table(key, reqs, parents, live, S, window)
                    entry, form = "attend_chunk_tree_window", (masks.data_ptr(), masks.shape[2], depths.data_ptr(), window, splits)
                elif window:
                    entry, form = "attend_chunk_window", (window, splits)
                else:
                    masks = None if parents is None else self._chunk_tree_table(key, reqs, parents, live, S)
                    mask = (0, 0) if masks is None else (masks.data_ptr(), masks.shape[2])
                    if splits != 1:
                        entry, form = "attend_chunk_split", mask + (splits,)
                    else:
                        entry, form = ("attend_chunk", ()) if masks is None else ("attend_chunk_masked", mask)
                # what every entry takes up to the tail stride, the form's own arguments in front of sm_scale, what closes every entry
                getattr(self.lib, entry)(handles, layer, q.data_ptr(), S, R, np.asarray([r.length & ~1 for r in reqs], dtype=np.uint32),
                                         np.asarray(live, dtype=np.uint32), k_new.data_ptr() + 2 * layer * k_new.stride(2),
                                         v_new.data_ptr() + 2 * layer * v_new.stride(2), k_new.stride(0), k_new.stride(1), tail_idx, kt, vt,
                                         self.L * row, *form, sm_scale, out.data_ptr(), lse.data_ptr() if keep_lse else 0, st.cuda_stream)
        return (out, lse, q) if keep_lse else out

    # ------------------------------------------------------------------ a prefix shared by several requests
    # (the bodies are SharedPrefixSteps': what follows is this connector's side of them)
    def _pool_check(self, what):
        if self.scheme not in FUSED:
            raise ValueError(f"{what}() needs an FP8, INT4 or MXFP4 pool")

    def _reqs(self, req_ids):
        return self._batch(req_ids)[1]

    def _prefix_handles(self, prefix_ids):
        import numpy as np
        return (np.asarray([self.requests[p].handle for p in prefix_ids], dtype=np.uint64),)

    def _own_decode(self, layer, req_ids, q, sm_scale, stream, window, gathered):
        import torch
        if gathered and stream is not None:                       # attend's body scales q on torch's current stream: behind the gather
            torch.cuda.current_stream().wait_stream(stream)
        out, lse, qs = self._attend_layers_lse(layer, 1, req_ids, q[None], sm_scale, stream, window)
        return out[0], lse, qs

    def _own_chunk(self, layer, req_ids, q, k_new, v_new, sm_scale, n_new, stream, window, parents, by_depth, **keep_lse):
        return self._chunk_step(layer, req_ids, q, k_new, v_new, sm_scale, n_new, stream, parents, 1, window, by_depth, **keep_lse)

    def _prefix_fold(self, handles, first, layer, req_ids, ahead, d_q, C, R, lens, n_q, depths, W, splits, sm_scale, d_out, d_lse, cuda_stream):
        """own_seen = length + ahead (0: a decode step, whose position is stored already; 1: a chunk step), under a window only"""
        import numpy as np
        if W:
            own = np.asarray([r.length for r in self._reqs(req_ids)], dtype=np.uint32)
            if ahead:
                own += np.uint32(ahead)
            self.lib.attend_prefix_fold_window(*handles, first, layer, d_q, C, R, lens, n_q, own, depths, W, splits, sm_scale, d_out, d_lse, cuda_stream)
        else:
            self.lib.attend_prefix_fold(*handles, first, layer, d_q, C, R, lens, n_q, splits, sm_scale, d_out, d_lse, cuda_stream)

    def _depth_table(self, req_ids, parents, live, S, W):
        key, reqs, _ = self._batch(req_ids)
        return self._chunk_tree_window_table(key, reqs, parents, live, S, W)[1].data_ptr()

    def attend_shared(self, layer: int, req_ids: Sequence[int], prefix_ids: Sequence[Optional[int]], q, sm_scale: float, prefix_lens=None,
                      stream=None, splits=0, window=None):
        """attend() for requests that SHARE A PREFIX without holding a copy of it: parallel samples of one prompt, beams, a system
        prompt in front of many users.  Shapes and result are attend()'s.  The members `req_ids` are ordinary requests that hold only
        what is their own (add_request, append / commit); a prefix is an ordinary request too, and nothing binds them -- the call
        names it: prefix_ids[b] = the request whose first prefix_lens[b] stored positions member b sees in front of its own, or None.
        prefix_lens[b] defaults to the prefix's length, which must then be even (an odd last position is held outside the pool and
        cannot be shared: pass prefix_lens, keeping that position in the member); a given one is even, >= 0 and at most the
        prefix's length rounded down to even.  Members of one prefix may see different lengths of it and need not be adjacent
        (shared_groups; q and the result are permuted only when they are not).
        The step: the members' own attention exactly as attend() issues it (plan, tails, the K pre-scale), with the log-sum-exp kept,
        then ONE speckv_ext_attend_prefix_fold call on the same stream: a workgroup walks a prefix's records ONCE for 64 query rows of
        its members and folds the result into theirs -- the softmax over prefix + own positions.  The prefix part takes the query in
        fp16 in every pool format.  splits: 0 = the library's rule cuts a long prefix of few members across the chip, 1 = never, N =
        forced (attend_chunk).  No member with a prefix (all None, or all lengths 0): attend()'s launches and bits.
        When to use which: fork() + attend() copies the prefix per request and reads it once per request and step; it stays the
        route for a FEW members or a short prefix.  This route reads the prefix once per 64 query rows -- 1/16 of the bytes at 64
        members of 4 query rows -- and stores it once, but the call has a floor of 0.13 ms.  Measured crossover, 64 own positions
        per member (profiles/shared_prefix.txt): the smallest member count from which this route is faster -- prefix 2k:
        256 over an FP8 pool, none up to 256 over INT4 and MXFP4; 8k: 64 over FP8, 256 over INT4 and MXFP4; 32k: 16 over FP8, 64 over
        INT4 and MXFP4.  At 64 members x 8k x 4 query rows it wins over FP8 (0.159 against 0.206 ms) and is 0.02 - 0.03 ms SLOWER
        over INT4 and MXFP4.
        window: None (the default) = a global layer: the step above, untouched.  An int W >= 1 is the call of a LOCAL
        (sliding-window) layer of a model that interleaves local and global layers -- a member holds only its own positions, so
        EVERY layer of such a model goes through this route.  The member's query sees the last W positions of prefix + own, itself
        included: the own step is attend(window=W) exactly as issued without a prefix (the window is relative), and the fold
        (speckv_ext_attend_prefix_fold_window with own_seen = the member's length) sees the prefix positions [max(0, prefix_lens[b]
        + length - W), prefix_lens[b]) and walks only their tiles (prefix_window_walk), so its cost follows W, not the prefix.  A
        member whose window lies wholly in its own part (length >= W) is not touched by the fold: it keeps the bits of
        attend(window=W).  A window that cuts nothing of any prefix issues the unwindowed fold, bit for bit.  Against fork() +
        attend(window=W) this route is about correctness and pool capacity -- the prefix is stored once on every layer -- not speed:
        that route walks only W / 32 tiles per member too (profiles/shared_prefix_window.txt).
        Anything malformed is a ValueError / KeyError before any library call: an unknown prefix, a prefix among the members, lists
        of the wrong length, bools or non-integers, a window that is not None or an int >= 1, a pool that is not FP8 / INT4 /
        MXFP4; a q that is no torch tensor is a TypeError."""
        return self._decode_shared(layer, req_ids, prefix_ids, q, sm_scale, prefix_lens, stream, splits, window)

    def attend_chunk_shared(self, layer: int, req_ids: Sequence[int], prefix_ids: Sequence[Optional[int]], q, k_new, v_new, sm_scale: float,
                            n_new=None, prefix_lens=None, stream=None, splits=0, window=None, parents=None):
        """attend_chunk() for members of a shared prefix: the member's OWN chunk -- a user's differing suffix behind a shared system
        prompt -- attends what the member holds and the chunk causally, as attend_chunk(splits=1) does, and the stored positions
        [0, prefix_lens[b]) of the request prefix_ids[b] in front of both.  Shapes, n_new, the K pre-scale and the result (zeros for
        positions >= n_new[b]) are attend_chunk's; prefix_ids, prefix_lens, splits and what is refused are attend_shared's.  The
        causal chunk route with the log-sum-exp requested, then ONE speckv_ext_attend_prefix_fold call with C = S on the same stream.
        Changes no state: commit(nodes=range(n)) stores the chunk in the MEMBER afterwards.  No member with a prefix: attend_chunk's
        launch and bits.
        window: None = a global layer, the step above.  An int W >= 1 = a LOCAL layer: the own part is attend_chunk(window=W) with
        the log-sum-exp kept, and the fold (speckv_ext_attend_prefix_fold_window, own_seen = length + 1, depth = the position's
        index) lets query position j see the prefix positions [max(0, prefix_lens[b] + length + 1 + j - W), prefix_lens[b]); a
        position whose window lies wholly in the member's own part (length + 1 + j >= W) is not touched by the fold.
        parents (a global layer): the new positions form a draft TREE (attend_chunk(parents=...), chunk_tree_masks) -- the masked
        chunk route with the log-sum-exp kept, then the fold above with n_q = the live nodes: the prefix part has no structure among
        rows, every live node sees all of it.  Afterwards commit(req_ids, k_new, v_new, nodes=accepted path) on the members, as for
        any tree step.  parents together with window is a ValueError, as in attend_chunk: attend_tree_shared is the tree step of a
        local layer."""
        W = self._shared_window(window)
        if W and parents is not None:
            raise ValueError("window does not combine with parents: a windowed layer takes a chain of new positions, not a tree "
                             "(attend_tree_shared is the tree step of a local layer)")
        return self._chunk_shared(layer, req_ids, prefix_ids, q, k_new, v_new, sm_scale, n_new, prefix_lens, stream, splits, window, parents,
                                  False, "attend_chunk_shared")

    def attend_tree_shared(self, layer: int, req_ids: Sequence[int], prefix_ids: Sequence[Optional[int]], q, k_new, v_new, sm_scale: float,
                           parents, n_new=None, prefix_lens=None, stream=None, splits=0, window=None):
        """attend_tree() for members of a shared prefix: the TREE step of one layer, global or local.  Shapes, parents, n_new, the K
        pre-scale and the result (zeros for dead nodes) are attend_tree's; prefix_ids, prefix_lens, splits and what is refused are
        attend_shared's.  window None (a global layer): exactly attend_chunk_shared(parents=parents) -- the same calls, the same
        bits.  window W >= 1 (a local layer): the own part is what attend_tree(window=W) issues, by depth
        (speckv_ext_attend_chunk_tree_window, the log-sum-exp kept), and the fold (speckv_ext_attend_prefix_fold_window, own_seen
        = length + 1) reads the SAME depth table the own call reads -- one table, one tree: node j of depth d sees the prefix
        positions [max(0, prefix_lens[b] + length + 1 + d - W), prefix_lens[b]), and none where its window lies wholly in the
        member's own part.  Afterwards commit(req_ids, k_new, v_new, nodes=accepted path) on the members.  Changes no state."""
        if parents is None:
            raise ValueError("parents: ints, or one list of ints per request")
        return self._chunk_shared(layer, req_ids, prefix_ids, q, k_new, v_new, sm_scale, n_new, prefix_lens, stream, splits, window, parents,
                                  True, "attend_tree_shared")

    def _tree_table(self, key, reqs, parents, n_new, n_layers, S):
        """The mask words of a tree step on the device, int32 [n_layers * batch][S] (every layer the same words), kept per
        (batch, epoch, layers, S, tree, live counts) as the gather indices of _held_rows are: the per-layer calls of a step find them
        there -- the tree is judged (tree_masks) when the words are made, a call that finds them compares two tuples."""
        one = len(parents) > 0 and isinstance(parents[0], numbers.Integral)      # one tree for every request
        tkey = (key, self._epoch, n_layers, S, tuple(parents) if one else tuple(map(tuple, parents)), None if n_new is None else tuple(n_new))
        if self._tree_key != tkey:
            words = self.tree_masks(parents, [r.length & 1 for r in reqs], n_new)
            if len(words[0]) != S:
                raise ValueError("parents: one entry per new position")
            self._tree_key, self._tree_masks = tkey, _device_index([w for row in words for w in row] * n_layers)
        return self._tree_masks

    def append_path(self, req_ids: Sequence[int], k_new, v_new, paths, parents=None, stream=None):
        """Commit, per request, the nodes paths[b] of a tree step's S new positions k_new[b], v_new[b] ([batch][S][layers][heads][dim]
        fp16): a chain from a child of the committed context down to some node, possibly empty -- the accepted path of a speculative
        step.  With parents (see tree_masks) the chain is checked against the tree: parents[path[0]] == -1 and parents[path[i]] ==
        path[i - 1]; without, the nodes must be in range and ascending.  A path that fails raises ValueError before any state changes.
        The path's rows are gathered to the front of a [batch][longest path] tensor on the stream of the writes and go through
        append_tokens with n_accept = len(path): the state that many single append() calls would leave.  Returns what append_tokens
        returns.  commit() leaves the same state with one launch and no gather."""
        import torch
        B, S = k_new.shape[0], k_new.shape[1]
        paths = self._checked_paths(req_ids, k_new, v_new, paths, parents)
        n_accept = [len(path) for path in paths]
        longest = max(n_accept, default=0)
        if longest == 0:
            return []
        with self._On(self, stream) as st:
            with torch.cuda.stream(st):
                idx = _device_index([b * S + (path[t] if t < len(path) else 0) for b, path in enumerate(paths) for t in range(longest)])
                shape = (B, longest, self.L, self.H, self.D)
                k_path = k_new.reshape(B * S, self.L, self.H, self.D).index_select(0, idx).view(shape)
                v_path = v_new.reshape(B * S, self.L, self.H, self.D).index_select(0, idx).view(shape)
        return self.append_tokens(req_ids, k_path, v_path, n_accept, stream)

    def _checked_paths(self, req_ids, k_new, v_new, paths, parents):
        """paths as lists of ints, judged as append_path's docstring says; raises ValueError, changes nothing."""
        B, S = k_new.shape[0], k_new.shape[1]
        paths = [[int(j) for j in path] for path in paths]
        if len(paths) != B or len(req_ids) != B or tuple(v_new.shape) != tuple(k_new.shape) or tuple(k_new.shape[2:]) != (self.L, self.H, self.D):
            raise ValueError("k_new / v_new must be [batch][S][layers][heads][dim], paths one list of nodes per request")
        trees = None
        if parents is not None:
            trees = self._tree_parents(parents, B)
            if len(trees[0]) != S:
                raise ValueError("parents: one entry per new position")
        for b, (rid, path) in enumerate(zip(req_ids, paths)):
            if not all(0 <= j < S for j in path):
                raise ValueError(f"request {rid}: path {path} leaves the step's 0..{S - 1} nodes")
            if trees is not None:
                if any(trees[b][j] != up for j, up in zip(path, [-1] + path)):
                    raise ValueError(f"request {rid}: path {path} is not a chain of parents from the committed context")
            elif any(j <= up for j, up in zip(path[1:], path)):
                raise ValueError(f"request {rid}: path {path} does not ascend")
            if self.requests[rid].length + len(path) > self.T:
                raise ValueError(f"request {rid} is full")
        return paths

    def commit(self, req_ids: Sequence[int], k_new, v_new, nodes, parents=None, stream=None):
        """Commit, per request, the step positions nodes[b] (in order) of the S new positions k_new[b], v_new[b] ([batch][S][layers]
        [heads][dim] fp16) with ONE speckv_ext_write_pairs call for the whole batch: nodes[b] = range(n) is append_tokens(n_accept = n),
        an accepted tree path is append_path -- the same pool records, lengths, tails and early plan, judged as append_path judges
        (ValueError before any state changes).  No page image is built: the encoder reads every pair's two rows where they lie, in
        k_new / v_new and in the tail tensors a pair consumes; the host computes their addresses.  What torch still does: the K
        pre-scale, a contiguous copy of k_new / v_new that are not, and one index_select per kind for the new tails (copies: the
        caller may reuse k_new).  Returns everything the asynchronous launch reads -- the (scaled) k_new, v_new and the consumed tail
        tensors -- for the caller to hold until the stream has passed the writes, as append() returns its sources.
        Large trees: without `parents` there is no bound on S, so the accepted path of a tree verified by attend_chunk(parents=...) is
        committed here as nodes=path (ascending node indices; the caller vouches that they are a chain of the tree).  With `parents`
        the path is checked against the tree and the tree keeps tree_masks' bound of 16 nodes."""
        import numpy as np
        import torch
        B, S = k_new.shape[0], k_new.shape[1]
        nodes = self._checked_paths(req_ids, k_new, v_new, nodes, parents)
        reqs = [self.requests[rid] for rid in req_ids]
        n_accept = [len(path) for path in nodes]
        pairs, tails = self.commit_plan([r.length for r in reqs], n_accept)
        if not pairs and not tails:
            return []
        used = [b for b, (r, n) in enumerate(zip(reqs, n_accept)) if n and r.length & 1]        # requests whose odd position finds its partner
        row_bytes = self.L * self.H * self.D * 2
        keep, tk, tv = [], None, None
        with self._On(self, stream) as st:
            with torch.cuda.stream(st):
                if self._kscale_inv is not None:
                    k_new = k_new * self._kscale_inv[None, None]
                k_new, v_new = k_new.contiguous(), v_new.contiguous()
                keep += [k_new, v_new]
                if tails:
                    it = _device_index([b * S + nodes[b][t] for b, t in tails])
                    tk = k_new.view(B * S, self.L, self.H, self.D).index_select(0, it)
                    tv = v_new.view(B * S, self.L, self.H, self.D).index_select(0, it)
                # addresses of the odd positions that pairs consume: rows of the last append's tail tensors, or per request
                tail_at = np.zeros((B, 2), dtype=np.uint64)
                if used and tuple(req_ids[b] for b in used) == self._tail_ids:
                    keep += [self._tail_k, self._tail_v]
                    at = np.arange(len(used), dtype=np.uint64) * np.uint64(row_bytes)
                    tail_at[used, 0], tail_at[used, 1] = at + np.uint64(self._tail_k.data_ptr()), at + np.uint64(self._tail_v.data_ptr())
                else:
                    for b in used:
                        k, v, row = reqs[b]._tail
                        if not (k.is_contiguous() and v.is_contiguous()):
                            k, v, row = reqs[b].tail_k.contiguous(), reqs[b].tail_v.contiguous(), None
                        keep += [k, v]
                        tail_at[b] = k.data_ptr() + (row or 0) * row_bytes, v.data_ptr() + (row or 0) * row_bytes
            if pairs:
                plan = np.asarray([x for group in pairs for x in group], dtype=np.int64)       # (b, page, source, source) per pair
                b_of, rows = plan[:, 0], np.empty((len(plan), 4), dtype=np.uint64)
                node_of = np.zeros((B, S + 1), dtype=np.int64)                                  # [b][source]; source -1 is the last column, unused
                for b, path in enumerate(nodes):
                    node_of[b, :len(path)] = path
                for half in (0, 1):
                    t = plan[:, 2 + half]
                    new_row = ((b_of * S + node_of[b_of, t]) * row_bytes).astype(np.uint64)
                    rows[:, half] = np.where(t < 0, tail_at[b_of, 0], new_row + np.uint64(k_new.data_ptr()))
                    rows[:, 2 + half] = np.where(t < 0, tail_at[b_of, 1], new_row + np.uint64(v_new.data_ptr()))
                handles = np.asarray([reqs[b].handle for b in b_of], dtype=np.uint64)
                self.lib.write_pairs(handles, plan[:, 1].astype(np.uint64), rows, self.region_pages, self.L, self.H * self.D * 2, st.cuda_stream)
        self._committed(req_ids, reqs, used, tails, tk, tv, n_accept)
        return keep

    # ------------------------------------------------------------------ rollback
    @staticmethod
    def truncate_plan(lengths: Sequence[int], new_lengths: Sequence[int]):
        """What cutting request b from lengths[b] back to new_lengths[b] positions comes to.  Returns (drops, reads): drops = [b] for the
        requests that only let go of the odd position they hold (an even new length below an odd length); reads = [(b, page of the K
        region of layer 0)] for the requests whose new last position new_len - 1 is the first half of a stored pair and has to come
        back out of the pool, page (new_len - 1) // 2 (an odd new length below the length: the position is always a stored one, and it
        replaces whatever the request held).  A request with new_len == length, or with two even lengths, appears in neither.
        ValueError for new_len > length or new_len < 0.  Pure python, no device."""
        drops, reads = [], []
        for b, (ln, new) in enumerate(zip(lengths, new_lengths)):
            ln, new = int(ln), int(new)
            if not 0 <= new <= ln:
                raise ValueError(f"request #{b}: cannot cut {ln} positions to {new}")
            if new == ln:
                continue
            if new & 1:
                reads.append((b, (new - 1) // 2))
            elif ln & 1:
                drops.append(b)
        return drops, reads

    def truncate(self, req_ids: Sequence[int], new_lengths: Sequence[int], stream=None):
        """Roll the requests back to new_lengths[b] <= length positions: afterwards lengths, tails and plan bookkeeping are those of a
        connector that had stopped there.  A request cut to an odd length inside stored pairs gets its new last position back as its
        tail: ONE speckv_ext_read_pairs call for the whole batch decodes that row -- the even half of page (new_len - 1) // 2 -- for
        every layer, K and V, into one [n][layers][heads][dim] tensor pair (the odd halves are not asked for and not read where the
        format keeps them apart).  No other launch; when no request needs a row back, no launch at all.  ValueError (truncate_plan)
        before any state changes.  The allocation keeps its size.

        K pre-scale (set_k_channel_scale): a row read back is what commit() stored, K / scale -- and that is what every tail holds
        (append() and commit() scale k_new before they keep a tail; kv_rows() scales tails and pages back alike).  So the row is
        installed as it comes, and the commit that pairs it with a new position writes it unscaled a second time: nothing here or
        there multiplies it again.  The row has been through the format once; its page is encoded again with its new partner.

        Records beyond the new length stay in the pool as stale bytes, and nothing clears them, because their values are never used:
        the attention kernels of all three families (FP8, INT4_G32, MXFP4) take their range from the plan's pos_end and set the scores
        of positions at or beyond it inside the last 32-position tile to -inf before the softmax -- they have to, a never-written
        position of score 0 would otherwise weigh exp(0 - max) -- and the weight of a masked position is exactly 0.  The held-row folds
        (attend_fold_held / _masked) never touch the pool.  The rewrite of a pair replaces the stale record whole.  Run:
        tests/test_gpu_rollback.py writes rows of 200x / 1000x the magnitude of the kept ones behind the cut and holds attend /
        attend_spec to the float64 reference, in the forms those calls select for small batches of up to 128 positions; the masking
        of the other forms (residue classes, the stream forms of large batches) was read in the source, not run against stale rows.
        One difference to a never-written page remains: a stale V row that is not finite (the caller stored inf or NaN there) times a
        weight of 0 is NaN where zeros gave 0.  A caller that may have committed non-finite rows rewrites or frees before it rolls back."""
        import numpy as np
        import torch
        reqs = [self.requests[rid] for rid in req_ids]
        new_lengths = [int(n) for n in new_lengths]
        if len(new_lengths) != len(reqs):
            raise ValueError("new_lengths: one length per request")
        drops, reads = self.truncate_plan([r.length for r in reqs], new_lengths)
        if all(n == r.length for n, r in zip(new_lengths, reqs)):
            return
        if reads:
            n = len(reads)
            row_bytes = self.L * self.H * self.D * 2
            with self._On(self, stream) as st:
                with torch.cuda.stream(st):
                    tk = torch.empty((n, self.L, self.H, self.D), dtype=torch.float16, device="cuda")
                    tv = torch.empty_like(tk)
                rows = np.zeros((n, 4), dtype=np.uint64)                                         # odd rows: 0 = not wanted
                at = np.arange(n, dtype=np.uint64) * np.uint64(row_bytes)
                rows[:, 0], rows[:, 2] = at + np.uint64(tk.data_ptr()), at + np.uint64(tv.data_ptr())
                handles = np.asarray([reqs[b].handle for b, _ in reads], dtype=np.uint64)
                firsts = np.asarray([page for _, page in reads], dtype=np.uint64)              # _page(0, 0, pos) = pos // 2
                self.lib.read_pairs(handles, firsts, rows, self.region_pages, self.L, self.H * self.D * 2, st.cuda_stream)
        touched = set(drops) | {b for b, _ in reads}
        for b in drops:
            reqs[b].clear_tail()
        for i, (b, _) in enumerate(reads):
            reqs[b].set_tail(tk, tv, i)                                                          # as _committed installs tails
        if reads:
            self._tail_ids, self._tail_k, self._tail_v = tuple(req_ids[b] for b, _ in reads), tk, tv
        elif any(req_ids[b] in self._tail_ids for b in touched):
            self._tail_ids, self._tail_k, self._tail_v = (), None, None
        for r, n in zip(reqs, new_lengths):
            r.length = n
        self._epoch += 1
        self._arg_key = self._fold_key = None                  # the plan names ranges that no longer hold: the next attend plans again
        self._plan_stream = None

    # ------------------------------------------------------------------ fork
    @staticmethod
    def fork_plan(src_lengths: Sequence[int], lengths: Sequence[int]):
        """What starting a request with the first lengths[b] positions of a request of src_lengths[b] positions comes to.  Returns
        (n_pages, tails): n_pages[b] = lengths[b] // 2 stored pairs to copy per (layer, kind) region; tails[b] = None for an even
        length, "held" for an odd length equal to the source's (the source holds that row outside the pool), "read" for an odd
        shorter one (the row is the even half of stored page (length - 1) // 2 of the source).  ValueError for
        lengths[b] > src_lengths[b] or lengths[b] < 0.  Pure python, no device."""
        n_pages, tails = [], []
        for b, (ln, new) in enumerate(zip(src_lengths, lengths)):
            ln, new = int(ln), int(new)
            if not 0 <= new <= ln:
                raise ValueError(f"request #{b}: cannot fork {new} positions out of {ln}")
            n_pages.append(new // 2)
            tails.append(None if not new & 1 else "held" if new == ln else "read")
        return n_pages, tails

    def fork(self, src_ids: Sequence[int], new_ids: Sequence[int], lengths: Optional[Sequence[int]] = None, stream=None):
        """Create the requests new_ids[b], each holding the first lengths[b] (default: all) positions of request src_ids[b]; a source
        may appear several times (parallel sampling, beams).  Afterwards lengths, tails, _epoch and the plan keys are those of
        requests written independently with the same values, and source and fork go their own ways: the counterpart of truncate().

        ONE speckv_ext_copy_runs call for the batch copies the stored records of the lengths[b] // 2 pairs of every (layer, kind)
        region -- records, not values: nothing is decoded, scaled or rounded again, every placement on either side (no call when no
        pair is stored).  An odd length needs its last row as the new request's tail: equal to the source's length, the row is a CLONE
        of the source's tail (never a view: the source stays free to change); shorter, it is the even half of stored page
        (length - 1) // 2, and at most ONE speckv_ext_read_pairs call reads those rows from the SOURCES into one [n][layers][heads][dim]
        tensor pair, as truncate() installs tails.  Tails are pre-scaled K like every tail (set_k_channel_scale): nothing is scaled
        twice.

        KeyError for an existing (or repeated) new id and for an unknown source, ValueError from fork_plan: before any allocation or
        change of state.  If a launch fails the allocations made here are freed again and the sources are untouched.  Returns the
        tensors the launches write, for the caller to hold until the stream has passed them."""
        import contextlib
        import numpy as np
        import torch
        src_ids, new_ids = list(src_ids), list(new_ids)
        if len(src_ids) != len(new_ids):
            raise ValueError("new_ids: one new request per source")
        for i, rid in enumerate(new_ids):
            if rid in self.requests or rid in new_ids[:i]:
                raise KeyError(f"request {rid} already exists")
        srcs = [self.requests[rid] for rid in src_ids]
        lengths = [r.length for r in srcs] if lengths is None else [int(n) for n in lengths]
        if len(lengths) != len(srcs):
            raise ValueError("lengths: one length per request")
        n_pages, tails = self.fork_plan([r.length for r in srcs], lengths)
        if not new_ids:
            return []
        reads = [b for b, t in enumerate(tails) if t == "read"]
        made, keep, tk, tv = [], [], None, None
        try:
            for rid in new_ids:
                self.add_request(rid)
                made.append(rid)
            news = [self.requests[rid] for rid in new_ids]
            if any(n_pages) or reads:
                with self._On(self, stream) as st:
                    if any(n_pages):
                        firsts = np.arange(2 * self.L, dtype=np.uint64) * np.uint64(self.region_pages)       # _page(layer, kind, 0)
                        self.lib.copy_runs(np.asarray([r.handle for r in srcs], dtype=np.uint64), np.asarray([r.handle for r in news], dtype=np.uint64),
                                           np.asarray(n_pages, dtype=np.uint64), firsts, st.cuda_stream)
                    if reads:
                        n = len(reads)
                        row_bytes = self.L * self.H * self.D * 2
                        with torch.cuda.stream(st):
                            tk = torch.empty((n, self.L, self.H, self.D), dtype=torch.float16, device="cuda")
                            tv = torch.empty_like(tk)
                        rows = np.zeros((n, 4), dtype=np.uint64)                                     # odd rows: 0 = not wanted
                        at = np.arange(n, dtype=np.uint64) * np.uint64(row_bytes)
                        rows[:, 0], rows[:, 2] = at + np.uint64(tk.data_ptr()), at + np.uint64(tv.data_ptr())
                        handles = np.asarray([srcs[b].handle for b in reads], dtype=np.uint64)
                        pages = np.asarray([(lengths[b] - 1) // 2 for b in reads], dtype=np.uint64)
                        self.lib.read_pairs(handles, pages, rows, self.region_pages, self.L, self.H * self.D * 2, st.cuda_stream)
                        keep += [tk, tv]
            with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():      # behind what produced the source's tail
                for b, t in enumerate(tails):
                    if t == "held":
                        news[b].set_tail(srcs[b].tail_k.clone(), srcs[b].tail_v.clone())
        except BaseException:
            for rid in made:
                self.free_request(rid)
            raise
        for i, b in enumerate(reads):
            news[b].set_tail(tk, tv, i)
        for r, n in zip(news, lengths):
            r.length = n
        self._epoch += 1
        return keep

    def append_tokens(self, req_ids: Sequence[int], k_new, v_new, n_accept: Sequence[int], stream=None):
        """Commit the first n_accept[b] (0..S) of the S new positions k_new[b], v_new[b] ([batch][S][layers][heads][dim] fp16) of every
        request -- the accepted prefix of a speculative step, or a chunk of a prompt onto a request that has positions already.
        Whole position pairs go to the pool, an odd remainder becomes the tail: the state a run of single append() calls would leave.
        One speckv_ext_write_strided_batch call per pair index over the requests that have that pair (at most S / 2 + 1 launches).
        n_accept[b] = 0 leaves the request untouched.  Returns the sources of the asynchronous writes, as append().
        commit() leaves the same state with one launch and no page images."""
        import torch
        B, S = k_new.shape[0], k_new.shape[1]
        n_accept = [int(n) for n in n_accept]
        reqs = [self.requests[rid] for rid in req_ids]
        if len(reqs) != B or len(n_accept) != B or tuple(v_new.shape) != tuple(k_new.shape) or tuple(k_new.shape[2:]) != (self.L, self.H, self.D):
            raise ValueError("k_new / v_new must be [batch][S][layers][heads][dim], n_accept one count per request")
        for rid, r, n in zip(req_ids, reqs, n_accept):
            if not 0 <= n <= S:
                raise ValueError(f"request {rid}: n_accept {n} outside 0..{S}")
            if r.length + n > self.T:
                raise ValueError(f"request {rid} is full")
        pairs, tails = self.commit_plan([r.length for r in reqs], n_accept)
        if not pairs and not tails:
            return []
        if self._kscale_inv is not None:
            k_new = k_new * self._kscale_inv[None, None]        # [batch][S][layers][heads][dim]
        used = [b for b, (r, n) in enumerate(zip(reqs, n_accept)) if n and r.length & 1]        # requests whose odd position finds its partner
        rank = {b: i for i, b in enumerate(used)}
        src = lambda b, t: B * S + rank[b] if t < 0 else b * S + t                              # row of the flat [new rows | odd positions] tensor
        keep = []
        with self._On(self, stream) as st:
            with torch.cuda.stream(st):                         # (the page images are built ON the stream the writes run on: append())
                kf, vf = k_new.reshape(B * S, self.L, self.H, self.D), v_new.reshape(B * S, self.L, self.H, self.D)
                if used:
                    if tuple(req_ids[b] for b in used) == self._tail_ids:
                        kt, vt = self._tail_k, self._tail_v
                    else:
                        kt = torch.stack([reqs[b].tail_k for b in used]); vt = torch.stack([reqs[b].tail_v for b in used])
                    kf, vf = torch.cat((kf, kt)), torch.cat((vf, vt))
                if pairs:
                    i0 = _device_index([src(b, s0) for group in pairs for b, _, s0, _ in group])
                    i1 = _device_index([src(b, s1) for group in pairs for b, _, _, s1 in group])
                    # page images of all pairs, pair index by pair index: [n][layer][kind][2 positions][heads][dim]
                    pair = torch.stack((torch.stack((kf.index_select(0, i0), kf.index_select(0, i1)), dim=2),
                                        torch.stack((vf.index_select(0, i0), vf.index_select(0, i1)), dim=2)), dim=2).contiguous()
                    keep.append(pair)
                if tails:
                    it = _device_index([src(b, t) for b, t in tails])
                    tk, tv = kf.index_select(0, it), vf.index_select(0, it)                     # copies: the caller may reuse k_new
            if pairs:
                import numpy as np
                step_bytes = pair[0].numel() * 2
                at = pair.data_ptr()
                for group in pairs:
                    if len(group) == 1:
                        self.lib.write_strided(reqs[group[0][0]].handle, group[0][1], self.region_pages, 2 * self.L, at, st.cuda_stream)
                    else:
                        srcs = np.arange(len(group), dtype=np.uint64) * np.uint64(step_bytes) + np.uint64(at)
                        self.lib.write_strided_batch([reqs[b].handle for b, _, _, _ in group], np.asarray([pg for _, pg, _, _ in group], dtype=np.uint64),
                                                     srcs, self.region_pages, 2 * self.L, st.cuda_stream)
                    at += len(group) * step_bytes
        self._committed(req_ids, reqs, used, tails, tk if tails else None, tv if tails else None, n_accept)
        return keep

    def _committed(self, req_ids, reqs, used, tails, tk, tv, n_accept):
        """The writes of a commit are queued: consumed tails go, the new ones (rows of tk / tv) come, lengths grow, and the next
        step's plan is made early.  Shared by append_tokens() and commit()."""
        for b in used:
            reqs[b].clear_tail()
        for i, (b, _) in enumerate(tails):
            reqs[b].set_tail(tk, tv, i)
        self._tail_ids, self._tail_k, self._tail_v = (tuple(req_ids[b] for b, _ in tails), tk, tv) if tails else ((), None, None)
        for r, n in zip(reqs, n_accept):
            r.length += n
        self._epoch += 1
        # the next step's attention plan while the host is ahead of the GPU, best effort, as append() makes it
        st = self._plan_stream
        if st is not None and self._arg_key is not None and self._arg_key[0][0] == tuple(req_ids) and self.scheme in FUSED:
            from .speckv_ctypes import SpeckvError
            try:
                if not self.lib.stream_is_capturing(st.cuda_stream):
                    self.plan_step(req_ids, st)
                    key, robjs, _ = self._batch(req_ids)
                    self._prepare_tails(req_ids, key, robjs, st)
                else:
                    self._arg_key = self._plan_stream = None
            except SpeckvError as e:
                self._arg_key = self._plan_stream = None
                if e.status != -4:                             # SPECKV_ERR_INVAL: the stream refuses the plan now; attend() plans again
                    raise
