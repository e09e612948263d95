"""The split pool ("K8V4"): a request's K rows in an FP8_E4M3 allocation, its V rows in an MXFP4 allocation, one chunk-attention launch
over both (speckv_ext_attend_chunk_kv).

Why: on KV-like data the decode-regime error of the 4-bit pools is K's (kv_accuracy.format_accuracy_cpu: MXFP4 / MXFP4 0.60-0.75, FP8 /
MXFP4 0.19-0.22 relative L2 against 0.13-0.18 for FP8 / FP8), while V in 4 bits costs a flat 0.13-0.14 in every regime.  2048 + 1088
bytes per position pair, layer and kind pair: 2.61 : 1 against fp16, 0.77 of an FP8 pool's bytes.

The engine keeps one scheme and one record stride per allocation, so a request is TWO allocations of T * L * H * D * 2 bytes, each laid
out as L regions of T / 2 pages (set_layout(T, L / 2, H, D, 2): 2 * (L / 2) regions): region l of the K allocation is layer l's K,
region l of the V allocation layer l's V.  Every write, copy and placement path of the library works per allocation unchanged.

  add_request / free_request / length   the two allocations of a request; nothing is bound for prefetch
  write_prefill                         one speckv_ext_write_runs per allocation; an odd last position waits in an fp16 tail
  attend                                one layer of the DECODE step (one new position per request, already held as the tail or stored):
                                        ONE speckv_ext_attend_kv_batch -- the batch kernel over FP8 keys and MXFP4 values, no fp16 tile is
                                        materialised -- and one speckv_ext_attend_fold_tail for the requests with an odd length;
                                        window=W: a sliding-window layer, ONE speckv_ext_attend_kv_batch_window that walks the window only
  attend_chunk                          one layer of a step of S >= 1 new positions per request -- a prefill chunk, a draft chain or tree --
                                        causal, under a window, a tree, a tree under a window, split over the chip (S = 1 works, but a
                                        64-row query block then carries rows_per_pos live rows: attend is the decode route)
  attend_spec                           one layer of a DRAFT step (S new positions per request, a chain or a tree) on the decode kernel: per
                                        group of 16 // rows_per_pos positions ONE speckv_ext_attend_kv_spec -- the stored positions walked
                                        once for up to 16 query rows per kv head, the tail and the new rows folded in inside that launch;
                                        window=W: the step on a sliding-window layer, ONE speckv_ext_attend_kv_spec_window per group
  attend_shared / attend_chunk_shared   attend / attend_chunk for members that SHARE A PREFIX without holding a copy of it: the own part as
                                        those methods issue it with the log-sum-exp kept, then ONE speckv_ext_attend_prefix_fold_kv launch
                                        that reads the prefix's FP8 keys and MXFP4 values once per 64 query rows and folds them in
  commit                                the accepted prefix of a step -- or, nodes=path, the accepted path of a tree step -- into the pool:
                                        one speckv_ext_write_pairs per allocation
  truncate                              roll requests back: ONE speckv_ext_read_pairs_kv brings the new odd last positions back as tails
  fork                                  new requests from positions others hold: ONE speckv_ext_copy_runs_kv copies the stored records of
                                        both allocations, at most ONE speckv_ext_read_pairs_kv reads the tails of odd shorter lengths
  kv_rows                               the stored rows of one layer and kind as fp16: one speckv_ext_fetch_range on the K or the V allocation
  load_paged / store_paged              positions between the pool and per-layer paged caches ([2, blocks, block_size, 8, 128], fp16 or
                                        bf16: vLLM's blocks), ONE speckv_ext_read_slots_kv / _write_slots_kv launch over both allocations
                                        and every layer; odd edges (a tail, a seam between two calls) travel as held rows

The bodies of attend_shared and attend_chunk_shared, the judgement of their lists (_shared_args, _shared_judge) and the judging half
of attend_chunk (_chunk_judge, _chunk_rows) are SharedPrefixSteps' (kv_shared.py), the same code SpeckvKVConnector runs; what is this
class's own there is the (K, V) handle arrays of a prefix, its decode and chunk step, the fold entry and the depth table.

Not in this class: the planned and captured decode route (plan_step, HIP graphs: attend stages its descriptors
per call), attend_spec over a shared prefix or for several layers at once, begin_step and
the K pre-scale (load_paged / store_paged have none either); the vLLM adapter builds a SpeckvKVConnector; a shared prefix is one
level deep and one layer per call."""
from typing import Dict, Optional, Sequence

from . import kv_connector as _kc
from .kv_connector import SpeckvKVConnector
from .kv_shared import SharedPrefixSteps, _is_int, paged_cache_geometry, tail_index
from .speckv_ctypes import SpeckvLib

K_SCHEME, V_SCHEME = 4, 5                # SPECKV_COMP_FP8_E4M3, SPECKV_COMP_MXFP4


class _SplitRequest:
    """the two handles, the length, and the fp16 K / V rows of an odd last position ([layers][heads][dim] each, contiguous)"""
    __slots__ = ("k_handle", "v_handle", "length", "tail_k", "tail_v")

    def __init__(self, k_handle, v_handle):
        self.k_handle, self.v_handle, self.length, self.tail_k, self.tail_v = k_handle, v_handle, 0, None, None


class SpeckvSplitKVConnector(SharedPrefixSteps):
    _On = SpeckvKVConnector._On          # the stream rule of the connector: torch's NULL stream goes through a side stream
    chunk_blocks = staticmethod(SpeckvKVConnector.chunk_blocks)
    _chunk_tree_parents = staticmethod(SpeckvKVConnector._chunk_tree_parents)
    _tree_parents = staticmethod(SpeckvKVConnector._tree_parents)       # (what _checked_paths judges commit(nodes=..., parents=...) with)

    def __init__(self, lib: SpeckvLib, num_layers: int, num_kv_heads: int = 8, head_dim: int = 128, max_tokens: int = 4096):
        if num_kv_heads * head_dim * 2 != 2048:
            raise ValueError("the page-wise layout needs num_kv_heads * head_dim == 1024 fp16 elements per position "
                             "(8 kv heads x 128: Llama-3 8B / 70B)")
        if max_tokens % 32:
            raise ValueError("max_tokens must be a multiple of 32 (tile size of the fused attention)")
        if not _is_int(num_layers) or num_layers < 2 or num_layers % 2:
            raise ValueError("num_layers must be even: an allocation's layout counts (K, V) region pairs, and a single-kind allocation "
                             "holds num_layers / 2 of them")
        self.lib = lib
        self.L, self.H, self.D, self.T = int(num_layers), num_kv_heads, head_dim, max_tokens
        self.requests: Dict[int, _SplitRequest] = {}
        self.region_pages = max_tokens // 2                   # pages of one layer's region, in either allocation
        self._side = None
        self._epoch = 0                                       # moves with every length: what a step derives from (batch, lengths) is keyed by it
        self._tails = (None, None, None, None)                # key, tail_idx, K rows, V rows of the step's requests with an odd length
        self._tree = (None, None, None)                       # key, mask rows, depths of the step's tree
        self._fold = (None,)                                  # attend: key, then what a step's calls share -- the count and device indices of the
                                                              # requests with an odd length, the handle arrays, the stored lengths,
                                                              # the query positions (attend under a window)
        self._spec = (None,)                                  # attend_spec: key, then the step's mask words and gather index on the device, the
                                                              # handle arrays and the stored lengths
        self._shared_key, self._shared_plan = None, None      # attend_shared / attend_chunk_shared: the judged call of a step (_shared_args)

    # ------------------------------------------------------------------ requests
    def add_request(self, req_id: int):
        """-> (K handle, V handle)"""
        if req_id in self.requests:
            raise KeyError(f"request {req_id} already exists")
        handles = []
        for scheme in (K_SCHEME, V_SCHEME):
            self.lib.set_compression_scheme(scheme)
            h = self.lib.alloc(self.T * self.L * self.H * self.D * 2)
            self.lib.set_layout(h, self.T, self.L // 2, self.H, self.D, 2)
            handles.append(h)
        self.requests[req_id] = _SplitRequest(*handles)
        self._epoch += 1
        return tuple(handles)

    def free_request(self, req_id: int):
        r = self.requests.pop(req_id)
        self._epoch += 1
        self._tails = (None, None, None, None)
        self.lib.free(r.k_handle)
        self.lib.free(r.v_handle)

    def length(self, req_id: int) -> int:
        return self.requests[req_id].length

    def _page(self, layer: int, pos: int) -> int:
        """the page of (layer, position) in either allocation"""
        return layer * self.region_pages + pos // 2

    # ------------------------------------------------------------------ writes
    def write_prefill(self, req_id: int, k, v, stream=None):
        """k, v: [layers][tokens][heads][dim] fp16 CUDA tensors of the prompt.  One asynchronous speckv_ext_write_runs per allocation (the
        layers' regions are page runs, read in place from k and from v); returns the tensors the launches read -- hold them until the
        stream has passed them."""
        r = self.requests[req_id]
        n = k.shape[1]
        if r.length:
            raise ValueError("write_prefill on a request that already has positions")
        if tuple(k.shape) != (self.L, n, self.H, self.D) or tuple(v.shape) != tuple(k.shape) or n > self.T:
            raise ValueError("k, v must be [layers][tokens][heads][dim], tokens <= max_tokens")
        even = n & ~1
        k = k.contiguous(); v = v.contiguous()
        if even:
            layer_bytes = n * self.H * self.D * 2
            firsts = [self._page(layer, 0) for layer in range(self.L)]
            with self._On(self, stream) as st:
                for handle, t in ((r.k_handle, k), (r.v_handle, v)):
                    self.lib.write_runs(handle, firsts, [t.data_ptr() + layer * layer_bytes for layer in range(self.L)], even // 2, st.cuda_stream)
        if n & 1:
            r.tail_k, r.tail_v = k[:, n - 1].contiguous().clone(), v[:, n - 1].contiguous().clone()
        r.length = n
        self._epoch += 1
        return [k, v]

    # ------------------------------------------------------------------ rows and paged caches (vLLM's blocks)
    def kv_rows(self, req_id: int, layer: int, kind: int, pos_begin: int = 0, pos_end: Optional[int] = None):
        """The stored rows [pos_begin, pos_end) of one layer (default: all of them) and kind (0 K, 1 V) as an fp16 tensor
        [positions][heads][dim], tail included; the contract of SpeckvKVConnector.kv_rows.  ONE speckv_ext_fetch_range on the K or
        the V allocation over the pages that hold the rows: the E4M3 values times their block scale, or the fp16 values of the MXFP4
        records."""
        import torch
        r = self.requests[req_id]
        pos_end = r.length if pos_end is None else pos_end
        if not 0 <= pos_begin <= pos_end <= r.length:
            raise ValueError(f"rows [{pos_begin}, {pos_end}) of a request with {r.length} positions")
        if kind not in (0, 1) or not 0 <= layer < self.L:
            raise ValueError(f"layer {layer} / kind {kind} outside 0..{self.L - 1} / 0..1")
        even = r.length & ~1
        lo, hi = pos_begin & ~1, min((pos_end + 1) & ~1, even)          # whole pages (2 positions each) of the stored part
        out = torch.empty((max(hi, pos_end) - lo, self.H, self.D), dtype=torch.float16, device="cuda")
        if hi > lo:
            with self._On(self, None) as st:
                self.lib.fetch_range(r.v_handle if kind else r.k_handle, self._page(layer, lo), (hi - lo) // 2, out.data_ptr(), False,
                                     st.cuda_stream)
        if pos_end > even:                                               # the odd last position lives in the tail
            out[even - lo] = (r.tail_v if kind else r.tail_k)[layer]
        return out[pos_begin - lo:pos_end - lo]

    @staticmethod
    def paged_plan(lengths: Sequence[int], firsts: Optional[Sequence[int]], counts: Sequence[int]):
        """The pure part of load_paged (firsts given) and store_paged (firsts=None: every span starts at its request's length): per
        span (first_token, n_tokens, slot_begin, held_in, held_out) as the one library call takes them.  slot_begin = the counts in
        front.  Read: held_in exactly when the span is not empty and ends on the request's odd last position -- that row lives in the
        tail, not in a page; never held_out.  Write: held_in exactly when a non-empty span starts on an odd stored boundary (the tail
        completes its first pair), held_out exactly when it is not empty and the new length is odd (the new tail); an empty span
        names the even position below its request's length, so that nothing of it is odd.  Raises ValueError for a span outside its
        request (read) or malformed counts; no connector state."""
        lengths, counts = [int(n) for n in lengths], [int(c) for c in counts]
        write = firsts is None
        firsts = lengths if write else [int(f) for f in firsts]
        if len(counts) != len(lengths) or len(firsts) != len(lengths):
            raise ValueError("paged_plan: one first position and one count per request")
        plan, at = [], 0
        for n, f, c in zip(lengths, firsts, counts):
            if c < 0 or n < 0 or f < 0 or (not write and f + c > n):
                raise ValueError(f"rows [{f}, {f} + {c}) of a request with {n} positions")
            if write:
                plan.append((f if c else f & ~1, c, at, bool(c and f & 1), bool(c and (f + c) & 1)))
            else:
                plan.append((f, c, at, bool(c and n & 1 and f + c == n), False))
            at += c
        return plan

    def _paged_call(self, what, req_ids, counts, slot_mapping, caches):
        """the judging both paged methods share -> (requests, counts, (slots per cache, kind stride, element type))"""
        import torch
        reqs = [self.requests[rid] for rid in req_ids]
        counts = [int(c) for c in counts]
        if len(counts) != len(reqs) or any(c < 0 for c in counts):
            raise ValueError(f"{what}: one non-negative count per request")
        if not isinstance(slot_mapping, torch.Tensor) or slot_mapping.dtype != torch.int64 or slot_mapping.dim() != 1 \
                or not slot_mapping.is_contiguous() or slot_mapping.numel() != sum(counts):
            raise ValueError(f"{what}: slot_mapping must be one contiguous int64 device tensor, the spans concatenated")
        geo, wrong = paged_cache_geometry(caches, self.L, bf16=True)
        if geo is None:                                               # no row route behind this class: the refusal names the cause
            raise ValueError(f"{what}: {wrong}")
        return reqs, counts, geo

    @staticmethod
    def _held_pair(r):
        """(K address, V address, the tensors) of a request's tail as a held row: fp16, contiguous, 16-byte aligned"""
        ok = lambda t: t.is_contiguous() and t.data_ptr() % 16 == 0
        if not (ok(r.tail_k) and ok(r.tail_v)):
            r.tail_k, r.tail_v = r.tail_k.contiguous().clone(), r.tail_v.contiguous().clone()
        return r.tail_k.data_ptr(), r.tail_v.data_ptr(), [r.tail_k, r.tail_v]

    def load_paged(self, req_ids: Sequence[int], firsts: Sequence[int], counts: Sequence[int], slot_mapping, caches, stream=None):
        """Pool -> paged caches; the contract of SpeckvKVConnector.load_paged(fused=True) over the split pool.  Positions [firsts[i],
        firsts[i] + counts[i]) of request req_ids[i] go into the slots slot_mapping[b_i : b_i + counts[i]] (b_i = the counts in front:
        ONE int64 device tensor for the call) of `caches`, per layer a [2, blocks, block_size, 8, 128] fp16 or bf16 tensor: the K
        plane from the request's FP8_E4M3 allocation, the V plane from its MXFP4 allocation -- the bits of kv_rows, for bf16 caches
        each rounded once.  Exactly ONE speckv_ext_read_slots_kv call for all requests, layers and both kinds; a span that ends on a
        request's odd last position hands tail_k / tail_v over as the held row.  A slot < 0 or beyond the cache is skipped.  Nothing
        is launched when every count is 0.  Changes no state.
        There is no other route in this class: caches of another geometry (paged_cache_geometry, kv_shared.py) are a ValueError that
        names what was wrong; what the library refuses passes through as SpeckvError."""
        import numpy as np
        reqs, counts, (n_slots, kind_stride, elem) = self._paged_call("load_paged", req_ids, counts, slot_mapping, caches)
        if len(firsts) != len(reqs):
            raise ValueError("load_paged: one first position per request")
        plan = self.paged_plan([r.length for r in reqs], firsts, counts)
        if not any(counts):
            return
        held, any_held = np.zeros(2 * len(reqs), dtype=np.uint64), False
        for i, (r, (_, _, _, h_in, _)) in enumerate(zip(reqs, plan)):
            if h_in:
                held[2 * i], held[2 * i + 1], _ = self._held_pair(r)
                any_held = True
        with self._On(self, stream) as st:
            self.lib.read_slots_kv(np.asarray([r.k_handle for r in reqs], dtype=np.uint64), np.asarray([r.v_handle for r in reqs], dtype=np.uint64),
                                   np.asarray([p[0] for p in plan], dtype=np.uint64), np.asarray([p[1] for p in plan], dtype=np.uint64),
                                   np.asarray([p[2] for p in plan], dtype=np.uint64), slot_mapping.data_ptr(), n_slots,
                                   np.asarray([c.data_ptr() for c in caches], dtype=np.uint64), 0, kind_stride, self.region_pages, st.cuda_stream,
                                   elem=elem, held_in=held if any_held else None, held_stride=self.H * self.D * 2)

    def store_paged(self, req_ids: Sequence[int], counts: Sequence[int], slot_mapping, caches, stream=None):
        """Paged caches -> pool; the contract of SpeckvKVConnector.store_paged(fused=True) over the split pool.  Request req_ids[i]
        gets counts[i] more positions, read from the slots slot_mapping[b_i : b_i + counts[i]] of `caches` (as load_paged): the K
        plane's rows are encoded as FP8_E4M3 into its K allocation, the V plane's as MXFP4 into its V allocation -- from bf16 caches
        the records of row.to(float16).  Exactly ONE speckv_ext_write_slots_kv call.  A request of odd length gives its tail as the
        held row that completes its pair; a new odd last position comes back through held rows -- one [tails][layers][heads][dim]
        fp16 tensor per kind for the call, row j becoming that request's tail_k / tail_v.  Lengths and the step bookkeeping move as
        in write_prefill.  A slot < 0 or beyond the cache is stored as a row of zeros.  Returns the tensors the launch reads (the
        held-in tails): hold them until the stream has passed the call; the caches and the mapping stay unchanged until then too.
        A request named twice, length + count > max_tokens, a malformed slot_mapping or caches of another geometry raise ValueError
        before any state changes."""
        import numpy as np
        import torch
        reqs, counts, (n_slots, kind_stride, elem) = self._paged_call("store_paged", req_ids, counts, slot_mapping, caches)
        if len(set(req_ids)) != len(reqs):
            raise ValueError("store_paged: a request named twice")
        for r, c in zip(reqs, counts):
            if r.length + c > self.T:
                raise ValueError(f"{r.length} + {c} positions in a request built for {self.T}")
        plan = self.paged_plan([r.length for r in reqs], None, counts)
        if not any(counts):
            return []
        n = len(reqs)
        h_in, h_out, read = np.zeros(2 * n, dtype=np.uint64), np.zeros(2 * n, dtype=np.uint64), []
        tails = [i for i, p in enumerate(plan) if p[4]]
        for i, (r, p) in enumerate(zip(reqs, plan)):
            if p[3]:
                h_in[2 * i], h_in[2 * i + 1], keep = self._held_pair(r)
                read += keep
        with self._On(self, stream) as st:
            tk = tv = None
            if tails:
                with torch.cuda.stream(st):
                    tk = torch.empty((len(tails), self.L, self.H, self.D), dtype=torch.float16, device=slot_mapping.device)
                    tv = torch.empty_like(tk)
                row = tk[0].numel() * 2
                for j, i in enumerate(tails):
                    h_out[2 * i], h_out[2 * i + 1] = tk.data_ptr() + j * row, tv.data_ptr() + j * row
            self.lib.write_slots_kv(np.asarray([r.k_handle for r in reqs], dtype=np.uint64), np.asarray([r.v_handle for r in reqs], dtype=np.uint64),
                                    np.asarray([p[0] for p in plan], dtype=np.uint64), np.asarray([p[1] for p in plan], dtype=np.uint64),
                                    np.asarray([p[2] for p in plan], dtype=np.uint64), slot_mapping.data_ptr(), n_slots,
                                    np.asarray([c.data_ptr() for c in caches], dtype=np.uint64), 0, kind_stride, self.region_pages, st.cuda_stream,
                                    elem=elem, held_in=h_in if read else None, held_stride=self.H * self.D * 2,
                                    held_out=h_out if tails else None)
        for r, c in zip(reqs, counts):
            if c:
                r.tail_k = r.tail_v = None
                r.length += c
        for j, i in enumerate(tails):
            reqs[i].tail_k, reqs[i].tail_v = tk[j], tv[j]
        self._epoch += 1
        return read

    # ------------------------------------------------------------------ attention
    def _step_tails(self, req_ids, reqs):
        """(tail_idx int32 [batch], K rows, V rows [n][layers][heads][dim] or None) of the requests with an odd length, once per step"""
        import torch
        key = (tuple(req_ids), self._epoch)
        if self._tails[0] != key:
            tail_idx, _ = tail_index(reqs)
            odd = [r for r in reqs if r.length & 1]
            tk = torch.stack([r.tail_k for r in odd]).contiguous() if odd else None
            tv = torch.stack([r.tail_v for r in odd]).contiguous() if odd else None
            self._tails = (key, tail_idx, tk, tv)
        return self._tails[1:]

    def _step_tree(self, req_ids, reqs, parents, live, S, window):
        """(mask rows int32 [batch][S][W], depths int32 [batch][S] or None) of a tree step on the device, once per (batch, lengths, tree,
        live counts, window): the static helpers of SpeckvKVConnector build both, the window folded into the rows"""
        import numbers
        import numpy as np
        import torch
        one = len(parents) > 0 and isinstance(parents[0], numbers.Integral)
        key = (tuple(req_ids), self._epoch, S, tuple(parents) if one else tuple(map(tuple, parents)), tuple(live), window)
        if self._tree[0] != key:
            rows = SpeckvKVConnector.chunk_tree_masks(parents, [r.length & 1 for r in reqs], live, window=window or None)
            on_device = lambda a: torch.from_numpy(a).pin_memory().to("cuda", non_blocking=True)
            masks = on_device(np.asarray(rows, dtype=np.uint32).view(np.int32))
            depths = None
            if window:
                depths = on_device(np.asarray(SpeckvKVConnector.chunk_tree_depths(parents, len(reqs)), dtype=np.uint32).view(np.int32))
            self._tree = (key, masks, depths)
        return self._tree[1:]

    def attend(self, layer: int, req_ids: Sequence[int], q, sm_scale: float, stream=None, window=None):
        """softmax(q.K^T * sm_scale).V of one layer for the batch over everything the requests hold -- the decode step.  q
        [batch][heads][g][dim] fp16 (g = 1..16 query rows per kv head, GQA); returns [batch][heads][g][dim] fp32, shapes as
        SpeckvKVConnector.attend.  Changes no state.
        window=W >= 1: a sliding-window (local) layer -- a request of `length` positions (the step's own included) attends the last
        W of them, its query at length - 1.  ONE speckv_ext_attend_kv_batch_window call in place of the batch call below: every request
        is walked from its window's tile in both allocations (SpeckvKVConnector.decode_window_range), ceil((W + 31) / 32) tiles at most
        whatever its context; the tail is always inside the window and is folded as without one.  window=None / 0: today's call.
        ONE speckv_ext_attend_kv_batch call (with a log-sum-exp buffer) over the stored positions, then -- only if some request has an
        odd length -- ONE speckv_ext_attend_fold_tail call that folds the fp16 tails into the rows of those requests.  The query enters
        the stored part as E4M3 x a row scale (the FP8 batch kernel's quantisation), the stored K as its E4M3 values with the block
        scale on the score, the stored V as the fp16 values of its MXFP4 records; the tail is folded with the fp16 query.
        The library serves allocations whose records lie in one run (an engine with one pool); for a striped or migrated placement it
        refuses with SpeckvError (status -4, SPECKV_ERR_INVAL) and the error passes through: there is no silent fall-back -- such
        a caller goes through attend_chunk with the step's new rows."""
        return self._attend_own(layer, req_ids, q, sm_scale, stream, window)[0]

    def _attend_own(self, layer, req_ids, q, sm_scale, stream, window):
        """attend's body: -> (out, lse [batch][heads][g] fp32 -- -inf for a request that holds nothing --, the query as the launches
        read it); attend_shared folds the prefix part into the first two"""
        import numpy as np
        import torch
        W = SpeckvKVConnector._decode_window(window)
        if len(q.shape) != 4:
            raise ValueError("q must be [batch][heads][g][dim]")
        B, H, G, D = (int(x) for x in q.shape)
        if (H, D) != (self.H, self.D) or B != len(req_ids) or not 1 <= G <= 16:
            raise ValueError("q must be [batch][heads][g][dim] with g = 1..16 and one row block per request")
        if not 0 <= layer < self.L:
            raise ValueError(f"layer {layer} outside 0..{self.L - 1}")
        reqs = [self.requests[r] for r in req_ids]
        out = torch.empty((B, H, G, D), dtype=torch.float32, device="cuda")
        lse = torch.empty((B, H, G), dtype=torch.float32, device="cuda")
        row = self.H * self.D
        with self._On(self, stream) as st:
            with torch.cuda.stream(st):
                q = q.contiguous()
                _, tk, tv = self._step_tails(req_ids, reqs)
                key = (tuple(req_ids), self._epoch)
                if self._fold[0] != key:          # once per step: the same for every layer (the host's share of a 256-request call counts)
                    odd = [b for b, r in enumerate(reqs) if r.length & 1]
                    self._fold = (key, len(odd), _kc._device_index(odd) if odd else None,
                                  np.asarray([r.k_handle for r in reqs], dtype=np.uint64), np.asarray([r.v_handle for r in reqs], dtype=np.uint64),
                                  np.asarray([r.length & ~1 for r in reqs], dtype=np.uint32),
                                  np.asarray([max(r.length, 1) - 1 for r in reqs], dtype=np.uint32))
                _, n_odd, rows, k_handles, v_handles, pos_end, q_pos = self._fold
            if W:
                self.lib.attend_kv_batch_window(k_handles, v_handles, layer, q.data_ptr(), G, pos_end, q_pos, W, sm_scale, out.data_ptr(),
                                                lse.data_ptr(), st.cuda_stream)
            else:
                self.lib.attend_kv_batch(k_handles, v_handles, layer, q.data_ptr(), G, pos_end, sm_scale, out.data_ptr(), lse.data_ptr(), st.cuda_stream)
            if n_odd:
                self.lib.attend_fold_tail(n_odd, rows.data_ptr(), self.H, G, q.data_ptr(), tk.data_ptr() + 2 * layer * row,
                                          tv.data_ptr() + 2 * layer * row, self.L * row, sm_scale, out.data_ptr(), lse.data_ptr(), st.cuda_stream)
        return out, lse, q

    def attend_chunk(self, layer: int, req_ids: Sequence[int], q, k_new, v_new, sm_scale: float, n_new=None, stream=None, splits=1,
                     window=None, parents=None):
        """One layer of a step of S >= 1 new positions per request over the split pool; conventions as SpeckvKVConnector.attend_chunk:
        q [batch][S][heads][rows_per_pos][dim] fp16 (rows_per_pos 1, 2, 4, 8 or 16), k_new / v_new [batch][S][layers][heads][dim] fp16,
        n_new optional counts <= S of live positions; returns [batch][S][heads][rows_per_pos][dim] fp32, zeros for rows that are not
        live.  Changes no state -- commit() stores the accepted prefix afterwards.  S = 1 is the decode step.
        ONE library call (speckv_ext_attend_chunk_kv) in every form: splits as attend_chunk (1 none, 0 the library's rule, N forced
        pieces); window W >= 1 a sliding-window layer; parents a tree of drafts (chunk_tree_masks); window together with parents goes by
        a node's DEPTH, as SpeckvKVConnector.attend_tree.  The stored K enters as its E4M3 values with the block scale on the score, the
        stored V as the fp16 values of its MXFP4 records, the query stays fp16."""
        return self._chunk_own(layer, req_ids, q, k_new, v_new, sm_scale, n_new, stream, splits, window, parents)

    def _chunk_own(self, layer, req_ids, q, k_new, v_new, sm_scale, n_new, stream, splits, window, parents, keep_lse=False):
        """attend_chunk's body.  keep_lse (attend_chunk_shared): the same call with d_lse given; returns (out, lse
        [batch][S][heads][rows_per_pos] fp32 with -inf where nothing was written, the query as the launch read it)"""
        import numpy as np
        import torch
        window = SpeckvKVConnector._chunk_window(window)
        reqs, live, (S, R), out, lse, some = self._chunk_judge(layer, req_ids, q, k_new, v_new, n_new, splits, parents, keep_lse)
        if not some:
            return (out, lse, q.contiguous()) if keep_lse else out
        row = self.H * self.D
        with self._On(self, stream) as st:
            with torch.cuda.stream(st):
                q = q.contiguous()
                k_new, v_new = self._chunk_rows(k_new, v_new)
                tail_idx, tk, tv = self._step_tails(req_ids, reqs)
                masks, depths = (None, None) if parents is None else self._step_tree(req_ids, reqs, parents, live, S, window)
            self.lib.attend_chunk_kv(np.asarray([r.k_handle for r in reqs], dtype=np.uint64), np.asarray([r.v_handle for r in reqs], dtype=np.uint64),
                                     layer, q.data_ptr(), S, R, np.asarray([r.length & ~1 for r in reqs], dtype=np.uint32),
                                     np.asarray(live, dtype=np.uint32), k_new.data_ptr() + 2 * layer * k_new.stride(2),
                                     v_new.data_ptr() + 2 * layer * v_new.stride(2), k_new.stride(0), k_new.stride(1), tail_idx,
                                     tk.data_ptr() + 2 * layer * row if tk is not None else 0, tv.data_ptr() + 2 * layer * row if tv is not None else 0,
                                     self.L * row, masks.data_ptr() if masks is not None else 0, masks.shape[2] if masks is not None else 0,
                                     depths.data_ptr() if depths is not None else 0, window, int(splits), sm_scale, out.data_ptr(),
                                     lse.data_ptr() if keep_lse else 0, st.cuda_stream)
        return (out, lse, q) if keep_lse else out

    # ------------------------------------------------------------------ a draft step on the decode kernel
    def attend_spec(self, layer: int, req_ids: Sequence[int], q, k_new, v_new, sm_scale: float, n_new=None, stream=None, parents=None,
                    window=None):
        """One layer of a step that carries S new positions per request -- draft tokens to verify -- on the DECODE kernel; signature and
        contract of SpeckvKVConnector.attend_spec.  q [batch][S][heads][rows_per_pos][dim] fp16; k_new / v_new
        [batch][S][layers][heads][dim] fp16, the positions that would follow each request's current length; n_new: optional per-request
        counts <= S of live positions (a ragged step); parents (SpeckvKVConnector.tree_masks): the new positions form a tree -- node j
        sees what the request holds, its ancestors and itself, not its siblings; None = a chain, which is the tree [-1, 0, 1, ...].
        Returns [batch][S][heads][rows_per_pos][dim] fp32.  Changes no state -- commit() stores the accepted prefix afterwards.
        The groups are SpeckvKVConnector.spec_groups(S, rows_per_pos): S * rows_per_pos <= 16 is one pass over the records, more goes
        in groups of 16 // rows_per_pos positions.  Each group is ONE speckv_ext_attend_kv_spec call and nothing else: the stored
        positions are walked once for the group's query rows (k_attend_k8v4<false, true>) and the rows held outside the pool -- the
        request's odd last position where it has one, then the new positions -- are folded in inside that launch; there is no tail
        fold and no fold launch.  A later group sees the earlier groups' positions as held positions through its columns of the
        step's mask table.  The query enters the stored part as E4M3 x a row scale, as in attend; the held part takes it in fp16.
        Rows of dead positions (>= n_new[b], or below a dead node) are the stored part alone, finite: zeros for a request that has
        nothing stored.  Indices, masks and handle arrays are derived once per (batch, lengths, S, tree, live counts).
        Against attend_chunk with the same step, the only other route (profiles/k8v4_spec_step.txt, 16 query rows per kv head): 0.34
        of its time at 256 requests x 2k stored positions, 0.25-0.26 at 256 x 8k, 0.49-0.51 at 8 x 32k -- faster at every shape
        measured; 1.07-1.31 single attend steps.
        window (None or 0: none, exactly the calls above; W >= 1: a sliding-window layer): each group is ONE
        speckv_ext_attend_kv_spec_window call and nothing else.  Node j of depth d (SpeckvKVConnector.chunk_tree_depths; a chain: j)
        sits at length + d and sees the last W positions up to itself: the stored ones from length + d + 1 - W on, masked per query row
        inside the kernel (k_attend_k8v4<true, true>; the walk starts at the tile of depth 0's bound, spec_window_range), the held ones
        through the words of tree_masks(window=W).  A dead node's rows are the stored positions its depth's window shows, finite; zeros
        where it shows none.  Against attend_chunk(window=W) with the same step, until now the only route on a
        local layer (profiles/k8v4_spec_window.txt; W = 1024, 16 query rows per kv head): 0.34-0.37 of its time at 256 requests x 2k
        and at 256 x 8k stored positions, 0.93-0.94 at 8 x 32k with (S, rows_per_pos) = (4, 4) and (2, 8); at 8 x 32k with (16, 1) the
        two are equal within the spread (1.01, spread 0.021): with few requests and 16 positions per step attend_chunk(window=W) is as
        good.  0.28-0.83 of an unwindowed attend_spec, 1.30-1.50 single attend(window=W) steps.
        Malformed arguments are a ValueError / KeyError before any library call; a placement the decode kernel does not serve
        (striped, migrated) is the library's SpeckvError, passed through as in attend."""
        import numbers
        import numpy as np
        import torch
        if len(q.shape) != 5:
            raise ValueError("q must be [batch][S][heads][rows_per_pos][dim]")
        B, S, H, R, D = (int(x) for x in q.shape)
        if (H, D) != (self.H, self.D) or B != len(req_ids):
            raise ValueError("q must be [batch][S][heads][rows_per_pos][dim] with one block per request")
        if tuple(k_new.shape) != (B, S, self.L, H, D) or tuple(v_new.shape) != (B, S, self.L, H, D):
            raise ValueError("k_new / v_new must be [batch][S][layers][heads][dim]")
        if not _is_int(layer) or not 0 <= layer < self.L:
            raise ValueError(f"layer {layer} outside 0..{self.L - 1}")
        groups = SpeckvKVConnector.spec_groups(S, R)
        W = SpeckvKVConnector._decode_window(window)
        if n_new is not None:
            n_new = [int(n) for n in n_new]
            if len(n_new) != B or not all(0 <= n <= S for n in n_new):
                raise ValueError("n_new: one count 0..S per request")
        reqs = [self.requests[r] for r in req_ids]
        if parents is not None:                       # (judged once per step, below: a walk over batch x S entries is the host's share of a call)
            parents = list(parents)
            shared = len(parents) > 0 and isinstance(parents[0], numbers.Integral)
            tree_key = tuple(parents) if shared else tuple(tuple(p) for p in parents)
        row = self.H * self.D
        out = torch.empty((B, S, H, R, D), dtype=torch.float32, device="cuda")
        if B == 0:
            return out
        with self._On(self, stream) as st:
            with torch.cuda.stream(st):
                _, tk, tv = self._step_tails(req_ids, reqs)
                key = (tuple(req_ids), self._epoch, S, None if parents is None else tree_key, None if n_new is None else tuple(n_new), W)
                if self._spec[0] != key:              # once per step: the same for every layer and group
                    trees = SpeckvKVConnector._tree_parents(list(range(-1, S - 1)) if parents is None else parents, B)
                    if len(trees[0]) != S:
                        raise ValueError("parents: one entry per new position")
                    words = SpeckvKVConnector.tree_masks(trees, [r.length & 1 for r in reqs], n_new, window=W or None)
                    depths = SpeckvKVConnector.chunk_tree_depths(trees, B) if W else None
                    idx, rank = [], 0
                    for b, r in enumerate(reqs):      # the tail first where the length is odd, then the new positions (_held_rows)
                        if r.length & 1:
                            idx += [B * S + rank] + [b * S + t for t in range(S)]
                            rank += 1
                        else:
                            idx += [b * S + t for t in range(S)] + [b * S + S - 1]       # (the last slot is never visible)
                    self._spec = (key, _kc._device_index([w for per_request in words for w in per_request]),     # [batch][S] words (< 2^17)
                                  _kc._device_index(idx), np.asarray([r.k_handle for r in reqs], dtype=np.uint64),
                                  np.asarray([r.v_handle for r in reqs], dtype=np.uint64), np.asarray([r.length & ~1 for r in reqs], dtype=np.uint32),
                                  _kc._device_index([d for per_request in depths for d in per_request]) if W else None,       # [batch][S] depths
                                  np.asarray([r.length for r in reqs], dtype=np.uint32))
                _, masks, idx, k_handles, v_handles, pos_end, depths, lengths = self._spec
                held = []
                for new, tails in ((k_new, tk), (v_new, tv)):
                    flat = new[:, :, layer].reshape(B * S, H, D)
                    if tails is not None:
                        flat = torch.cat((flat, tails[:, layer]), dim=0)
                    held.append(flat.index_select(0, idx))                              # [batch * (1 + S)][heads][dim]
                kh, vh = held
                parts = []
                for j0, n in groups:
                    g = n * R
                    parts.append((j0, n, g, q[:, j0:j0 + n].permute(0, 2, 1, 3, 4).reshape(B, H, g, D).contiguous(),
                                  torch.empty((B, H, g, D), dtype=torch.float32, device="cuda")))
            for j0, n, g, qg, og in parts:
                if W:                                 # a sliding-window layer: the same launch, the stored positions masked per row by its depth
                    self.lib.attend_kv_spec_window(k_handles, v_handles, layer, qg.data_ptr(), g, R, pos_end, lengths, depths.data_ptr() + 4 * j0, W,
                                                   kh.data_ptr(), vh.data_ptr(), (1 + S) * row, row, masks.data_ptr() + 4 * j0, S, sm_scale,
                                                   og.data_ptr(), 0, st.cuda_stream)
                    continue
                self.lib.attend_kv_spec(k_handles, v_handles, layer, qg.data_ptr(), g, R, pos_end, kh.data_ptr(), vh.data_ptr(), (1 + S) * row, row,
                                        masks.data_ptr() + 4 * j0, S, sm_scale, og.data_ptr(), 0, st.cuda_stream)
            with torch.cuda.stream(st):
                for j0, n, g, qg, og in parts:
                    out[:, j0:j0 + n] = og.view(B, H, n, R, D).permute(0, 2, 1, 3, 4)
        return out

    # ------------------------------------------------------------------ a prefix shared by several requests
    # (the bodies are SharedPrefixSteps': this connector's side of them, then the two methods)
    def _prefix_handles(self, prefix_ids):
        import numpy as np
        return (np.asarray([self.requests[p].k_handle for p in prefix_ids], dtype=np.uint64),
                np.asarray([self.requests[p].v_handle for p in prefix_ids], dtype=np.uint64))

    def _own_decode(self, layer, req_ids, q, sm_scale, stream, window, gathered):
        return self._attend_own(layer, req_ids, q, sm_scale, stream, window)

    def _own_chunk(self, layer, req_ids, q, k_new, v_new, sm_scale, n_new, stream, window, parents, by_depth, keep_lse=False):
        if not keep_lse:
            return self.attend_chunk(layer, req_ids, q, k_new, v_new, sm_scale, n_new, stream, 1, window, parents)
        return self._chunk_own(layer, req_ids, q, k_new, v_new, sm_scale, n_new, stream, 1, window, parents, keep_lse=True)

    def _prefix_fold(self, handles, first, layer, req_ids, ahead, d_q, C, R, lens, n_q, depths, W, splits, sm_scale, d_out, d_lse, cuda_stream):
        """own_seen = length + ahead (0: a decode step, whose position is held already; 1: a chunk step), with and without a window"""
        import numpy as np
        own = np.asarray([self.requests[r].length for r in req_ids], dtype=np.uint32)
        if ahead:
            own += np.uint32(ahead)
        self.lib.attend_prefix_fold_kv(*handles, first, layer, d_q, C, R, lens, n_q, own, depths, W, splits, sm_scale, d_out, d_lse, cuda_stream)

    def _depth_table(self, req_ids, parents, live, S, W):
        return self._step_tree(req_ids, self._reqs(req_ids), parents, live, S, W)[1].data_ptr()

    def attend_shared(self, layer: int, req_ids: Sequence[int], prefix_ids: Sequence[Optional[int]], q, sm_scale: float, prefix_lens=None,
                      stream=None, splits=0, window=None):
        """attend() for requests that SHARE A PREFIX without holding a copy of it (parallel samples of one prompt, beams, a system prompt
        in front of many users); the contract of SpeckvKVConnector.attend_shared over the split pool.  Shapes and result are attend()'s.
        A prefix is an ordinary split request the call names: prefix_ids[b] = the request whose first prefix_lens[b] stored positions
        member b sees in front of its own, or None.  prefix_lens[b] defaults to the prefix's length, which must then be even; a given
        one is even, >= 0 and at most the prefix's length rounded down to even.  A prefix may not be a member; members of one prefix
        may see different lengths of it and need not be adjacent (shared_groups; q and the result are permuted only when they are not).
        g is 1, 2, 4, 8 or 16.
        The step: the members' own attention exactly as attend(window=window) issues it (speckv_ext_attend_kv_batch[_window] and the
        tail fold), with the log-sum-exp kept, then ONE speckv_ext_attend_prefix_fold_kv call on the same stream with C = 1, own_seen =
        the member's length and the chain depth 0: a workgroup walks the prefix's FP8 key records and MXFP4 value records ONCE for 64
        query rows of its members and folds the result into theirs -- the softmax over prefix + own positions.  THE OWN PART TAKES THE
        QUERY AS E4M3 x A ROW SCALE, as attend does; THE PREFIX PART TAKES IT IN fp16.  splits: 0 = the library's rule cuts a long
        prefix of few members across the chip, 1 = never, N = forced.  window None = a global layer; an int W >= 1 = a local layer:
        the member's query sees the last W positions of prefix + own, the fold the prefix positions [max(0, prefix_lens[b] + length -
        W), prefix_lens[b]); a member with length >= W keeps the bits of attend(window=W).  No member with a prefix (all None, or all
        lengths 0): attend()'s launches and bits.  The pool holds the prefix once: (members - 1) x prefix pairs x 3136 bytes per layer
        less than members that each hold a copy.
        Anything malformed is a ValueError / KeyError before any library call; a q that is no torch tensor is a TypeError."""
        return self._decode_shared(layer, req_ids, prefix_ids, q, sm_scale, prefix_lens, stream, splits, window)

    def attend_chunk_shared(self, layer: int, req_ids: Sequence[int], prefix_ids: Sequence[Optional[int]], q, k_new, v_new, sm_scale: float,
                            n_new=None, prefix_lens=None, stream=None, splits=0, window=None, parents=None):
        """attend_chunk() for members of a shared prefix; the contract of SpeckvKVConnector.attend_chunk_shared over the split pool.  The
        member's OWN step -- a user's differing suffix behind a shared system prompt, a draft chain or tree -- is what
        attend_chunk(splits=1, window=window, parents=parents) issues (ONE speckv_ext_attend_chunk_kv call) with the log-sum-exp kept;
        then ONE speckv_ext_attend_prefix_fold_kv call with C = S, n_q = the live counts and own_seen = length + 1 on the same stream
        folds in the stored positions [0, prefix_lens[b]) of the request prefix_ids[b].  Shapes, n_new and the result (zeros for
        positions >= n_new[b]) are attend_chunk's; prefix_ids, prefix_lens, splits and what is refused are attend_shared's.  Both
        parts take the query in fp16.  window W >= 1: query position j sees the prefix positions [max(0, prefix_lens[b] + length + 1
        + j - W), prefix_lens[b]).  parents: the prefix part has no structure among rows, every live node sees all of it; parents
        together with window goes by a node's DEPTH as attend_chunk does -- the fold reads the same depth table the own call reads,
        node j of depth d sees from max(0, prefix_lens[b] + length + 1 + d - W) on -- so this one method is the tree step of a local
        layer too.  Changes no state: commit() stores the accepted positions in the MEMBER afterwards.  No member with a prefix:
        attend_chunk(splits=1)'s launch and bits."""
        return self._chunk_shared(layer, req_ids, prefix_ids, q, k_new, v_new, sm_scale, n_new, prefix_lens, stream, splits, window, parents,
                                  parents is not None, "attend_chunk_shared")

    # ------------------------------------------------------------------ commit
    def commit(self, req_ids: Sequence[int], k_new, v_new, n_accept: Optional[Sequence[int]] = None, stream=None, *, nodes=None, parents=None):
        """Store the first n_accept[b] (0..S) of the S new positions k_new[b], v_new[b] ([batch][S][layers][heads][dim] fp16) of every
        request: the tail and the new rows are paired into pages, a leftover odd position becomes the tail (SpeckvKVConnector.commit_plan).
        TWO library calls for the whole batch, one speckv_ext_write_pairs per allocation, rows read where they lie.  That entry numbers
        the pages of a pair j = 0 .. 2 n_layers - 1 as (layer j / 2, kind j % 2) and reads row d_rows[2 kind (+ 1)] + (j / 2) *
        layer_stride; a single-kind allocation of L regions is addressed with n_layers = L / 2, layer_stride = two real layer strides,
        the even / odd rows of real layer 0 in the "K" slots and the same rows of real layer 1 in the "V" slots -- region j then reads
        the row of real layer j.  Returns what the asynchronous launches read, to be held until the stream has passed them.
        nodes (keyword, in place of n_accept: exactly one of the two is given): nodes[b] = the accepted path of a TREE step, the step
        positions to store in order -- the contract of SpeckvKVConnector.commit, judged by its rules (_checked_paths): with `parents`
        (SpeckvKVConnector.tree_masks) the path must be a chain of the tree from a child of the committed context, without, the
        caller vouches for ascending node indices (the path of a large tree verified by attend_chunk(parents=...)).  ValueError before
        any state changes.  The launches are the same two calls; only the row addresses and the gather of the new tails follow
        nodes[b][t] instead of t.  nodes[b] = range(n) stores what n_accept[b] = n stores."""
        import numpy as np
        import torch
        B, S = k_new.shape[0], k_new.shape[1]
        if (n_accept is None) == (nodes is None):
            raise ValueError("commit: exactly one of n_accept and nodes")
        if nodes is not None:
            nodes = SpeckvKVConnector._checked_paths(self, req_ids, k_new, v_new, nodes, parents)
            n_accept = [len(path) for path in nodes]
        elif parents is not None:
            raise ValueError("commit: parents judges nodes; n_accept names a prefix of the step")
        n_accept = [int(n) for n in n_accept]
        reqs = [self.requests[rid] for rid in req_ids]
        if len(reqs) != B or len(n_accept) != B or tuple(v_new.shape) != tuple(k_new.shape) or tuple(k_new.shape[2:]) != (self.L, self.H, self.D):
            raise ValueError("k_new / v_new must be [batch][S][layers][heads][dim], n_accept one count per request")
        for rid, r, n in zip(req_ids, reqs, n_accept):
            if not 0 <= n <= S:
                raise ValueError(f"request {rid}: n_accept {n} outside 0..{S}")
            if r.length + n > self.T:
                raise ValueError(f"request {rid} is full")
        pairs, tails = SpeckvKVConnector.commit_plan([r.length for r in reqs], n_accept)
        if not pairs and not tails:
            return []
        used = [b for b, (r, n) in enumerate(zip(reqs, n_accept)) if n and r.length & 1]        # requests whose odd position finds its partner
        layer_bytes = self.H * self.D * 2
        row_bytes = self.L * layer_bytes
        keep, tk, tv = [], None, None
        with self._On(self, stream) as st:
            with torch.cuda.stream(st):
                k_new, v_new = k_new.contiguous(), v_new.contiguous()
                keep += [k_new, v_new]
                if tails:                                                                       # copies: the caller may reuse k_new
                    it = _kc._device_index([b * S + (t if nodes is None else nodes[b][t]) for b, t in tails])
                    tk = k_new.view(B * S, self.L, self.H, self.D).index_select(0, it)
                    tv = v_new.view(B * S, self.L, self.H, self.D).index_select(0, it)
            if pairs:
                plan = np.asarray([x for group in pairs for x in group], dtype=np.int64)       # (b, page of layer 0, source, source) per pair
                b_of = plan[:, 0]
                tail_at = np.zeros((B, 2), dtype=np.uint64)
                for b in used:
                    keep += [reqs[b].tail_k, reqs[b].tail_v]
                    tail_at[b] = reqs[b].tail_k.data_ptr(), reqs[b].tail_v.data_ptr()
                node_of = None
                if nodes is not None:                                                           # [b][source] -> the step position it names
                    node_of = np.zeros((B, S + 1), dtype=np.int64)                              # (source -1 is the last column, unused)
                    for b, path in enumerate(nodes):
                        node_of[b, :len(path)] = path
                for kind, (new, handle) in enumerate(((k_new, "k_handle"), (v_new, "v_handle"))):
                    rows = np.empty((len(plan), 4), dtype=np.uint64)
                    for half in (0, 1):
                        t = plan[:, 2 + half]
                        at = np.maximum(t, 0) if node_of is None else node_of[b_of, t]
                        new_row = ((b_of * S + at) * row_bytes).astype(np.uint64) + np.uint64(new.data_ptr())
                        rows[:, half] = np.where(t < 0, tail_at[b_of, kind], new_row)          # real layer 0: the "K" slots
                        rows[:, 2 + half] = rows[:, half] + np.uint64(layer_bytes)             # real layer 1: the "V" slots
                    handles = np.asarray([getattr(reqs[b], handle) for b in b_of], dtype=np.uint64)
                    self.lib.write_pairs(handles, plan[:, 1].astype(np.uint64), rows, self.region_pages, self.L // 2, 2 * layer_bytes, st.cuda_stream)
        for b in used:
            reqs[b].tail_k = reqs[b].tail_v = None
        for i, (b, _) in enumerate(tails):
            reqs[b].tail_k, reqs[b].tail_v = tk[i], tv[i]
        for r, n in zip(reqs, n_accept):
            r.length += n
        self._epoch += 1
        return keep

    # ------------------------------------------------------------------ rollback and fork
    def _moved(self):
        """lengths, tails or the set of requests changed: nothing a step derived from them holds any longer"""
        self._epoch += 1
        self._tails = (None, None, None, None)
        self._tree = (None, None, None)
        self._fold = (None,)
        self._spec = (None,)
        self._shared_key, self._shared_plan = None, None

    def _read_tails(self, reqs, positions, st):
        """The rows of the EVEN stored positions positions[i] of reqs[i], every layer, K and V, as one [n][layers][heads][dim] fp16 tensor
        pair: ONE speckv_ext_read_pairs_kv call on stream st.  Pair i is page positions[i] // 2 of layer 0's region in both
        allocations, page_step = one region, n_layers = the real layers (no re-addressing as in commit: the entry knows the split
        layout); the odd halves are not asked for."""
        import numpy as np
        import torch
        n = len(reqs)
        layer_bytes = self.H * self.D * 2
        with torch.cuda.stream(st):
            tk = torch.empty((n, self.L, self.H, self.D), dtype=torch.float16, device="cuda")
            tv = torch.empty_like(tk)
        rows = np.zeros((n, 4), dtype=np.uint64)                                                 # odd rows: 0 = not wanted
        at = np.arange(n, dtype=np.uint64) * np.uint64(self.L * layer_bytes)
        rows[:, 0], rows[:, 2] = at + np.uint64(tk.data_ptr()), at + np.uint64(tv.data_ptr())
        self.lib.read_pairs_kv(np.asarray([r.k_handle for r in reqs], dtype=np.uint64), np.asarray([r.v_handle for r in reqs], dtype=np.uint64),
                               np.asarray([self._page(0, pos) for pos in positions], dtype=np.uint64), rows, self.region_pages, self.L,
                               layer_bytes, st.cuda_stream)
        return tk, tv

    def truncate(self, req_ids: Sequence[int], new_lengths: Sequence[int], stream=None):
        """Roll the requests back to new_lengths[b] <= length positions; the contract of SpeckvKVConnector.truncate, planned by its
        truncate_plan: afterwards lengths, tails, _epoch and every per-step cache are those of a connector that had stopped there.  A
        request cut to an odd length inside stored pairs gets its new last position back as its tail: ONE speckv_ext_read_pairs_kv
        call for the whole batch decodes that row -- the even half of page (new_len - 1) // 2 of every layer's region, in the K
        allocation and in the V allocation -- into one [n][layers][heads][dim] tensor pair; the odd halves are null (not stored, and
        in the FP8 allocation not read).  No other launch; when no request needs a row back, no launch at all.  ValueError
        (truncate_plan) and KeyError before any state changes.  The allocations keep their size.

        The row that comes back has been through its format once -- K through FP8_E4M3 with its page's block scale, V through MXFP4
        with its group codes -- and it is encoded AGAIN with its new partner when the next commit completes its pair: the block scale
        (K) and the 32-element group codes (V) are then chosen over the new pair, so the row's stored values may move once more by the
        formats' rounding.  The tail itself is exactly the decoded stored row, bit for bit what kv_rows returned for it.

        Records beyond the new length stay in both allocations as stale bytes, and nothing clears them, because their values are never
        used.  Every K8V4 body takes its range from pos_end (length & ~1) and a page holds two positions, so a stale PAGE is either
        wholly behind pos_end or rewritten whole by the commit that completes it: the decode kernel (k_attend_k8v4, all four
        instances) sets the score of a position at or beyond pos_end inside the last 32-position tile to -inf before the softmax, which
        gives it weight exactly 0, and drops the MXFP4 block code of such a page; the chunk and prefix kernels (k_attend_chunk /
        k_attend_prefix, the K8V4 instances) score such positions -inf too and stage their V as zeros, against pos_end and against the
        prefix length, which attend_shared bounds by the prefix's length rounded down to even.  tests/test_gpu_k8v4_lifecycle.py
        commits rows of 200x and 1000x the kept magnitude behind the cut and holds attend, attend(window=W), attend_spec,
        attend_chunk and attend_shared over a cut prefix to the float64 reference.  One difference
        to a never-written page remains, as in SpeckvKVConnector.truncate: a stale V row that is not finite times a weight of 0 is
        NaN; a caller that may have committed non-finite rows frees before it rolls back."""
        reqs = [self.requests[rid] for rid in req_ids]
        new_lengths = [int(n) for n in new_lengths]
        if len(new_lengths) != len(reqs):
            raise ValueError("new_lengths: one length per request")
        drops, reads = SpeckvKVConnector.truncate_plan([r.length for r in reqs], new_lengths)
        if all(n == r.length for n, r in zip(new_lengths, reqs)):
            return
        tk = tv = None
        if reads:
            with self._On(self, stream) as st:
                tk, tv = self._read_tails([reqs[b] for b, _ in reads], [new_lengths[b] - 1 for b, _ in reads], st)
        for b in drops:
            reqs[b].tail_k = reqs[b].tail_v = None
        for i, (b, _) in enumerate(reads):
            reqs[b].tail_k, reqs[b].tail_v = tk[i], tv[i]
        for r, n in zip(reqs, new_lengths):
            r.length = n
        self._moved()

    def fork(self, src_ids: Sequence[int], new_ids: Sequence[int], lengths: Optional[Sequence[int]] = None, stream=None):
        """Create the requests new_ids[b], each holding the first lengths[b] (default: all) positions of request src_ids[b]; the contract
        of SpeckvKVConnector.fork, planned by its fork_plan.  A source may appear several times (parallel sampling, beams).  Afterwards
        lengths, tails and _epoch are those of requests written independently with the same values, and source and fork go their
        own ways.

        ONE speckv_ext_copy_runs_kv call for the batch copies the stored records of the lengths[b] // 2 pairs of every layer's region
        in BOTH allocations -- records, not values: the FP8 bytes with their block scales (scale table included) and the MXFP4 nibble
        rows with their codes, nothing decoded or rounded again, so every reader gives the fork the source's bits (no call when no
        pair is stored).  An odd length needs its last row as the new request's tail: equal to the source's length, the row is a CLONE
        of the source's tail (never a view); shorter, it is the even half of stored page (length - 1) // 2, and at most ONE
        speckv_ext_read_pairs_kv call reads those rows from the SOURCES, as truncate() installs tails.

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
        n_pages, tails = SpeckvKVConnector.fork_plan([r.length for r in srcs], lengths)
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
                        firsts = np.arange(self.L, dtype=np.uint64) * np.uint64(self.region_pages)          # _page(layer, 0)
                        handles = lambda rs, name: np.asarray([getattr(r, name) for r in rs], dtype=np.uint64)
                        self.lib.copy_runs_kv(handles(srcs, "k_handle"), handles(srcs, "v_handle"), handles(news, "k_handle"), handles(news, "v_handle"),
                                              np.asarray(n_pages, dtype=np.uint64), firsts, st.cuda_stream)
                    if reads:
                        tk, tv = self._read_tails([srcs[b] for b in reads], [lengths[b] - 1 for b in reads], st)
                        keep += [tk, tv]
            with torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext():      # behind what produced the source's tail
                for b, t in enumerate(tails):
                    if t == "held":
                        news[b].tail_k, news[b].tail_v = srcs[b].tail_k.clone(), srcs[b].tail_v.clone()
        except BaseException:
            for rid in made:
                self.free_request(rid)
            raise
        for i, b in enumerate(reads):
            news[b].tail_k, news[b].tail_v = tk[i], tv[i]
        for r, n in zip(news, lengths):
            r.length = n
        self._moved()
        return keep
