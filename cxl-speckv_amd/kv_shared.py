"""What SpeckvKVConnector and SpeckvSplitKVConnector share word for word, one body each in SharedPrefixSteps: the steps over members of
a SHARED PREFIX (attend_shared, attend_chunk_shared, attend_tree_shared) and the judging half of a chunk step.  A connector inherits it
and supplies what differs between one allocation per request and two:
  _pool_check(what), _reqs(req_ids)  the refusal of a pool the fused attention cannot read; the request objects of a batch
  _prefix_handles(prefix_ids)        the handle arrays of the prefix requests, as a tuple: one array, or (K, V) of the split pool
  _own_decode / _own_chunk(...)      its own decode / chunk step with the log-sum-exp kept -> (out, lse, q as launched)
  _prefix_fold(...)                  the fold launch (which entry, and whether own_seen is built, is the connector's)
  _depth_table(...)                  the device depth table of a tree under a window, the one its own chunk step has just read"""
import numbers
from typing import Optional, Sequence

SPLITS_RULE = "splits must be 0 (the library's rule), 1 (no pieces) or a forced piece count 2..64"
PARENTS_RULE = "parents: one tree per request, or one tree for all"


def _is_int(x):
    """an integer of any kind (python's, numpy's), but no bool"""
    return isinstance(x, numbers.Integral) and not isinstance(x, bool)


def tail_index(reqs):
    """(int32 [batch]: the rank of a request among those with an odd length -- the row of its fp16 tail --, -1 for an even length;
    how many are odd)"""
    import numpy as np
    tail_idx, rank = np.full(len(reqs), -1, dtype=np.int32), 0
    for b, r in enumerate(reqs):
        if r.length & 1:
            tail_idx[b] = rank
            rank += 1
    return tail_idx, rank


def paged_cache_geometry(caches, n_layers, bf16=False):
    """Whether the one-launch paged transfers (speckv_ext_read_slots / _write_slots and their _ex, _kmul and _kv forms) can address
    `caches`: per layer a [2, blocks, block_size, heads, dim] fp16 tensor whose slots are 2048-byte rows one block after the other,
    16-byte aligned, the same for all n_layers caches.  bf16=True: the caches may all be bfloat16 instead.  Only shapes, strides,
    dtype and alignment are looked at.  Returns (geometry, None) or (None, what was wrong); geometry = (slots per cache, bytes
    between the K and the V plane), with bf16=True the element type (SLOT_ELEM_*: 0 fp16, 1 bf16) third."""
    import torch
    if len(caches) != n_layers:
        return None, f"{len(caches)} caches for {n_layers} layers"
    geo = None
    dtype = caches[0].dtype if bf16 and len(caches) and caches[0].dtype == torch.bfloat16 else torch.float16
    for c in caches:
        if c.dtype != dtype:
            return None, f"a cache of {c.dtype} among caches of {dtype}" + ("" if bf16 else " (fp16 only)")
        if c.dim() != 5 or c.shape[0] != 2 or c.shape[3] * c.shape[4] * 2 != 2048:
            return None, f"a cache of shape {tuple(c.shape)}: [2, blocks, block_size, heads, dim] with heads * dim * 2 == 2048 bytes is needed"
        if tuple(c.stride()[2:]) != (c.shape[3] * c.shape[4], c.shape[4], 1) or c.stride(1) != c.shape[2] * 1024:
            return None, f"a cache with strides {tuple(c.stride())}: its slots must be 2048-byte rows one block after the other"
        if c.data_ptr() % 16 or (c.stride(0) * 2) % 16:
            return None, "a cache whose K or V plane is not 16-byte aligned"
        g = (c.shape[1] * c.shape[2], c.stride(0) * 2)
        if geo is not None and g != geo:
            return None, "caches that differ in their slot count or in the distance between their K and V planes"
        geo = g
    if geo is None:
        return None, "no caches"
    if bf16:
        return geo + (1 if dtype == torch.bfloat16 else 0,), None
    return geo, None


class SharedPrefixSteps:
    def _pool_check(self, what):
        pass

    def _reqs(self, req_ids):
        return [self.requests[r] for r in req_ids]

    # ------------------------------------------------------------------ the judging half of a chunk step
    def _chunk_judge(self, layer, req_ids, q, k_new, v_new, n_new, splits, parents, keep_lse):
        """What attend_chunk judges in front of any library call, in this order: splits, the pool, the shapes, layer, n_new, the
        query blocks, the requests, max_tokens, the tree.  -> (the requests, the live counts, (S, rows_per_pos), out, lse or None,
        whether any row is live); out is zeroed where some row may stay unwritten."""
        import torch
        if not _is_int(splits) or not 0 <= splits <= 64:
            raise ValueError(SPLITS_RULE)
        self._pool_check("attend_chunk")
        if len(q.shape) != 5:
            raise ValueError("q must be [batch][S][heads][rows_per_pos][dim]")
        B, S, H, R, D = (int(x) for x in q.shape)
        want = (B, S, self.L, self.H, self.D)
        if (H, D) != (self.H, self.D) or tuple(k_new.shape) != want or tuple(v_new.shape) != want or B != len(req_ids) or S < 1:
            raise ValueError("q must be [batch][S][heads][rows_per_pos][dim], k_new / v_new [batch][S][layers][heads][dim], S >= 1")
        if not 0 <= layer < self.L:
            raise ValueError(f"layer {layer} outside 0..{self.L - 1}")
        if n_new is None:
            live = [S] * B
        else:
            live = [int(n) for n in n_new]
            if len(live) != B or not all(0 <= n <= S for n in live):
                raise ValueError("n_new: one count 0..S per request")
        counts, _ = self.chunk_blocks(live, R)
        reqs = self._reqs(req_ids)
        for r, n in zip(reqs, live):
            if r.length + n > self.T:
                raise ValueError(f"a request of {r.length} positions cannot take {n} more: max_tokens is {self.T}")
        if parents is not None:
            trees = self._chunk_tree_parents(parents, B)                  # judged in front of any library call
            if trees and len(trees[0]) != S:
                raise ValueError("parents: one entry per new position")
        out = (torch.empty if n_new is None and parents is None else torch.zeros)((B, S, H, R, D), dtype=torch.float32, device="cuda")
        lse = torch.full((B, S, H, R), float("-inf"), dtype=torch.float32, device="cuda") if keep_lse else None
        return reqs, live, (S, R), out, lse, any(counts)

    def _chunk_rows(self, k_new, v_new):
        """k_new, v_new as the chunk launch reads them: in place through their strides where those allow it, contiguous copies
        (made on torch's current stream) otherwise"""
        in_place = lambda t: (t.stride(4) == 1 and t.stride(3) == self.D and t.stride(2) % 8 == 0 and t.stride(1) % 8 == 0 and
                              t.stride(1) >= self.H * self.D and t.stride(0) % 8 == 0 and t.data_ptr() % 16 == 0)
        if in_place(k_new) and in_place(v_new) and k_new.stride() == v_new.stride():
            return k_new, v_new
        return k_new.contiguous(), v_new.contiguous()

    # ------------------------------------------------------------------ a prefix shared by several requests
    @staticmethod
    def shared_groups(req_ids: Sequence[int], prefix_ids: Sequence[Optional[int]]):
        """How a call over members with shared prefixes is laid out for speckv_ext_attend_prefix_fold: (order, prefixes, first_member).
        order = the indices 0..batch-1 so that the members of one prefix are adjacent -- the prefixes in the order of their first
        member, the members of a prefix in the caller's order (stable), the members without a prefix (None) last, in the caller's order;
        prefixes = the prefix id of every group; first_member = the exclusive prefix of the groups' sizes, len(prefixes) + 1 entries
        (the members behind first_member[-1] have no prefix).  An input that is already laid out so gives order == list(range(batch))."""
        if len(prefix_ids) != len(req_ids):
            raise ValueError("prefix_ids: one prefix id or None per request")
        groups, none = {}, []
        for b, p in enumerate(prefix_ids):
            (none if p is None else groups.setdefault(p, [])).append(b)
        order, first = [], [0]
        for members in groups.values():
            order += members
            first.append(len(order))
        return order + none, list(groups), first

    @staticmethod
    def _shared_window(window):
        """window as the shared-prefix calls take it: None -> 0 (no window), an int >= 1 -> itself; anything else -- 0, a negative, a
        bool, a float, a string -- is a ValueError"""
        if window is None:
            return 0
        if not _is_int(window) or not 1 <= window <= 0xFFFFFFFF:
            raise ValueError("window must be None (no window) or a count of positions >= 1")
        return int(window)

    @staticmethod
    def _shared_tensors(what, **tensors):
        """The rows of a shared-prefix call are torch tensors: the fold reads them by data_ptr() behind the own step, and the grouped
        order gathers them with index_select, so None or an object that merely has a shape is a TypeError here -- behind the
        judgement of the lists, in front of any library call -- and not an AttributeError somewhere inside the step"""
        import torch
        for name, t in tensors.items():
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{what}(): {name} must be a torch tensor, not {type(t).__name__}")

    @staticmethod
    def prefix_window_walk(first_member: Sequence[int], prefix_lens: Sequence[int], own_seen: Sequence[int], n_new: Sequence[int], window):
        """Which tiles of its prefix a group of a shared-prefix call walks under a window (speckv_ext_prefix_window_walk restated).
        Group g = the members first_member[g] .. first_member[g + 1] - 1 (shared_groups); member m sees prefix_lens[m] (even)
        positions of the prefix in front of its own, own_seen[m] of its OWN positions are seen by its query position of depth 0,
        itself included (a decode step: its length; a chunk or tree step: length + 1), and it brings n_new[m] live positions.  The
        row of depth d sees [lo, prefix_lens[m]) of the prefix, lo = max(0, prefix_lens[m] + own_seen[m] + d - W) (W None: 0), and
        nothing where that is empty.  A member COUNTS when n_new[m] > 0, prefix_lens[m] > 0 and its depth-0 bound -- its lowest --
        is below prefix_lens[m].  The group's blocks walk the 32-position tiles [first_tile, first_tile + n_tiles): first_tile =
        (the lowest depth-0 bound of the members that count) >> 5, n_tiles = ceil(max_len / 32) - first_tile with max_len their
        largest prefix_lens; (0, 0) for a group no member of which counts -- it has no blocks.  Returns one (first_tile, n_tiles)
        per group.  Pure python, no device."""
        W = SharedPrefixSteps._shared_window(window)
        first = list(first_member)
        if not first or first[0] != 0 or any(not _is_int(x) for x in first) or any(b < a for a, b in zip(first, first[1:])):
            raise ValueError("first_member: ints ascending from 0, one more than there are groups")
        n = first[-1]
        lens, seen, live = list(prefix_lens), list(own_seen), list(n_new)
        if not (len(lens) == len(seen) == len(live) == n) or not all(_is_int(x) and x >= 0 for x in lens + seen + live) or any(x & 1 for x in lens):
            raise ValueError("prefix_lens (even), own_seen, n_new: one count >= 0 per member")
        walks = []
        for a, b in zip(first, first[1:]):
            bounds = [(max(0, lens[m] + seen[m] - W) if W else 0, lens[m]) for m in range(a, b) if live[m] and lens[m]]
            bounds = [(lo, n_pre) for lo, n_pre in bounds if lo < n_pre]
            if not bounds:
                walks.append((0, 0))
                continue
            t_first = min(lo for lo, _ in bounds) >> 5
            walks.append((t_first, (max(n_pre for _, n_pre in bounds) + 31) // 32 - t_first))
        return walks

    @staticmethod
    def _shared_permutation(order):
        """(idx, inv) on the device, made on torch's current stream: x.index_select(0, idx) is x in the grouped order,
        y.index_select(0, inv) is y back in the caller's"""
        import torch
        inv = [0] * len(order)
        for at, b in enumerate(order):
            inv[b] = at
        both = torch.tensor([order, inv], dtype=torch.int64).pin_memory().to("cuda", non_blocking=True)
        return both[0], both[1]

    def _shared_args(self, req_ids, prefix_ids, prefix_lens, splits, what, window=None):
        """The shared-prefix arguments of a call, judged in front of any library call and kept for the other layers of the step: the
        judgement depends on the lists and on what the requests hold, so it is keyed by the lists (values AND types: True == 1), the
        window (value and type, judged by _shared_window in front of it) and `_epoch`, like the attention plan.  None when no member
        sees a prefix; otherwise (order or None when the batch is laid out already, the members in that order, the groups' handle
        arrays as _prefix_handles gives them, first_member and the members' prefix lengths in that order as the arrays the entry
        takes).  What is kept holds handles and lengths: it is right only while EVERY method that changes a request's length or
        handle, or the set of requests, moves `_epoch` -- a new state-changing method must move it too."""
        import numpy as np
        key = (what, self._epoch, tuple(req_ids), tuple(prefix_ids), tuple(map(type, prefix_ids)), type(splits), splits,
               None if prefix_lens is None else (tuple(prefix_lens), tuple(map(type, prefix_lens))), type(window), window)
        if self._shared_key == key:
            return self._shared_plan
        plan = self._shared_judge(req_ids, prefix_ids, prefix_lens, splits, what)
        if plan is not None:
            order, prefixes, first, lens = plan
            if order is not None:
                req_ids, lens = [req_ids[b] for b in order], [lens[b] for b in order]
            plan = (order, list(req_ids), self._prefix_handles(prefixes), np.asarray(first, dtype=np.uint32), np.asarray(lens, dtype=np.uint32))
        self._shared_key, self._shared_plan = key, plan
        return plan

    def _shared_judge(self, req_ids, prefix_ids, prefix_lens, splits, what):
        """_shared_args' judgement: (order or None, the groups' prefix ids, first_member, the members' prefix lengths in the CALLER's
        order) -- or None when no member sees a prefix"""
        self._pool_check(what)
        B = len(req_ids)
        if len(prefix_ids) != B or (prefix_lens is not None and len(prefix_lens) != B):
            raise ValueError("prefix_ids (and prefix_lens): one entry per request")
        if not _is_int(splits) or not 0 <= splits <= 64:
            raise ValueError(SPLITS_RULE)
        for r in req_ids:
            self.requests[r]                                              # KeyError: an unknown member
        members, lens = set(req_ids), []
        for b, p in enumerate(prefix_ids):
            if p is None:
                if prefix_lens is not None and prefix_lens[b] is not None and (not _is_int(prefix_lens[b]) or prefix_lens[b] != 0):
                    raise ValueError("prefix_lens: a member without a prefix takes 0 or None")
                lens.append(0)
                continue
            if not _is_int(p):
                raise ValueError("prefix_ids: request ids (ints) or None")
            if p not in self.requests:
                raise KeyError(f"prefix request {p} does not exist")
            if p in members:
                raise ValueError(f"request {p} is a member of the call and cannot be its prefix")
            have = self.requests[p].length
            if prefix_lens is None or prefix_lens[b] is None:
                if have & 1:
                    raise ValueError(f"prefix request {p} holds an odd number of positions ({have}): pass prefix_lens and keep the "
                                     "last position in the member (only whole stored pairs can be shared)")
                lens.append(have)
            else:
                n = prefix_lens[b]
                if not _is_int(n) or n < 0 or n & 1 or n > (have & ~1):
                    raise ValueError(f"prefix_lens: even ints in 0..{have & ~1} for prefix request {p}")
                lens.append(int(n))
        if not any(lens):
            return None
        order, prefixes, first = self.shared_groups(req_ids, prefix_ids)
        return (None if order == list(range(B)) else order, prefixes, first, lens)

    def _decode_shared(self, layer, req_ids, prefix_ids, q, sm_scale, prefix_lens, stream, splits, window):
        """attend_shared's body: the window and the lists judged, the tensor and its shape, the fall-through without a prefix, the
        gather into the grouped order, the connector's own step with the log-sum-exp, ONE fold, the way back"""
        import numpy as np
        import torch
        W = self._shared_window(window)
        plan = self._shared_args(req_ids, prefix_ids, prefix_lens, splits, "attend_shared", window)
        self._shared_tensors("attend_shared", q=q)
        if len(q.shape) != 4 or q.shape[0] != len(req_ids):
            raise ValueError("q must be [batch][heads][g][dim]")
        if plan is None:
            return self.attend(layer, req_ids, q, sm_scale, stream, window)
        order, req_ids, handles, first, lens = plan
        G = int(q.shape[2])
        if G not in (1, 2, 4, 8, 16):
            raise ValueError("attend_shared() takes 1, 2, 4, 8 or 16 query rows per kv head")
        if order is not None:                                     # the gather runs on the stream the launches go to, as they do
            with self._On(self, stream) as st, torch.cuda.stream(st):
                idx, inv = self._shared_permutation(order)
                q = q.index_select(0, idx)
        out, lse, qs = self._own_decode(layer, req_ids, q, sm_scale, stream, window, order is not None)
        with self._On(self, stream) as st:
            self._prefix_fold(handles, first, layer, req_ids, 0, qs.data_ptr(), 1, G, lens, np.ones(len(req_ids), dtype=np.uint32), 0, W,
                              int(splits), sm_scale, out.data_ptr(), lse.data_ptr(), st.cuda_stream)
            if order is not None:                                 # the way back: behind the fold, on its stream
                with torch.cuda.stream(st):
                    out = out.index_select(0, inv)
        return out

    def _chunk_shared(self, layer, req_ids, prefix_ids, q, k_new, v_new, sm_scale, n_new, prefix_lens, stream, splits, window, parents, by_depth,
                      what):
        """attend_chunk_shared's and attend_tree_shared's body: by_depth = a tree whose window, if any, goes by a node's depth"""
        import numpy as np
        import torch
        W = self._shared_window(window)
        by_depth = by_depth and W != 0                            # a tree without a window is the masked chunk
        plan = self._shared_args(req_ids, prefix_ids, prefix_lens, splits, what, window)
        self._shared_tensors(what, q=q, k_new=k_new, v_new=v_new)
        if plan is None:
            return self._own_chunk(layer, req_ids, q, k_new, v_new, sm_scale, n_new, stream, window, parents, by_depth)
        order, req_ids, handles, first, lens = plan
        if order is not None:
            if n_new is not None:
                if len(n_new) != len(order):
                    raise ValueError("n_new: one count 0..S per request")
                n_new = [n_new[b] for b in order]
            if parents is not None:
                parents = list(parents)
                if parents and not isinstance(parents[0], numbers.Integral):          # one tree per request: in the members' order
                    if len(parents) != len(order):
                        raise ValueError(PARENTS_RULE)
                    parents = [parents[b] for b in order]
            with self._On(self, stream) as st, torch.cuda.stream(st):     # the gather runs on the stream the launches go to
                idx, inv = self._shared_permutation(order)
                q, k_new, v_new = q.index_select(0, idx), k_new.index_select(0, idx), v_new.index_select(0, idx)
        out, lse, qs = self._own_chunk(layer, req_ids, q, k_new, v_new, sm_scale, n_new, stream, window, parents, by_depth, keep_lse=True)
        B, S, _, R, _ = (int(x) for x in qs.shape)
        live = [S] * B if n_new is None else [int(n) for n in n_new]
        if any(live) or order is not None:
            with self._On(self, stream) as st:
                if any(live):
                    depths = 0
                    if by_depth:                                  # the table the own call has just read (kept per tree and window)
                        with torch.cuda.stream(st):
                            depths = self._depth_table(req_ids, parents, live, S, W)
                    self._prefix_fold(handles, first, layer, req_ids, 1, qs.data_ptr(), S, R, lens, np.asarray(live, dtype=np.uint32), depths, W,
                                      int(splits), sm_scale, out.data_ptr(), lse.data_ptr(), st.cuda_stream)
                if order is not None:                             # the way back: behind the fold, on its stream
                    with torch.cuda.stream(st):
                        out = out.index_select(0, inv)
        return out
