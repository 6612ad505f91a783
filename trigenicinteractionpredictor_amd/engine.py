"""Device engine: PyTorch-ROCm tensors for storage, libmmsbm.so for all compute.

One ``EMEngine`` = one GPU context (include/mmsbm.h) holding the train/test link sets (as the
engine's work plan), a workspace and B batched samples (independent EM restarts) of
theta f64[B][P][K] and p f64[B][R][K^3].  Nothing here computes on the host: every numeric step
is a HIP kernel.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib


def _ptr(t: torch.Tensor) -> int:
    return t.data_ptr()


def _host_ptr(a: np.ndarray):
    return a.ctypes.data_as(ctypes.c_void_p) if a.size else None


class EMEngine:
    KERNELS = ("pass_a", "pass_b", "fin")   # kernel ids of include/mmsbm.h's timing calls
    # what each id launches, by plan family (plan_info "small_k"): the large-K kernels (0) run
    # pass A, the gene kernel and the update; the small-K plan (1) pass A, pass B and fin; the
    # fused small-K plans (2: three streams, 3: stream 0 with Y entries) one E-step and fin
    LABELS = {0: {"pass_a": 0, "gene": 1, "fin": 2},
              1: {"pass_a": 0, "pass_b": 1, "fin": 2},
              2: {"fused": 0, "fin": 2},
              3: {"fused": 0, "fin": 2}}

    FAMILIES = {None: _lib.FAMILY_AUTO, "auto": _lib.FAMILY_AUTO, "sku": _lib.FAMILY_SKU,
                "sky": _lib.FAMILY_SKY}

    def __init__(self, K: int, P: int, B: int = 1, R: int = 2, eps: float = 1e-10, device=None,
                 family=None):
        """family (K <= 12, include/mmsbm.h mmsbm_set_family): "sku", "sky" or None / "auto"
        (SK_U at B = 1, SK_Y from B = 2).  A sample's bits depend on the family and on nothing
        else, so a driver whose engines differ in B for one run fixes it (family_for_batch)."""
        if not torch.cuda.is_available():
            raise RuntimeError("EMEngine needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.lib = _lib.load()
        if device is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        else:
            d = torch.device(device)
            self.device = torch.device("cuda", d.index if d.index is not None else torch.cuda.current_device())
        self.K, self.P, self.B, self.R, self.eps = int(K), int(P), int(B), int(R), float(eps)
        self.K3 = self.K ** 3
        ctx = ctypes.c_void_p()
        _lib.check(self.lib.mmsbm_create(self.device.index, ctypes.byref(ctx)))
        self.ctx = ctx
        _lib.check(self.lib.mmsbm_set_shape(self.ctx, self.K, self.R, self.B, self.P, self.eps))
        if family not in self.FAMILIES:
            raise ValueError("family %r: one of sku, sky, auto" % (family,))
        _lib.check(self.lib.mmsbm_set_family(self.ctx, self.FAMILIES[family]))
        self.active = self.B
        self._sets = set()
        self.workspace = None
        self._scan_ws = None      # scan_top's scratch and rank order (built on first use)
        self._scan_order = None
        self._partners_ws = None  # partners_top's scratch
        self._census_ws = None    # census's scratch
        self._pair_census_ws = None   # pair_census's scratch
        self._scan_above_ws = None    # scan_above's scratch
        self.theta = torch.zeros((self.B, self.P, self.K), dtype=torch.float64, device=self.device)
        self.pr = torch.zeros((self.B, self.R, self.K3), dtype=torch.float64, device=self.device)

    def _stream(self, stream=None) -> int:
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        return s.cuda_stream

    # ---------------------------------------------------------------- setup
    def set_links(self, which: int, ids: np.ndarray, counts: np.ndarray, deg: np.ndarray = None):
        """ids int32[E][3] (the keys' string-sorted gene ids), counts int32[E][R], in the link
        dict's insertion order.  deg: the reference's `counter` over ALL train links (a
        link-sharded rank passes the global one); by default the engine counts `ids`."""
        ids = np.ascontiguousarray(ids, dtype=np.int32).reshape(-1, 3)
        counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1, self.R)
        if deg is not None and which == _lib.SET_TRAIN:
            d = np.ascontiguousarray(deg, dtype=np.int32)
            _lib.check(self.lib.mmsbm_set_degree(self.ctx, _host_ptr(d)))
        _lib.check(self.lib.mmsbm_set_links(self.ctx, which, _host_ptr(ids), _host_ptr(counts),
                                            int(ids.shape[0])))
        self._sets.add(which)
        self._alloc_workspace()

    def _alloc_workspace(self):
        nbytes = ctypes.c_int64()
        _lib.check(self.lib.mmsbm_workspace_bytes(self.ctx, ctypes.byref(nbytes)))
        need = max(int(nbytes.value), 256)
        if self.workspace is None or self.workspace.numel() < need:
            self.workspace = torch.empty(need, dtype=torch.uint8, device=self.device)
        _lib.check(self.lib.mmsbm_set_workspace(self.ctx, _ptr(self.workspace), self.workspace.numel()))

    def plan_info(self, which: int = _lib.SET_TRAIN) -> dict:
        v = (ctypes.c_int64 * 16)()
        _lib.check(self.lib.mmsbm_plan_info(self.ctx, which, v))
        keys = ("observations", "rows", "rows_stream0", "wg_stream0", "wg_stream12", "wg_spartial",
                "partial_rows", "genes_per_wg_max", "v_genes", "partial_rows_stream0", "small_k",
                "units", "plan_cus", "unit_target", "y_entries", "gm_groups")
        return dict(zip(keys, [int(x) for x in v]))

    # ------------------------------------------------------------ parameters
    def upload(self, theta: np.ndarray, pr: np.ndarray):
        """theta [B][P][K]; pr in the reference nesting [B][K][K][K][R]."""
        theta = np.asarray(theta, dtype=np.float64).reshape(self.B, self.P, self.K)
        pr = np.asarray(pr, dtype=np.float64).reshape(self.B, self.K3, self.R)
        self.theta.copy_(torch.from_numpy(np.ascontiguousarray(theta)))
        self.pr.copy_(torch.from_numpy(np.ascontiguousarray(pr.transpose(0, 2, 1))))

    # ---------------------------------------------------------- sample slots
    # A restart pool (restarts.run_pool) retires converged samples: it refills a slot with the next
    # pending sample, or moves the last live slot into it and shrinks the active prefix.
    def set_active(self, n: int):
        """Iterate / evaluate samples [0, n) only (include/mmsbm.h mmsbm_set_active)."""
        if not 0 < n <= self.B:
            raise ValueError("active samples %d outside [1, %d]" % (n, self.B))
        _lib.check(self.lib.mmsbm_set_active(self.ctx, int(n)))
        self.active = int(n)

    def upload_slot(self, b: int, theta: np.ndarray, pr: np.ndarray):
        """One sample's theta [P][K] and pr [K][K][K][R] into slot b."""
        th = np.asarray(theta, dtype=np.float64).reshape(self.P, self.K)
        p = np.asarray(pr, dtype=np.float64).reshape(self.K3, self.R)
        self.theta[b].copy_(torch.from_numpy(np.ascontiguousarray(th)))
        self.pr[b].copy_(torch.from_numpy(np.ascontiguousarray(p.T)))

    def download_slot(self, b: int):
        """-> theta [P][K], pr [K][K][K][R] of slot b (host numpy)."""
        th = self.theta[b].cpu().numpy()
        pr = self.pr[b].cpu().numpy().T.reshape(self.K, self.K, self.K, self.R)
        return th, np.ascontiguousarray(pr)

    def move_slot(self, dst: int, src: int):
        """Slot src's parameters into slot dst (a device copy: the bits travel unchanged)."""
        if dst != src:
            self.theta[dst].copy_(self.theta[src])
            self.pr[dst].copy_(self.pr[src])

    def download(self):
        """-> theta [B][P][K], pr [B][K][K][K][R] (host numpy)."""
        th = self.theta.cpu().numpy()
        pr = self.pr.cpu().numpy().transpose(0, 2, 1).reshape(self.B, self.K, self.K, self.K, self.R)
        return th, np.ascontiguousarray(pr)

    # --------------------------------------------------------------- compute
    def iterate(self, n_iters: int = 1, stream=None):
        if _lib.SET_TRAIN not in self._sets:
            raise RuntimeError("train links not set")
        _lib.check(self.lib.mmsbm_iterate(self.ctx, _ptr(self.theta), _ptr(self.pr), int(n_iters),
                                          self._stream(stream)))

    def accumulate(self, nth: torch.Tensor, S: torch.Tensor, stream=None):
        """Link-sharded step 1 (include/mmsbm.h): this context's sums nth [B][P][K], S [B][R][K^3]."""
        if _lib.SET_TRAIN not in self._sets:
            raise RuntimeError("train links not set")
        _lib.check(self.lib.mmsbm_accumulate(self.ctx, _ptr(self.theta), _ptr(self.pr), _ptr(nth),
                                             _ptr(S), self._stream(stream)))

    def mstep(self, nth: torch.Tensor, S: torch.Tensor, stream=None):
        """Link-sharded step 2: M-step from the summed nth / S (ZeroDivisionError like :1018)."""
        _lib.check(self.lib.mmsbm_mstep(self.ctx, _ptr(self.theta), _ptr(self.pr), _ptr(nth), _ptr(S),
                                        self._stream(stream)))

    def loglik_async(self, which: int = _lib.SET_TRAIN, out: torch.Tensor = None, stream=None):
        """[B] device tensor; the kernels write the active prefix only, slots outside it read NaN
        (the fill touches no word the launch writes, so its stream does not matter)."""
        if out is None:
            out = torch.empty(self.B, dtype=torch.float64, device=self.device)
        if self.active < self.B:
            out[self.active:] = float("nan")
        _lib.check(self.lib.mmsbm_loglik(self.ctx, which, _ptr(self.theta), _ptr(self.pr), _ptr(out),
                                         self._stream(stream)))
        return out

    def loglik(self, which: int = _lib.SET_TRAIN) -> np.ndarray:
        """[B] host array; slots outside the active prefix read NaN."""
        if which not in self._sets:
            out = np.zeros(self.B)
        else:
            out = self.loglik_async(which).cpu().numpy()
        out[self.active:] = np.nan
        return out

    def predict(self, ids: np.ndarray) -> np.ndarray:
        """P(r=1) for each row of ids int32[n][3] -> [B][n] (host); rows of slots outside the
        active prefix are NaN (the kernel covers the active samples only)."""
        n = int(ids.shape[0])
        out = torch.empty((self.B, max(n, 1)), dtype=torch.float64, device=self.device)
        if self.active < self.B:
            out[self.active:] = float("nan")
        if n:
            ids_d = torch.from_numpy(np.ascontiguousarray(ids, dtype=np.int32)).to(self.device)
            _lib.check(self.lib.mmsbm_predict(self.ctx, _ptr(ids_d), n, _ptr(self.theta), _ptr(self.pr),
                                              _ptr(out), self._stream()))
        return out[:, :n].cpu().numpy()

    def scan_top_async(self, n: int, known: np.ndarray = None, sample: int = None, stream=None):
        """scan_top without the host copy: -> device tensors (scores f64[n], ids int32[n][3],
        count int64[1]); rows from `count` on are NaN / -1.  Nothing synchronises."""
        from .scan import rank_order
        n = int(n)
        known = np.zeros(0, np.int64) if known is None else np.ascontiguousarray(known, dtype=np.int64)
        if known.size > 1 and not (known[1:] > known[:-1]).all():
            raise ValueError("known keys must be sorted and unique (scan.known_keys)")
        if sample is not None and not 0 <= int(sample) < self.active:
            raise ValueError("sample %r outside the active prefix [0, %d)" % (sample, self.active))
        nbytes = ctypes.c_int64()
        _lib.check(self.lib.mmsbm_scan_workspace_bytes(self.ctx, n, ctypes.byref(nbytes)))
        if self._scan_ws is None or self._scan_ws.numel() < nbytes.value:
            self._scan_ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=self.device)
        if self._scan_order is None:
            self._scan_order = torch.from_numpy(rank_order(max(self.P, 1))).to(self.device)
        known_d = torch.from_numpy(known).to(self.device)
        scores = torch.empty(n, dtype=torch.float64, device=self.device)
        ids = torch.empty((n, 3), dtype=torch.int32, device=self.device)
        count = torch.empty(1, dtype=torch.int64, device=self.device)
        _lib.check(self.lib.mmsbm_scan_topn(
            self.ctx, _ptr(self._scan_order), _ptr(known_d) if known.size else None, int(known.size),
            _ptr(self.theta), _ptr(self.pr), -1 if sample is None else int(sample), n,
            _ptr(self._scan_ws), self._scan_ws.numel(), _ptr(scores), _ptr(ids), _ptr(count),
            self._stream(stream)))
        return scores, ids, count

    def scan_top(self, n: int, known: np.ndarray = None, sample: int = None, stream=None):
        """The n most probable triples of distinct genes (include/mmsbm.h mmsbm_scan_topn):
        -> (scores f64[n'], ids int32[n'][3] in key order) on the host, best first, n' <= n.
        known: sorted int64 packed keys to skip (scan.known_keys); sample: a slot of the active
        prefix, or None for the mean over it."""
        scores, ids, count = self.scan_top_async(n, known, sample, stream)
        if stream is not None:
            stream.synchronize()
        m = int(count.cpu()[0])
        return scores[:m].cpu().numpy(), ids[:m].cpu().numpy()

    def partners_top_async(self, queries, n: int, known=None, sample: int = None, stream=None):
        """partners_top without the host copy: -> device tensors (scores f64[Q][n],
        ids int32[Q][n][3], counts int64[Q]); row i answers queries[i], its rows from counts[i] on
        are NaN / -1.  Nothing synchronises."""
        from .scan import rank_order
        n = int(n)
        queries = np.ascontiguousarray(queries, dtype=np.int32).reshape(-1)
        Q = int(queries.size)
        off = pairs = None
        if known is not None:
            off = np.ascontiguousarray(known[0], dtype=np.int64).reshape(-1)
            pairs = np.ascontiguousarray(known[1], dtype=np.int64).reshape(-1)
            if off.size != Q + 1 or off[0] < 0 or (np.diff(off) < 0).any() or off[-1] > pairs.size:
                raise ValueError("known offsets must be %d non-decreasing indices into the pair keys "
                                 "(scan.partner_known)" % (Q + 1))
            rising = pairs[1:] > pairs[:-1]
            starts = off[1:-1]
            rising[starts[(starts > 0) & (starts < pairs.size)] - 1] = True   # a new query's slice
            if not rising[int(off[0]):max(int(off[-1]) - 1, int(off[0]))].all():
                raise ValueError("each query's known pair keys must be sorted and unique "
                                 "(scan.partner_known)")
        if sample is not None and not 0 <= int(sample) < self.active:
            raise ValueError("sample %r outside the active prefix [0, %d)" % (sample, self.active))
        nbytes = ctypes.c_int64()
        _lib.check(self.lib.mmsbm_partners_workspace_bytes(self.ctx, Q, n, ctypes.byref(nbytes)))
        if self._partners_ws is None or self._partners_ws.numel() < nbytes.value:
            self._partners_ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=self.device)
        if self._scan_order is None:
            self._scan_order = torch.from_numpy(rank_order(max(self.P, 1))).to(self.device)
        off_d = pairs_d = None
        if off is not None:
            off_d = torch.from_numpy(off).to(self.device)
            pairs_d = torch.from_numpy(pairs if pairs.size else np.zeros(1, np.int64)).to(self.device)
        scores = torch.empty((Q, n), dtype=torch.float64, device=self.device)
        ids = torch.empty((Q, n, 3), dtype=torch.int32, device=self.device)
        counts = torch.empty(Q, dtype=torch.int64, device=self.device)
        _lib.check(self.lib.mmsbm_partners_topn(
            self.ctx, _ptr(self._scan_order), _host_ptr(queries), Q,
            _ptr(off_d) if off_d is not None else None, _ptr(pairs_d) if pairs_d is not None else None,
            _ptr(self.theta), _ptr(self.pr), -1 if sample is None else int(sample), n,
            _ptr(self._partners_ws), self._partners_ws.numel(), _ptr(scores), _ptr(ids), _ptr(counts),
            self._stream(stream)))
        return scores, ids, counts

    def partners_top(self, queries, n: int, known=None, sample: int = None, stream=None):
        """For each query gene id, its n most probable partner pairs (include/mmsbm.h
        mmsbm_partners_topn): -> one (scores f64[n'], ids int32[n'][3]) pair per query on the host,
        best first, n' <= n; an id row is the whole triple in key order, the query included.
        known: (known_off, known_pairs) of scan.partner_known for these queries; sample: a slot of
        the active prefix, or None for the mean over it."""
        scores, ids, counts = self.partners_top_async(queries, n, known, sample, stream)
        if stream is not None:
            stream.synchronize()
        counts, scores, ids = counts.cpu().numpy(), scores.cpu().numpy(), ids.cpu().numpy()
        return [(scores[i, :int(m)].copy(), ids[i, :int(m)].copy()) for i, m in enumerate(counts)]

    def census_async(self, thresholds, known: np.ndarray = None, sample: int = None, stream=None):
        """census without the host copy: -> device tensors (counts int64[len(thresholds)] in the
        caller's order, total int64[1]).  Nothing synchronises."""
        from .scan import census_chunks, rank_order
        max_m = int(self.lib.mmsbm_census_max_m())
        chunks, perm = census_chunks(thresholds, max_m)      # ValueError on a NaN or infinite one
        known = np.zeros(0, np.int64) if known is None else np.ascontiguousarray(known, dtype=np.int64)
        if known.size > 1 and not (known[1:] > known[:-1]).all():
            raise ValueError("known keys must be sorted and unique (scan.known_keys)")
        if sample is not None and not 0 <= int(sample) < self.active:
            raise ValueError("sample %r outside the active prefix [0, %d)" % (sample, self.active))
        nbytes = ctypes.c_int64()
        _lib.check(self.lib.mmsbm_census_workspace_bytes(self.ctx, max(c.size for c in chunks),
                                                         ctypes.byref(nbytes)))
        if self._census_ws is None or self._census_ws.numel() < nbytes.value:
            self._census_ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=self.device)
        if self._scan_order is None:
            self._scan_order = torch.from_numpy(rank_order(max(self.P, 1))).to(self.device)
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(s):      # the tensors below belong to the stream the kernels run on
            known_d = torch.from_numpy(known).to(self.device)
            outs = []
            for chunk in chunks:
                thr_d = torch.from_numpy(chunk if chunk.size else np.zeros(1)).to(self.device)
                out = torch.empty(chunk.size + 1, dtype=torch.int64, device=self.device)
                _lib.check(self.lib.mmsbm_scan_census(
                    self.ctx, _ptr(self._scan_order), _ptr(known_d) if known.size else None, int(known.size),
                    _ptr(self.theta), _ptr(self.pr), -1 if sample is None else int(sample), _ptr(thr_d),
                    int(chunk.size), _ptr(self._census_ws), self._census_ws.numel(), _ptr(out), s.cuda_stream))
                outs.append(out)
            total = outs[-1][-1:]
            if len(outs) == 1 and (perm == np.arange(perm.size)).all():
                counts = outs[0][:-1]      # one call, thresholds already ascending: nothing to put back
            else:            # sorted position i answers the caller's thresholds[perm[i]]
                counts = torch.empty(perm.size, dtype=torch.int64, device=self.device)
                counts[torch.from_numpy(perm).to(self.device)] = torch.cat([o[:-1] for o in outs])
        return counts, total

    def census(self, thresholds, known: np.ndarray = None, sample: int = None, stream=None):
        """The score census (include/mmsbm.h mmsbm_scan_census): -> (counts int64[len(thresholds)],
        total int) on the host; counts[i] = the eligible triples (those scan_top ranks: distinct
        genes, key not in `known`) whose score is >= thresholds[i], total = the eligible triples.
        The thresholds may come in any order, with duplicates, in any number or none; a NaN or an
        infinite one raises ValueError.  known, sample: as for scan_top.  The scores are scan_top's
        bit for bit, so census(scan_top(n)[0]) numbers that list's entries."""
        counts, total = self.census_async(thresholds, known, sample, stream)
        if stream is not None:
            stream.synchronize()
        return counts.cpu().numpy(), int(total.cpu()[0])

    # -------------------------------------------------------- threshold scan
    def _scan_above(self, threshold, known, sample, stream, limit):
        """-> (scores f64[n] and packed keys int64[n] on the device, sorted by the scan's total
        order; the kernel's count int64[1] on the device; the census's count n; the launch stream)."""
        from .scan import LimitError
        threshold = float(threshold)
        if not np.isfinite(threshold):
            raise ValueError("the threshold must be a finite number")
        counts, _ = self.census_async([threshold], known, sample, stream)    # validates known and sample
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(s):
            n = int(counts.cpu()[0])        # the same score bits: exactly the rows the kernel will find
        if n > int(limit):
            raise LimitError(n, int(limit))
        known = np.zeros(0, np.int64) if known is None else np.ascontiguousarray(known, dtype=np.int64)
        nbytes = ctypes.c_int64()
        _lib.check(self.lib.mmsbm_scan_above_workspace_bytes(self.ctx, ctypes.byref(nbytes)))
        if self._scan_above_ws is None or self._scan_above_ws.numel() < nbytes.value:
            self._scan_above_ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=self.device)
        with torch.cuda.stream(s):      # the tensors below belong to the stream the kernels run on
            known_d = torch.from_numpy(known).to(self.device)
            scores = torch.empty(n, dtype=torch.float64, device=self.device)
            keys = torch.empty(n, dtype=torch.int64, device=self.device)
            found = torch.empty(1, dtype=torch.int64, device=self.device)
            _lib.check(self.lib.mmsbm_scan_above(
                self.ctx, _ptr(self._scan_order), _ptr(known_d) if known.size else None, int(known.size),
                _ptr(self.theta), _ptr(self.pr), -1 if sample is None else int(sample), threshold, n,
                _ptr(self._scan_above_ws), self._scan_above_ws.numel(), _ptr(scores) if n else None,
                _ptr(keys) if n else None, _ptr(found), s.cuda_stream))
            # the rows arrive in any order; two stable sorts give the scan's: score descending,
            # equal scores by key ascending
            keys, at = torch.sort(keys, stable=True)
            scores = scores[at]
            scores, at = torch.sort(scores, descending=True, stable=True)
            keys = keys[at]
        return scores, keys, found, n, s

    def _keys_to_ids(self, keys: torch.Tensor) -> torch.Tensor:
        """Packed keys int64[n] (device) -> gene ids int32[n][3] in key order."""
        P = max(self.P, 1)
        order = self._scan_order
        return torch.stack([order[keys // (P * P)], order[(keys // P) % P], order[keys % P]], dim=1)

    def scan_above_async(self, threshold, known: np.ndarray = None, sample: int = None, stream=None,
                         limit: int = 1 << 26):
        """scan_above without the host copy: -> device tensors (scores f64[n], ids int32[n][3]) on
        the launch stream.  The number of rows comes from the census first (one host read of one
        integer); a count above `limit` raises before anything is launched for the list."""
        scores, keys, _, _, s = self._scan_above(threshold, known, sample, stream, limit)
        with torch.cuda.stream(s):
            return scores, self._keys_to_ids(keys)

    def scan_above(self, threshold, known: np.ndarray = None, sample: int = None, stream=None,
                   limit: int = 1 << 26):
        """Every eligible triple (those scan_top ranks: distinct genes, key not in `known`) whose
        score is >= threshold (include/mmsbm.h mmsbm_scan_above): -> (scores f64[n], ids int32[n][3]
        in key order) on the host, sorted by the scan's total order (score descending, equal scores
        by packed key ascending), n = census([threshold]).  The scores are scan_top's bit for bit, so
        the first rows are scan_top's list.  A NaN or infinite threshold raises ValueError, as does a
        count above `limit` (scan.LimitError, with the count and the limit): 16 bytes per row on the
        device, twice that while sorting.  known, sample: as for scan_top."""
        scores, keys, found, n, s = self._scan_above(threshold, known, sample, stream, limit)
        with torch.cuda.stream(s):
            ids = self._keys_to_ids(keys).cpu().numpy()
            scores, found = scores.cpu().numpy(), int(found.cpu()[0])
        assert found == n, "mmsbm_scan_above found %d rows where the census counted %d" % (found, n)
        return scores, ids

    def scan_top_any(self, n: int, known: np.ndarray = None, sample: int = None, limit: int = 1 << 26):
        """scan_top for any n >= 1: -> (scores f64[n'], ids int32[n'][3]) on the host, best first,
        n' <= n.  Up to mmsbm_scan_max_n() it is scan_top; above, censuses bracket a threshold
        between the eligible total and the last score of scan_top(max) (scan.bracket_threshold),
        scan_above fetches what lies at or above it and the list is cut to n.  Exact: the three
        kernels see the same score bits under the same total order.  `limit`: as for scan_above
        (reached only when more than that many triples tie around rank n)."""
        from .scan import bracket_threshold
        n = int(n)
        if n < 1:
            raise ValueError("scan_top_any needs n >= 1")
        max_n = int(self.lib.mmsbm_scan_max_n())
        if n <= max_n:
            return self.scan_top(n, known, sample)
        scores, ids = self.scan_top(max_n, known, sample)
        if scores.size < max_n:         # fewer eligible triples than that: this is all of them
            return scores, ids
        lo = bracket_threshold(n, float(scores[-1]), lambda t: self.census(t, known, sample)[0])
        scores, ids = self.scan_above(lo, known, sample, limit=limit)
        return scores[:n], ids[:n]

    # ----------------------------------------------------------- pair census
    def _pair_census_rank(self, thresholds, known, sample, stream):
        """The pair census in rank positions: -> (device int32 [P][P][len(thresholds)], filled for
        x < y only, thresholds in the caller's order; the launch stream).  One call of
        mmsbm_pair_census per mmsbm_pair_census_max_m() thresholds."""
        from .scan import census_chunks, rank_order
        max_m = int(self.lib.mmsbm_pair_census_max_m())
        chunks, perm = census_chunks(thresholds, max_m)      # ValueError on a NaN or infinite one
        known = np.zeros(0, np.int64) if known is None else np.ascontiguousarray(known, dtype=np.int64)
        if known.size > 1 and not (known[1:] > known[:-1]).all():
            raise ValueError("known keys must be sorted and unique (scan.known_keys)")
        if sample is not None and not 0 <= int(sample) < self.active:
            raise ValueError("sample %r outside the active prefix [0, %d)" % (sample, self.active))
        nbytes = ctypes.c_int64()
        _lib.check(self.lib.mmsbm_pair_census_workspace_bytes(self.ctx, max(c.size for c in chunks),
                                                              ctypes.byref(nbytes)))
        if self._pair_census_ws is None or self._pair_census_ws.numel() < nbytes.value:
            self._pair_census_ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=self.device)
        if self._scan_order is None:
            self._scan_order = torch.from_numpy(rank_order(max(self.P, 1))).to(self.device)
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(s):      # the tensors below belong to the stream the kernels run on
            known_d = torch.from_numpy(known).to(self.device)
            outs = []
            for chunk in chunks:
                thr_d = torch.from_numpy(chunk if chunk.size else np.zeros(1)).to(self.device)
                out = torch.empty((self.P, self.P, chunk.size), dtype=torch.int32, device=self.device)
                _lib.check(self.lib.mmsbm_pair_census(
                    self.ctx, _ptr(self._scan_order), _ptr(known_d) if known.size else None, int(known.size),
                    _ptr(self.theta), _ptr(self.pr), -1 if sample is None else int(sample), _ptr(thr_d),
                    int(chunk.size), _ptr(self._pair_census_ws), self._pair_census_ws.numel(),
                    _ptr(out) if chunk.size else None, s.cuda_stream))
                outs.append(out)
            if len(outs) == 1 and (perm == np.arange(perm.size)).all():
                mat = outs[0]           # one call, thresholds already ascending: nothing to put back
            else:            # sorted position i answers the caller's thresholds[perm[i]]
                mat = torch.empty((self.P, self.P, perm.size), dtype=torch.int32, device=self.device)
                mat[:, :, torch.from_numpy(perm).to(self.device)] = torch.cat(outs, dim=2)
        return mat, s

    def pair_census_async(self, thresholds, known: np.ndarray = None, sample: int = None, stream=None):
        """pair_census without the host copy: -> a device tensor int32 [P][P][len(thresholds)] in
        gene ids, symmetric with a zero diagonal, thresholds in the caller's order.  Nothing
        synchronises."""
        from .scan import rank_of, rank_order
        mat, s = self._pair_census_rank(thresholds, known, sample, stream)
        with torch.cuda.stream(s):
            rank = torch.from_numpy(rank_of(rank_order(self.P))).to(self.device)
            mat = mat + mat.transpose(0, 1)             # x < y was filled, the rest is zero
            return mat[rank][:, rank].contiguous()      # [g1][g2] = [rank[g1]][rank[g2]]

    def pair_census(self, thresholds, known: np.ndarray = None, sample: int = None, stream=None):
        """The pair census (include/mmsbm.h mmsbm_pair_census): -> int32 [P][P][len(thresholds)] on
        the host; [g1][g2][i] = the eligible triples (those scan_top ranks: distinct genes, key not
        in `known`) that contain the genes g1 and g2 and score >= thresholds[i]: the predicted,
        unmeasured interactions of the double-mutant query (g1, g2).  Symmetric, zero diagonal.
        The thresholds may come in any order, with duplicates, in any number or none; a NaN or an
        infinite one raises ValueError.  known, sample: as for census; the scores are the census's
        bit for bit, so the sum over g1 < g2 is three times census(thresholds)."""
        mat = self.pair_census_async(thresholds, known, sample, stream)
        if stream is not None:
            stream.synchronize()
        return mat.cpu().numpy()

    def pairs_top(self, n: int, threshold: float, known: np.ndarray = None, sample: int = None):
        """The n pairs with the most eligible triples scoring >= threshold: -> (counts int64[n'],
        eligible int64[n'] = the pair's eligible triples in all (scan.pair_eligible), ids
        int32[n'][2] in key order) on the host, n' = min(n, C(P, 2)).  Ordered by count descending,
        equal counts by the pair's rank-position key x P + y ascending.  The selection is one
        torch.topk on the device over count * P^2 + (P^2 - 1 - key)."""
        from .scan import pair_eligible, rank_order
        mat, s = self._pair_census_rank([float(threshold)], known, sample, None)
        P = self.P
        n = max(0, min(int(n), P * (P - 1) // 2))
        with torch.cuda.stream(s):
            key = torch.arange(P * P, dtype=torch.int64, device=self.device)
            upper = (key // P) < (key % P)
            combined = torch.where(upper, mat[:, :, 0].reshape(-1).to(torch.int64) * (P * P) + (P * P - 1 - key),
                                   torch.full_like(key, -1))
            best, _ = torch.topk(combined, n)
        best = best.cpu().numpy()
        counts = best // (P * P)
        key = P * P - 1 - best % (P * P)
        order = rank_order(max(P, 1))
        ids = np.stack([order[key // P], order[key % P]], axis=1).astype(np.int32).reshape(-1, 2)
        eligible = pair_eligible(P, known)[ids[:, 0], ids[:, 1]].astype(np.int64)
        return counts.astype(np.int64), eligible, ids

    def gene_census(self, thresholds, known: np.ndarray = None, sample: int = None):
        """-> int64 [P][len(thresholds)] on the host: the eligible triples that contain each gene
        and score >= each threshold.  The row sums of the pair matrix halved: every triple of a gene
        sits in two of the gene's pairs."""
        mat = self.pair_census_async(thresholds, known, sample)
        return (mat.sum(dim=1, dtype=torch.int64) // 2).cpu().numpy()

    # ---------------------------------------------------------- measurement
    def kernels(self) -> dict:
        """{label: kernel id} of the kernels one iteration launches, in launch order (LABELS)."""
        return dict(self.LABELS[self.plan_info(_lib.SET_TRAIN)["small_k"]])

    def _kid(self, kernel) -> int:
        if kernel in self.KERNELS:
            return self.KERNELS.index(kernel)
        for labels in self.LABELS.values():
            if kernel in labels:
                return labels[kernel]
        raise KeyError(kernel)

    def time_kernel(self, kernel: str, n: int = 50, stream=None) -> float:
        """Average device ms of n back-to-back launches of one kernel of the iteration (a label
        of kernels() or an id name of KERNELS); the parameters are unchanged."""
        ms = ctypes.c_double()
        _lib.check(self.lib.mmsbm_time_kernel(self.ctx, self._kid(kernel), _ptr(self.theta),
                                              _ptr(self.pr), int(n), self._stream(stream),
                                              ctypes.byref(ms)))
        return ms.value

    def timing(self, stride: int = 1):
        """Record HIP event pairs around the kernels of every `stride`-th iteration (0: off)."""
        _lib.check(self.lib.mmsbm_timing(self.ctx, int(stride)))

    def timing_result(self, kernel: str = "pass_a"):
        """-> (summed device ms, launches) of one kernel since timing(stride)."""
        tot, cnt = ctypes.c_double(), ctypes.c_int64()
        _lib.check(self.lib.mmsbm_timing_result(self.ctx, self._kid(kernel),
                                                ctypes.byref(tot), ctypes.byref(cnt)))
        return tot.value, cnt.value

    def synchronize(self):
        torch.cuda.synchronize(self.device)

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.mmsbm_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
