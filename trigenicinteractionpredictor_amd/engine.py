"""Device engine: PyTorch-ROCm tensors for storage, libmmsbm.so for all compute.

One ``EMEngine`` = one GPU context (include/mmsbm.h) holding the train/test link sets (as the
engine's work plan), a workspace and B batched samples (independent EM restarts) of
theta f64[B][P][K] and p f64[B][R][K^3].  Nothing here computes on the host: every numeric step
is a HIP kernel.
"""
from __future__ import annotations

import contextlib
import ctypes

import numpy as np
import torch

from . import _lib
from .scan import (LimitError, bracket_threshold, census_chunks, check_known_keys, check_pair_mask,
                   check_partner_known, check_screen_known, pair_eligible, rank_of, rank_order, screen_pairs,
                   vote_level_chunks)

_CURRENT_STREAM = contextlib.nullcontext()     # a scan call without a stream: nothing to make current


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
        self._scan_ws = {}        # the scan families' scratch, by family (scan_workspace)
        self._scan_order = None   # their rank order (scan_order: built on first use)
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

    # --------------------------------------------------------- scan families
    # The scan, the partner scan, the census, the pair census, the threshold scan and the vote scan
    # share what is below: one check of the sample, one rank order, one scratch tensor per family and one context
    # that owns every tensor of a call.
    def _sample(self, sample) -> int:
        """A slot of the active prefix, or None (-1 in C) for the mean over it."""
        if sample is None:
            return -1
        if not 0 <= int(sample) < self.active:
            raise ValueError("sample %r outside the active prefix [0, %d)" % (sample, self.active))
        return int(sample)

    @property
    def scan_order(self) -> torch.Tensor:
        """scan.rank_order(P) on the device, int32[P]: the first argument of every scan family's C
        call.  Built by whichever call comes first, and complete before it returns, so every
        stream may read it."""
        if self._scan_order is None:
            self._scan_order = torch.from_numpy(rank_order(max(self.P, 1))).to(self.device)
            torch.cuda.current_stream(self.device).synchronize()
        return self._scan_order

    def scan_workspace(self, family: str, *size_args) -> torch.Tensor:
        """The scratch of one family ("scan", "partners", "census", "pair_census", "scan_above",
        "scan_votes", "scan_quorum", "scan_spread", "screen", "pair_votes"), grown to what mmsbm_<family>_workspace_bytes(ctx, *size_args) asks: uint8 on the device.
        The screen scan's statistics (screen_quorum_*, screen_spread_*) run in the "screen" scratch,
        the partner scan's (partners_quorum_*, partners_spread_*) in the "partners" scratch."""
        nbytes = ctypes.c_int64()
        _lib.check(getattr(self.lib, "mmsbm_%s_workspace_bytes" % family)(self.ctx, *size_args,
                                                                          ctypes.byref(nbytes)))
        ws = self._scan_ws.get(family)
        if ws is None or ws.numel() < nbytes.value:
            ws = self._scan_ws[family] = torch.empty(int(nbytes.value), dtype=torch.uint8, device=self.device)
        return ws

    @contextlib.contextmanager
    def _scan_call(self, known, sample, stream, mask=None):
        """One call of a scan family: checks `known` and `sample`, makes the launch stream current
        and uploads the keys; -> (head, the stream), head = the C calls' (ctx, order, known or NULL,
        n_known, theta, pr, sample).  Whatever the call uploads or allocates it creates inside, so
        every tensor belongs to the stream its kernels run on.  mask: a pair mask (scan.pair_mask) for
        the masked entries, checked and uploaded here too; the head then is theirs, the mask behind
        n_known."""
        known = check_known_keys(known)
        sample = self._sample(sample)
        if mask is not None:
            mask = check_pair_mask(mask, self.P)
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        with torch.cuda.stream(s) if stream is not None else _CURRENT_STREAM:
            known_d = torch.from_numpy(known).to(self.device) if known.size else None
            head = (self.ctx, _ptr(self.scan_order), _ptr(known_d) if known.size else None, int(known.size))
            if mask is not None:
                words = mask if mask.flags.writeable else mask.copy()   # torch takes no read-only array
                mask_d = torch.from_numpy(words.view(np.int32)).to(self.device)   # the same 32-bit words
                head += (_ptr(mask_d),)
            yield head + (_ptr(self.theta), _ptr(self.pr), sample), s

    def _per_threshold(self, family, entry, plan, call, shape, dtype, axis):
        """The census families' loop inside a _scan_call: one call of `entry` per chunk of `plan`
        (scan.census_chunks) into a tensor of shape(len(chunk)) -> (the chunks' first len(chunk)
        entries along `axis`, joined and put back in the caller's threshold order; the last chunk's
        whole output).  An output without elements is passed as NULL."""
        (chunks, perm), (head, s) = plan, call
        ws = self.scan_workspace(family, max(c.size for c in chunks))
        outs = []
        for chunk in chunks:
            thr_d = torch.from_numpy(chunk if chunk.size else np.zeros(1)).to(self.device)
            out = torch.empty(shape(chunk.size), dtype=dtype, device=self.device)
            _lib.check(entry(*head, _ptr(thr_d), int(chunk.size), _ptr(ws), ws.numel(),
                             _ptr(out) if out.numel() else None, s.cuda_stream))
            outs.append(out)
        parts = [o.narrow(axis, 0, c.size) for o, c in zip(outs, chunks)]
        if len(parts) == 1 and (perm == np.arange(perm.size)).all():
            return parts[0], outs[-1]   # one call, thresholds already ascending: nothing to put back
        joined = torch.cat(parts, dim=axis)     # sorted position i answers the caller's thresholds[perm[i]]
        perm_d = torch.from_numpy(perm).to(self.device)
        return torch.empty_like(joined).index_copy_(axis, perm_d, joined), outs[-1]

    def scan_top_async(self, n: int, known: np.ndarray = None, sample: int = None, stream=None, mask=None):
        """scan_top without the host copy: -> device tensors (scores f64[n], ids int32[n][3],
        count int64[1]); rows from `count` on are NaN / -1.  Nothing synchronises."""
        n = int(n)
        entry = self.lib.mmsbm_scan_topn if mask is None else self.lib.mmsbm_scan_topn_masked
        with self._scan_call(known, sample, stream, mask) as (head, s):
            ws = self.scan_workspace("scan", n)
            scores = torch.empty(n, dtype=torch.float64, device=self.device)
            ids = torch.empty((n, 3), dtype=torch.int32, device=self.device)
            count = torch.empty(1, dtype=torch.int64, device=self.device)
            _lib.check(entry(*head, n, _ptr(ws), ws.numel(), _ptr(scores), _ptr(ids), _ptr(count), s.cuda_stream))
        return scores, ids, count

    def scan_top(self, n: int, known: np.ndarray = None, sample: int = None, stream=None, mask=None):
        """The n most probable triples of distinct genes (include/mmsbm.h mmsbm_scan_topn):
        -> (scores f64[n'], ids int32[n'][3] in key order) on the host, best first, n' <= n.
        known: sorted int64 packed keys to skip (scan.known_keys); sample: a slot of the active
        prefix, or None for the mean over it.  mask: as for census (mmsbm_scan_topn_masked): the
        exact top n over the triples without a blocked pair; None: the unmasked call."""
        scores, ids, count = self.scan_top_async(n, known, sample, stream, mask)
        if stream is not None:
            stream.synchronize()
        m = int(count.cpu()[0])
        return scores[:m].cpu().numpy(), ids[:m].cpu().numpy()

    def partners_top_async(self, queries, n: int, known=None, sample: int = None, stream=None, mask=None):
        """partners_top without the host copy: -> device tensors (scores f64[Q][n],
        ids int32[Q][n][3], counts int64[Q]); row i answers queries[i], its rows from counts[i] on
        are NaN / -1.  Nothing synchronises."""
        n = int(n)
        queries = np.ascontiguousarray(queries, dtype=np.int32).reshape(-1)
        Q = int(queries.size)
        off, pairs = (None, None) if known is None else check_partner_known(known, Q)
        entry = self.lib.mmsbm_partners_topn if mask is None else self.lib.mmsbm_partners_topn_masked
        with self._scan_call(None, sample, stream, mask) as ((ctx, order, _, _, *params), s):   # no key table
            ws = self.scan_workspace("partners", Q, n)   # params: the mask (if any), theta, pr, the sample
            off_d = pairs_d = None
            if off is not None:
                off_d = torch.from_numpy(off).to(self.device)
                pairs_d = torch.from_numpy(pairs if pairs.size else np.zeros(1, np.int64)).to(self.device)
            scores = torch.empty((Q, n), dtype=torch.float64, device=self.device)
            ids = torch.empty((Q, n, 3), dtype=torch.int32, device=self.device)
            counts = torch.empty(Q, dtype=torch.int64, device=self.device)
            _lib.check(entry(
                ctx, order, _host_ptr(queries), Q, _ptr(off_d) if off_d is not None else None,
                _ptr(pairs_d) if pairs_d is not None else None, *params, n, _ptr(ws), ws.numel(),
                _ptr(scores), _ptr(ids), _ptr(counts), s.cuda_stream))
        return scores, ids, counts

    def partners_top(self, queries, n: int, known=None, sample: int = None, stream=None, mask=None):
        """For each query gene id, its n most probable partner pairs (include/mmsbm.h
        mmsbm_partners_topn): -> one (scores f64[n'], ids int32[n'][3]) pair per query on the host,
        best first, n' <= n; an id row is the whole triple in key order, the query included.
        known: (known_off, known_pairs) of scan.partner_known for these queries; sample: a slot of
        the active prefix, or None for the mean over it.  mask: a pair mask (scan.pair_mask;
        mmsbm_partners_topn_masked): a pair that is blocked, or holds a gene that forms a blocked pair
        with the query, is no candidate; a query with none left gets an empty list."""
        scores, ids, counts = self.partners_top_async(queries, n, known, sample, stream, mask)
        if stream is not None:
            stream.synchronize()
        counts, scores, ids = counts.cpu().numpy(), scores.cpu().numpy(), ids.cpu().numpy()
        return [(scores[i, :int(m)].copy(), ids[i, :int(m)].copy()) for i, m in enumerate(counts)]

    # ----------------------------------------------------- partner statistics
    @property
    def partners_stat_max_depth(self) -> int:
        """mmsbm_partners_stat_max_depth(): the deepest per-element sorted lists the partner scan's
        statistics kernel holds (quorum_max_depth, and spread_max_trim + 1)."""
        return int(self.lib.mmsbm_partners_stat_max_depth())

    def _partners_stat_top_async(self, queries, n, stat, arg, known, stream, mask):
        """mmsbm_partners_stat_topn -> device tensors as partners_top_async returns them."""
        n = int(n)
        queries = np.ascontiguousarray(queries, dtype=np.int32).reshape(-1)
        Q = int(queries.size)
        off, pairs = (None, None) if known is None else check_partner_known(known, Q)
        with self._scan_call(None, None, stream, mask) as ((ctx, order, _, _, *rest), s):   # no key table
            # rest: the mask (if any), theta, pr and the sample, which the stat entry does not take
            mask_p, (theta, pr, _) = (rest[0], rest[1:]) if mask is not None else (None, rest)
            ws = self.scan_workspace("partners", Q, n)
            off_d = pairs_d = None
            if off is not None:
                off_d = torch.from_numpy(off).to(self.device)
                pairs_d = torch.from_numpy(pairs if pairs.size else np.zeros(1, np.int64)).to(self.device)
            scores = torch.empty((Q, n), dtype=torch.float64, device=self.device)
            ids = torch.empty((Q, n, 3), dtype=torch.int32, device=self.device)
            counts = torch.empty(Q, dtype=torch.int64, device=self.device)
            _lib.check(self.lib.mmsbm_partners_stat_topn(
                ctx, order, _host_ptr(queries), Q, _ptr(off_d) if off_d is not None else None,
                _ptr(pairs_d) if pairs_d is not None else None, mask_p, theta, pr, stat, arg, n, _ptr(ws),
                ws.numel(), _ptr(scores), _ptr(ids), _ptr(counts), s.cuda_stream))
        return scores, ids, counts

    def partners_quorum_top_async(self, queries, n: int, min_votes: int = None, known=None, stream=None,
                                  mask=None):
        """partners_quorum_top without the host copy: -> device tensors as partners_top_async returns
        them.  Nothing synchronises."""
        m = self._screen_votes(min_votes)       # ValueError before anything is uploaded
        return self._partners_stat_top_async(queries, n, _lib.MMSBM_PARTNERS_STAT_QUORUM, m, known, stream, mask)

    def partners_quorum_top(self, queries, n: int, min_votes: int = None, known=None, stream=None, mask=None):
        """For each query gene id, its n partner pairs with the highest quorum score (include/mmsbm.h
        mmsbm_partners_stat_topn, MMSBM_PARTNERS_STAT_QUORUM): q_m = the m-th largest of the active
        slots' own partners_top(sample=s) words, m = min_votes (None: every active slot, the minimum
        over them; 1: the maximum).  At least m restarts score a pair at or above T exactly when its
        q_m >= T.  -> lists as partners_top returns them, best first under its total order.
        min_votes outside [1, active] raises ValueError; a depth min(m, active - m + 1) above
        partners_stat_max_depth raises MMSBMError (MMSBM_ERR_UNSUPPORTED).  known, mask: as for
        partners_top."""
        return self._screen_lists(self.partners_quorum_top_async(queries, n, min_votes, known, stream, mask), stream)

    def partners_spread_top_async(self, queries, n: int, trim: int = 0, known=None, stream=None, mask=None):
        """partners_spread_top without the host copy: -> device tensors as partners_top_async returns
        them.  Nothing synchronises."""
        trim = self._spread_trim(trim)          # ValueError before anything is uploaded
        return self._partners_stat_top_async(queries, n, _lib.MMSBM_PARTNERS_STAT_SPREAD, trim, known, stream, mask)

    def partners_spread_top(self, queries, n: int, trim: int = 0, known=None, stream=None, mask=None):
        """For each query gene id, the n partner pairs on which the active slots disagree most
        (mmsbm_partners_stat_topn, MMSBM_PARTNERS_STAT_SPREAD): ranked by d_t = q_{1+t} - q_{ns-t},
        t = trim, over the ns = active slots' own partners_top(sample=s) words (trim = 0: max - min).
        -> lists as partners_top returns them.  Fewer than two active slots and a trim outside
        spread_trims' rule raise ValueError; a legal trim above partners_stat_max_depth - 1 raises
        MMSBMError (MMSBM_ERR_UNSUPPORTED).  known, mask: as for partners_top."""
        return self._screen_lists(self.partners_spread_top_async(queries, n, trim, known, stream, mask), stream)

    # ----------------------------------------------------------- screen scan
    @contextlib.contextmanager
    def _screen_call(self, pairs, known, sample, stream, mask, n):
        """One call of the screen scan inside a _scan_call: checks the pairs and `known`, uploads the
        slices and sizes the scratch; -> (Q, the C calls' arguments up to the sample, the scratch's
        (pointer, bytes), the stream)."""
        pairs = screen_pairs(pairs, self.P)
        Q = int(pairs.shape[0])
        off, thirds = (None, None) if known is None else check_screen_known(known, Q)
        with self._scan_call(None, sample, stream, mask) as ((ctx, order, _, _, *rest), s):   # no key table
            mask_p, params = (rest[0], rest[1:]) if mask is not None else (None, rest)
            ws = self.scan_workspace("screen", Q, int(n))
            off_d = thirds_d = None
            if off is not None:
                off_d = torch.from_numpy(off).to(self.device)
                thirds_d = torch.from_numpy(thirds if thirds.size else np.zeros(1, np.int32)).to(self.device)
            yield Q, (ctx, order, _host_ptr(pairs), Q, _ptr(off_d) if off_d is not None else None,
                      _ptr(thirds_d) if thirds_d is not None else None, mask_p, *params), (_ptr(ws), ws.numel()), s

    def screen_top_async(self, pairs, n: int, known=None, sample: int = None, stream=None, mask=None):
        """screen_top without the host copy: -> device tensors (scores f64[Q][n], ids int32[Q][n][3],
        counts int64[Q]); row i answers pairs[i], its rows from counts[i] on are NaN / -1.  Nothing
        synchronises."""
        n = int(n)
        with self._screen_call(pairs, known, sample, stream, mask, n) as (Q, head, ws, s):
            scores = torch.empty((Q, n), dtype=torch.float64, device=self.device)
            ids = torch.empty((Q, n, 3), dtype=torch.int32, device=self.device)
            counts = torch.empty(Q, dtype=torch.int64, device=self.device)
            _lib.check(self.lib.mmsbm_screen_topn(*head, n, *ws, _ptr(scores), _ptr(ids), _ptr(counts),
                                                  s.cuda_stream))
        return scores, ids, counts

    def screen_top(self, pairs, n: int, known=None, sample: int = None, stream=None, mask=None):
        """For each query pair of gene ids, its n most probable third genes (include/mmsbm.h
        mmsbm_screen_topn): -> one (scores f64[n'], ids int32[n'][3]) pair per query on the host,
        best first, n' <= n; an id row is the whole triple in key order, the pair included.
        known: (known_off, known_thirds) of scan.screen_known for these pairs; sample: a slot of the
        active prefix, or None for the mean over it; mask: a pair mask (scan.pair_mask): a third gene
        that forms a blocked pair with either gene of the query is not eligible, and a query whose own
        pair is blocked has no candidate."""
        scores, ids, counts = self.screen_top_async(pairs, n, known, sample, stream, mask)
        if stream is not None:
            stream.synchronize()
        counts, scores, ids = counts.cpu().numpy(), scores.cpu().numpy(), ids.cpu().numpy()
        return [(scores[i, :int(m)].copy(), ids[i, :int(m)].copy()) for i, m in enumerate(counts)]

    def screen_scores_async(self, pairs, known=None, sample: int = None, stream=None, mask=None):
        """screen_scores without the host copy: -> a device tensor f64[Q][P] indexed by the third
        gene's id.  Nothing synchronises."""
        with self._screen_call(pairs, known, sample, stream, mask, 0) as (Q, head, ws, s):
            out = torch.empty((Q, self.P), dtype=torch.float64, device=self.device)
            _lib.check(self.lib.mmsbm_screen_scores(*head, *ws, _ptr(out), s.cuda_stream))
            rank = torch.from_numpy(rank_of(rank_order(self.P))).to(self.device)
            return out[:, rank].contiguous()    # [q][g] = the kernel's [q][rank[g]]

    def screen_scores(self, pairs, known=None, sample: int = None, stream=None, mask=None):
        """Every query pair's whole score row (include/mmsbm.h mmsbm_screen_scores): -> f64[Q][P] on
        the host, [i][g] = the score of the triple of pairs[i] and the gene with id g: the pair's
        predicted interaction profile across the array.  NaN where g is not eligible (the pair's own
        genes, the thirds of `known`, what `mask` blocks); elsewhere exactly the bits screen_top
        ranks.  known, sample, mask: as for screen_top."""
        out = self.screen_scores_async(pairs, known, sample, stream, mask)
        if stream is not None:
            stream.synchronize()
        return out.cpu().numpy()

    # ------------------------------------------------------ screen statistics
    @property
    def screen_stat_max_depth(self) -> int:
        """mmsbm_screen_stat_max_depth(): the deepest per-element sorted lists the screen scan's
        statistics kernel holds (quorum_max_depth, and spread_max_trim + 1)."""
        return int(self.lib.mmsbm_screen_stat_max_depth())

    def _screen_votes(self, min_votes) -> int:
        """-> min_votes as an int (None: every active slot, as quorum_top defaults); ValueError
        outside [1, active]."""
        ns = self.active
        m = ns if min_votes is None else int(min_votes)
        if not 1 <= m <= ns:
            raise ValueError("min_votes %d outside [1, %d], the scored slots" % (m, ns))
        return m

    def _screen_stat_top_async(self, pairs, n, stat, arg, known, stream, mask):
        """mmsbm_screen_stat_topn -> device tensors as screen_top_async returns them."""
        n = int(n)
        with self._screen_call(pairs, known, None, stream, mask, n) as (Q, head, ws, s):
            scores = torch.empty((Q, n), dtype=torch.float64, device=self.device)
            ids = torch.empty((Q, n, 3), dtype=torch.int32, device=self.device)
            counts = torch.empty(Q, dtype=torch.int64, device=self.device)
            # head ends with the sample, which the stat entries do not take
            _lib.check(self.lib.mmsbm_screen_stat_topn(*head[:-1], stat, arg, n, *ws, _ptr(scores), _ptr(ids),
                                                       _ptr(counts), s.cuda_stream))
        return scores, ids, counts

    def _screen_stat_scores_async(self, pairs, stat, arg, known, stream, mask):
        """mmsbm_screen_stat_scores -> a device tensor as screen_scores_async returns it."""
        with self._screen_call(pairs, known, None, stream, mask, 0) as (Q, head, ws, s):
            out = torch.empty((Q, self.P), dtype=torch.float64, device=self.device)
            _lib.check(self.lib.mmsbm_screen_stat_scores(*head[:-1], stat, arg, *ws, _ptr(out), s.cuda_stream))
            rank = torch.from_numpy(rank_of(rank_order(self.P))).to(self.device)
            return out[:, rank].contiguous()    # [q][g] = the kernel's [q][rank[g]]

    def _screen_lists(self, tensors, stream):
        """screen_top's host lists from the device tensors of a *_top_async."""
        scores, ids, counts = tensors
        if stream is not None:
            stream.synchronize()
        counts, scores, ids = counts.cpu().numpy(), scores.cpu().numpy(), ids.cpu().numpy()
        return [(scores[i, :int(m)].copy(), ids[i, :int(m)].copy()) for i, m in enumerate(counts)]

    def screen_quorum_top_async(self, pairs, n: int, min_votes: int = None, known=None, stream=None, mask=None):
        """screen_quorum_top without the host copy: -> device tensors as screen_top_async returns
        them.  Nothing synchronises."""
        m = self._screen_votes(min_votes)       # ValueError before anything is uploaded
        return self._screen_stat_top_async(pairs, n, _lib.MMSBM_SCREEN_STAT_QUORUM, m, known, stream, mask)

    def screen_quorum_top(self, pairs, n: int, min_votes: int = None, known=None, stream=None, mask=None):
        """For each query pair of gene ids, its n third genes with the highest quorum score
        (include/mmsbm.h mmsbm_screen_stat_topn, MMSBM_SCREEN_STAT_QUORUM): q_m = the m-th largest of
        the active slots' own screen_scores(sample=s) words, m = min_votes (None: every active slot,
        the minimum over them; 1: the maximum).  At least m restarts score a third gene at or above T
        exactly when its q_m >= T.  -> lists as screen_top returns them, best first under its total
        order.  min_votes outside [1, active] raises ValueError; a depth min(m, active - m + 1) above
        screen_stat_max_depth raises MMSBMError (MMSBM_ERR_UNSUPPORTED).  known, mask: as for
        screen_top."""
        return self._screen_lists(self.screen_quorum_top_async(pairs, n, min_votes, known, stream, mask), stream)

    def screen_quorum_scores_async(self, pairs, min_votes: int = None, known=None, stream=None, mask=None):
        """screen_quorum_scores without the host copy: -> a device tensor f64[Q][P] indexed by the
        third gene's id.  Nothing synchronises."""
        m = self._screen_votes(min_votes)
        return self._screen_stat_scores_async(pairs, _lib.MMSBM_SCREEN_STAT_QUORUM, m, known, stream, mask)

    def screen_quorum_scores(self, pairs, min_votes: int = None, known=None, stream=None, mask=None):
        """Every query pair's whole row of quorum scores (mmsbm_screen_stat_scores): -> f64[Q][P] on
        the host indexed by gene id as screen_scores returns it, NaN where the gene is not eligible;
        elsewhere exactly the bits screen_quorum_top ranks, each one the word of one slot's
        screen_scores row.  min_votes, known, mask: as for screen_quorum_top."""
        out = self.screen_quorum_scores_async(pairs, min_votes, known, stream, mask)
        if stream is not None:
            stream.synchronize()
        return out.cpu().numpy()

    def screen_spread_top_async(self, pairs, n: int, trim: int = 0, known=None, stream=None, mask=None):
        """screen_spread_top without the host copy: -> device tensors as screen_top_async returns
        them.  Nothing synchronises."""
        trim = self._spread_trim(trim)          # ValueError before anything is uploaded
        return self._screen_stat_top_async(pairs, n, _lib.MMSBM_SCREEN_STAT_SPREAD, trim, known, stream, mask)

    def screen_spread_top(self, pairs, n: int, trim: int = 0, known=None, stream=None, mask=None):
        """For each query pair of gene ids, the n third genes on which the active slots disagree most
        (mmsbm_screen_stat_topn, MMSBM_SCREEN_STAT_SPREAD): ranked by d_t = q_{1+t} - q_{ns-t},
        t = trim, over the ns = active slots' own screen_scores words (trim = 0: max - min).
        -> lists as screen_top returns them.  Fewer than two active slots and a trim outside
        spread_trims' rule raise ValueError; a legal trim above screen_stat_max_depth - 1 raises
        MMSBMError (MMSBM_ERR_UNSUPPORTED).  known, mask: as for screen_top."""
        return self._screen_lists(self.screen_spread_top_async(pairs, n, trim, known, stream, mask), stream)

    def screen_spread_scores_async(self, pairs, trim: int = 0, known=None, stream=None, mask=None):
        """screen_spread_scores without the host copy: -> a device tensor f64[Q][P] indexed by the
        third gene's id.  Nothing synchronises."""
        trim = self._spread_trim(trim)
        return self._screen_stat_scores_async(pairs, _lib.MMSBM_SCREEN_STAT_SPREAD, trim, known, stream, mask)

    def screen_spread_scores(self, pairs, trim: int = 0, known=None, stream=None, mask=None):
        """Every query pair's whole row of spreads (mmsbm_screen_stat_scores): -> f64[Q][P] on the
        host indexed by gene id, NaN where the gene is not eligible; elsewhere >= +0 and exactly the
        bits screen_spread_top ranks.  trim, known, mask: as for screen_spread_top."""
        out = self.screen_spread_scores_async(pairs, trim, known, stream, mask)
        if stream is not None:
            stream.synchronize()
        return out.cpu().numpy()

    def census_async(self, thresholds, known: np.ndarray = None, sample: int = None, stream=None, mask=None):
        """census without the host copy: -> device tensors (counts int64[len(thresholds)] in the
        caller's order, total int64[1]).  Nothing synchronises."""
        plan = self._census_plan(thresholds)
        with self._scan_call(known, sample, stream, mask) as call:
            return self._census(plan, call, mask is not None)

    def _census_plan(self, thresholds):
        return census_chunks(thresholds, int(self.lib.mmsbm_census_max_m()))   # ValueError on a NaN or infinite one

    def _census(self, plan, call, masked=False):
        """census_async inside a _scan_call: every chunk's output is its counts and then the total
        of the eligible triples (an empty chunk: the call that returns the total).  masked: the
        _scan_call took a mask, so the entry is the masked one."""
        entry = self.lib.mmsbm_scan_census_masked if masked else self.lib.mmsbm_scan_census
        counts, last = self._per_threshold("census", entry, plan, call, lambda m: (m + 1,), torch.int64, 0)
        return counts, last[-1:]

    def census(self, thresholds, known: np.ndarray = None, sample: int = None, stream=None, mask=None):
        """The score census (include/mmsbm.h mmsbm_scan_census): -> (counts int64[len(thresholds)],
        total int) on the host; counts[i] = the eligible triples (those scan_top ranks: distinct
        genes, key not in `known`) whose score is >= thresholds[i], total = the eligible triples.
        The thresholds may come in any order, with duplicates, in any number or none; a NaN or an
        infinite one raises ValueError.  known, sample: as for scan_top.  The scores are scan_top's
        bit for bit, so census(scan_top(n)[0]) numbers that list's entries.
        mask: a pair mask (scan.pair_mask; include/mmsbm.h mmsbm_scan_census_masked): a triple that
        contains a blocked pair of genes is not eligible either; None: the unmasked call."""
        counts, total = self.census_async(thresholds, known, sample, stream, mask)
        if stream is not None:
            stream.synchronize()
        return counts.cpu().numpy(), int(total.cpu()[0])

    # -------------------------------------------------------- threshold scan
    def _scan_above(self, threshold, known, sample, stream, limit, mask=None):
        """-> (scores f64[n] and packed keys int64[n] on the device, sorted by the scan's total
        order; the kernel's count int64[1] on the device; the census's count n; the launch stream)."""
        threshold = float(threshold)
        if not np.isfinite(threshold):
            raise ValueError("the threshold must be a finite number")
        plan = self._census_plan([threshold])
        with self._scan_call(known, sample, stream, mask) as call:    # one upload of the keys for both kernels
            head, s = call
            masked = mask is not None
            # the same score bits: exactly the rows the kernel will find
            n = int(self._census(plan, call, masked)[0].cpu()[0])
            if n > int(limit):
                raise LimitError(n, int(limit))
            ws = self.scan_workspace("scan_above")
            scores = torch.empty(n, dtype=torch.float64, device=self.device)
            keys = torch.empty(n, dtype=torch.int64, device=self.device)
            found = torch.empty(1, dtype=torch.int64, device=self.device)
            entry = self.lib.mmsbm_scan_above_masked if masked else self.lib.mmsbm_scan_above
            _lib.check(entry(*head, threshold, n, _ptr(ws), ws.numel(), _ptr(scores) if n else None,
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
        order = self.scan_order
        return torch.stack([order[keys // (P * P)], order[(keys // P) % P], order[keys % P]], dim=1)

    def scan_above_async(self, threshold, known: np.ndarray = None, sample: int = None, stream=None,
                         limit: int = 1 << 26, mask=None):
        """scan_above without the host copy: -> device tensors (scores f64[n], ids int32[n][3]) on
        the launch stream.  The number of rows comes from the census first (one host read of one
        integer); a count above `limit` raises before anything is launched for the list."""
        scores, keys, _, _, s = self._scan_above(threshold, known, sample, stream, limit, mask)
        with torch.cuda.stream(s):
            return scores, self._keys_to_ids(keys)

    def scan_above(self, threshold, known: np.ndarray = None, sample: int = None, stream=None,
                   limit: int = 1 << 26, mask=None):
        """Every eligible triple (those scan_top ranks: distinct genes, key not in `known`) whose
        score is >= threshold (include/mmsbm.h mmsbm_scan_above): -> (scores f64[n], ids int32[n][3]
        in key order) on the host, sorted by the scan's total order (score descending, equal scores
        by packed key ascending), n = census([threshold]).  The scores are scan_top's bit for bit, so
        the first rows are scan_top's list.  A NaN or infinite threshold raises ValueError, as does a
        count above `limit` (scan.LimitError, with the count and the limit): 16 bytes per row on the
        device, twice that while sorting.  known, sample: as for scan_top.  mask: as for census
        (mmsbm_scan_above_masked); n = census([threshold], mask=mask) then."""
        scores, keys, found, n, s = self._scan_above(threshold, known, sample, stream, limit, mask)
        with torch.cuda.stream(s):
            ids = self._keys_to_ids(keys).cpu().numpy()
            scores, found = scores.cpu().numpy(), int(found.cpu()[0])
        assert found == n, "the threshold scan found %d rows where the census counted %d" % (found, n)
        return scores, ids

    def scan_top_any(self, n: int, known: np.ndarray = None, sample: int = None, limit: int = 1 << 26, mask=None):
        """scan_top for any n >= 1: -> (scores f64[n'], ids int32[n'][3]) on the host, best first,
        n' <= n.  Up to mmsbm_scan_max_n() it is scan_top; above, censuses bracket a threshold
        between the eligible total and the last score of scan_top(max) (scan.bracket_threshold),
        scan_above fetches what lies at or above it and the list is cut to n.  Exact: the three
        kernels see the same score bits under the same total order.  `limit`: as for scan_above
        (reached only when more than that many triples tie around rank n).
        mask: a pair mask (scan.pair_mask), handed to each of the three calls: the same route over
        the masked-eligible triples."""
        n = int(n)
        if n < 1:
            raise ValueError("scan_top_any needs n >= 1")
        max_n = int(self.lib.mmsbm_scan_max_n())
        if n <= max_n:
            return self.scan_top(n, known, sample, mask=mask)
        scores, ids = self.scan_top(max_n, known, sample, mask=mask)
        if scores.size < max_n:         # fewer eligible triples than that: this is all of them
            return scores, ids
        lo = bracket_threshold(n, float(scores[-1]), lambda t: self.census(t, known, sample, mask=mask)[0])
        scores, ids = self.scan_above(lo, known, sample, limit=limit, mask=mask)
        return scores[:n], ids[:n]

    # ------------------------------------------------------------- vote scan
    def _votes_call(self, call, threshold, min_votes, capacity, masked=False):
        """One mmsbm_scan_votes inside a _scan_call: -> device tensors (hist int64[ns + 1],
        votes int32[capacity], scores f64[capacity], keys int64[capacity], count int64[1]); the rows
        in arrival order.  capacity = 0: the histogram-only call, the row arrays NULL.  masked: the
        _scan_call took a mask, so the entry is the masked one."""
        head, s = call
        entry = self.lib.mmsbm_scan_votes_masked if masked else self.lib.mmsbm_scan_votes
        ns = self.active if head[-1] < 0 else 1
        ws = self.scan_workspace("scan_votes")
        hist = torch.empty(ns + 1, dtype=torch.int64, device=self.device)
        votes = torch.empty(capacity, dtype=torch.int32, device=self.device)
        scores = torch.empty(capacity, dtype=torch.float64, device=self.device)
        keys = torch.empty(capacity, dtype=torch.int64, device=self.device)
        count = torch.empty(1, dtype=torch.int64, device=self.device)
        _lib.check(entry(*head, threshold, int(min_votes), int(capacity), _ptr(ws), ws.numel(), _ptr(hist),
                         *(_ptr(t) if capacity else None for t in (scores, keys, votes)), _ptr(count), s.cuda_stream))
        return hist, votes, scores, keys, count

    def _vote_args(self, threshold, min_votes, sample):
        """-> (threshold as a float, min_votes as an int; None: every scored slot); ValueError on a
        NaN or infinite threshold and on min_votes outside [1, the scored slots]."""
        threshold = float(threshold)
        if not np.isfinite(threshold):
            raise ValueError("the threshold must be a finite number")
        ns = self.active if sample is None else 1
        min_votes = ns if min_votes is None else int(min_votes)
        if not 1 <= min_votes <= ns:
            raise ValueError("min_votes %d outside [1, %d], the scored slots" % (min_votes, ns))
        return threshold, min_votes

    def vote_census_async(self, threshold, known: np.ndarray = None, sample: int = None, stream=None, mask=None):
        """vote_census without the host copy: -> the device tensor hist int64[ns + 1].  Nothing
        synchronises."""
        threshold, _ = self._vote_args(threshold, None, sample)
        with self._scan_call(known, sample, stream, mask) as call:
            return self._votes_call(call, threshold, 1, 0, mask is not None)[0]

    def vote_census(self, threshold, known: np.ndarray = None, sample: int = None, stream=None, mask=None):
        """The vote histogram (include/mmsbm.h mmsbm_scan_votes): -> hist int64[ns + 1] on the host,
        hist[v] = the eligible triples (those scan_top ranks: distinct genes, key not in `known`)
        that exactly v of the scored slots score >= threshold.  The scored slots are the ns = active
        slots for sample = None and that one slot (ns = 1) otherwise; a slot's score carries the bits
        census(sample=slot) sees, so hist.sum() is the census's total and sum(v * hist[v]) the sum
        of the slots' census counts at the threshold.  A NaN or infinite threshold raises
        ValueError.  known, sample: as for scan_top.  mask: as for census (mmsbm_scan_votes_masked);
        hist.sum() then is census([], mask=mask)'s total."""
        hist = self.vote_census_async(threshold, known, sample, stream, mask)
        if stream is not None:
            stream.synchronize()
        return hist.cpu().numpy()

    def _consensus(self, threshold, min_votes, known, sample, stream, limit, mask=None):
        """-> (hist, votes int32[n], scores f64[n] and packed keys int64[n] on the device, sorted by
        votes descending, then score descending, then key ascending; the list call's count int64[1]
        on the device; the histogram's count n; the launch stream)."""
        threshold, min_votes = self._vote_args(threshold, min_votes, sample)
        masked = mask is not None
        with self._scan_call(known, sample, stream, mask) as call:    # one upload of the keys for both calls
            hist = self._votes_call(call, threshold, min_votes, 0, masked)[0]
            n = int(hist[min_votes:].sum().cpu())   # the same votes: exactly the rows the list call will find
            if n > int(limit):
                raise LimitError(n, int(limit))
            _, votes, scores, keys, found = self._votes_call(call, threshold, min_votes, n, masked)
            # the rows arrive in any order; three stable sorts, the last key first
            keys, at = torch.sort(keys, stable=True)
            votes, scores = votes[at], scores[at]
            scores, at = torch.sort(scores, descending=True, stable=True)
            votes, keys = votes[at], keys[at]
            votes, at = torch.sort(votes, descending=True, stable=True)
            scores, keys = scores[at], keys[at]
        return hist, votes, scores, keys, found, n, call[1]

    def consensus_async(self, threshold, min_votes: int = None, known: np.ndarray = None, sample: int = None,
                        stream=None, limit: int = 1 << 26, mask=None):
        """consensus without the host copy: -> device tensors (votes int32[n], scores f64[n],
        ids int32[n][3]) on the launch stream.  The number of rows comes from a histogram-only call
        first (one host read of one integer); a count above `limit` raises before the list call."""
        _, votes, scores, keys, _, _, s = self._consensus(threshold, min_votes, known, sample, stream, limit, mask)
        with torch.cuda.stream(s):
            return votes, scores, self._keys_to_ids(keys)

    def consensus(self, threshold, min_votes: int = None, known: np.ndarray = None, sample: int = None,
                  stream=None, limit: int = 1 << 26, mask=None):
        """Every eligible triple that at least min_votes of the scored slots score >= threshold
        (include/mmsbm.h mmsbm_scan_votes; min_votes = None: all of them): -> (votes int32[n],
        scores f64[n], ids int32[n][3] in key order) on the host, sorted by votes descending, then
        score descending, then packed key ascending; n = vote_census(threshold)[min_votes:].sum().
        A row's score is the ensemble score, scan_top's and scan_above's bits for the same `sample`.
        A NaN or infinite threshold and min_votes outside [1, the scored slots] raise ValueError, as
        does a count above `limit` (scan.LimitError, with the count and the limit): 20 bytes per row
        on the device, twice that while sorting.  known, sample: as for scan_top.  mask: as for census
        (mmsbm_scan_votes_masked)."""
        _, votes, scores, keys, found, n, s = self._consensus(threshold, min_votes, known, sample, stream, limit,
                                                              mask)
        with torch.cuda.stream(s):
            ids = self._keys_to_ids(keys).cpu().numpy()
            votes, scores, found = votes.cpu().numpy(), scores.cpu().numpy(), int(found.cpu()[0])
        assert found == n, "mmsbm_scan_votes found %d rows where its histogram counted %d" % (found, n)
        return votes, scores, ids

    # ----------------------------------------------------------- quorum scan
    @property
    def quorum_max_depth(self) -> int:
        """mmsbm_scan_quorum_max_depth(): the deepest per-element sorted list the kernel holds."""
        return int(self.lib.mmsbm_scan_quorum_max_depth())

    def quorum_depth(self, min_votes: int = None, sample: int = None) -> int:
        """The sorted-list depth quorum_top(., min_votes, sample=sample) needs: min(m, ns - m + 1)
        for m = min_votes (None: every scored slot) of the ns scored slots; quorum_top takes it up to
        quorum_max_depth.  ValueError for min_votes outside [1, ns]."""
        ns = self.active if sample is None else 1
        m = ns if min_votes is None else int(min_votes)
        if not 1 <= m <= ns:
            raise ValueError("min_votes %d outside [1, %d], the scored slots" % (m, ns))
        return min(m, ns - m + 1)

    def quorum_top_async(self, n: int, min_votes: int = None, known: np.ndarray = None, sample: int = None,
                         stream=None, mask=None):
        """quorum_top without the host copy: -> device tensors (scores f64[n], ids int32[n][3],
        count int64[1]); rows from `count` on are NaN / -1.  Nothing synchronises."""
        n = int(n)
        self.quorum_depth(min_votes, sample)    # ValueError before anything is uploaded
        m = (self.active if sample is None else 1) if min_votes is None else int(min_votes)
        entry = self.lib.mmsbm_scan_quorum_topn if mask is None else self.lib.mmsbm_scan_quorum_topn_masked
        with self._scan_call(known, sample, stream, mask) as (head, s):
            ws = self.scan_workspace("scan_quorum", n)
            scores = torch.empty(n, dtype=torch.float64, device=self.device)
            ids = torch.empty((n, 3), dtype=torch.int32, device=self.device)
            count = torch.empty(1, dtype=torch.int64, device=self.device)
            _lib.check(entry(*head, m, n, _ptr(ws), ws.numel(), _ptr(scores), _ptr(ids), _ptr(count), s.cuda_stream))
        return scores, ids, count

    def quorum_top(self, n: int, min_votes: int = None, known: np.ndarray = None, sample: int = None, stream=None,
                   mask=None):
        """The n eligible triples with the highest quorum score (include/mmsbm.h
        mmsbm_scan_quorum_topn): q_m = the m-th largest of the scored slots' own scores, m = min_votes
        (None: every scored slot, the minimum over them; 1: the maximum).  -> (scores f64[n'],
        ids int32[n'][3] in key order) on the host, best first under scan_top's total order, n' <= n.
        A triple has at least m votes at threshold t (vote_census, consensus) exactly when its
        q_m >= t.  The scored slots are the active slots for sample = None and that one slot
        otherwise, where the list is scan_top's for that sample, bit for bit.  min_votes outside
        [1, the scored slots] raises ValueError; a quorum_depth above quorum_max_depth raises
        MMSBMError (MMSBM_ERR_UNSUPPORTED).  known, sample: as for scan_top.  mask: as for census
        (mmsbm_scan_quorum_topn_masked): the exact top n over the triples without a blocked pair."""
        scores, ids, count = self.quorum_top_async(n, min_votes, known, sample, stream, mask)
        if stream is not None:
            stream.synchronize()
        m = int(count.cpu()[0])
        return scores[:m].cpu().numpy(), ids[:m].cpu().numpy()

    # ---------------------------------------------------------- dispute scan
    @property
    def spread_max_trim(self) -> int:
        """mmsbm_scan_spread_max_trim(): the largest trim the kernel holds sorted lists for."""
        return int(self.lib.mmsbm_scan_spread_max_trim())

    def spread_trims(self) -> list:
        """The trims spread_top takes for the current active prefix: t >= 0 with active - 2 t >= 2,
        up to spread_max_trim.  Empty with fewer than two active slots."""
        return [t for t in range(self.spread_max_trim + 1) if self.active - 2 * t >= 2]

    def _spread_trim(self, trim) -> int:
        """-> trim as an int; ValueError for fewer than two active slots and for an illegal trim."""
        ns, trim = self.active, int(trim)
        if ns < 2:
            raise ValueError("%d active slot: one restart has no spread" % ns)
        if trim < 0 or ns - 2 * trim < 2:
            raise ValueError("trim %d outside [0, %d]: %d active slots must keep two scores"
                             % (trim, (ns - 2) // 2, ns))
        return trim

    def spread_top_async(self, n: int, trim: int = 0, known: np.ndarray = None, stream=None, mask=None):
        """spread_top without the host copy: -> device tensors (scores f64[n], ids int32[n][3],
        count int64[1]); rows from `count` on are NaN / -1.  Nothing synchronises."""
        n = int(n)
        trim = self._spread_trim(trim)      # ValueError before anything is uploaded
        entry = self.lib.mmsbm_scan_spread_topn if mask is None else self.lib.mmsbm_scan_spread_topn_masked
        with self._scan_call(known, None, stream, mask) as (head, s):
            ws = self.scan_workspace("scan_spread", n)
            scores = torch.empty(n, dtype=torch.float64, device=self.device)
            ids = torch.empty((n, 3), dtype=torch.int32, device=self.device)
            count = torch.empty(1, dtype=torch.int64, device=self.device)
            _lib.check(entry(*head, trim, n, _ptr(ws), ws.numel(), _ptr(scores), _ptr(ids), _ptr(count),
                             s.cuda_stream))
        return scores, ids, count

    def spread_top(self, n: int, trim: int = 0, known: np.ndarray = None, stream=None, mask=None):
        """The n eligible triples on which the active slots disagree most (include/mmsbm.h
        mmsbm_scan_spread_topn): ranked by d_t = q_{1+t} - q_{ns-t}, t = trim, q_m quorum_top's m-th
        largest of the ns = active slots' own scores.  trim = 0: the range max - min; 1: without the
        single highest and the single lowest restart; (ns - 2) // 2 on an even ns: the gap between
        the two middle scores.  -> (scores f64[n'], ids int32[n'][3] in key order) on the host, best
        first under scan_top's total order, n' <= n.  Fewer than two active slots and a trim outside
        spread_trims' rule (t >= 0, ns - 2 t >= 2) raise ValueError; a legal trim above
        spread_max_trim raises MMSBMError (MMSBM_ERR_UNSUPPORTED).  known: as for scan_top.  mask: as
        for census (mmsbm_scan_spread_topn_masked): the exact top n over the triples without a
        blocked pair."""
        scores, ids, count = self.spread_top_async(n, trim, known, stream, mask)
        if stream is not None:
            stream.synchronize()
        m = int(count.cpu()[0])
        return scores[:m].cpu().numpy(), ids[:m].cpu().numpy()

    # ----------------------------------------------------------- pair census
    def _pair_census_rank(self, thresholds, known, sample, stream, mask=None):
        """The pair census in rank positions: -> (device int32 [P][P][len(thresholds)], filled for
        x < y only, thresholds in the caller's order; the launch stream).  One call of
        mmsbm_pair_census (with a mask: mmsbm_pair_census_masked) per mmsbm_pair_census_max_m()
        thresholds."""
        plan = census_chunks(thresholds, int(self.lib.mmsbm_pair_census_max_m()))   # ValueError on a NaN or infinite one
        entry = self.lib.mmsbm_pair_census if mask is None else self.lib.mmsbm_pair_census_masked
        with self._scan_call(known, sample, stream, mask) as call:
            mat, _ = self._per_threshold("pair_census", entry, plan, call,
                                         lambda m: (self.P, self.P, m), torch.int32, 2)
        return mat, call[1]

    def _pair_matrix_ids(self, mat, s):
        """A pair matrix in rank positions, filled for x < y (device int32 [P][P][.]) on its launch
        stream s -> the symmetric matrix in gene ids."""
        with torch.cuda.stream(s):
            rank = torch.from_numpy(rank_of(rank_order(self.P))).to(self.device)
            mat = mat + mat.transpose(0, 1)             # x < y was filled, the rest is zero
            return mat[rank][:, rank].contiguous()      # [g1][g2] = [rank[g1]][rank[g2]]

    def pair_census_async(self, thresholds, known: np.ndarray = None, sample: int = None, stream=None, mask=None):
        """pair_census without the host copy: -> a device tensor int32 [P][P][len(thresholds)] in
        gene ids, symmetric with a zero diagonal, thresholds in the caller's order.  Nothing
        synchronises."""
        mat, s = self._pair_census_rank(thresholds, known, sample, stream, mask)
        return self._pair_matrix_ids(mat, s)

    def pair_census(self, thresholds, known: np.ndarray = None, sample: int = None, stream=None, mask=None):
        """The pair census (include/mmsbm.h mmsbm_pair_census): -> int32 [P][P][len(thresholds)] on
        the host; [g1][g2][i] = the eligible triples (those scan_top ranks: distinct genes, key not
        in `known`) that contain the genes g1 and g2 and score >= thresholds[i]: the predicted,
        unmeasured interactions of the double-mutant query (g1, g2).  Symmetric, zero diagonal.
        The thresholds may come in any order, with duplicates, in any number or none; a NaN or an
        infinite one raises ValueError.  known, sample: as for census; the scores are the census's
        bit for bit, so the sum over g1 < g2 is three times census(thresholds).  mask: as for census
        (mmsbm_pair_census_masked): a blocked pair's entries are zero and the sum is three times
        census(thresholds, mask=mask)."""
        mat = self.pair_census_async(thresholds, known, sample, stream, mask)
        if stream is not None:
            stream.synchronize()
        return mat.cpu().numpy()

    def pairs_top(self, n: int, threshold: float, known: np.ndarray = None, sample: int = None, mask=None):
        """The n pairs with the most eligible triples scoring >= threshold: -> (counts int64[n'],
        eligible int64[n'] = the pair's eligible triples in all (scan.pair_eligible), ids
        int32[n'][2] in key order) on the host, n' = min(n, C(P, 2)).  Ordered by count descending,
        equal counts by the pair's rank-position key x P + y ascending.  The selection is one
        torch.topk on the device over count * P^2 + (P^2 - 1 - key).  mask: as for census; counts and
        eligible then are the masked ones (a blocked pair: 0 and 0)."""
        mat, s = self._pair_census_rank([float(threshold)], known, sample, None, mask)
        return self._pairs_select(n, mat, s, known, mask)

    def _pairs_select(self, n, mat, s, known, mask):
        """pairs_top's and pairs_consensus_top's selection: the n best pairs of column 0 of a pair
        matrix in rank positions (device int32 [P][P][.], filled for x < y) on its launch stream s ->
        (counts, eligible, ids) as pairs_top documents them."""
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
        eligible = pair_eligible(P, known, mask)[ids[:, 0], ids[:, 1]].astype(np.int64)
        return counts.astype(np.int64), eligible, ids

    def gene_census(self, thresholds, known: np.ndarray = None, sample: int = None, mask=None):
        """-> int64 [P][len(thresholds)] on the host: the eligible triples that contain each gene
        and score >= each threshold.  The row sums of the pair matrix halved: every triple of a gene
        sits in two of the gene's pairs.  mask: as for pair_census."""
        mat = self.pair_census_async(thresholds, known, sample, mask=mask)
        return (mat.sum(dim=1, dtype=torch.int64) // 2).cpu().numpy()

    # ------------------------------------------------------ pair vote census
    def _pair_votes_rank(self, threshold, levels, known, sample, stream, mask=None):
        """The pair vote census in rank positions: -> (device int32 [P][P][len(levels)], filled for
        x < y only, levels in the caller's order; the launch stream).  One call of mmsbm_pair_votes
        (with a mask: mmsbm_pair_votes_masked) per mmsbm_pair_votes_max_m() levels."""
        threshold, _ = self._vote_args(threshold, None, sample)     # ValueError on a NaN or infinite one
        ns = self.active if sample is None else 1
        chunks, perm = vote_level_chunks(levels, ns, int(self.lib.mmsbm_pair_votes_max_m()))
        entry = self.lib.mmsbm_pair_votes if mask is None else self.lib.mmsbm_pair_votes_masked
        with self._scan_call(known, sample, stream, mask) as (head, s):
            ws = self.scan_workspace("pair_votes")
            outs = []
            for chunk in chunks:    # the levels are read on the host before the call returns
                out = torch.empty((self.P, self.P, chunk.size), dtype=torch.int32, device=self.device)
                _lib.check(entry(*head, threshold, _host_ptr(chunk), int(chunk.size), _ptr(ws), ws.numel(),
                                 _ptr(out) if out.numel() else None, s.cuda_stream))
                outs.append(out)
            if len(outs) == 1 and (perm == np.arange(perm.size)).all():
                return outs[0], s   # one call, levels already ascending: nothing to put back
            joined = torch.cat(outs, dim=2)     # sorted position i answers the caller's levels[perm[i]]
            perm_d = torch.from_numpy(perm).to(self.device)
            return torch.empty_like(joined).index_copy_(2, perm_d, joined), s

    def pair_vote_census_async(self, threshold, levels=None, known: np.ndarray = None, sample: int = None,
                               stream=None, mask=None):
        """pair_vote_census without the host copy: -> a device tensor int32 [P][P][len(levels)] in
        gene ids, symmetric with a zero diagonal, levels in the caller's order.  Nothing
        synchronises."""
        mat, s = self._pair_votes_rank(threshold, levels, known, sample, stream, mask)
        return self._pair_matrix_ids(mat, s)

    def pair_vote_census(self, threshold, levels=None, known: np.ndarray = None, sample: int = None, stream=None,
                         mask=None):
        """The pair vote census (include/mmsbm.h mmsbm_pair_votes): -> int32 [P][P][len(levels)] on
        the host; [g1][g2][i] = the eligible triples (those scan_top ranks: distinct genes, key not
        in `known`) that contain the genes g1 and g2 and that at least levels[i] of the scored slots
        score >= threshold: the interactions of the double-mutant query (g1, g2) that the restarts
        agree on, where pair_census counts on their mean.  Symmetric, zero diagonal.  The scored
        slots are vote_census's: the ns = active slots for sample = None, that one slot otherwise.
        levels = None: 1..ns.  The levels may come in any order, with duplicates, in any number or
        none; one outside [1, ns] and a NaN or infinite threshold raise ValueError.  The sum over
        g1 < g2 of column i is three times vote_census(threshold)[levels[i]:].sum(), and column i is
        the scatter to their pairs of consensus(threshold, levels[i])'s triples.  known, sample,
        mask: as for vote_census (mmsbm_pair_votes_masked): a blocked pair's entries are zero."""
        mat = self.pair_vote_census_async(threshold, levels, known, sample, stream, mask)
        if stream is not None:
            stream.synchronize()
        return mat.cpu().numpy()

    def pairs_consensus_top(self, n: int, threshold: float, min_votes: int = None, known: np.ndarray = None,
                            sample: int = None, mask=None):
        """The n pairs with the most eligible triples that at least min_votes of the scored slots
        (None: all of them) score >= threshold: -> (counts int64[n'], eligible int64[n'], ids
        int32[n'][2]) exactly as pairs_top returns and orders them, the counts being
        pair_vote_census's at levels = [min_votes].  With sample = s it is pairs_top(n, threshold,
        sample=s).  min_votes outside [1, the scored slots] and a NaN or infinite threshold raise
        ValueError."""
        threshold, min_votes = self._vote_args(threshold, min_votes, sample)
        mat, s = self._pair_votes_rank(threshold, [min_votes], known, sample, None, mask)
        return self._pairs_select(n, mat, s, known, mask)

    def gene_vote_census(self, threshold, levels=None, known: np.ndarray = None, sample: int = None, mask=None):
        """-> int64 [P][len(levels)] on the host: the eligible triples that contain each gene and
        have at least each level of votes at the threshold.  The row sums of pair_vote_census's
        matrix halved, as gene_census forms its counts.  mask: as for pair_vote_census."""
        mat = self.pair_vote_census_async(threshold, levels, known, sample, mask=mask)
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
