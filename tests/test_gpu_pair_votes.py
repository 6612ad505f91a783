"""Pair vote census (include/mmsbm.h mmsbm_pair_votes / mmsbm_pair_votes_masked,
EMEngine.pair_vote_census / pairs_consensus_top / gene_vote_census, the scan driver's
--pair-consensus and --gene-consensus) against the numpy float64 reference of
tests/pair_votes_ref.py, which scatters every eligible triple with enough votes to its three pairs.

The counts are integers, so the tests demand equality.  Every threshold a test chooses comes from
votes_ref.clear_thresholds over the scores of ALL slots, which asserts on the reference alone that
it is more than 1e-7 relative from every slot's score: the project's RTOL of 1e-9 then cannot move a
vote.  Two thresholds are used, near the median (nearly every tile has hits: the level walk) and at
a high quantile (nearly every tile leaves at the first ballot).  The identities with the vote scan
and the pair census need no such precondition: one score phase serves them all, bit for bit.
"""
import ctypes
import os
from math import comb

import numpy as np
import pytest

import census_ref
import converged_ref as cr
import masked_ref
import pair_census_ref
import pair_votes_ref as ref
import scan_ref
import votes_ref
from golden_util import GOLDEN
from scan_gpu import SENTINEL, Raw, engine

pytestmark = pytest.mark.gpu

BIG = (10, 70, 31, 3)       # K, P, seed, B of the identity, mask and grid tests: 54,740 triples


def check(eng, per, keys, t, levels=None, known=None, sample=None, ns=None, **kw):
    """The precondition on the reference alone, then the whole matrix equal to the reference,
    symmetric and with a zero diagonal.  per: every slot's reference scores; ns: the active prefix."""
    per = np.asarray(per)
    if sample is not None:
        per = per[sample:sample + 1]
    elif ns is not None:
        per = per[:ns]
    census_ref.assert_clear(per.reshape(-1), [t])
    P = eng.P
    lv = list(range(1, per.shape[0] + 1)) if levels is None else levels
    _, want = ref.ref_pairs(per, keys, P, t, lv, known=known)
    got = eng.pair_vote_census(t, levels, known, sample, **kw)
    assert got.dtype == np.int32 and got.shape == (P, P, len(lv))
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got, got.transpose(1, 0, 2))
    assert not got[np.arange(P), np.arange(P)].any()
    return got


# ------------------------------------------------------------------ 1. shapes
@pytest.mark.parametrize("P", [1, 2, 3, 4, 15, 16, 17, 33, 65, 70])
def test_shapes(P):
    """Padded rows and columns, one and several row blocks, and P < 3 (all zeros)."""
    K, B = 3, 3
    c = votes_ref.case(K, P, 11 + P, B)
    assert c.keys.size == comb(P, 3)
    eng = engine(c.theta, c.pr)
    if P < 3:
        for kn in (None, np.array([7], dtype=np.int64)):
            got = eng.pair_vote_census(0.5, None, kn)
            assert got.shape == (P, P, 3) and got.dtype == np.int32 and not got.any()
    else:
        hit = 0
        for t in ref.two_thresholds(c.per, 65, 0.99):
            got = check(eng, c.per, c.keys, t)
            check(eng, c.per, c.keys, t, known=c.keys[::3].copy())
            assert got.max() <= P - 2
            hit += int(got.any())
        assert hit or P < 15
    eng.close()


# ------------------------------------------------------------------ 2. every KS template
@pytest.mark.parametrize("K", [1, 2, 4, 5, 10, 12, 13, 17, 30, 32])
def test_every_ks_template(K):
    """K = 1 .. 32 in steps of 4 and K that is no multiple of 4; the ensemble kernel (sample = None)
    and the single-sample kernel (sample = 1)."""
    P, B = 40, 3
    c = votes_ref.case(K, P, 100 + K, B)
    eng = engine(c.theta, c.pr)
    if K == 1:      # a slot's scores all equal its p_1[0][0][0]: no gaps to sit in, so bracket them
        s = c.pr[:, 0, 0, 0, 1]
        ts = [float(s.min() * (1 - 1e-6)), float(s.max() * (1 + 1e-6))]
    else:
        ts = ref.two_thresholds(c.per, 257, 0.99)
    for t in ts:
        got = check(eng, c.per, c.keys, t)
        one = check(eng, c.per, c.keys, t, sample=1)
        assert one.shape == (P, P, 1)
        if K == 1:
            full = (P - 2) * (1 - np.eye(P, dtype=np.int32))
            for m in range(B):
                np.testing.assert_array_equal(got[:, :, m], full if t == ts[0] else 0 * full)
            np.testing.assert_array_equal(one[:, :, 0], full if t == ts[0] else 0 * full)
    if K > 1:
        assert eng.pair_vote_census(ts[0], [B]).any()       # near the median the slots agree on some triples
    eng.close()


# ------------------------------------------------------------------ 3. levels
def test_levels():
    K, P, B = 10, 40, 8
    c = votes_ref.case(K, P, 7, B)
    eng = engine(c.theta, c.pr)
    assert eng.lib.mmsbm_pair_votes_max_m() == 8
    t, hi = ref.two_thresholds(c.per, 257, 0.99)
    tail = ref.hist_tail(c.per, c.keys, t, range(1, 9))
    assert tail[7] > 0 and tail[0] < comb(P, 3)           # on the reference: every level has hits, and misses
    all8 = check(eng, c.per, c.keys, t)                 # None: 1..8 in one call
    np.testing.assert_array_equal(check(eng, c.per, c.keys, t, list(range(1, 9))), all8)
    check(eng, c.per, c.keys, hi)
    dup = check(eng, c.per, c.keys, t, [2, 2, 5, 5, 5, 8])
    np.testing.assert_array_equal(dup, all8[:, :, [1, 1, 4, 4, 4, 7]])
    down = check(eng, c.per, c.keys, t, [8, 6, 3, 3, 1])           # the caller's order comes back
    np.testing.assert_array_equal(down, all8[:, :, [7, 5, 2, 2, 0]])
    eleven = [8, 1, 7, 2, 6, 3, 5, 4, 4, 8, 1]                      # two calls of the kernel
    np.testing.assert_array_equal(check(eng, c.per, c.keys, t, eleven, c.keys[::5].copy()),
                                  check(eng, c.per, c.keys, t, None, c.keys[::5].copy())[:, :, [v - 1 for v in eleven]])
    none = eng.pair_vote_census(t, [])
    assert none.shape == (P, P, 0) and none.dtype == np.int32
    assert eng.gene_vote_census(t, []).shape == (P, 0)
    for bad in ([0], [9], [1, 2, 9], [-1]):
        with pytest.raises(ValueError, match="outside"):
            eng.pair_vote_census(t, bad)
    with pytest.raises(ValueError):
        eng.pair_vote_census(t, [2], sample=0)          # one scored slot
    for bad_t in (float("nan"), float("inf")):
        with pytest.raises(ValueError, match="finite"):
            eng.pair_vote_census(bad_t)
        with pytest.raises(ValueError, match="finite"):
            eng.pairs_consensus_top(3, bad_t)
    with pytest.raises(ValueError):
        eng.pairs_consensus_top(3, t, 9)
    with pytest.raises(ValueError):
        eng.pair_vote_census(t, sample=8)               # outside the active prefix
    eng.close()


# ------------------------------------------------------------------ 4. a partial prefix
def test_partial_prefix():
    K, P, B = 10, 40, 3
    c = votes_ref.case(K, P, 110, B)
    eng = engine(c.theta, c.pr)
    eng.set_active(2)
    t, _ = ref.two_thresholds(c.per, 257, 0.99)
    got = check(eng, c.per, c.keys, t, ns=2)
    assert got.shape == (P, P, 2) and got[:, :, 1].any()
    check(eng, c.per, c.keys, t, [2, 1], c.keys[::3].copy(), ns=2)
    with pytest.raises(ValueError, match=r"outside \[1, 2\]"):
        eng.pair_vote_census(t, [3])
    # and in C: a level of 3 with two scored slots
    import torch
    from trigenicinteractionpredictor_amd import _lib
    raw = PairVotesRaw(eng, "pair_votes")
    out = raw.full((P, P, 1), torch.int32)
    assert raw.votes(t, [3], [out], sample=-1) == _lib.MMSBM_ERR_INVALID and raw.intact()
    assert raw.votes(t, [2], [out], sample=-1) == _lib.MMSBM_OK
    np.testing.assert_array_equal(out.cpu().numpy()[:, :, 0], ref.ref_rank(c.per, c.keys, P, t, [2], ns=2)[:, :, 0])
    eng.close()


# ------------------------------------------------------------------ 5. identities
@pytest.mark.parametrize("with_known", [False, True], ids=["all", "known"])
def test_identities_with_the_vote_scan_and_the_pair_census(with_known):
    """Exact, no precondition on the thresholds: AT scores of the scan list."""
    K, P, seed, B = BIG
    th, pr = scan_ref.random_params(K, P, seed, B)
    eng = engine(th, pr)
    kn = scan_ref.ref_scores(th[0], pr[0])[1][::4].copy() if with_known else None
    scores, _ = eng.scan_top(50, kn)
    upper = np.triu(np.ones((P, P), dtype=bool), k=1)
    order = np.asarray(eng.scan_order.cpu())
    rank = np.empty(P, dtype=np.int64)
    rank[order] = np.arange(P)
    for t in (float(scores[0]), float(scores[49]), float(np.nextafter(scores[25], 1.0))):
        hist = eng.vote_census(t, kn)
        mat = eng.pair_vote_census(t, None, kn)
        genes = eng.gene_vote_census(t, None, kn)
        assert genes.dtype == np.int64 and genes.shape == (P, B)
        np.testing.assert_array_equal(genes, mat.sum(axis=1, dtype=np.int64) // 2)
        for level in range(1, B + 1):
            tail = int(hist[level:].sum())
            assert mat[upper][:, level - 1].sum(dtype=np.int64) == 3 * tail
            assert genes[:, level - 1].sum() == 3 * tail
            # the scatter of consensus(threshold, level)'s ids
            _, _, ids = eng.consensus(t, level, kn)
            assert ids.shape == (tail, 3)
            want = np.zeros((P, P), dtype=np.int32)
            for x, y in ((0, 1), (0, 2), (1, 2)):
                np.add.at(want, (ids[:, x], ids[:, y]), 1)
                np.add.at(want, (ids[:, y], ids[:, x]), 1)
            np.testing.assert_array_equal(mat[:, :, level - 1], want)
        assert hist[1:].sum() > 0
        for s in range(B):
            np.testing.assert_array_equal(eng.pair_vote_census(t, [1], kn, sample=s),
                                          eng.pair_census([t], kn, sample=s))
    eng.close()


# ------------------------------------------------------------------ 6. pairs_consensus_top
def test_pairs_consensus_top():
    from trigenicinteractionpredictor_amd.scan import pair_eligible
    K, P, B = 5, 33, 3
    c = votes_ref.case(K, P, 71, B)
    eng = engine(c.theta, c.pr)
    t, _ = ref.two_thresholds(c.per, 257, 0.99)
    for kn in (None, c.keys[::3].copy()):
        el = pair_eligible(P, kn)
        for votes in (None, 1, 2):
            rank_mat = ref.ref_rank(c.per, c.keys, P, t, [B if votes is None else votes], known=kn)
            for n in (1, 10, comb(P, 2), comb(P, 2) + 5):
                counts, eligible, ids = eng.pairs_consensus_top(n, t, votes, kn)
                want_counts, want_ids = pair_census_ref.top_pairs(rank_mat[:, :, 0], n)
                assert counts.dtype == np.int64 and eligible.dtype == np.int64 and ids.dtype == np.int32
                assert counts.shape == (min(n, comb(P, 2)),) and ids.shape == (min(n, comb(P, 2)), 2)
                np.testing.assert_array_equal(counts, want_counts)
                np.testing.assert_array_equal(ids, want_ids)
                np.testing.assert_array_equal(eligible, el[ids[:, 0], ids[:, 1]])
                assert (counts <= eligible).all()
            assert 0 < counts.max() and np.unique(counts).size < counts.size      # real ties, ordered by key
        for s in (0, 2):        # one scored slot: pairs_top of that slot
            got = eng.pairs_consensus_top(20, t, None, kn, sample=s)
            want = eng.pairs_top(20, t, kn, sample=s)
            assert all(g.dtype == w.dtype and g.tobytes() == w.tobytes() for g, w in zip(got, want))
            assert got[0].max() > 0
    eng.close()


# ------------------------------------------------------------------ 7. the mask
def test_the_mask():
    from trigenicinteractionpredictor_amd.scan import pair_mask
    K, P, seed, B = BIG
    c = votes_ref.case(K, P, seed, B)
    eng = engine(c.theta, c.pr)
    order, rank = scan_ref.rank_tables(P)
    universe = [int(g) for g in range(P) if g % 2 == 0 or g % 7 == 0]      # a good half of the genes
    pairs = [(universe[0], universe[5]), (universe[3], universe[20]), (universe[10], universe[11]),
             (universe[-1], universe[2])]
    mask = pair_mask(P, pairs=pairs, genes=universe)
    np.testing.assert_array_equal(mask, masked_ref.naive_from_ids(P, pairs, universe))
    blocked_keys = masked_ref.expand(mask, P)
    assert 0 < blocked_keys.size < c.keys.size
    zero = masked_ref.naive_mask(P, [])
    full = masked_ref.full_mask(P)
    upper = np.triu(np.ones((P, P), dtype=bool), k=1)
    for t in ref.two_thresholds(c.per, 257, 0.99):
        for kn in (None, c.keys[::4].copy()):
            free = eng.pair_vote_census(t, None, kn)
            # the all-zero mask is the unmasked call
            np.testing.assert_array_equal(eng.pair_vote_census(t, None, kn, mask=zero), free)
            # a mask is the key table it stands for, on the GPU and in the reference
            union = np.union1d(np.zeros(0, np.int64) if kn is None else kn, blocked_keys).astype(np.int64)
            got = eng.pair_vote_census(t, None, kn, mask=mask)
            np.testing.assert_array_equal(got, eng.pair_vote_census(t, None, union))
            np.testing.assert_array_equal(got, ref.ref_pairs(c.per, c.keys, P, t, [1, 2, 3], known=union)[1])
            # blocked pairs' rows are zero: the listed pairs and every pair that leaves the universe
            for g1, g2 in pairs:
                assert not got[g1, g2].any() and not got[g2, g1].any()
            outside = np.setdiff1d(np.arange(P), universe)
            assert not got[outside].any() and not got[:, outside].any() and free[outside].any()
            # pair sums = 3 x the masked histogram's tail
            hist = eng.vote_census(t, kn, mask=mask)
            np.testing.assert_array_equal(got[upper].sum(axis=0, dtype=np.int64),
                                          [3 * int(hist[v:].sum()) for v in (1, 2, 3)])
            np.testing.assert_array_equal(eng.gene_vote_census(t, None, kn, mask=mask),
                                          got.sum(axis=1, dtype=np.int64) // 2)
            # one sample under the mask: the masked pair census
            np.testing.assert_array_equal(eng.pair_vote_census(t, [1], kn, sample=1, mask=mask),
                                          eng.pair_census([t], kn, sample=1, mask=mask))
            # every pair blocked: nothing
            assert not eng.pair_vote_census(t, None, kn, mask=full).any()
            counts, eligible, _ = eng.pairs_consensus_top(5, t, 1, kn, mask=full)
            assert counts.tolist() == [0] * 5 and eligible.tolist() == [0] * 5
        assert got.any()
    eng.close()


# ------------------------------------------------------------------ 8. grid, batch, repeats
def test_grid_batch_and_repeats(monkeypatch):
    K, P, seed, B = BIG
    c = votes_ref.case(K, P, seed, B)
    eng = engine(c.theta, c.pr)
    th0, p0 = eng.theta.cpu().numpy().copy(), eng.pr.cpu().numpy().copy()
    known = c.keys[1::5].copy()
    mask = masked_ref.random_mask(P)
    t, _ = ref.two_thresholds(c.per, 257, 0.99)
    want = check(eng, c.per, c.keys, t, None, known)
    want_one = check(eng, c.per, c.keys, t, None, known, sample=2)
    want_masked = eng.pair_vote_census(t, None, known, mask=mask)
    for grid in ("1", "7"):
        monkeypatch.setenv("MMSBM_PAIR_VOTES_GRID", grid)
        np.testing.assert_array_equal(eng.pair_vote_census(t, None, known), want)
        if grid == "1":
            np.testing.assert_array_equal(eng.pair_vote_census(t, None, known, sample=2), want_one)
            np.testing.assert_array_equal(eng.pair_vote_census(t, None, known, mask=mask), want_masked)
    monkeypatch.delenv("MMSBM_PAIR_VOTES_GRID")
    # a repeated call: the call zeroes its output (the allocator hands the last matrix back)
    np.testing.assert_array_equal(eng.pair_vote_census(t, None, known), want)
    assert eng.theta.cpu().numpy().tobytes() == th0.tobytes()
    assert eng.pr.cpu().numpy().tobytes() == p0.tobytes()
    # a slot of the batch = an engine that holds that sample alone
    solo = engine(c.theta[2:3], c.pr[2:3])
    for sample in (0, None):
        np.testing.assert_array_equal(solo.pair_vote_census(t, None, known, sample=sample), want_one)
    solo.close()
    eng.close()


def test_async_call_returns_a_device_tensor():
    import torch
    K, P, B = 3, 33, 3
    c = votes_ref.case(K, P, 11 + P, B)
    eng = engine(c.theta, c.pr)
    t, _ = ref.two_thresholds(c.per, 65, 0.99)
    stream = torch.cuda.Stream(eng.device)
    for st in (None, stream):
        mat = eng.pair_vote_census_async(t, [3, 1], stream=st)
        (stream if st is not None else torch.cuda.current_stream(eng.device)).synchronize()
        assert mat.is_cuda and mat.dtype == torch.int32
        np.testing.assert_array_equal(mat.cpu().numpy(), eng.pair_vote_census(t, [3, 1], stream=st))
    eng.close()


# ------------------------------------------------------------------ 9. the C entries as C sees them
class PairVotesRaw(Raw):
    """scan_gpu.Raw with the pair vote census's entries.  By position in the unmasked C call:
    0 ctx, 1 order, 2 known, 3 n_known, 4 theta, 5 pr, 6 sample, 7 threshold, 8 levels_host, 9 M,
    10 and 11 the workspace, 12 out_counts, 13 stream."""
    ENTRY = dict(Raw.ENTRY, pair_votes="mmsbm_pair_votes")

    def votes(self, threshold, levels, outs, n_levels=None, **kw):
        self.levels = np.ascontiguousarray(levels, dtype=np.int32)      # on the host, alive over the call
        m = self.levels.size if n_levels is None else n_levels
        return self.call((float(threshold), self.levels.ctypes.data_as(ctypes.c_void_p), m), outs, **kw)

    def masked(self, mask_ptr, threshold, levels, outs, sample=-1):
        eng = self.eng
        self.levels = np.ascontiguousarray(levels, dtype=np.int32)
        self.outs = outs
        rc = eng.lib.mmsbm_pair_votes_masked(
            eng.ctx, eng.scan_order.data_ptr(), None, 0, mask_ptr, eng.theta.data_ptr(), eng.pr.data_ptr(), sample,
            float(threshold), self.levels.ctypes.data_as(ctypes.c_void_p), int(self.levels.size), self.ws.data_ptr(),
            self.ws.numel(), *[None if o is None else o.data_ptr() for o in outs], eng._stream())
        self.torch.cuda.synchronize(eng.device)
        return rc


def test_raw_calls_check_everything_before_any_device_call():
    import torch
    from trigenicinteractionpredictor_amd import _lib
    INVALID, UNSUPPORTED, OK = _lib.MMSBM_ERR_INVALID, _lib.MMSBM_ERR_UNSUPPORTED, _lib.MMSBM_OK
    K, P, B = 3, 33, 3
    c = votes_ref.case(K, P, 11 + P, B)
    eng = engine(c.theta, c.pr)
    nbytes = ctypes.c_int64(-1)
    assert eng.lib.mmsbm_pair_votes_workspace_bytes(eng.ctx, None) == INVALID
    assert eng.lib.mmsbm_pair_votes_workspace_bytes(None, ctypes.byref(nbytes)) == INVALID and nbytes.value == -1
    assert eng.lib.mmsbm_pair_votes_workspace_bytes(eng.ctx, ctypes.byref(nbytes)) == OK and nbytes.value > 0
    raw = PairVotesRaw(eng, "pair_votes")
    assert raw.ws.numel() == nbytes.value
    t, _ = ref.two_thresholds(c.per, 65, 0.99)
    out = raw.full((P, P, 9), torch.int32)
    ws = raw.ws.data_ptr()
    # null pointers, the threshold, the sample, the key table, the workspace, M < 0
    for i, bad in ((0, None), (1, None), (4, None), (5, None), (8, None), (12, None), (7, float("nan")),
                   (7, float("inf")), (7, float("-inf")), (6, 3), (6, -2), (3, -1), (3, 5), (10, None), (10, ws + 8),
                   (11, 16), (11, nbytes.value - 1), (9, -1)):
        assert raw.votes(t, [1, 2, 3], [out], sample=-1, replace=[(i, bad)]) == INVALID, (i, bad)
        assert raw.intact(), (i, bad)
    # the levels: outside [1, ns], decreasing; one slot has one level
    for levels, sample in (([0], -1), ([4], -1), ([1, 2, 4], -1), ([2, 1], -1), ([1, 3, 2], -1), ([-5], -1),
                           ([2], 0), ([1, 2], 1)):
        assert raw.votes(t, levels, [out], sample=sample) == INVALID, levels
        assert raw.intact() and b"levels" in eng.lib.mmsbm_last_error()
    # M above the cap
    assert raw.votes(t, [1] * 9, [out], sample=-1) == UNSUPPORTED and raw.intact()
    assert b"cap" in eng.lib.mmsbm_last_error()
    # M = 0: OK, nothing written, the levels and the output may be NULL
    assert raw.votes(t, [], [out], sample=-1) == OK and raw.intact()
    assert raw.votes(t, [1], [out], n_levels=0, sample=-1) == OK and raw.intact()
    assert raw.call((t, None, 0), [None], sample=-1) == OK
    # the masked entry: a NULL mask, and the unmasked entry's checks behind it
    zero = raw.upload(masked_ref.naive_mask(P, []).view(np.int32))
    assert raw.masked(None, t, [1, 2, 3], [out]) == INVALID and raw.intact()
    assert b"mask" in eng.lib.mmsbm_last_error()
    assert raw.masked(zero.data_ptr() + 2, t, [1, 2, 3], [out]) == INVALID and raw.intact()
    assert raw.masked(zero.data_ptr(), t, [1, 4], [out]) == INVALID and raw.intact()
    assert raw.masked(zero.data_ptr(), float("nan"), [1], [out]) == INVALID and raw.intact()
    assert raw.masked(zero.data_ptr(), t, [1] * 9, [out]) == UNSUPPORTED and raw.intact()
    assert raw.masked(zero.data_ptr(), t, [], [out]) == OK and raw.intact()
    # and what a good call writes: rank positions, x < y only, into a dirty matrix; duplicates are fine
    want = ref.ref_rank(c.per, c.keys, P, t, [1, 2, 2, 3])
    for call in (lambda o: raw.votes(t, [1, 2, 2, 3], [o], sample=-1),
                 lambda o: raw.masked(zero.data_ptr(), t, [1, 2, 2, 3], [o])):
        dirty = raw.full((P, P, 4), torch.int32, 1)
        assert call(dirty) == OK
        np.testing.assert_array_equal(dirty.cpu().numpy(), want)
    eng.close()


def test_unsupported_shapes_are_refused():
    """Scratch contexts without links: no shape (K = 0), P = 16385, and an ensemble whose W tile
    exceeds the LDS (16 slots at K = 32).  Every buffer has its full size all the same."""
    import torch
    from trigenicinteractionpredictor_amd import _lib
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    stream = torch.cuda.current_stream(dev).cuda_stream
    levels = np.array([1], dtype=np.int32)
    lv = levels.ctypes.data_as(ctypes.c_void_p)
    nbytes = ctypes.c_int64(-1)
    ctx = ctypes.c_void_p()
    _lib.check(lib.mmsbm_create(dev.index, ctypes.byref(ctx)))
    try:
        assert lib.mmsbm_pair_votes_workspace_bytes(ctx, ctypes.byref(nbytes)) == _lib.MMSBM_ERR_UNSUPPORTED
        assert nbytes.value == -1 and b"K=" in lib.mmsbm_last_error()
        some = torch.zeros(1 << 16, dtype=torch.int32, device=dev)
        out = torch.full((16,), SENTINEL, dtype=torch.int32, device=dev)
        rc = lib.mmsbm_pair_votes(ctx, some.data_ptr(), None, 0, some.data_ptr(), some.data_ptr(), 0, 0.5, lv, 1,
                                  some.data_ptr(), some.numel() * 4, out.data_ptr(), stream)
        assert rc == _lib.MMSBM_ERR_UNSUPPORTED
        # P above the cap
        K, P = 2, 16385
        _lib.check(lib.mmsbm_set_shape(ctx, K, 2, 1, P, 1e-10))
        assert lib.mmsbm_pair_votes_workspace_bytes(ctx, ctypes.byref(nbytes)) == _lib.MMSBM_ERR_UNSUPPORTED
        assert nbytes.value == -1 and b"16384" in lib.mmsbm_last_error()
        order = torch.arange(P, dtype=torch.int32, device=dev)
        theta = torch.full((1, P, K), 0.5, dtype=torch.float64, device=dev)
        pr = torch.full((1, 2, K ** 3), 0.5, dtype=torch.float64, device=dev)
        _lib.check(lib.mmsbm_scan_votes_workspace_bytes(ctx, ctypes.byref(nbytes)))    # that family's cap is higher
        ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
        mask = torch.zeros((16400, 513), dtype=torch.int32, device=dev)
        rc = lib.mmsbm_pair_votes(ctx, order.data_ptr(), None, 0, theta.data_ptr(), pr.data_ptr(), 0, 0.5, lv, 1,
                                  ws.data_ptr(), ws.numel(), out.data_ptr(), stream)
        assert rc == _lib.MMSBM_ERR_UNSUPPORTED
        rc = lib.mmsbm_pair_votes_masked(ctx, order.data_ptr(), None, 0, mask.data_ptr(), theta.data_ptr(),
                                         pr.data_ptr(), 0, 0.5, lv, 1, ws.data_ptr(), ws.numel(), out.data_ptr(),
                                         stream)
        assert rc == _lib.MMSBM_ERR_UNSUPPORTED
        # at the cap itself the workspace is served
        _lib.check(lib.mmsbm_set_shape(ctx, K, 2, 1, 16384, 1e-10))
        assert lib.mmsbm_pair_votes_workspace_bytes(ctx, ctypes.byref(nbytes)) == _lib.MMSBM_OK
        # an ensemble whose W tile exceeds the LDS: 16 slots x 16 rows x 34 doubles > 64 KiB
        K, P, B = 32, 40, 16
        _lib.check(lib.mmsbm_set_shape(ctx, K, 2, B, P, 1e-10))
        _lib.check(lib.mmsbm_pair_votes_workspace_bytes(ctx, ctypes.byref(nbytes)))
        ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
        theta = torch.full((B, P, K), 1.0 / K, dtype=torch.float64, device=dev)
        pr = torch.full((B, 2, K ** 3), 0.5, dtype=torch.float64, device=dev)
        big = torch.full((P, P, 1), SENTINEL, dtype=torch.int32, device=dev)
        rc = lib.mmsbm_pair_votes(ctx, order.data_ptr(), None, 0, theta.data_ptr(), pr.data_ptr(), -1, 0.5, lv, 1,
                                  ws.data_ptr(), ws.numel(), big.data_ptr(), stream)
        assert rc == _lib.MMSBM_ERR_UNSUPPORTED and b"LDS" in lib.mmsbm_last_error()
        torch.cuda.synchronize(dev)
        assert bool((out == SENTINEL).all()) and bool((big == SENTINEL).all())
    finally:
        lib.mmsbm_destroy(ctx)


# ------------------------------------------------------------------ 10. converged fits
def test_converged_restarts_as_three_slots():
    """tests/golden/converged/A_s{1,2,3}_T300.npz as one ensemble (converged_ref.scan_set)."""
    s = cr.scan_set("A300")
    assert s.per.shape[0] == 3
    eng = engine(s.theta, s.pr)
    used = 0
    for t in ref.two_thresholds(s.per, 257, 0.99):
        for kn in (None, s.known["fold"]):
            got = check(eng, s.per, s.keys, t, None, kn)
            tail = ref.hist_tail(s.per, s.keys, t, [1, 2, 3], known=kn)
            np.testing.assert_array_equal(ref.upper_sums(got), 3 * tail)
            used += int(tail[0] > 0 and tail[2] < s.keys.size)
        check(eng, s.per, s.keys, t, [1], sample=1)
    assert used >= 2
    eng.close()


# ------------------------------------------------------------------ 11. the driver
@pytest.mark.parametrize("allow", [False, True], ids=["all", "allow-genes"])
def test_driver_writes_the_two_tables(tmp_path, allow):
    import random
    from trigenicinteractionpredictor_amd import Model, _lib, scan
    from trigenicinteractionpredictor_amd.engine import EMEngine
    from trigenicinteractionpredictor_amd.restarts import stream_states
    g = os.path.join(GOLDEN, "tiny")
    train, test = os.path.join(g, "train.dat"), os.path.join(g, "test.dat")
    K, B, iters, seed, T, M, top = 3, 3, 5, 1, 0.3, 2, 7
    model = Model()
    model.get_traintest(train, test)
    P = model.P
    files = [str(tmp_path / f) for f in ("top.tsv", "pairs.tsv", "genes.tsv", "allow.txt")]
    argv = ["-t", train, "-e", test, "-k", str(K), "-n", str(B), "-i", str(iters), "--seed", str(seed), "--top",
            str(top), "-o", files[0], "--pair-consensus", files[1], "--pair-votes", str(M), "--gene-consensus",
            files[2], "--pair-threshold", str(T)]
    mask = None
    if allow:
        universe = [i for i in range(P) if i % 3 != 1]
        with open(files[3], "w", encoding="utf-8") as f:
            f.write("".join("%s\n" % model.id_gene[i] for i in universe))
        argv += ["--allow-genes", files[3]]
        mask = scan.pair_mask(P, genes=universe)
    assert scan.main(argv, out=lambda *a: None) == 0
    _, pairs, genes = (open(f, encoding="utf-8").read().rstrip("\n").split("\n") for f in files[:3])
    # the same engine state
    random.seed(seed)
    eng = EMEngine(K, P, B=B, R=model.R, eps=model.eps)
    eng.set_links(_lib.SET_TRAIN, *model._link_arrays(0))
    for b, (_, theta, pr) in enumerate(stream_states(model, K, range(B))):
        eng.upload_slot(b, theta, pr)
    eng.iterate(iters)
    known = scan.known_keys(model, ("train", "test"))
    kw = {} if mask is None else {"mask": mask}
    counts, eligible, ids = eng.pairs_consensus_top(top, T, M, known, **kw)
    gene_counts = eng.gene_vote_census(T, [3, 2, 1], known, **kw)
    eng.close()
    assert pairs[:4] == ["# samples\t%d" % B, "# threshold\t%r" % T, "# min votes\t%d" % M,
                         "rank\tcount\teligible\tids\tnames"]
    rows = [ln.split("\t") for ln in pairs[4:]]
    assert len(rows) == top and counts.max() > 0
    assert rows == [[str(i + 1), str(int(n)), str(int(e)), scan.pair_key(a, b),
                     "_".join(sorted((model.id_gene[int(a)], model.id_gene[int(b)])))]
                    for i, (n, e, (a, b)) in enumerate(zip(counts, eligible, ids))]
    assert genes[:3] == ["# samples\t%d" % B, "# threshold\t%r" % T, "gene\tname\t3\t2\t1"]
    rows = [ln.split("\t") for ln in genes[3:]]
    assert rows == [[str(i), model.id_gene[i]] + [str(int(v)) for v in gene_counts[i]] for i in range(P)]
    assert gene_counts.any() and (np.diff(gene_counts, axis=1) >= 0).all()
    if allow:
        outside = [i for i in range(P) if i % 3 == 1]
        assert not gene_counts[outside].any() and all(int(a) % 3 != 1 and int(b) % 3 != 1 for a, b in ids[counts > 0])
