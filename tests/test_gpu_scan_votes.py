"""Vote scan (include/mmsbm.h mmsbm_scan_votes, EMEngine.vote_census / consensus, the scan driver's
--consensus) against the numpy float64 reference of tests/votes_ref.py over all C(P, 3) triples of
every slot, and against the product's own census and threshold scan.

A threshold is first shown, on the reference alone, to lie more than 1e-7 relative from every score
of every slot (census_ref.assert_clear over the concatenated scores), so that an error of
RTOL = 1e-9 in a slot's score cannot move a vote; then the histogram, the SET of returned keys and
each row's votes must equal the reference's exactly and each row's score must lie within RTOL of the
reference's slot-order mean.  The order of the list is checked on the product's own bits.
"""
import ctypes
import os
from math import ceil, comb

import numpy as np
import pytest

import census_ref
import scan_gpu
import scan_ref
import scan_rule
import votes_ref
from golden_util import GOLDEN
from scan_gpu import engine
from scan_ref import packed

pytestmark = pytest.mark.gpu

CASES = [(3, 37, 3, 11), (10, 50, 8, 5), (5, 33, 2, 3), (13, 40, 4, 7)]     # (K, P, B, seed)


class Raw(scan_gpu.Raw):
    ENTRY = dict(scan_gpu.Raw.ENTRY, scan_votes="mmsbm_scan_votes")


def assert_list_properties(v, s, ids, P):
    """The list itself: dtypes, unique keys, its order (votes descending, then score descending,
    then key ascending), ids = keys_to_ids(keys).  -> the packed keys."""
    assert v.dtype == np.int32 and s.dtype == np.float64 and ids.dtype == np.int32
    assert v.ndim == 1 and s.shape == v.shape and ids.shape == (v.size, 3)
    keys = packed(ids, P)
    assert np.unique(keys).size == keys.size
    dv, ds, dk = np.diff(v), np.diff(s), np.diff(keys)
    assert (dv <= 0).all()
    assert (ds[dv == 0] <= 0).all()
    assert (dk[(dv == 0) & (ds == 0)] > 0).all()
    np.testing.assert_array_equal(ids, scan_ref.keys_to_ids(keys, P))
    return keys


def exclusions(keys, P, seed=5):
    """None, a random 5 % of the keys, all keys of one a."""
    pick = np.random.default_rng(seed).random(keys.size) < 0.05
    return [None, keys[pick].copy(), keys[keys // (P * P) == 3].copy()]


def check(eng, per, keys, t, known=None, sample=None, min_votes=None):
    """One threshold against the reference: the histogram, then for each min_votes the set of rows,
    each row's votes and score, and the list's own order.  per: the scores of the scored slots."""
    P, ns = eng.P, per.shape[0]
    census_ref.assert_clear(per.reshape(-1), [t])
    votes_r, keys_r, mean_r, hist_r = votes_ref.ref_votes(per, keys, t, known=known)
    hist = eng.vote_census(t, known, sample=sample)
    assert hist.dtype == np.int64 and hist.shape == (ns + 1,)
    np.testing.assert_array_equal(hist, hist_r)
    for m in sorted({1, ceil(ns / 2), ns}) if min_votes is None else min_votes:
        v, s, ids = eng.consensus(t, m, known, sample=sample)
        got = assert_list_properties(v, s, ids, P)
        want = votes_ref.ref_hits(votes_r, keys_r, mean_r, m)
        np.testing.assert_array_equal(np.sort(got), np.array(sorted(want), dtype=np.int64))
        assert v.size == hist_r[m:].sum()
        at = np.searchsorted(keys_r, got)
        np.testing.assert_array_equal(v, votes_r[at])
        np.testing.assert_allclose(s, mean_r[at], rtol=scan_ref.RTOL, atol=0)
    return hist


# ------------------------------------------------------------------ 1. the reference
@pytest.mark.parametrize("K,P,B,seed", CASES + [(K, P, B, seed) for K, _, B, seed in CASES for P in (20, 53)])
def test_against_the_reference(K, P, B, seed):
    """P = 53: interior tiles, boundary tiles and a ragged last tile; P = 20: boundary tiles only."""
    c = votes_ref.case(K, P, seed, B)
    thresholds = votes_ref.clear_thresholds(c.per, 65)
    eng = engine(c.theta, c.pr)
    total = comb(P, 3)
    for known in exclusions(c.keys, P):
        for q in (0.1, 0.5, 0.9):
            hist = check(eng, c.per, c.keys, votes_ref.at_quantile(c.per, thresholds, q), known)
            assert hist.sum() == total - (0 if known is None else known.size) and hist[0] < hist.sum()
        # below every score: every eligible triple has every vote and is listed (many flushes of
        # the staging buffer); above every score: none has any
        hist = check(eng, c.per, c.keys, float(thresholds[0]), known, min_votes=[1])
        assert hist.tolist() == [0] * B + [total - (0 if known is None else known.size)]
        hist = check(eng, c.per, c.keys, float(thresholds[-1]), known, min_votes=[1, B])
        assert hist.tolist() == [total - (0 if known is None else known.size)] + [0] * B
    # at its own P a case has every counter in use at the median (tests/test_votes_host.py)
    if (K, P, B, seed) in CASES:
        hist = check(eng, c.per, c.keys, votes_ref.near_median(c.per), min_votes=range(1, B + 1))
        assert (hist > 0).all()
    eng.close()


@pytest.mark.parametrize("P", [2, 3])
def test_one_triple_and_none(P):
    c = votes_ref.case(3, P, 11, 3)
    eng = engine(c.theta, c.pr)
    if P == 2:
        for sample in (None, 1):
            hist = eng.vote_census(0.5, sample=sample)
            assert hist.tolist() == [0] * (4 if sample is None else 2)
            v, s, ids = eng.consensus(1e-300, 1, sample=sample)
            assert v.shape == (0,) and s.shape == (0,) and ids.shape == (0, 3)
            assert v.dtype == np.int32 and s.dtype == np.float64 and ids.dtype == np.int32
    else:
        lo, hi = np.sort(c.per[:, 0])[[0, -1]]
        for t, votes in ((lo * 0.5, 3), (hi * 2, 0), ((np.sort(c.per[:, 0])[1] + hi) / 2, 1)):
            census_ref.assert_clear(c.per.reshape(-1), [t])
            hist = eng.vote_census(t)
            assert hist.tolist() == [int(v == votes) for v in range(4)]
            v, s, ids = eng.consensus(t, 1)
            assert v.tolist() == ([votes] if votes else [])
            if votes:
                assert ids.tolist() == scan_ref.keys_to_ids(c.keys, 3).tolist()
                np.testing.assert_allclose(s, c.mean, rtol=scan_ref.RTOL, atol=0)
    eng.close()


# ------------------------------------------------------------------ 2. the family's bits
def test_exact_identities_with_the_census_and_the_threshold_scan():
    """Product against product, no tolerance."""
    K, P, B, seed = 10, 53, 4, 21
    c = votes_ref.case(K, P, seed, B)
    t = votes_ref.near_median(c.per)
    lo = float(votes_ref.clear_thresholds(c.per)[0])                # below every score of every slot
    known = c.keys[1::9].copy()
    eng = engine(c.theta, c.pr)
    hist = eng.vote_census(t, known)
    total = eng.census([], known)[1]
    assert hist.sum() == total == c.keys.size - known.size and (hist > 0).all()
    slot_counts = [int(eng.census([t], known, sample=s)[0][0]) for s in range(B)]
    assert (np.arange(B + 1) * hist).sum() == sum(slot_counts)
    # the rows are the slots' threshold scans combined
    lists = [set(packed(eng.scan_above(t, known, sample=s)[1], P).tolist()) for s in range(B)]
    v1, s1, ids1 = eng.consensus(t, 1, known)
    keys1 = packed(ids1, P)
    assert set(keys1.tolist()) == set.union(*lists)
    assert v1.tolist() == [sum(k in li for li in lists) for k in keys1.tolist()]
    vB, sB, idsB = eng.consensus(t, None, known)                     # None: every slot
    assert set(packed(idsB, P).tolist()) == set.intersection(*lists) and (vB == B).all() and vB.size > 0
    for m in range(1, B + 1):                                        # each cut is the head of the list
        v, s, ids = eng.consensus(t, m, known)
        n = int((v1 >= m).sum())
        assert v.size == n == hist[m:].sum()
        assert v.tobytes() == v1[:n].tobytes() and s.tobytes() == s1[:n].tobytes() and ids.tobytes() == ids1[:n].tobytes()
    # a row's score is the ensemble's, bit for bit
    s_all, ids_all = eng.scan_above(lo, known)
    assert s_all.size == total
    bits = dict(zip(packed(ids_all, P).tolist(), s_all.view(np.int64).tolist()))
    assert [bits[k] for k in keys1.tolist()] == s1.view(np.int64).tolist()
    # one slot: [total - c, c], through the batch and alone
    for s in range(B):
        np.testing.assert_array_equal(eng.vote_census(t, known, sample=s), [total - slot_counts[s], slot_counts[s]])
    s = 2
    solo = engine(c.theta[s:s + 1], c.pr[s:s + 1])
    want = eng.consensus(t, 1, known, sample=s)
    assert want[0].size == slot_counts[s] and (want[0] == 1).all()
    above = eng.scan_above(t, known, sample=s)
    assert want[1].tobytes() == above[0].tobytes() and want[2].tobytes() == above[1].tobytes()
    for sample in (None, 0):                                         # an ensemble of one is that sample
        np.testing.assert_array_equal(solo.vote_census(t, known, sample=sample), [total - slot_counts[s], slot_counts[s]])
        got = solo.consensus(t, 1, known, sample=sample)
        assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
    solo.close()
    # a shrunken active prefix: the first two slots
    eng.set_active(2)
    two = engine(c.theta[:2], c.pr[:2])
    h2 = eng.vote_census(t, known)
    assert h2.shape == (3,)
    np.testing.assert_array_equal(h2, two.vote_census(t, known))
    np.testing.assert_array_equal(h2, votes_ref.ref_votes(c.per, c.keys, t, ns=2, known=known)[3])
    for m in (1, 2):
        assert all(g.tobytes() == w.tobytes() for g, w in zip(eng.consensus(t, m, known), two.consensus(t, m, known)))
    with pytest.raises(ValueError):
        eng.consensus(t, 3, known)                                   # more votes than scored slots
    two.close()
    eng.close()


# ------------------------------------------------------------------ 3. kernel variants
@pytest.mark.parametrize("K", [3, 7, 10, 13, 18, 23, 27, 30])
def test_every_chain_length(K):
    """KS = ceil(K / 4) = 1..8, the ensemble instantiation (B = 2) and the single-sample one."""
    P, B = 53, 2
    c = votes_ref.case(K, P, 300 + K, B)
    assert scan_rule.width(K, B) == 4
    eng = engine(c.theta, c.pr)
    known = exclusions(c.keys, P)[1]
    hist = check(eng, c.per, c.keys, votes_ref.near_median(c.per), known)
    assert (hist > 0).all()
    t1 = votes_ref.near_median(c.per[1:2])
    hist = check(eng, c.per[1:2], c.keys, t1, known, sample=1)
    assert (hist > 0).all()
    eng.close()


@pytest.mark.parametrize("ns,width", [(3, 4), (5, 2), (9, 1)])
def test_every_row_block_width(ns, width):
    K, P = 30, 53
    assert scan_rule.width(K, ns) == width
    c = votes_ref.case(K, P, 330, 9)
    eng = engine(c.theta, c.pr)
    eng.set_active(ns)
    per = c.per[:ns]
    hist = check(eng, per, c.keys, votes_ref.near_median(per), exclusions(c.keys, P)[1])
    assert hist.shape == (ns + 1,) and hist.sum() > 0
    eng.close()


def test_an_ensemble_beyond_the_lds_is_refused():
    from trigenicinteractionpredictor_amd import _lib
    K, P, B = 30, 53, 16
    assert scan_rule.width(K, B) == 0 and scan_rule.last_supported(K) == 15
    th, pr = scan_ref.random_params(K, P, 331, B)
    eng = engine(th, pr)
    with pytest.raises(_lib.MMSBMError) as e:
        eng.vote_census(0.5)
    assert e.value.code == _lib.MMSBM_ERR_UNSUPPORTED
    raw = Raw(eng, "scan_votes")
    outs = votes_outs(raw, B, 8)
    assert raw.call((0.5, 1, 8), outs, sample=-1) == _lib.MMSBM_ERR_UNSUPPORTED and raw.intact()
    # the context stays usable: one slot, and the largest ensemble that fits
    s, keys = scan_ref.ref_scores(th[3], pr[3])
    check(eng, s[None], keys, votes_ref.near_median(s[None]), sample=3)
    eng.set_active(15)
    assert eng.vote_census(0.5).sum() == comb(P, 3)
    eng.close()


# ------------------------------------------------------------------ 4. grid
def test_nothing_depends_on_the_grid(monkeypatch):
    K, P, B, seed = CASES[3]
    c = votes_ref.case(K, 53, seed, B)
    t = votes_ref.near_median(c.per)
    known = c.keys[2::7].copy()
    eng = engine(c.theta, c.pr)
    want_h, want = eng.vote_census(t, known), eng.consensus(t, 2, known)
    assert want[0].size > 1000 and (want_h > 0).all()
    for grid in ("1", "7", None, None):                              # the default grid, and a repeated call
        if grid is None:
            monkeypatch.delenv("MMSBM_SCAN_VOTES_GRID", raising=False)
        else:
            monkeypatch.setenv("MMSBM_SCAN_VOTES_GRID", grid)
        np.testing.assert_array_equal(eng.vote_census(t, known), want_h)
        assert all(g.tobytes() == w.tobytes() for g, w in zip(eng.consensus(t, 2, known), want))
    eng.close()


# ------------------------------------------------------------------ 5. the C call
SENTINEL_ROWS = 64
SENTINEL = scan_gpu.SENTINEL


def votes_outs(raw, ns, rows, null=False):
    """The five outputs of mmsbm_scan_votes, full of the sentinel: hist [ns + 1], then scores, keys
    and votes with SENTINEL_ROWS sentinel rows behind `rows` (None each with null), the count."""
    torch = raw.torch
    arrays = [None] * 3 if null else [raw.full((rows + SENTINEL_ROWS,), dt) for dt in (torch.float64, torch.int64,
                                                                                      torch.int32)]
    return [raw.full((ns + 1 + SENTINEL_ROWS,), torch.int64), *arrays, raw.full((1,), torch.int64)]


def intact(outs):
    return all(bool((o == SENTINEL).all()) for o in outs if o is not None)


def votes_call(raw, ns, t, min_votes, capacity, null=False, rows=None, **kw):
    """-> (return code, hist, scores, keys, votes, count) on the host; the arrays whole, sentinel
    rows included."""
    outs = votes_outs(raw, ns, max(capacity, 0) if rows is None else rows, null)
    rc = raw.call((float(t), min_votes, capacity), outs, **kw)
    return (rc, *[None if o is None else o.cpu().numpy() for o in outs[:4]], int(outs[4].cpu()[0]))


def test_c_call_and_its_capacity_guard():
    K, P, B, seed = CASES[3]
    c = votes_ref.case(K, P, seed, B)
    t = votes_ref.near_median(c.per)
    eng = engine(c.theta, c.pr)
    m = 2
    want_h = eng.vote_census(t)
    v, s, ids = eng.consensus(t, m)
    want = dict(zip(packed(ids, P).tolist(), zip(v.tolist(), s.tolist())))
    count = len(want)
    assert count > 1000 and count == want_h[m:].sum()
    raw = Raw(eng, "scan_votes")
    for cap in (0, count - 1, count, count + 5):
        rc, hist, sc, ky, vt, n = votes_call(raw, B, t, m, cap, sample=-1)
        assert rc == 0 and n == count                                # always the full count
        np.testing.assert_array_equal(hist[:B + 1], want_h)
        assert (hist[B + 1:] == SENTINEL).all()
        k = min(cap, count)
        rows = dict(zip(ky[:k].tolist(), zip(vt[:k].tolist(), sc[:k].tolist())))
        assert len(rows) == k and all(want.get(key) == row for key, row in rows.items())
        if cap >= count:
            assert rows == want
        # nothing at or past min(count, capacity): the rest of the arrays and the sentinel rows
        assert (sc[k:] == SENTINEL).all() and (ky[k:] == SENTINEL).all() and (vt[k:] == SENTINEL).all()
    # a histogram-only call with NULL arrays
    rc, hist, _, _, _, n = votes_call(raw, B, t, m, 0, null=True, sample=-1)
    assert rc == 0 and n == count
    np.testing.assert_array_equal(hist[:B + 1], want_h)
    # the same workspace at another cut and back: the cursor and the histogram start from zero
    rc, hist, _, _, _, n = votes_call(raw, B, t, B, 0, null=True, sample=-1)
    assert rc == 0 and n == want_h[B] and 0 < n < count
    np.testing.assert_array_equal(hist[:B + 1], want_h)
    rc, hist, _, _, _, n = votes_call(raw, 1, t, 1, 0, null=True, sample=1)
    assert rc == 0 and hist[:2].tolist() == [comb(P, 3) - n, n] and n == eng.census([t], sample=1)[0][0]
    rc, hist, _, _, _, n = votes_call(raw, B, t, m, 0, null=True, sample=-1)
    assert rc == 0 and n == count
    eng.close()


# ------------------------------------------------------------------ 6. refusals
def test_refusals_leave_the_outputs_and_the_context_intact():
    from trigenicinteractionpredictor_amd import _lib
    from trigenicinteractionpredictor_amd.scan import LimitError
    K, P, B, seed = CASES[0]
    c = votes_ref.case(K, P, seed, B)
    t = votes_ref.near_median(c.per)
    eng = engine(c.theta, c.pr)
    eng.set_active(2)
    ns = 2
    raw = Raw(eng, "scan_votes")
    INVALID = _lib.MMSBM_ERR_INVALID

    def refused(t=t, min_votes=1, capacity=16, null=False, nulls=(), **kw):
        outs = votes_outs(raw, ns, 16, null)
        for i in nulls:
            outs[i] = None
        rc = raw.call((float(t), min_votes, capacity), outs, **dict({"sample": -1}, **kw))
        return rc == INVALID and intact(outs)

    for bad in (float("nan"), float("inf"), float("-inf")):          # a non-finite threshold
        assert refused(t=bad)
        for call in (eng.vote_census, eng.vote_census_async, eng.consensus, eng.consensus_async):
            with pytest.raises(ValueError):
                call(bad)
    assert refused(capacity=-1)                                      # negative capacity
    assert refused(null=True)                                        # null row arrays, capacity > 0
    for i in (1, 2, 3):
        assert refused(nulls=(i,))                                   # any one of them
    assert refused(nulls=(0,)) and refused(nulls=(0,), capacity=0)   # no out_hist
    assert refused(nulls=(4,)) and refused(nulls=(4,), capacity=0)   # no out_count
    for i in (0, 1, 4, 5):                                           # ctx, order, theta, pr
        assert refused(replace=[(i, None)])
    for m in (0, -1, ns + 1, B):                                     # min_votes outside [1, ns]
        assert refused(min_votes=m)
    assert refused(min_votes=2, sample=0)                            # one slot has one vote
    for m in (0, 3):
        with pytest.raises(ValueError):
            eng.consensus(t, m)
    with pytest.raises(ValueError):
        eng.consensus(t, 2, sample=1)
    for sample in (2, 3, -2):                                        # outside the active prefix
        assert refused(sample=sample)
    for sample in (2, 3, -1):
        with pytest.raises(ValueError):
            eng.vote_census(t, sample=sample)
    assert refused(n_known=3) and refused(n_known=-1)                # keys announced, none given
    with pytest.raises(ValueError):
        eng.consensus(t, known=np.array([5, 3], dtype=np.int64))     # unsorted
    assert refused(ws=(raw.ws.data_ptr(), raw.ws.numel() - 1))       # too small
    assert refused(ws=(raw.ws.data_ptr() + 8, raw.ws.numel() - 8))   # misaligned
    assert refused(ws=(0, raw.ws.numel()))                           # missing
    nbytes = ctypes.c_int64()
    assert eng.lib.mmsbm_scan_votes_workspace_bytes(None, ctypes.byref(nbytes)) == INVALID
    assert eng.lib.mmsbm_scan_votes_workspace_bytes(eng.ctx, None) == INVALID
    # a limit below the count: the error holds the count, and the list call is not made
    count = int(eng.vote_census(t)[1:].sum())
    assert count > 100
    with pytest.raises(ValueError, match=str(count)) as e:
        eng.consensus(t, 1, limit=count - 1)
    assert isinstance(e.value, LimitError) and (e.value.count, e.value.limit) == (count, count - 1)
    with pytest.raises(LimitError):
        eng.consensus_async(t, 1, limit=count - 1)
    # after all of it the context answers, through the C call and the binding
    rc, hist, sc, ky, vt, n = votes_call(raw, ns, t, 1, count, sample=-1)
    assert rc == 0 and n == count
    v, s, ids = eng.consensus(t, 1, limit=count)
    assert v.size == count and sorted(packed(ids, P).tolist()) == sorted(ky[:count].tolist())
    check(eng, c.per[:2], c.keys, t)
    eng.close()


def test_async_calls_return_device_tensors():
    import torch
    K, P, B, seed = CASES[2]
    c = votes_ref.case(K, P, seed, B)
    t = votes_ref.near_median(c.per)
    eng = engine(c.theta, c.pr)
    stream = torch.cuda.Stream(eng.device)
    for st in (None, stream):
        hist = eng.vote_census_async(t, stream=st)
        votes, scores, ids = eng.consensus_async(t, 1, stream=st)
        (stream if st is not None else torch.cuda.current_stream(eng.device)).synchronize()
        assert all(x.is_cuda for x in (hist, votes, scores, ids))
        np.testing.assert_array_equal(hist.cpu().numpy(), eng.vote_census(t, stream=st))
        want = eng.consensus(t, 1, stream=st)
        assert all(g.cpu().numpy().tobytes() == w.tobytes() for g, w in zip((votes, scores, ids), want))
    eng.close()


# ------------------------------------------------------------------ 7. the driver
def test_driver_writes_the_consensus_table(tmp_path):
    import random
    from trigenicinteractionpredictor_amd import Model, _lib, scan
    from trigenicinteractionpredictor_amd.engine import EMEngine
    from trigenicinteractionpredictor_amd.restarts import stream_states
    g = os.path.join(GOLDEN, "small")
    train, test = os.path.join(g, "train.dat"), os.path.join(g, "test.dat")
    K, B, iters, seed = 3, 3, 5, 1
    base = ["-t", train, "-e", test, "-k", str(K), "-n", str(B), "-i", str(iters), "--seed", str(seed), "--top", "10"]
    # a first run finds a threshold with a list of modest length: the smallest census count >= 100
    grid = ",".join("%.2f" % v for v in np.arange(99, 0, -1) / 100)
    files = [str(tmp_path / f) for f in ("top0.tsv", "census0.tsv")]
    assert scan.main(base + ["-o", files[0], "--census", files[1], "--thresholds", grid], out=lambda *a: None) == 0
    lines = open(files[1], encoding="utf-8").read().rstrip("\n").split("\n")
    total = int(lines[0].split("\t")[1])
    T = min((ln.split("\t") for ln in lines[2:] if int(ln.split("\t")[1]) >= 100), key=lambda r: int(r[1]))[0]
    # the run under test: a mean >= T needs one slot >= T, so M = 1 lists at least those 100
    M = 1
    files = [str(tmp_path / f) for f in ("top.tsv", "consensus.tsv")]
    rc = scan.main(base + ["-o", files[0], "--consensus", files[1], "--consensus-threshold", T, "--min-votes", str(M)],
                   out=lambda *a: None)
    assert rc == 0
    lines = open(files[1], encoding="utf-8").read().rstrip("\n").split("\n")
    assert lines[0] == "# samples\t%d" % B and lines[1] == "# threshold\t%r" % float(T)
    header = [ln.split("\t") for ln in lines[2:3 + B]]
    assert [h[:2] for h in header] == [["# votes", str(v)] for v in range(B, -1, -1)]
    hist = {int(h[1]): int(h[2]) for h in header}
    assert sum(hist.values()) == total                               # the census total of the first run
    assert lines[3 + B].split("\t") == ["rank", "votes", "probability", "ids", "names"]
    rows = [ln.split("\t") for ln in lines[4 + B:]]
    assert len(rows) == sum(c for v, c in hist.items() if v >= M) >= 100
    assert [int(r[0]) for r in rows] == list(range(1, len(rows) + 1))
    # the rows are EMEngine.consensus on the same engine state
    model = Model()
    model.get_traintest(train, test)
    random.seed(seed)
    eng = EMEngine(K, model.P, B=B, R=model.R, eps=model.eps)
    eng.set_links(_lib.SET_TRAIN, *model._link_arrays(0))
    for b, (_, theta, pr) in enumerate(stream_states(model, K, range(B))):
        eng.upload_slot(b, theta, pr)
    eng.iterate(iters)
    known = scan.known_keys(model, ("train", "test"))
    np.testing.assert_array_equal(eng.vote_census(float(T), known), [hist[v] for v in range(B + 1)])
    votes, scores, ids = eng.consensus(float(T), M, known)
    eng.close()
    assert [[r[1], r[2], r[3]] for r in rows] == [[str(int(v)), repr(float(p)), "_".join(str(int(x)) for x in row)]
                                                  for v, p, row in zip(votes, scores, ids)]
    assert all(r[4] == "_".join(sorted(model.id_gene[int(x)] for x in r[3].split("_"))) for r in rows)
    # the default M is every restart
    files = [str(tmp_path / f) for f in ("top2.tsv", "consensus2.tsv")]
    assert scan.main(base + ["-o", files[0], "--consensus", files[1], "--consensus-threshold", T],
                     out=lambda *a: None) == 0
    lines2 = open(files[1], encoding="utf-8").read().rstrip("\n").split("\n")
    assert lines2[:4 + B] == lines[:4 + B] and len(lines2) - (4 + B) == hist[B]
    # a count above --consensus-limit is refused, with the count, before anything is written
    out = str(tmp_path / "refused.tsv")
    rc = scan.main(base + ["-o", out, "--consensus", str(tmp_path / "refused.votes.tsv"), "--consensus-threshold", T,
                           "--min-votes", str(M), "--consensus-limit", str(len(rows) - 1)], out=lambda *a: None)
    assert rc == 2 and not os.path.exists(out) and not os.path.exists(str(tmp_path / "refused.votes.tsv"))
