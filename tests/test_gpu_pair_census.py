"""Pair census (include/mmsbm.h mmsbm_pair_census, EMEngine.pair_census / pairs_top / gene_census,
Model.novel_pair_counts / predict_query_pairs / novel_gene_counts, the scan driver's --pairs and
--gene-census) against the numpy float64 reference of tests/pair_census_ref.py, which scatters
every eligible reference score at or above a threshold to its three pairs.

The counts are integers, so the tests demand equality.  Wherever a test chooses thresholds it first
asserts, on the reference alone, that every threshold is more than 1e-7 relative from every
reference score (census_ref.assert_clear): the project's RTOL of 1e-9 then cannot move a score
across a threshold.  The identity with the census needs no such precondition: the pair census forms
its scores with the census's own score phase, bit for bit.
"""
import ctypes
import functools
import os
from math import comb

import numpy as np
import pytest

import census_ref
import pair_census_ref as ref
import scan_ref
from golden_util import GOLDEN
from scan_gpu import Raw, engine, fixture_case, random_case

pytestmark = pytest.mark.gpu


def check(eng, scores, keys, thresholds, known=None, sample=0):
    """The precondition on the reference alone, then the whole matrix equal to the reference,
    symmetric and with a zero diagonal."""
    census_ref.assert_clear(scores, thresholds)
    P = eng.P
    _, want = ref.ref_pairs(scores, keys, P, thresholds, known)
    got = eng.pair_census(thresholds, known, sample=sample)
    assert got.dtype == np.int32 and got.shape == (P, P, len(thresholds))
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got, got.transpose(1, 0, 2))
    assert not got[np.arange(P), np.arange(P)].any()
    return got


# ------------------------------------------------------------------ 1. exact counts on fixtures
FIXTURES = [("tiny", "K10_s1", 25), ("multi", "K3_s4", 25)]


@pytest.mark.parametrize("exclude", [(), ("train",), ("train", "test")], ids=["all", "train", "novel"])
@pytest.mark.parametrize("fold,name,it", FIXTURES, ids=["%s-%s" % c[:2] for c in FIXTURES])
def test_exact_matrix_on_reference_parameters(fold, name, it, exclude):
    theta, pr, P, _, known, scores, keys = fixture_case(fold, name, it)
    thresholds = census_ref.gap_thresholds(scores, 9)       # 9 gaps (+ 2 adjacent ones when they are new),
    assert 12 <= thresholds.size <= 14               # below the minimum, above the maximum, a duplicate
    thresholds = thresholds[:12]                     # 12 thresholds: two calls of the kernel
    eng = engine(theta[None], pr[None])
    assert eng.lib.mmsbm_pair_census_max_m() == 8
    got = check(eng, scores, keys, thresholds, known[exclude])
    assert got.max() > 0 and got.max() <= P - 2
    eng.close()


# ------------------------------------------------------------------ 2. shapes
@pytest.mark.parametrize("P", [1, 2, 3, 4, 15, 16, 17, 33, 65, 70])
def test_gene_counts(P):
    """Padded rows and columns, one and several row blocks, and P < 3 (all zeros)."""
    theta, pr, scores, keys = random_case(3, P, 11 + P)
    assert scores.size == comb(P, 3)
    eng = engine(theta[None], pr[None])
    if P < 3:
        got = eng.pair_census([1e-300, 0.5, 0.1])
        assert got.shape == (P, P, 3) and got.dtype == np.int32 and not got.any()
        got = eng.pair_census([1e-300, 0.5, 0.1], np.array([7], dtype=np.int64))
        assert got.shape == (P, P, 3) and not got.any()
    else:
        thresholds = census_ref.gap_thresholds(scores, 6)
        check(eng, scores, keys, thresholds)
        check(eng, scores, keys, thresholds, keys[::3].copy())
    eng.close()


@pytest.mark.parametrize("K", [1, 2, 4, 5, 10, 12, 13, 17, 30, 32])
def test_group_counts(K):
    """Every KS template (K = 1 .. 32 in steps of 4) and K that is no multiple of 4."""
    P = 40
    theta, pr, scores, keys = random_case(K, P, 100 + K)
    eng = engine(theta[None], pr[None])
    if K == 1:      # every score equals p_1[0][0][0]: one distinct value, no gaps to sit in
        s = float(pr[0, 0, 0, 1])
        thresholds = np.array([s * (1 - 1e-6), s * (1 + 1e-6)])
    else:
        thresholds = census_ref.gap_thresholds(scores, 6)
    got = check(eng, scores, keys, thresholds)
    if K == 1:
        np.testing.assert_array_equal(got[:, :, 0], (P - 2) * (1 - np.eye(P, dtype=np.int32)))
        assert not got[:, :, 1].any()
    eng.close()


# ------------------------------------------------------------------ 3. identity with the census
@pytest.mark.parametrize("mode", ["sample", "ensemble"])
def test_pair_sums_are_three_times_the_census(mode):
    """Exact, no precondition: the pair census scores carry the census's (the scan's) bits."""
    K, P, N = 10, 70, 50
    th, pr = scan_ref.random_params(K, P, 31, B=3)
    eng = engine(th, pr)
    sample = 1 if mode == "sample" else None
    if mode == "ensemble":
        eng.set_active(2)                              # a B = 3 engine with 2 active slots
    known = random_case(K, P, 32)[3][::4].copy()       # sorted packed keys of a quarter of the triples
    for kn in (None, known):
        scores, _ = eng.scan_top(N, kn, sample=sample)
        assert scores.size == N
        thresholds = scores[np.linspace(0, N - 1, 8).astype(int)]      # AT scores of the scan list
        census, _ = eng.census(thresholds, kn, sample=sample)
        assert census.tolist() == (scores[None, :] >= thresholds[:, None]).sum(axis=1).tolist()
        got = eng.pair_census(thresholds, kn, sample=sample)
        upper = np.triu(np.ones((P, P), dtype=bool), k=1)
        np.testing.assert_array_equal(got[upper].sum(axis=0, dtype=np.int64), 3 * census)
        genes = eng.gene_census(thresholds, kn, sample=sample)
        assert genes.dtype == np.int64 and genes.shape == (P, 8)
        np.testing.assert_array_equal(genes.sum(axis=0), 3 * census)
        np.testing.assert_array_equal(genes, got.sum(axis=1, dtype=np.int64) // 2)
    eng.close()


# ------------------------------------------------------------------ 4. batch, grid, repeats
def test_batch_grid_and_repeats(monkeypatch):
    K, P = 10, 70
    th, pr = scan_ref.random_params(K, P, 41, B=3)
    scores, keys = scan_ref.ref_scores(th[2], pr[2])
    thresholds = census_ref.gap_thresholds(scores, 6)
    known = keys[1::5].copy()
    eng = engine(th, pr)
    th0, p0 = eng.theta.cpu().numpy().copy(), eng.pr.cpu().numpy().copy()
    want = check(eng, scores, keys, thresholds, known, sample=2)
    solo = engine(th[2:3], pr[2:3])                    # the same parameters in a B = 1 engine
    for sample in (0, None):                           # an ensemble of one is that sample
        np.testing.assert_array_equal(solo.pair_census(thresholds, known, sample=sample), want)
    solo.close()
    for grid in ("1", "7"):
        monkeypatch.setenv("MMSBM_PAIR_CENSUS_GRID", grid)
        np.testing.assert_array_equal(eng.pair_census(thresholds, known, sample=2), want)
    monkeypatch.delenv("MMSBM_PAIR_CENSUS_GRID")
    # a repeated call: the call zeroes its output (the allocator hands the last matrix back)
    np.testing.assert_array_equal(eng.pair_census(thresholds, known, sample=2), want)
    assert eng.theta.cpu().numpy().tobytes() == th0.tobytes()
    assert eng.pr.cpu().numpy().tobytes() == p0.tobytes()
    # the ensemble mean, added in slot order
    per = [scan_ref.ref_scores(th[b], pr[b])[0] for b in range(3)]
    mean3 = ((per[0] + per[1]) + per[2]) / 3
    check(eng, mean3, keys, census_ref.gap_thresholds(mean3, 6), known, sample=None)
    eng.close()


def test_the_call_zeroes_a_dirty_output():
    """The raw C call into a matrix full of ones returns the counts, not counts + 1."""
    import torch
    K, P = 3, 33
    theta, pr, scores, keys = random_case(K, P, 11 + P)
    eng = engine(theta[None], pr[None])
    thresholds = np.sort(census_ref.gap_thresholds(scores, 4))[:6]
    census_ref.assert_clear(scores, thresholds)
    want, _ = ref.ref_pairs(scores, keys, P, thresholds)
    raw = Raw(eng, "pair_census", thresholds.size)
    thr = raw.upload(thresholds)
    out = raw.full((P, P, thresholds.size), torch.int32, 1)
    assert raw.call((thr.data_ptr(), thresholds.size), [out]) == 0
    np.testing.assert_array_equal(out.cpu().numpy(), want)         # rank positions, x < y only
    eng.close()


# ------------------------------------------------------------------ 5. exclusion
def test_exclusion_one_gene_one_pair_everything():
    from trigenicinteractionpredictor_amd.scan import rank_order
    K, P = 3, 70
    theta, pr, scores, keys = random_case(K, P, 51)
    thresholds = census_ref.gap_thresholds(scores, 5)
    eng = engine(theta[None], pr[None])
    order = rank_order(P)
    a, b, c = keys // (P * P), (keys // P) % P, keys % P
    # every triple of one gene (rank positions 0, 20 and P - 1): its row and column are zero
    for g in (0, 20, P - 1):
        known = keys[(a == g) | (b == g) | (c == g)].copy()
        assert known.size == comb(P - 1, 2)
        got = check(eng, scores, keys, thresholds, known)
        assert not got[order[g]].any() and not got[:, order[g]].any() and got.any()
    # every triple that contains one pair: that pair is zero, both ways
    for x, y in ((0, 1), (5, 40), (P - 2, P - 1), (15, 16)):
        known = keys[((a == x) | (b == x)) & ((b == y) | (c == y))].copy()
        assert known.size == P - 2
        got = check(eng, scores, keys, thresholds, known)
        assert not got[order[x], order[y]].any() and not got[order[y], order[x]].any()
    # every triple: nothing
    got = check(eng, scores, keys, thresholds, keys.copy())
    assert not got.any()
    eng.close()


# ------------------------------------------------------------------ 6. dense and empty
@pytest.mark.parametrize("K,P,B", [(3, 70, 1), (10, 37, 1), (10, 37, 2)])
def test_dense_and_empty(K, P, B):
    """Below every score: every eligible triple through all three pair roles, = pair_eligible."""
    from trigenicinteractionpredictor_amd.scan import pair_eligible
    th, pr = scan_ref.random_params(K, P, 61, B=B)
    per = [scan_ref.ref_scores(th[b], pr[b]) for b in range(B)]
    keys = per[0][1]
    scores = per[0][0] if B == 1 else (per[0][0] + per[1][0]) / 2
    eng = engine(th, pr)
    sample = 0 if B == 1 else None
    lo, hi = scores.min() * (1 - 1e-3), scores.max() * (1 + 1e-3)
    census_ref.assert_clear(scores, [lo, hi])
    for kn in (None, keys[::3].copy()):
        got = eng.pair_census([lo], kn, sample=sample)
        np.testing.assert_array_equal(got[:, :, 0], pair_eligible(P, kn))
        assert not eng.pair_census([hi], kn, sample=sample).any()
        both = check(eng, scores, keys, [hi, lo, lo], kn, sample=sample)   # descending, a duplicate
        np.testing.assert_array_equal(both[:, :, 1], got[:, :, 0])
    none = eng.pair_census([])
    assert none.shape == (P, P, 0) and none.dtype == np.int32
    assert eng.gene_census([]).shape == (P, 0)
    eng.close()


# ------------------------------------------------------------------ 7. pairs_top
def test_pairs_top_is_the_lexsort_of_the_reference():
    from trigenicinteractionpredictor_amd.scan import pair_eligible
    K, P = 5, 33
    theta, pr, scores, keys = random_case(K, P, 71)
    known = keys[::3].copy()
    eng = engine(theta[None], pr[None])
    t = float(np.sort(census_ref.gap_thresholds(scores, 5))[3])      # a gap in the middle of the range
    census_ref.assert_clear(scores, [t])
    for kn in (None, known):
        rank_mat, _ = ref.ref_pairs(scores, keys, P, [t], kn)
        el = pair_eligible(P, kn)
        for n in (1, 10, comb(P, 2) - 1, comb(P, 2), comb(P, 2) + 5):
            counts, eligible, ids = eng.pairs_top(n, t, kn)
            want_counts, want_ids = ref.top_pairs(rank_mat[:, :, 0], n)
            assert counts.dtype == np.int64 and eligible.dtype == np.int64 and ids.dtype == np.int32
            assert counts.shape == (min(n, comb(P, 2)),) and ids.shape == (min(n, comb(P, 2)), 2)
            np.testing.assert_array_equal(counts, want_counts)
            np.testing.assert_array_equal(ids, want_ids)
            np.testing.assert_array_equal(eligible, el[ids[:, 0], ids[:, 1]])
            assert (counts <= eligible).all()
        assert 0 < counts.max() and np.unique(counts).size < counts.size      # real ties, ordered by key
    eng.close()


def test_pairs_top_all_equal_counts_go_by_key():
    """K = 1: every score equals p_1[0][0][0], every pair has P - 2 hits: the order is the key's."""
    from trigenicinteractionpredictor_amd.scan import rank_order
    P = 13
    th = np.ones((1, P, 1))
    pr = np.zeros((1, 1, 1, 1, 2))
    pr[..., 1], pr[..., 0] = 0.3, 0.7
    eng = engine(th, pr)
    counts, eligible, ids = eng.pairs_top(1000, 0.3 * (1 - 1e-6))
    assert counts.tolist() == [P - 2] * comb(P, 2) and eligible.tolist() == counts.tolist()
    order = rank_order(P)
    x, y = np.triu_indices(P, k=1)                     # row-major: x P + y ascending
    np.testing.assert_array_equal(ids, np.stack([order[x], order[y]], axis=1))
    counts, _, ids = eng.pairs_top(3, 0.3 * (1 + 1e-6))
    assert counts.tolist() == [0, 0, 0] and ids.tolist() == [[0, 1], [0, 10], [0, 11]]
    eng.close()


# ------------------------------------------------------------------ 8. errors
def test_caps_and_errors():
    import torch
    from trigenicinteractionpredictor_amd import _lib
    theta, pr, scores, keys = random_case(10, 40, 110)
    eng = engine(theta[None], pr[None])
    max_m = eng.lib.mmsbm_pair_census_max_m()
    assert max_m == 8
    nbytes = ctypes.c_int64()
    assert eng.lib.mmsbm_pair_census_workspace_bytes(eng.ctx, max_m, ctypes.byref(nbytes)) == 0
    assert eng.lib.mmsbm_pair_census_workspace_bytes(eng.ctx, max_m + 1, ctypes.byref(nbytes)) == _lib.MMSBM_ERR_UNSUPPORTED
    assert eng.lib.mmsbm_pair_census_workspace_bytes(eng.ctx, max_m, None) == _lib.MMSBM_ERR_INVALID
    raw = Raw(eng, "pair_census", max_m)
    thr = raw.upload(np.linspace(0.1, 0.9, max_m + 1))
    out = raw.full((40, 40, max_m + 1), torch.int32, 0)
    assert raw.call((thr.data_ptr(), max_m + 1), [out]) == _lib.MMSBM_ERR_UNSUPPORTED
    assert b"cap" in eng.lib.mmsbm_last_error()
    # by position in the C call: 1 order, 4 theta, 6 sample, 7 thresholds, 9 and 10 workspace, 11 out
    for i, bad in ((1, None), (4, None), (7, None), (11, None), (6, 1), (6, -2), (10, 16), (9, None)):
        assert raw.call((thr.data_ptr(), max_m), [out], replace=[(i, bad)]) == _lib.MMSBM_ERR_INVALID, i
    with pytest.raises(ValueError):
        eng.pair_census([0.5, float("nan")])
    with pytest.raises(ValueError):
        eng.pair_census([float("inf")])
    with pytest.raises(ValueError):
        eng.pair_census([0.5], known=np.array([5, 3], dtype=np.int64))
    with pytest.raises(ValueError):
        eng.pair_census([0.5], sample=1)               # B = 1: outside the active prefix
    with pytest.raises(ValueError):
        eng.pairs_top(3, 0.5, sample=-1)
    eng.close()


# ------------------------------------------------------------------ 9. Model and driver
@functools.lru_cache(maxsize=None)
def fitted_model():
    from trigenicinteractionpredictor_amd import Model
    from trigenicinteractionpredictor_amd.scan import known_keys
    import random
    m = Model()
    m.get_traintest(os.path.join(GOLDEN, "tiny", "train.dat"), os.path.join(GOLDEN, "tiny", "test.dat"))
    random.seed(1)
    m.initialize_parameters(10)
    for _ in range(5):
        m.make_iteration()
    theta, pr = np.array(m.theta), np.array(m.pr)
    scores, keys = scan_ref.ref_scores(theta, pr)
    return m, scores, keys, known_keys(m, ("train",)), known_keys(m)


def test_model_query_pairs_and_gene_counts():
    from trigenicinteractionpredictor_amd.scan import pair_eligible
    m, scores, keys, known_train, known_all = fitted_model()
    P = m.P
    thresholds = census_ref.gap_thresholds(scores, 5)
    census_ref.assert_clear(scores, thresholds)
    t = float(np.sort(thresholds)[3])
    for exclude, known in ((("train", "test"), known_all), (("train",), known_train)):
        rank_mat, gene_mat = ref.ref_pairs(scores, keys, P, thresholds, known)
        np.testing.assert_array_equal(m.novel_pair_counts(thresholds, exclude), gene_mat)
        got = m.novel_gene_counts(thresholds, exclude)
        assert got.dtype == np.int64 and got.shape == (P, thresholds.size)
        np.testing.assert_array_equal(got, ref.ref_gene_counts(scores, keys, P, thresholds, known))
        rows = m.predict_query_pairs(5, t, exclude)
        want_counts, want_ids = ref.top_pairs(ref.ref_pairs_rank(scores, keys, P, [t], known)[:, :, 0], 5)
        el = pair_eligible(P, known)
        assert len(rows) == 5
        for (count, eligible, key, names), n, (i, j) in zip(rows, want_counts, want_ids):
            assert key == "%d_%d" % (i, j) and sorted(key.split("_")) == key.split("_")   # as `links` spells it
            assert names == sorted([m.id_gene[int(i)], m.id_gene[int(j)]])
            assert count == n and eligible == el[i, j] and count <= eligible
            assert isinstance(count, int) and isinstance(eligible, int)
    assert [r[0] for r in rows] == sorted((r[0] for r in rows), reverse=True)
    assert m.predict_query_pairs(2, t, ("train",)) == rows[:2]


def test_driver_writes_the_pair_and_gene_tables(tmp_path):
    from trigenicinteractionpredictor_amd import Model, scan
    g = os.path.join(GOLDEN, "tiny")
    files = [str(tmp_path / name) for name in ("top.tsv", "pairs.tsv", "genes.tsv")]
    rc = scan.main(["-t", os.path.join(g, "train.dat"), "-e", os.path.join(g, "test.dat"), "-k", "3",
                    "-n", "2", "-i", "5", "--seed", "1", "--top", "7", "-o", files[0], "--pairs", files[1],
                    "--pair-threshold", "0.3", "--gene-census", files[2], "--thresholds", "0.1,0.5,0.01"],
                   out=lambda *a: None)
    assert rc == 0
    top, pairs, genes = (open(f, encoding="utf-8").read().rstrip("\n").split("\n") for f in files)
    m = Model()
    m.get_traintest(os.path.join(g, "train.dat"), os.path.join(g, "test.dat"))
    assert top[0].split("\t") == ["rank", "probability", "ids", "names"] and len(top) == 8
    assert pairs[0].split("\t") == ["rank", "count", "eligible", "ids", "names"] and len(pairs) == 8
    rows = [ln.split("\t") for ln in pairs[1:]]
    assert [int(r[0]) for r in rows] == list(range(1, 8))
    counts = [int(r[1]) for r in rows]
    assert counts == sorted(counts, reverse=True)
    el = scan.pair_eligible(m.P, scan.known_keys(m))
    for r in rows:
        i, j = (int(x) for x in r[3].split("_"))
        assert r[3] == scan.pair_key(i, j) and int(r[2]) == el[i, j] and int(r[1]) <= int(r[2])
        assert r[4] == "_".join(sorted([m.id_gene[i], m.id_gene[j]]))
    assert genes[0].split("\t") == ["gene", "name", "0.5", "0.1", "0.01"] and len(genes) == m.P + 1
    rows = [ln.split("\t") for ln in genes[1:]]
    assert [int(r[0]) for r in rows] == list(range(m.P)) and [r[1] for r in rows] == [m.id_gene[i] for i in range(m.P)]
    assert all(0 <= int(r[2]) <= int(r[3]) <= int(r[4]) <= comb(m.P - 1, 2) for r in rows)
