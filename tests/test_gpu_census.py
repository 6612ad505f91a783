"""Score census (include/mmsbm.h mmsbm_scan_census, EMEngine.census, Model.novel_census /
novel_rank / heldout_ranks, the scan driver's --census and --heldout-ranks) against the numpy float64
reference counter of tests/census_ref.py over all C(P, 3) triples.

The counts are integers, so the tests demand equality.  Wherever a test chooses thresholds it first
asserts, on the reference alone, that every threshold is more than 1e-7 relative from every
reference score (census_ref.assert_clear): the project's RTOL of 1e-9 then cannot move a score
across a threshold.  The identity with the scan needs no such precondition: the census forms its
scores with the scan's own score phase, bit for bit.
"""
import ctypes
import functools
import itertools
import os
from math import comb

import numpy as np
import pytest

import census_ref as ref
import scan_ref
from golden_util import GOLDEN
from scan_gpu import Raw, engine, fixture_case, random_case

pytestmark = pytest.mark.gpu


def check(eng, scores, keys, thresholds, known=None, sample=0):
    """The precondition on the reference alone, then equal counts and total."""
    ref.assert_clear(scores, thresholds)
    want, want_total = ref.ref_census(scores, keys, thresholds, known)
    got, got_total = eng.census(thresholds, known, sample=sample)
    assert got.dtype == np.int64 and got.shape == want.shape and isinstance(got_total, int)
    np.testing.assert_array_equal(got, want)
    assert got_total == want_total
    return got, got_total


# ------------------------------------------------------------------ 1. exact counts on fixtures
FIXTURES = [("tiny", "K10_s1", 25), ("small", "K10_s1", 5), ("multi", "K3_s4", 25)]


@pytest.mark.parametrize("exclude", [(), ("train",), ("train", "test")], ids=["all", "train", "novel"])
@pytest.mark.parametrize("fold,name,it", FIXTURES, ids=["%s-%s" % c[:2] for c in FIXTURES])
def test_exact_counts_on_reference_parameters(fold, name, it, exclude):
    theta, pr, P, _, known, scores, keys = fixture_case(fold, name, it)
    thresholds = ref.gap_thresholds(scores, 60)      # midpoints of gaps, adjacent gaps, below the
    assert thresholds.size >= 8                      # minimum, above the maximum, one duplicate
    assert np.unique(thresholds).size == thresholds.size - 1
    eng = engine(theta[None], pr[None])
    got, total = check(eng, scores, keys, thresholds, known[exclude])
    assert total == comb(P, 3) - known[exclude].size     # known_keys holds distinct-gene keys only
    assert got.max() == total and got.min() == 0
    eng.close()


# ------------------------------------------------------------------ 2. shapes
@pytest.mark.parametrize("P", [0, 1, 2, 3, 4, 15, 16, 17, 33, 65, 70])
def test_gene_counts(P):
    """Padded rows and columns, one and several row blocks, and the counts of P < 3 (all 0).  P = 0
    is no shape of the engine (mmsbm_set_shape refuses P < 1, before and after the census), so no
    census can be asked of it: the case asserts that refusal."""
    from trigenicinteractionpredictor_amd import _lib
    if P == 0:
        from trigenicinteractionpredictor_amd.engine import EMEngine
        with pytest.raises(_lib.MMSBMError) as e:
            EMEngine(3, 0)
        assert e.value.code == _lib.MMSBM_ERR_INVALID
        return
    theta, pr, scores, keys = random_case(3, P, 11 + P)
    assert scores.size == comb(P, 3)
    eng = engine(theta[None], pr[None])
    if P < 3:
        counts, total = eng.census([1e-300, 0.5, 0.1])
        assert counts.tolist() == [0, 0, 0] and total == 0
    else:
        thresholds = ref.gap_thresholds(scores, 40)
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
        thresholds = ref.gap_thresholds(scores, 40)
    check(eng, scores, keys, thresholds)
    eng.close()


# ------------------------------------------------------------------ 3. identity with the scan
@pytest.mark.parametrize("mode", ["sample", "ensemble"])
def test_census_at_the_scores_of_a_scan_list_numbers_the_list(mode):
    """Exact, no precondition: the census scores carry the scan's bits."""
    K, P, N = 10, 70, 50
    th, pr = scan_ref.random_params(K, P, 31, B=3)
    eng = engine(th, pr)
    sample = 1 if mode == "sample" else None
    if mode == "ensemble":
        eng.set_active(2)                              # a B = 3 engine with 2 active slots
    known = random_case(K, P, 32)[3][::4].copy()       # sorted packed keys of a quarter of the triples
    for kn in (None, known):
        scores, ids = eng.scan_top(N, kn, sample=sample)
        assert scores.size == N
        counts, total = eng.census(scores, kn, sample=sample)
        np.testing.assert_array_equal(counts, (scores[None, :] >= scores[:, None]).sum(axis=1))
        assert total == comb(P, 3) - (0 if kn is None else kn.size)
        above, _ = eng.census(np.nextafter(scores[:1], np.inf), kn, sample=sample)
        assert above.tolist() == [0]
    eng.close()


# ------------------------------------------------------------------ 4. batch and grid
def test_batch_grid_and_repeats(monkeypatch):
    K, P = 10, 70
    th, pr = scan_ref.random_params(K, P, 41, B=3)
    scores, keys = scan_ref.ref_scores(th[2], pr[2])
    thresholds = ref.gap_thresholds(scores, 100)
    known = keys[1::5].copy()
    eng = engine(th, pr)
    th0, p0 = eng.theta.cpu().numpy().copy(), eng.pr.cpu().numpy().copy()
    want = check(eng, scores, keys, thresholds, known, sample=2)
    solo = engine(th[2:3], pr[2:3])                    # the same parameters in a B = 1 engine
    for sample in (0, None):                           # an ensemble of one is that sample
        got = solo.census(thresholds, known, sample=sample)
        np.testing.assert_array_equal(got[0], want[0])
        assert got[1] == want[1]
    solo.close()
    for grid in ("1", "7"):
        monkeypatch.setenv("MMSBM_CENSUS_GRID", grid)
        got = eng.census(thresholds, known, sample=2)
        np.testing.assert_array_equal(got[0], want[0])
        assert got[1] == want[1]
    monkeypatch.delenv("MMSBM_CENSUS_GRID")
    again = eng.census(thresholds, known, sample=2)    # a repeated call
    np.testing.assert_array_equal(again[0], want[0])
    assert again[1] == want[1]
    assert eng.theta.cpu().numpy().tobytes() == th0.tobytes()
    assert eng.pr.cpu().numpy().tobytes() == p0.tobytes()
    # the ensemble mean, added in slot order
    per = [scan_ref.ref_scores(th[b], pr[b])[0] for b in range(3)]
    mean3 = ((per[0] + per[1]) + per[2]) / 3
    check(eng, mean3, keys, ref.gap_thresholds(mean3, 100), known, sample=None)
    eng.close()


# ------------------------------------------------------------------ 5. exclusion
def test_exclusion_one_gene_everything_random_and_edge_tiles():
    K, P = 3, 70
    theta, pr, scores, keys = random_case(K, P, 51)
    thresholds = ref.gap_thresholds(scores, 40)
    eng = engine(theta[None], pr[None])
    a, b, c = keys // (P * P), (keys // P) % P, keys % P
    # every triple of one gene (rank positions 0, 20 and P - 1: a dense known list for one a)
    for g in (0, 20, P - 1):
        known = keys[(a == g) | (b == g) | (c == g)].copy()
        assert known.size == comb(P - 1, 2)
        _, total = check(eng, scores, keys, thresholds, known)
        assert total == comb(P - 1, 3)
    # a random 30 %
    pick = np.random.default_rng(5).random(keys.size) < 0.3
    check(eng, scores, keys, thresholds, keys[pick].copy())
    # known keys in the first, the last and diagonal tiles (b and c in one 16-tile, a inside it too)
    triples = [(0, 1, 2), (0, 1, 15), (P - 3, P - 2, P - 1), (0, P - 2, P - 1), (5, 33, 34), (15, 16, 17),
               (16, 17, 18), (31, 32, 47), (47, 48, 63), (63, 64, 69), (0, 15, 16), (17, 20, 31)]
    known = np.sort(np.array([(x * P + y) * P + z for x, y, z in triples], dtype=np.int64))
    _, total = check(eng, scores, keys, thresholds, known)
    assert total == comb(P, 3) - len(triples)
    # keys of no triple are ignored
    junk = np.sort(np.concatenate([known, [(5 * P + 5) * P + 9, (9 * P + 4) * P + 2, P ** 3 + 7]]))
    check(eng, scores, keys, thresholds, junk)
    eng.close()


def test_everything_known_counts_nothing():
    P = 33
    theta, pr, scores, keys = random_case(3, P, 11 + P)
    eng = engine(theta[None], pr[None])
    thresholds = ref.gap_thresholds(scores, 20)
    counts, total = check(eng, scores, keys, thresholds, keys.copy())
    assert total == 0 and not counts.any()
    eng.close()


# ------------------------------------------------------------------ 6. ties
def test_ties_one_group():
    """K = 1: every score equals s = p_1[0][0][0]."""
    P = 37
    th = np.ones((1, P, 1))
    pr = np.zeros((1, 1, 1, 1, 2))
    pr[..., 1], pr[..., 0] = 0.3, 0.7
    eng = engine(th, pr)
    s = 0.3
    counts, total = eng.census([s * (1 - 1e-6), s * (1 + 1e-6)])
    assert total == comb(P, 3) and counts.tolist() == [total, 0]
    top, _ = eng.scan_top(1)
    counts, _ = eng.census([top[0], np.nextafter(top[0], np.inf)])       # at its own value: all
    assert counts.tolist() == [total, 0]
    eng.close()


def test_ties_duplicated_theta_rows():
    """Two groups of genes with identical rows: at most 8 distinct score values, each class counted
    whole at its own value."""
    K, P = 5, 20
    th, pr = scan_ref.random_params(K, 2, 7)
    th = th[:, np.random.default_rng(3).integers(0, 2, P)]     # every gene one of two rows
    eng = engine(th, pr)
    n = comb(P, 3)
    scores, _ = eng.scan_top(4096)
    assert scores.size == n
    values = np.unique(scores)
    assert 1 < values.size <= 8
    counts, total = eng.census(values)
    assert total == n
    np.testing.assert_array_equal(counts, [(scores >= v).sum() for v in values])
    strictly, _ = eng.census(np.nextafter(values, np.inf))
    np.testing.assert_array_equal(strictly, [(scores > v).sum() for v in values])
    assert (counts - strictly).max() > 1                        # real ties
    eng.close()


# ------------------------------------------------------------------ 7. every score binned, 8. caps
def grid_thresholds(scores, n, slack):
    """n + slack thresholds on a linear grid across the score range, those that violate the
    precondition dropped (at most 5 %, asserted on the reference alone), cut to n."""
    grid = np.linspace(scores.min() * 0.999, scores.max() * 1.001, n + slack)
    ok = ref.clear_of_scores(scores, grid)
    assert (~ok).sum() <= 0.05 * grid.size
    return grid[ok][:n] if slack else grid[ok]


def test_every_score_binned_by_1024_thresholds():
    theta, pr, scores, keys = random_case(10, 70, 71)
    eng = engine(theta[None], pr[None])
    thresholds = grid_thresholds(scores, 1024, 0)
    assert thresholds.size >= 0.95 * 1024
    counts, total = check(eng, scores, keys, thresholds)
    assert counts[0] == total and counts[-1] == 0 and np.unique(counts).size > 500
    eng.close()


def test_threshold_caps():
    from trigenicinteractionpredictor_amd import _lib
    theta, pr, scores, keys = random_case(10, 70, 71)
    eng = engine(theta[None], pr[None])
    max_m = eng.lib.mmsbm_census_max_m()
    assert max_m == 1024
    both = grid_thresholds(scores, max_m + 1, 100)
    assert both.size == max_m + 1
    rng = np.random.default_rng(9)
    check(eng, scores, keys, rng.permutation(both[:max_m]))          # one call of max_m
    check(eng, scores, keys, rng.permutation(both))                  # two calls through the binding
    # M = 0: the total only
    counts, total = eng.census([])
    assert counts.shape == (0,) and counts.dtype == np.int64 and total == comb(70, 3)
    # the C ABI refuses M above the cap
    import torch
    nbytes = ctypes.c_int64()
    assert eng.lib.mmsbm_census_workspace_bytes(eng.ctx, max_m + 1, ctypes.byref(nbytes)) == _lib.MMSBM_ERR_UNSUPPORTED
    raw = Raw(eng, "census", max_m)
    thr = raw.upload(np.sort(both))
    assert raw.call((thr.data_ptr(), max_m + 1), [raw.full((max_m + 2,), torch.int64, 0)]) == _lib.MMSBM_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        eng.census([0.5, float("nan")])
    with pytest.raises(ValueError):
        eng.census([0.5], known=np.array([5, 3], dtype=np.int64))
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
    return m, theta, pr, scores, keys, known_keys(m, ("train",)), known_keys(m)


def listed_score(theta, pr, ids):
    """do_prediction in numpy for rows of gene ids, in the order given."""
    p1 = pr[..., 1]
    return np.einsum("nx,ny,nz,xyz->n", theta[ids[:, 0]], theta[ids[:, 1]], theta[ids[:, 2]], p1)


def rank_bounds(scores, keys, known, s, key):
    """The ranks the reference allows a listed triple of reference score s: 1 + the eligible scores
    clearly above it, plus at most those within 1e-8 relative of it (the triple itself left out)."""
    el = np.ones(keys.size, bool) if not len(known) else ~np.isin(keys, known)
    near = el & (np.abs(scores - s) <= 1e-8 * abs(s)) & (keys != key)
    above = int((el & (scores > s) & ~near & (keys != key)).sum())
    return 1 + above, 1 + above + int(near.sum())


def test_model_novel_census_and_rank():
    from trigenicinteractionpredictor_amd.scan import pack_keys, rank_of, rank_order
    m, theta, pr, scores, keys, known_train, known_all = fitted_model()
    P = m.P
    thresholds = ref.gap_thresholds(scores, 30)
    ref.assert_clear(scores, thresholds)
    for exclude, known in ((("train", "test"), known_all), (("train",), known_train), ((), np.zeros(0, np.int64))):
        counts, total = m.novel_census(thresholds, exclude)
        want, want_total = ref.ref_census(scores, keys, thresholds, known)
        np.testing.assert_array_equal(counts, want)
        assert total == want_total
    # listed triples with gaps: more than 1e-7 relative from every other reference score; some
    # measured (excluded themselves), given as ids or names and in any gene order
    order = np.argsort(scores)
    s = scores[order]
    clear = np.flatnonzero((np.diff(s)[1:] > 1e-7 * s[2:]) & (np.diff(s)[:-1] > 1e-7 * s[1:-1])) + 1
    assert clear.size > 100
    pick = order[clear[np.linspace(0, clear.size - 1, 16).astype(int)]]
    measured = np.intersect1d(np.flatnonzero(np.isin(keys, known_all)), order[clear])
    assert measured.size >= 4
    pick = np.concatenate([pick, measured[:4]])
    ids = scan_ref.keys_to_ids(keys[pick], P)
    rng = np.random.default_rng(2)
    triples = []
    for n, row in enumerate(ids):
        row = rng.permutation(row)
        triples.append([m.id_gene[int(g)] for g in row] if n % 2 else [int(g) for g in row])
    rows = m.novel_rank(triples)
    assert len(rows) == len(pick)
    for (rank, p, key), i, row in zip(rows, pick, ids):
        assert key == "_".join(str(int(g)) for g in row)                  # as `links` spells it
        assert p == m.do_prediction(*key.split("_"))
        np.testing.assert_allclose(p, scores[i], rtol=scan_ref.RTOL)
        lo, hi = rank_bounds(scores, keys, known_all, scores[i], keys[i])
        assert lo == hi == rank, (key, rank, lo, hi)
    assert pack_keys(ids, rank_of(rank_order(P)), P).tolist() == keys[pick].tolist()


def test_model_heldout_ranks():
    m, theta, pr, scores, keys, known_train, _ = fitted_model()
    from trigenicinteractionpredictor_amd.scan import pack_keys, rank_of, rank_order
    rows = m.heldout_ranks()
    assert len(rows) == len(m.test_links) > 0
    assert [(r[0], r[2]) for r in rows] == sorted((r[0], r[2]) for r in rows)     # by rank, then key
    assert sorted(r[2] for r in rows) == sorted(m.test_links.keys())
    rank = rank_of(rank_order(m.P))
    exact = 0
    for r, p, key, real in rows:
        assert real == (0 if m.test_links[key][0] else 1)
        ids = np.array([[int(g) for g in key.split("_")]])
        s = float(listed_score(theta, pr, ids)[0])
        np.testing.assert_allclose(p, s, rtol=scan_ref.RTOL)
        distinct = len(set(ids[0].tolist())) == 3
        lo, hi = rank_bounds(scores, keys, known_train, s, int(pack_keys(ids, rank, m.P)[0]) if distinct else -1)
        assert lo <= r <= hi, (key, r, lo, hi)
        exact += lo == hi
    assert exact >= len(rows) // 2          # most test links have gaps: their rank is determined


def test_driver_writes_sorted_reproducible_census_tables(tmp_path):
    from trigenicinteractionpredictor_amd import scan
    g = os.path.join(GOLDEN, "tiny")
    texts = []
    for name in ("a", "b"):
        files = [str(tmp_path / (name + ext)) for ext in (".tsv", ".census.tsv", ".ranks.tsv")]
        rc = scan.main(["-t", os.path.join(g, "train.dat"), "-e", os.path.join(g, "test.dat"), "-k", "3",
                        "-n", "2", "-i", "5", "--seed", "1", "--top", "10", "-o", files[0],
                        "--census", files[1], "--thresholds", "0.5,0.9,0.01,0.1", "--heldout-ranks", files[2]],
                       out=lambda *a: None)
        assert rc == 0
        texts.append([open(f, encoding="utf-8").read() for f in files])
    assert texts[0] == texts[1]
    top, census, ranks = (t.rstrip("\n").split("\n") for t in texts[0])
    assert top[0].split("\t") == ["rank", "probability", "ids", "names"] and len(top) == 11
    # the census table: thresholds descending, counts rising, fraction = count / total
    assert census[0].split("\t")[0] == "# total" and census[1].split("\t") == ["threshold", "count", "fraction"]
    total = int(census[0].split("\t")[1])
    rows = [ln.split("\t") for ln in census[2:]]
    assert [float(r[0]) for r in rows] == [0.9, 0.5, 0.1, 0.01]
    counts = [int(r[1]) for r in rows]
    assert counts == sorted(counts) and 0 <= counts[0] and counts[-1] <= total
    assert [float(r[2]) for r in rows] == [c / total for c in counts]
    n_test = sum(1 for _ in open(os.path.join(g, "test.dat"), encoding="utf-8"))
    from trigenicinteractionpredictor_amd import Model
    m = Model()
    m.get_traintest(os.path.join(g, "train.dat"), os.path.join(g, "test.dat"))
    assert total == comb(m.P, 3) - scan.known_keys(m).size
    # the held-out table: one row per test link, by rank then key
    assert ranks[0].split("\t") == ["rank", "probability", "ids", "real"]
    rows = [ln.split("\t") for ln in ranks[1:]]
    assert len(rows) == len(m.test_links) <= n_test
    assert [(int(r[0]), r[2]) for r in rows] == sorted((int(r[0]), r[2]) for r in rows)
    assert all(int(r[0]) >= 1 and 0.0 <= float(r[1]) <= 1.0 and r[3] in ("0", "1") for r in rows)
    assert sorted(r[2] for r in rows) == sorted(m.test_links.keys())
