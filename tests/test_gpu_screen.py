"""Screen scan (include/mmsbm.h mmsbm_screen_topn / mmsbm_screen_scores, EMEngine.screen_top /
screen_scores, Model.predict_screen / predict_profiles, the scan driver's --screen) against a numpy
float64 reference (tests/screen_ref.py), which tests/test_screen_host.py ties to the all-triples
scorer.

A query's list is the exact top N under a total order (score descending, packed triple key
ascending), so the tests demand the identical ordered id list.  Each first asserts, on the reference
alone, that every adjacent relative gap inside the reference's top N + 1 exceeds 1e-9 (the project's
RTOL; the kernel's re-association error is about K^2 2^-53), so the order is determined.  On the
converged fits the order is not determined and the set at a clear cut is compared instead
(tests/converged_ref.py).  No query is skipped.
"""
import ctypes
import functools
import os
import random

import numpy as np
import pytest

import converged_ref
import scan_ref
import screen_ref as ref
from golden_util import GOLDEN
from scan_gpu import EXCLUDES, SENTINEL, engine, fixture_case
from scan_ref import bits

pytestmark = pytest.mark.gpu

RTOL = scan_ref.RTOL


def same_rows(x, y):
    return bits(x[0]) == bits(y[0]) and bits(x[1]) == bits(y[1])


def to_ids(P, position_pairs):
    """Pairs of rank positions -> int32[Q][2] gene ids."""
    order, _ = scan_ref.rank_tables(P)
    return order[np.asarray(position_pairs, dtype=np.int64).reshape(-1, 2)].astype(np.int32)


def rank_rows(P, rows):
    """screen_scores' [Q][gene id] -> [Q][rank position]."""
    order, _ = scan_ref.rank_tables(P)
    return rows[:, order]


def csr(slices):
    off = np.zeros(len(slices) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in slices])
    flat = np.concatenate([np.asarray(s, dtype=np.int32) for s in slices]) if slices else np.zeros(0, np.int32)
    return off, flat.astype(np.int32)


def named_thirds(P, pair, scores, ids, rows_by_id):
    """The entries of a screen_scores row (by gene id) that a list's triples name."""
    third = [[g for g in row.tolist() if g not in (int(pair[0]), int(pair[1]))] for row in ids]
    assert all(len(t) == 1 for t in third)
    return rows_by_id[[t[0] for t in third]] if third else np.zeros(0)


# ------------------------------------------------------------------ 1. exact lists and rows
CASES = [(3, 37, 3, 11), (10, 50, 8, 5), (5, 33, 2, 3), (13, 40, 4, 7), (2, 18, 1, 4), (32, 35, 2, 9), (12, 70, 1, 1)]


def case_queries(P, seed):
    rng = np.random.default_rng(seed + 100)
    return np.array([rng.choice(P, 2, replace=False) for _ in range(32)], dtype=np.int32)


@pytest.mark.parametrize("K,P,B,seed", CASES, ids=["K%d-P%d-B%d" % c[:3] for c in CASES])
def test_exact_lists_and_rows(K, P, B, seed):
    th, pr = scan_ref.random_params(K, P, seed, B)
    pairs = case_queries(P, seed)
    assert pairs.shape == (32, 2)
    eng = engine(th, pr)
    for sample in (0, None):
        want = [ref.ref_rows(th, pr, *ref.positions(P, pr_), sample) for pr_ in pairs]
        rows = eng.screen_scores(pairs, sample=sample)
        assert rows.shape == (32, P) and rows.dtype == np.float64
        for i, pair in enumerate(pairs):
            x, y = ref.positions(P, pair)
            ref.check_row(rank_rows(P, rows)[i], want[i], ref.eligible(P, x, y))
        for N in (8, P):
            lists = eng.screen_top(pairs, N, sample=sample)
            assert len(lists) == 32
            for i, pair in enumerate(pairs):
                x, y = ref.positions(P, pair)
                assert lists[i][0].size == min(N, P - 2)
                ref.check_list(lists[i], want[i], P, x, y, N)
                # the list's scores are the row's words
                assert bits(named_thirds(P, pair, *lists[i], rows[i])) == bits(lists[i][0])
    eng.close()


@pytest.mark.parametrize("K,P,B,seed", CASES[:2], ids=["K%d-P%d-B%d" % c[:3] for c in CASES[:2]])
def test_rows_of_every_pair(K, P, B, seed):
    th, pr = scan_ref.random_params(K, P, seed, B)
    x, y = np.triu_indices(P, k=1)
    pairs = to_ids(P, np.stack([x, y], axis=1))
    eng = engine(th, pr)
    for sample in (0, None):
        rows = rank_rows(P, eng.screen_scores(pairs, sample=sample))
        assert rows.shape == (P * (P - 1) // 2, P)
        for i in range(pairs.shape[0]):
            ref.check_row(rows[i], ref.ref_rows(th, pr, int(x[i]), int(y[i]), sample),
                          ref.eligible(P, int(x[i]), int(y[i])))
    eng.close()


# ------------------------------------------------------------------ 2. regions and edges
def edge_positions(P):
    """x = 0, y = P - 1, y = x + 1 (an empty middle region), x and y on both sides of a 16-boundary."""
    cand = [(0, P - 1), (0, 1), (P - 2, P - 1), (P // 2, P // 2 + 1), (15, 16), (14, 17), (16, 17), (3, 32), (31, 33),
            (1, P - 2), (0, P // 2), (15, 47), (47, 48), (20, 64)]
    out = []
    for x, y in cand:
        if 0 <= x < y < P and (x, y) not in out:
            out.append((x, y))
    return out


@pytest.mark.parametrize("P", [1, 2, 3, 4, 15, 16, 17, 31, 32, 33, 47, 65])
def test_regions_and_small_gene_counts(P):
    import torch
    K, N = 3, 80
    th, pr = scan_ref.random_params(K, P, 40 + P, 2)
    eng = engine(th, pr)
    assert eng.screen_top([], 8) == [] and eng.screen_scores([]).shape == (0, P)     # no queries: nothing to write
    if P == 1:
        eng.close()
        return
    base = edge_positions(P)
    assert base
    # 33 queries: the edges cycled, one pair given as (g2, g1), a repeated query
    pos = [base[i % len(base)] for i in range(33)]
    pairs = to_ids(P, pos)
    pairs[1] = pairs[0][::-1]
    for Q in (1, 15, 16, 17, 33):
        for sample in (0, None):
            sd, idd, cd = eng.screen_top_async(pairs[:Q], N, sample=sample)
            rows = eng.screen_scores(pairs[:Q], sample=sample)
            torch.cuda.synchronize()
            sd, idd, cd = sd.cpu().numpy(), idd.cpu().numpy(), cd.cpu().numpy()
            assert cd.dtype == np.int64 and cd.tolist() == [max(P - 2, 0)] * Q
            for i in range(Q):
                x, y = ref.positions(P, pairs[i])
                n = int(cd[i])
                assert np.isnan(sd[i, n:]).all() and not np.isnan(sd[i, :n]).any() and (idd[i, n:] == -1).all()
                want = ref.ref_rows(th, pr, x, y, sample)
                ref.check_row(rank_rows(P, rows)[i], want, ref.eligible(P, x, y))
                if P >= 3:
                    ref.check_list((sd[i, :n], idd[i, :n]), want, P, x, y, N)
                else:
                    assert np.isnan(rows[i]).all()
            if Q > 1:       # (g2, g1) is (g1, g2); a repeated query repeats its answer
                assert bits(sd[1]) == bits(sd[0]) and bits(idd[1]) == bits(idd[0]) and bits(rows[1]) == bits(rows[0])
            for i in range(len(base), Q):
                j = i % len(base)
                if j != 1:
                    assert bits(sd[i]) == bits(sd[j]) and bits(idd[i]) == bits(idd[j]) and bits(rows[i]) == bits(rows[j])
    eng.close()


# ------------------------------------------------------------------ 3. independence
def test_a_query_does_not_depend_on_the_call(monkeypatch):
    K, P, B, seed = CASES[1]
    th, pr = scan_ref.random_params(K, P, seed, B)
    rng = np.random.default_rng(2)
    others = np.array([rng.choice(P, 2, replace=False) for _ in range(40)], dtype=np.int32)
    q = np.array([[7, 31]], dtype=np.int32)
    N = 16
    eng = engine(th, pr)
    th0, p0 = bits(eng.theta.cpu().numpy()), bits(eng.pr.cpu().numpy())
    for sample in (0, None):
        (solo,) = eng.screen_top(q, N, sample=sample)
        solo_row = eng.screen_scores(q, sample=sample)[0]
        x, y = ref.positions(P, q[0])
        ref.check_list(solo, ref.ref_rows(th, pr, x, y, sample), P, x, y, N)
        calls = [(np.concatenate([others[:at], q, others[at:]]), at) for at in (0, 17, 40)]
        calls.append((np.concatenate([q[:, ::-1], others]), 0))
        for chunk in (None, 1, 16, 17):
            if chunk is None:
                monkeypatch.delenv("MMSBM_SCREEN_CHUNK", raising=False)
            else:
                monkeypatch.setenv("MMSBM_SCREEN_CHUNK", str(chunk))    # read at every call
            for pairs, at in calls:
                lists = eng.screen_top(pairs, N, sample=sample)
                rows = eng.screen_scores(pairs, sample=sample)
                assert same_rows(lists[at], solo), (sample, chunk, at)
                assert bits(rows[at]) == bits(solo_row), (sample, chunk, at)
        monkeypatch.delenv("MMSBM_SCREEN_CHUNK", raising=False)
    assert bits(eng.theta.cpu().numpy()) == th0 and bits(eng.pr.cpu().numpy()) == p0
    eng.close()


def test_the_pass_boundary_with_exclusion_and_a_mask(monkeypatch):
    """Every query of a call under each pass size: the known slices and the outputs are indexed by
    the query's place in the call, not in the pass."""
    K, P, B, seed = CASES[0]
    th, pr = scan_ref.random_params(K, P, seed, B)
    pairs = case_queries(P, seed)
    mask, _ = converged_ref.random_pair_mask(P)
    rng = np.random.default_rng(9)
    known = csr([np.sort(rng.choice(P, int(rng.integers(0, 6)), replace=False)) for _ in range(32)])
    eng = engine(th, pr)
    monkeypatch.delenv("MMSBM_SCREEN_CHUNK", raising=False)
    want = eng.screen_top(pairs, 12, known, mask=mask)
    want_rows = eng.screen_scores(pairs, known, mask=mask)
    for chunk in (1, 16, 17):
        monkeypatch.setenv("MMSBM_SCREEN_CHUNK", str(chunk))
        got = eng.screen_top(pairs, 12, known, mask=mask)
        assert all(same_rows(a, b) for a, b in zip(got, want)), chunk
        assert bits(eng.screen_scores(pairs, known, mask=mask)) == bits(want_rows), chunk
    eng.close()


# ------------------------------------------------------------------ 4. every instantiation
@pytest.mark.parametrize("K", [1, 5, 9, 13, 17, 21, 25, 32])
def test_every_instantiation(K):
    """One K per KS = ceil(K / 4) = 1..8, a single sample of a batch of two."""
    P, N = 35, 8
    th, pr = scan_ref.random_params(K, P, 200 + K, 2)
    pairs = to_ids(P, [(0, 34), (3, 4), (15, 16), (10, 30), (16, 33), (1, 17), (33, 34), (0, 1)])
    eng = engine(th, pr)
    lists = eng.screen_top(pairs, N, sample=1)
    rows = rank_rows(P, eng.screen_scores(pairs, sample=1))
    eng.close()
    for i, pair in enumerate(pairs):
        x, y = ref.positions(P, pair)
        want = ref.ref_rows(th, pr, x, y, 1)
        ref.check_row(rows[i], want, ref.eligible(P, x, y))
        if K == 1:      # theta = 1: every score is p_1[0][0][0], the order is by key alone
            assert (lists[i][0] == pr[1, 0, 0, 0, 1]).all()
            np.testing.assert_array_equal(lists[i][1], ref.want_list(want, P, x, y, N)[1])
        else:
            ref.check_list(lists[i], want, P, x, y, N)


# ------------------------------------------------------------------ 5. ties
def test_ties_resolve_by_packed_triple_key():
    # K = 1: every score is bit-equal, so every list is ascending in c and hence in key
    P = 40
    th, pr = scan_ref.random_params(1, P, 3, 2)
    pos = [(0, 39), (5, 6), (16, 31), (38, 39), (0, 1)]
    eng = engine(th, pr)
    for sample in (0, None):
        for (x, y), (s, ids) in zip(pos, eng.screen_top(to_ids(P, pos), P, sample=sample)):
            assert s.size == P - 2 and np.unique(s.view(np.int64)).size == 1
            c = np.array([c for c in range(P) if c not in (x, y)])
            keys = ref.row_keys(P, x, y)[c]
            assert (np.diff(keys) > 0).all()
            np.testing.assert_array_equal(ids, scan_ref.keys_to_ids(keys, P))
    eng.close()
    # K = 4: two genes share one theta row and sit in the same region of the query: they tie and are
    # listed by key, the smaller position first
    K = 4
    th, pr = scan_ref.random_params(K, P, 8)
    order, _ = scan_ref.rank_tables(P)
    x, y = 10, 25
    twins = [(2, 7), (12, 20), (30, 38)]        # one pair of positions per region
    for a, b in twins:
        th[0, order[b]] = th[0, order[a]]
    eng = engine(th, pr)
    ((s, ids),) = eng.screen_top(to_ids(P, [(x, y)]), P)
    rows = rank_rows(P, eng.screen_scores(to_ids(P, [(x, y)])))[0]
    eng.close()
    got = scan_ref.packed(ids, P)
    for a, b in twins:
        assert rows[a].tobytes() == rows[b].tobytes()
        ka, kb = ref.row_keys(P, x, y)[[a, b]]
        ia, ib = int(np.flatnonzero(got == ka)[0]), int(np.flatnonzero(got == kb)[0])
        assert ib == ia + 1 and s[ia].tobytes() == s[ib].tobytes()


# ------------------------------------------------------------------ 6. exclusion
def fixture_queries(m, n_measured=12, n_random=12):
    rng = np.random.default_rng(4)
    pairs = []
    for key in list(m.links)[:400]:
        ids = [int(t) for t in key.split("_")]
        if len(set(ids)) == 3 and len(pairs) < n_measured:
            pairs.append((ids[0], ids[2]) if len(pairs) % 2 else (ids[2], ids[1]))
    pairs += [tuple(int(g) for g in rng.choice(m.P, 2, replace=False)) for _ in range(n_random)]
    return np.array(pairs, dtype=np.int32)


@pytest.mark.parametrize("exclude", EXCLUDES, ids=["all", "no-train", "novel"])
@pytest.mark.parametrize("fold,name", [("multi", "K3_s4"), ("small", "K10_s1")])
def test_exclusion(fold, name, exclude):
    from trigenicinteractionpredictor_amd.scan import screen_known
    fx = fixture_case(fold, name, 25)
    theta, pr, P, m = fx.theta, fx.pr, fx.P, fx.model
    pairs = fixture_queries(m)
    N = 16
    off, thirds = known = screen_known(m, pairs, exclude)
    if exclude:
        assert thirds.size > 0
    eng = engine(theta[None], pr[None])
    lists = eng.screen_top(pairs, N, known, sample=0)
    rows = rank_rows(P, eng.screen_scores(pairs, known, sample=0))
    eng.close()
    tables = [m.links if which == "train" else m.test_links for which in exclude]
    for i, pair in enumerate(pairs):
        x, y = ref.positions(P, pair)
        ok = ref.eligible(P, x, y, thirds[off[i]:off[i + 1]])
        want = ref.ref_row(theta, pr, x, y)
        ref.check_list(lists[i], want, P, x, y, N, ok)
        ref.check_row(rows[i], want, ok)
        for row in lists[i][1]:
            key = "_".join(str(int(g)) for g in row)
            assert not any(key in t for t in tables)


# ------------------------------------------------------------------ 7. mask
def masks_of(P):
    from trigenicinteractionpredictor_amd.scan import pair_mask
    genes = np.sort(np.random.default_rng(6).choice(P, 20, replace=False))
    return {"random": converged_ref.random_pair_mask(P)[0], "allow": pair_mask(P, genes=genes)}


@pytest.mark.parametrize("which", ["random", "allow"])
def test_a_mask_is_the_blocked_thirds_added_to_known(which):
    K, P, B, seed = CASES[1]
    th, pr = scan_ref.random_params(K, P, seed, B)
    mask = masks_of(P)[which]
    order, rank = scan_ref.rank_tables(P)
    # the case's queries, a query whose own pair is blocked and one inside the allowed genes
    bx, by = np.nonzero(np.triu(np.unpackbits(mask.view(np.uint8), axis=1, bitorder="little")[:P, :P], 1))
    free = [(x, y) for x in range(P) for y in (x + 1, x + 2) if y < P and ref.eligible(P, x, y, mask=mask).sum() >= 5][:2]
    assert bx.size and free
    pairs = np.concatenate([case_queries(P, seed), to_ids(P, [(int(bx[0]), int(by[0]))]), to_ids(P, free)])
    rng = np.random.default_rng(8)
    base = [np.sort(rng.choice(P, 3, replace=False)) for _ in range(pairs.shape[0])]
    oks = [ref.eligible(P, *ref.positions(P, pair), mask=mask) for pair in pairs]
    merged = csr([np.union1d(b, np.flatnonzero(~ok)) for b, ok in zip(base, oks)])
    eng = engine(th, pr)
    for sample in (0, None):
        for N in (8, P):
            got = eng.screen_top(pairs, N, csr(base), sample=sample, mask=mask)
            want = eng.screen_top(pairs, N, merged, sample=sample)
            assert all(same_rows(a, b) for a, b in zip(got, want))
        rows = eng.screen_scores(pairs, csr(base), sample=sample, mask=mask)
        assert bits(rows) == bits(eng.screen_scores(pairs, merged, sample=sample))
        own = 32                        # the query whose own pair is blocked: no candidate
        assert got[own][0].size == 0 and got[own][1].shape == (0, 3) and np.isnan(rows[own]).all()
        for i in (33, 33 + len(free) - 1):
            assert got[i][0].size >= 5 - 3
        # against the reference
        for i, pair in enumerate(pairs):
            x, y = ref.positions(P, pair)
            ok = ref.eligible(P, x, y, base[i], mask)
            ref.check_row(rank_rows(P, rows)[i], ref.ref_rows(th, pr, x, y, sample), ok)
        # an all-zero mask is no mask
        zero = np.zeros_like(mask)
        assert all(same_rows(a, b) for a, b in zip(eng.screen_top(pairs, 8, csr(base), sample=sample, mask=zero),
                                                   eng.screen_top(pairs, 8, csr(base), sample=sample)))
        assert bits(eng.screen_scores(pairs, sample=sample, mask=zero)) == bits(eng.screen_scores(pairs, sample=sample))
    eng.close()


# ------------------------------------------------------------------ 8. converged fits
@pytest.mark.parametrize("label", ["A300", "A1000", "C20"])
def test_converged_fits(label):
    """Rows within RTOL; at each query's middle clear cut in [4, 64] the returned set is the
    reference's and the list is sorted by its own bits (converged_ref.check_set_cut): on these fits a
    row holds many gaps at or below 1e-9, so the order is not the reference's to determine."""
    S = converged_ref.scan_set(label)
    P, B = S.P, S.theta.shape[0]
    assert B == (1 if label == "C20" else 3)
    rng = np.random.default_rng(7)
    pos = [tuple(sorted(int(v) for v in rng.choice(P, 2, replace=False))) for _ in range(32)]
    pairs = to_ids(P, pos)
    eng = engine(S.theta, S.pr)
    for sample in (0, None):
        scores = S.per[0] if sample == 0 else S.mean
        rows = rank_rows(P, eng.screen_scores(pairs, sample=sample))
        cuts, refs = [], []
        for i, (x, y) in enumerate(pos):
            c = np.array([c for c in range(P) if c not in (x, y)])
            keys = ref.row_keys(P, x, y)[c]
            at = np.searchsorted(S.keys, keys)
            np.testing.assert_array_equal(S.keys[at], keys)
            want = scores[at]
            assert np.isnan(rows[i, [x, y]]).all()
            np.testing.assert_allclose(rows[i, c], want, rtol=RTOL, atol=0)
            clear = converged_ref.clear_cuts(np.sort(want)[::-1], 4, 64)
            assert clear.size, (label, sample, (x, y))       # no query is skipped
            cuts.append(int(clear[clear.size // 2]))
            refs.append((want, keys))
        for n in sorted(set(cuts)):
            idx = [i for i, c in enumerate(cuts) if c == n]
            lists = eng.screen_top(pairs[idx], n, sample=sample)
            for i, (s, ids) in zip(idx, lists):
                converged_ref.check_set_cut(s, ids, refs[i][0], refs[i][1], n, None, P)
    eng.close()


# ------------------------------------------------------------------ 9. Model and driver
@functools.lru_cache(maxsize=None)
def fitted_model():
    from trigenicinteractionpredictor_amd import Model
    m = Model()
    m.get_traintest(os.path.join(GOLDEN, "tiny", "train.dat"), os.path.join(GOLDEN, "tiny", "test.dat"))
    random.seed(1)
    m.initialize_parameters(10)
    for _ in range(5):
        m.make_iteration()
    return m


def test_model_predict_screen_is_predict_third():
    from trigenicinteractionpredictor_amd.scan import screen_known
    m = fitted_model()
    theta, pr = np.array(m.theta, dtype=np.float64), np.array(m.pr, dtype=np.float64)
    queries = [(5, 12), (0, 1), (m.P - 1, 3)]
    n = 12
    for exclude in (("train", "test"), ("train",), ()):
        lists = m.predict_screen(queries, n, exclude=exclude)
        assert len(lists) == len(queries)
        off, thirds = screen_known(m, queries, exclude)
        for i, (g1, g2) in enumerate(queries):
            x, y = ref.positions(m.P, (g1, g2))
            ok = ref.eligible(m.P, x, y, thirds[off[i]:off[i + 1]])
            assert ref.want_list(ref.ref_row(theta, pr, x, y), m.P, x, y, n, ok)[2] > 1e-9   # the order is determined
            third = m.predict_third(g1, g2, n, exclude=exclude)
            assert [r[1:] for r in lists[i]] == [r[1:] for r in third]         # keys and names
            np.testing.assert_allclose([r[0] for r in lists[i]], [r[0] for r in third], rtol=1e-9, atol=0)
    assert m.predict_screen([(m.id_gene[5], "12")], n) == m.predict_screen([(5, 12)], n) == m.predict_screen([(12, 5)], n)
    assert m.predict_screen([], n) == []
    with pytest.raises(ValueError):
        m.predict_screen([(5, 5)], 3)
    with pytest.raises(IndexError):
        m.predict_screen([(5, m.P)], 3)
    with pytest.raises(KeyError):
        m.predict_screen([("no-such-gene", 5)], 3)


def test_model_predict_profiles_is_do_prediction():
    from trigenicinteractionpredictor_amd.scan import screen_known
    m = fitted_model()
    queries = [(5, 12), (0, 1), (m.P - 1, 3), (7, 20)]
    prof = m.predict_profiles(queries, exclude=())
    assert prof.shape == (len(queries), m.P) and prof.dtype == np.float64
    for i, (g1, g2) in enumerate(queries):
        assert np.flatnonzero(np.isnan(prof[i])).tolist() == sorted((g1, g2))
    rng = np.random.default_rng(0)
    for _ in range(50):
        i = int(rng.integers(len(queries)))
        g1, g2 = queries[i]
        g = int(rng.choice([g for g in range(m.P) if g not in (g1, g2)]))
        key = sorted((str(g1), str(g2), str(g)))                # the reference's key order: slots 1, 2, 3
        np.testing.assert_allclose(prof[i, g], m.do_prediction(*key), rtol=RTOL, atol=0)
    # the excluded thirds are NaN, the rest keeps its bits
    novel = m.predict_profiles(queries)
    off, thirds = screen_known(m, queries)
    order, _ = scan_ref.rank_tables(m.P)
    assert thirds.size
    for i in range(len(queries)):
        gone = order[thirds[off[i]:off[i + 1]]]
        assert np.isnan(novel[i, gone]).all()
        keep = np.ones(m.P, dtype=bool)
        keep[gone] = False
        assert bits(novel[i, keep]) == bits(prof[i, keep])


DRIVER = ["-t", os.path.join(GOLDEN, "tiny", "train.dat"), "-e", os.path.join(GOLDEN, "tiny", "test.dat"), "-k", "3",
          "-n", "1", "-i", "5", "--seed", "1", "--top", "10"]


def run_driver(tmp_path, name, extra):
    from trigenicinteractionpredictor_amd import scan
    out = str(tmp_path / name)
    assert scan.main(DRIVER + ["-o", out] + extra, out=lambda *a: None) == 0
    with open(out, encoding="utf-8") as f:
        return f.read()


def parse_table(path):
    with open(path, encoding="utf-8") as f:
        lines = f.read().rstrip("\n").split("\n")
    assert lines[0].split("\t") == ["query", "rank", "probability", "ids", "names"]
    return [ln.split("\t") for ln in lines[1:]]


@functools.lru_cache(maxsize=None)
def driver_model():
    """What the driver's engine holds after DRIVER's fit: one restart from the same seed."""
    from trigenicinteractionpredictor_amd import Model
    m = Model()
    m.get_traintest(DRIVER[1], DRIVER[3])
    random.seed(1)
    m.initialize_parameters(3)
    m.make_iterations(5)
    return m


def check_table(rows, m, pairs, lists, n):
    assert len(rows) == sum(len(l) for l in lists) > 0
    at = 0
    for (g1, g2), want in zip(pairs, lists):
        a, b = sorted((int(g1), int(g2)), key=str)
        assert len(want) <= n       # fewer: the query has fewer eligible third genes (a blocked pair: none)
        for rank, (p, key, names) in enumerate(want, 1):
            r = rows[at]
            at += 1
            assert r[0] == "%s_%s" % (m.id_gene[a], m.id_gene[b]) and int(r[1]) == rank
            assert r[3] == key and r[4].split("_") == names
            np.testing.assert_allclose(float(r[2]), p, rtol=RTOL, atol=0)


def test_driver_screen_tables(tmp_path):
    m = driver_model()
    qfile = tmp_path / "q.txt"
    qfile.write_text("# queries\n7\t3\n%s %s\n11 4\n" % (m.id_gene[4], m.id_gene[10]))
    pairs = [(7, 3), (4, 10), (11, 4)]
    screen = str(tmp_path / "s.tsv")
    # --query-pairs
    main = run_driver(tmp_path, "a.tsv", ["--screen", screen, "--query-pairs", str(qfile), "--screen-top", "6"])
    check_table(parse_table(screen), m, pairs, m.predict_screen(pairs, 6), 6)
    # without screen options the driver's files are what they were
    census = [str(tmp_path / n) for n in ("c1.tsv", "c2.tsv")]
    plain = run_driver(tmp_path, "b.tsv", ["--census", census[0]])
    assert main == plain
    assert run_driver(tmp_path, "c.tsv", ["--census", census[1], "--screen", screen, "--screen-best", "4"]) == plain
    assert open(census[0]).read() == open(census[1]).read()
    # --screen-best: the pairs --pairs ranks first, default rows per query
    best = [tuple(int(g) for g in r[2].split("_")) for r in m.predict_query_pairs(4, 0.5)]
    assert len(best) == 4
    check_table(parse_table(screen), m, best, m.predict_screen(best, 20), 20)
    # --allow-genes, from both sources
    allow = tmp_path / "allow.txt"
    genes = list(range(0, m.P, 2)) + [3, 7, 11]
    allow.write_text("\n".join(str(g) for g in genes) + "\n")
    mask = m.pair_mask(genes=genes)
    run_driver(tmp_path, "d.tsv", ["--screen", screen, "--query-pairs", str(qfile), "--screen-top", "5", "--allow-genes",
                                   str(allow)])
    want = m.predict_screen(pairs, 5, mask=mask)
    check_table(parse_table(screen), m, pairs, want, 5)
    assert all(int(g) in genes for rows in want for _, key, _ in rows for g in key.split("_"))
    run_driver(tmp_path, "e.tsv", ["--screen", screen, "--screen-best", "3", "--screen-top", "5", "--allow-genes",
                                   str(allow), "--pair-threshold", "0.15"])
    ranked = m.predict_query_pairs(3, 0.15, mask=mask)
    assert all(r[0] > 0 for r in ranked)        # pairs with hits: none of them is a blocked pair
    best = [tuple(int(g) for g in r[2].split("_")) for r in ranked]
    want = m.predict_screen(best, 5, mask=mask)
    assert [len(w) for w in want] == [5, 5, 5]
    check_table(parse_table(screen), m, best, want, 5)


# ------------------------------------------------------------------ 10. refusals
class RawScreen:
    """mmsbm_screen_topn / mmsbm_screen_scores as C sees them, on sentinel-filled outputs."""

    def __init__(self, eng, Q, N):
        import torch
        self.eng, self.torch, self.Q, self.N = eng, torch, Q, N
        self.ws = eng.scan_workspace("screen", Q, N)
        full = lambda shape, dtype: torch.full(shape, SENTINEL, dtype=dtype, device=eng.device)
        self.lists = [full((Q, N), torch.float64), full((Q, N, 3), torch.int32), full((Q,), torch.int64)]
        self.rows = [full((Q, eng.P), torch.float64)]

    def args(self, pairs, lists=True):
        eng = self.eng
        self.pairs = np.ascontiguousarray(pairs, dtype=np.int32)
        outs = self.lists if lists else self.rows
        return [eng.ctx, eng.scan_order.data_ptr(), self.pairs.ctypes.data_as(ctypes.c_void_p), self.Q, None, None, None,
                eng.theta.data_ptr(), eng.pr.data_ptr(), 0, *([self.N] if lists else []), self.ws.data_ptr(),
                self.ws.numel(), *[o.data_ptr() for o in outs], eng._stream()]

    def call(self, args, lists=True):
        rc = (self.eng.lib.mmsbm_screen_topn if lists else self.eng.lib.mmsbm_screen_scores)(*args)
        self.torch.cuda.synchronize(self.eng.device)
        return rc

    def intact(self):
        return all(bool((o == SENTINEL).all()) for o in self.lists + self.rows)


def test_refusals_leave_the_outputs_and_the_context_alone():
    import torch
    from trigenicinteractionpredictor_amd import _lib
    from trigenicinteractionpredictor_amd.scan import pair_mask
    INVALID, UNSUPPORTED = _lib.MMSBM_ERR_INVALID, _lib.MMSBM_ERR_UNSUPPORTED
    P, Q, N = 20, 3, 8
    th, pr = scan_ref.random_params(3, P, 5, 2)
    eng = engine(th, pr)
    assert eng.lib.mmsbm_screen_max_n() == 1024
    good = [[1, 2], [3, 19], [0, 7]]
    raw = RawScreen(eng, Q, N)
    # in the argument lists: 0 ctx, 1 order, 2 pairs, 3 Q, 4 known_off, 5 known_thirds, 6 mask, 7 theta, 8 pr,
    # 9 sample; then N (lists only), ws, ws_bytes, the outputs, the stream
    for lists in (True, False):
        w = 11 if lists else 10          # the workspace pointer
        n_out = 3 if lists else 1
        bad = [("null ctx", good, [(0, None)], INVALID), ("null order", good, [(1, None)], INVALID),
               ("null pairs", good, [(2, None)], INVALID), ("null theta", good, [(7, None)], INVALID),
               ("null pr", good, [(8, None)], INVALID), ("known_off alone", good, [(4, raw.ws.data_ptr())], INVALID),
               ("sample -2", good, [(9, -2)], INVALID), ("sample 2", good, [(9, 2)], INVALID),
               ("id P", [[1, 2], [3, P], [0, 7]], [], INVALID), ("id -1", [[1, 2], [3, 4], [-1, 7]], [], INVALID),
               ("equal ids", [[1, 2], [5, 5], [0, 7]], [], INVALID), ("Q -1", good, [(3, -1)], INVALID),
               ("Q 65536", good, [(3, 65536)], INVALID), ("no ws", good, [(w, None)], INVALID),
               ("misaligned ws", good, [(w, raw.ws.data_ptr() + 8)], INVALID),
               ("small ws", good, [(w + 1, raw.ws.numel() // 2)], INVALID)]
        bad += [("null output %d" % i, good, [(w + 2 + i, None)], INVALID) for i in range(n_out)]
        if lists:
            bad += [("N 0", good, [(10, 0)], UNSUPPORTED), ("N 1025", good, [(10, 1025)], UNSUPPORTED),
                    ("N -1", good, [(10, -1)], UNSUPPORTED)]
        for what, pairs, replace, code in bad:
            args = raw.args(pairs, lists)
            for i, v in replace:
                args[i] = v
            assert raw.call(args, lists) == code, (what, lists)
            assert raw.intact(), (what, lists)
            assert eng.lib.mmsbm_last_error()
    # the context is usable afterwards, through the same scratch and outputs
    assert raw.call(raw.args(good)) == 0 and raw.call(raw.args(good, False), False) == 0
    want = eng.screen_top(good, N, sample=0)      # the raw calls score slot 0
    for i in range(Q):
        assert bits(raw.lists[0][i].cpu().numpy()) == bits(want[i][0])
        assert bits(raw.lists[1][i].cpu().numpy()) == bits(want[i][1])
    assert raw.lists[2].cpu().tolist() == [N] * Q
    assert bits(rank_rows(P, eng.screen_scores(good, sample=0))) == bits(raw.rows[0].cpu().numpy())
    # Q = 0 returns OK and writes nothing
    raw = RawScreen(eng, Q, N)
    for lists in (True, False):
        args = raw.args(good, lists)
        args[3] = 0
        assert raw.call(args, lists) == 0 and raw.intact()
    # the workspace query refuses what the calls refuse
    nbytes = ctypes.c_int64(-7)
    for q, n, code in ((3, 1025, UNSUPPORTED), (3, -1, UNSUPPORTED), (-1, 8, INVALID), (65536, 8, INVALID)):
        assert eng.lib.mmsbm_screen_workspace_bytes(eng.ctx, q, n, ctypes.byref(nbytes)) == code and nbytes.value == -7
    assert eng.lib.mmsbm_screen_workspace_bytes(eng.ctx, 3, 0, ctypes.byref(nbytes)) == 0
    assert 0 < nbytes.value <= raw.ws.numel()       # the rows-only plan fits every list plan
    assert eng.lib.mmsbm_screen_workspace_bytes(None, 3, 8, ctypes.byref(nbytes)) == INVALID
    assert eng.lib.mmsbm_screen_workspace_bytes(eng.ctx, 3, 8, None) == INVALID
    eng.close()

    # shapes: a mask above the pair mask's cap, P above the packed key's; checked before the workspace, so a
    # small scratch and any device pointer for the rank order do
    for P, masked in ((16400, True), (2000001, False)):
        from trigenicinteractionpredictor_amd.engine import EMEngine
        big = EMEngine(1, P, B=1)
        scratch = torch.zeros(4096, dtype=torch.uint8, device=big.device)
        outs = [torch.full((1, 4), SENTINEL, dtype=torch.float64, device=big.device),
                torch.full((1, 4, 3), SENTINEL, dtype=torch.int32, device=big.device),
                torch.full((1,), SENTINEL, dtype=torch.int64, device=big.device)]
        pairs = np.array([[0, 1]], dtype=np.int32)
        rc = big.lib.mmsbm_screen_topn(big.ctx, big.theta.data_ptr(), pairs.ctypes.data_as(ctypes.c_void_p), 1, None,
                                       None, scratch.data_ptr() if masked else None, big.theta.data_ptr(),
                                       big.pr.data_ptr(), 0, 4, scratch.data_ptr(), scratch.numel(),
                                       *[o.data_ptr() for o in outs], big._stream())
        torch.cuda.synchronize()
        assert rc == UNSUPPORTED, P
        assert all(bool((o == SENTINEL).all()) for o in outs)
        if masked:          # without the mask the same shape is served
            assert len(big.screen_top(pairs, 4)[0][0]) == 4
            with pytest.raises(ValueError):
                big.screen_top(pairs, 4, mask=np.zeros((16, 1), dtype=np.uint32))
        big.close()

    # K outside [1, MMSBM_MAX_K] and R < 2: mmsbm_set_shape accepts neither, so the one context that
    # has them is a fresh one (K = R = 0)
    lib = _lib.load()
    ctx = ctypes.c_void_p()
    assert lib.mmsbm_create(0, ctypes.byref(ctx)) == 0
    dev = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    out = torch.full((64,), SENTINEL, dtype=torch.float64, device="cuda")
    pairs = np.array([[0, 1]], dtype=np.int32)
    nbytes = ctypes.c_int64(-7)
    assert lib.mmsbm_screen_workspace_bytes(ctx, 1, 4, ctypes.byref(nbytes)) == UNSUPPORTED and nbytes.value == -7
    rc = lib.mmsbm_screen_scores(ctx, dev.data_ptr(), pairs.ctypes.data_as(ctypes.c_void_p), 1, None, None, None,
                                 dev.data_ptr(), dev.data_ptr(), 0, dev.data_ptr(), dev.numel(), out.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == UNSUPPORTED and bool((out == SENTINEL).all())
    assert lib.mmsbm_set_shape(ctx, 33, 2, 1, 10, 1e-10) == UNSUPPORTED
    assert lib.mmsbm_set_shape(ctx, 3, 1, 1, 10, 1e-10) == UNSUPPORTED
    assert lib.mmsbm_screen_workspace_bytes(ctx, 1, 4, ctypes.byref(nbytes)) == UNSUPPORTED
    assert lib.mmsbm_set_shape(ctx, 3, 2, 1, 10, 1e-10) == 0
    assert lib.mmsbm_screen_workspace_bytes(ctx, 1, 4, ctypes.byref(nbytes)) == 0 and nbytes.value > 0
    lib.mmsbm_destroy(ctx)


def test_python_checks():
    th, pr = scan_ref.random_params(3, 20, 5)
    eng = engine(th, pr)
    off = np.array([0, 2, 4], dtype=np.int64)
    pairs = [(1, 2), (3, 4)]
    with pytest.raises(ValueError):
        eng.screen_top(pairs, 8, (off, np.array([5, 4, 7, 9])))       # an unsorted slice
    with pytest.raises(ValueError):
        eng.screen_top(pairs, 8, (off, np.array([4, 5, 9, 9])))       # a repeated entry
    with pytest.raises(ValueError):
        eng.screen_scores(pairs, (off[:2], np.array([4, 5])))         # offsets of another Q
    with pytest.raises(ValueError):
        eng.screen_top([(1, 1)], 8)
    with pytest.raises(IndexError):
        eng.screen_top([(1, 20)], 8)
    with pytest.raises(ValueError):
        eng.screen_top(pairs, 8, sample=1)
    # positions equal to x or y, or beyond the table, are ignored; a position may fall between slices
    got = eng.screen_top(pairs, 20, (off, np.array([4, 99, 5, 7])))
    assert [g[0].size for g in got] == [17, 16]
    eng.close()
