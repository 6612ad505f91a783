"""Partner scan (include/mmsbm.h mmsbm_partners_topn, EMEngine.partners_top, Model.predict_partners /
predict_third, the scan driver's --gene / --all-genes) against a numpy float64 reference
(tests/partners_ref.py), which is itself tied to the pinned C oracle.

A query's row is the exact top N under a total order (score descending, packed triple key
ascending), so the tests demand the identical ordered id list.  Each first asserts, on the reference
alone, that every adjacent relative gap inside the reference's top N + 1 of every query exceeds 1e-9
(the project's RTOL; the kernel's re-association error is about K^3 2^-53 <= 4e-12), so the order is
determined.  No query is skipped.
"""
import functools
import itertools
import os
import random

import numpy as np
import pytest

import partners_ref as ref
import scan_ref
from golden_util import GOLDEN, load
from scan_gpu import engine, fixture_case
from scan_ref import bits

pytestmark = pytest.mark.gpu

RTOL = scan_ref.RTOL


def slices(known):
    off, pairs = known
    return [pairs[off[i]:off[i + 1]] for i in range(off.size - 1)]


def same_rows(x, y):
    return bits(x[0]) == bits(y[0]) and bits(x[1]) == bits(y[1])


def candidates(P):
    return (P - 1) * (P - 2) // 2 if P >= 3 else 0


# ------------------------------------------------------------------ the reference vs the oracle
def test_reference_scorer_matches_the_c_oracle():
    from oracle import c_oracle
    theta, pr, P, _ = fixture_case("small", "K10_s1", 5)[:4]
    rng = np.random.default_rng(0)
    scores, ids = [], []
    for q in (0, 1, 137, 150, 298, 299):                     # every region, the edges of the order
        s, tk, _ = ref.ref_query(theta, pr, q)
        assert s.size == candidates(P) == 44551
        pick = rng.choice(s.size, 334, replace=False)
        scores.append(s[pick])
        ids.append(scan_ref.keys_to_ids(tk[pick], P))
    scores, ids = np.concatenate(scores), np.concatenate(ids)
    assert scores.size >= 2000
    np.testing.assert_allclose(scores, c_oracle.predict(ids, theta, pr), rtol=RTOL, atol=0)


# ------------------------------------------------------------------ 1. exact lists on fixtures
CASES = [("tiny", "K10_s1", 25, 64, 4.9e-6), ("tiny", "K10_s1", 25, 741, 7.1e-7),
         ("tiny", "K3_s1", 5, 64, 1.5e-6), ("multi", "K3_s4", 25, 64, 2.2e-6),
         ("edge", "K3_s5", 25, 66, 4.6e-5), ("small", "K10_s1", 25, 64, 5.6e-8),
         ("small", "K10_s1", 25, 256, 3.0e-8), ("small", "K10_s1", 5, 128, 1.7e-8)]


@pytest.mark.parametrize("exclude", [False, True], ids=["all", "novel"])
@pytest.mark.parametrize("fold,name,it,n,gap", CASES,
                         ids=["%s-%s-it%d-N%d" % c[:4] for c in CASES])
def test_exact_lists_for_every_query(fold, name, it, n, gap, exclude):
    from trigenicinteractionpredictor_amd.scan import partner_known
    theta, pr, P, m = fixture_case(fold, name, it)[:4]
    queries = list(range(P))
    known = partner_known(m, queries) if exclude else None
    eng = engine(theta[None], pr[None])
    rows = eng.partners_top(queries, n, known, sample=0)
    eng.close()
    assert len(rows) == P
    per_query = slices(known) if exclude else [None] * P
    gaps = [ref.check_query(rows[g], theta, pr, g, n, per_query[g]) for g in queries]
    if not exclude:
        assert min(gaps) >= 0.9 * gap        # the fixture's recorded minimum (two digits)
    else:
        assert sum(len(k) for k in per_query) > 0


# ------------------------------------------------------------------ 2. the regions
@pytest.mark.parametrize("P", [1, 2, 3, 4, 16, 17, 33])
def test_regions_and_small_gene_counts(P):
    """Every query (first, last and middle rank positions among them) with N at least the candidate
    count: the whole region structure comes back, then part and all of it excluded."""
    import torch
    N = 512
    th, pr = scan_ref.random_params(3, P, 40 + P)
    eng = engine(th, pr)
    queries = list(range(P))
    order, rank = scan_ref.rank_tables(P)
    assert {int(rank[g]) for g in queries} >= {0, P // 2, P - 1}
    sd, idd, cd = eng.partners_top_async(queries, N)
    torch.cuda.synchronize()
    sd, idd, cd = sd.cpu().numpy(), idd.cpu().numpy(), cd.cpu().numpy()
    assert cd.dtype == np.int64 and cd.tolist() == [candidates(P)] * P
    if P == 3:
        assert cd.tolist() == [1, 1, 1]
    for g in queries:
        n = int(cd[g])
        assert np.isnan(sd[g, n:]).all() and not np.isnan(sd[g, :n]).any()
        assert (idd[g, n:] == -1).all()
        ref.check_query((sd[g, :n], idd[g, :n]), th[0], pr[0], g, N)
    # exclusion: a third of every query's pairs; the last query loses all of them
    rng = np.random.default_rng(P)
    off, pairs = [0], []
    for g in queries:
        _, _, pk = ref.ref_query(th[0], pr[0], int(rank[g]))
        drop = np.sort(pk[rng.random(pk.size) < 1 / 3]) if g != queries[-1] else np.sort(pk)
        # keys of no candidate are ignored: a pair that names q, one beyond the table
        junk = np.array([int(rank[g]) * P + P - 1, P * P + 5], dtype=np.int64)
        drop = np.unique(np.concatenate([drop, junk]))
        pairs.append(drop)
        off.append(off[-1] + drop.size)
    known = (np.array(off, dtype=np.int64), np.concatenate(pairs) if pairs else np.zeros(0, np.int64))
    rows = eng.partners_top(queries, N, known)
    for g, sl in zip(queries, slices(known)):
        _, _, pk = ref.ref_query(th[0], pr[0], int(rank[g]))
        assert rows[g][0].size == candidates(P) - np.isin(pk, sl).sum()
        ref.check_query(rows[g], th[0], pr[0], g, N, sl)
    assert rows[queries[-1]][0].size == 0 and rows[queries[-1]][1].shape == (0, 3)
    # no queries: nothing to write
    assert eng.partners_top([], 8) == []
    eng.close()


# ------------------------------------------------------------------ 3. schedule independence
def test_rows_do_not_depend_on_the_other_queries():
    from trigenicinteractionpredictor_amd.scan import partner_known
    theta, pr, P, m = fixture_case("tiny", "K10_s1", 25)[:4]
    N = 64
    eng = engine(theta[None], pr[None])
    th0, p0 = bits(eng.theta.cpu().numpy()), bits(eng.pr.cpu().numpy())
    queries = list(range(P))
    every = eng.partners_top(queries, N, partner_known(m, queries))
    again = eng.partners_top(queries, N, partner_known(m, queries))
    assert all(same_rows(a, b) for a, b in zip(every, again))
    for g in queries:                                        # one query per call
        (solo,) = eng.partners_top([g], N, partner_known(m, [g]))
        assert same_rows(solo, every[g]), g
    shuffled = queries[::-1] + queries[::3] + [7, 7, 7]        # reversed and duplicated
    rows = eng.partners_top(shuffled, N, partner_known(m, shuffled))
    assert len(rows) == len(shuffled)
    for g, row in zip(shuffled, rows):
        assert same_rows(row, every[g]), g
    assert bits(eng.theta.cpu().numpy()) == th0 and bits(eng.pr.cpu().numpy()) == p0
    eng.close()


def test_one_query_spread_over_the_device_equals_its_row_in_a_full_call():
    """P = 300: a Q = 1 call gives the query hundreds of workgroups and two merge levels, the
    Q = P call a handful and one."""
    theta, pr, P, _ = fixture_case("small", "K10_s1", 25)[:4]
    N = 64
    order, _ = scan_ref.rank_tables(P)
    eng = engine(theta[None], pr[None])
    every = eng.partners_top(list(range(P)), N, sample=0)
    for q in (0, 150, P - 1):                               # first, middle and last rank position
        g = int(order[q])
        (solo,) = eng.partners_top([g], N, sample=0)
        assert same_rows(solo, every[g]), q
        ref.check_query(solo, theta, pr, g, N)
    eng.close()


# ------------------------------------------------------------------ 4. ensemble and slots
def test_ensemble_and_slots():
    from trigenicinteractionpredictor_amd._lib import MMSBMError
    _, vec, _, _ = load("tiny", "K10_s1")
    thetas = np.stack([vec["theta_%d" % it] for it in (1, 5, 25)])
    prs = np.stack([vec["pr_%d" % it] for it in (1, 5, 25)])
    P, N = thetas.shape[1], 64
    queries = list(range(P))
    _, rank = scan_ref.rank_tables(P)
    per = [[ref.ref_query(thetas[b], prs[b], int(rank[g]))[0] for g in queries] for b in range(3)]
    eng = engine(thetas, prs)
    # the mean over the active prefix, added in slot order
    rows = eng.partners_top(queries, N, sample=None)
    for g in queries:
        ref.check_query(rows[g], thetas[0], prs[0], g, N, scores=((per[0][g] + per[1][g]) + per[2][g]) / 3)
    # one slot of the batch = an engine holding only that sample, bit for bit
    for b in range(3):
        mine = eng.partners_top(queries, N, sample=b)
        solo = engine(thetas[b:b + 1], prs[b:b + 1])
        theirs = solo.partners_top(queries, N, sample=0)
        mean1 = solo.partners_top(queries, N, sample=None)   # an ensemble of one is that sample
        solo.close()
        for g in queries:
            assert same_rows(mine[g], theirs[g]) and same_rows(mine[g], mean1[g]), (b, g)
            ref.check_query(mine[g], thetas[b], prs[b], g, N)
    # a shorter active prefix
    eng.set_active(2)
    rows = eng.partners_top(queries, N, sample=None)
    for g in queries:
        ref.check_query(rows[g], thetas[0], prs[0], g, N, scores=(per[0][g] + per[1][g]) / 2)
    with pytest.raises((ValueError, MMSBMError)):
        eng.partners_top(queries, N, sample=2)
    eng.close()


# ------------------------------------------------------------------ 5. ties
def key_order_ids(P, q, n, skip=0):
    """The first candidates of rank position q by packed triple key alone."""
    keys = sorted((lambda t: (t[0] * P + t[1]) * P + t[2])(sorted((q, b, c)))
                  for b, c in itertools.combinations([x for x in range(P) if x != q], 2))
    return scan_ref.keys_to_ids(np.array(keys[skip:skip + n], dtype=np.int64), P)


def test_ties_resolve_by_packed_triple_key():
    K, P, N = 5, 37, 50
    order, rank = scan_ref.rank_tables(P)
    th, pr = scan_ref.random_params(K, 1, 7)
    th = np.repeat(th, P, axis=1)                       # every gene the same row
    eng = engine(th, pr)
    for q in (0, P - 1):          # one region each (q < b < c, b < c < q): one contraction, one score
        g = int(order[q])
        ((s, ids),) = eng.partners_top([g], N)
        assert np.unique(s.view(np.int64)).size == 1
        np.testing.assert_array_equal(ids, key_order_ids(P, q, N))
    eng.close()
    # a middle query crosses all three regions, whose contractions round differently: dyadic
    # parameters make every sum exact, so all (P - 1)(P - 2) / 2 scores share their bits
    K = 4
    row = np.array([0.5, 0.25, 0.125, 0.125])
    rng = np.random.default_rng(3)
    p1 = rng.integers(0, 9, (K, K, K)) / 8.0
    th = np.repeat(row[None, None, :], P, axis=1)
    pr = np.stack([1.0 - p1, p1], axis=-1)[None]
    eng = engine(th, pr)
    q = 18
    g = int(order[q])
    ((s, ids),) = eng.partners_top([g], N)
    assert np.unique(s.view(np.int64)).size == 1
    assert s[0] == np.einsum("x,y,z,xyz->", row, row, row, p1)
    np.testing.assert_array_equal(ids, key_order_ids(P, q, N))
    # the first ten excluded: the list moves on by ten
    first = key_order_ids(P, q, 10)
    pos = np.sort(rank[first.astype(np.int64)], axis=1)
    pair = np.array([[x for x in r if x != q] for r in pos.tolist()], dtype=np.int64)
    known = (np.array([0, 10], dtype=np.int64), np.sort(pair[:, 0] * P + pair[:, 1]))
    ((s2, ids2),) = eng.partners_top([g], N, known)
    np.testing.assert_array_equal(ids2, key_order_ids(P, q, N, skip=10))
    assert bits(s2) == bits(s)
    eng.close()


# ------------------------------------------------------------------ 6. larger K
@pytest.mark.parametrize("K,B", [(13, 1), (30, 1), (30, 4), (32, 2)], ids=["K13", "K30", "K30xB4", "K32xB2"])
def test_larger_k(K, B):
    """K padding, the large-K LDS sizing and the narrower row blocks of the ensemble."""
    P, N = 48, 64
    th, pr = scan_ref.random_params(K, P, 100 + K + B, B)
    _, rank = scan_ref.rank_tables(P)
    queries = list(range(P))
    eng = engine(th, pr)
    rows = eng.partners_top(queries, N)
    eng.close()
    for g in queries:
        total = ref.ref_query(th[0], pr[0], int(rank[g]))[0]
        for b in range(1, B):
            total = total + ref.ref_query(th[b], pr[b], int(rank[g]))[0]
        ref.check_query(rows[g], th[0], pr[0], g, N, scores=total / B)


@pytest.mark.parametrize("K", [1, 2])
def test_smallest_k(K):
    P, N = 20, 64
    th, pr = scan_ref.random_params(K, P, 60 + K)
    order, rank = scan_ref.rank_tables(P)
    queries = list(range(P))
    eng = engine(th, pr)
    rows = eng.partners_top(queries, N)
    eng.close()
    for g in queries:
        if K == 1:      # theta = 1: every score is p_1[0][0][0], the order is by key alone
            assert (rows[g][0] == pr[0, 0, 0, 0, 1]).all()
            np.testing.assert_array_equal(rows[g][1], key_order_ids(P, int(rank[g]), N))
        else:
            ref.check_query(rows[g], th[0], pr[0], g, N)


# ------------------------------------------------------------------ 7. the genome-wide scan
def test_the_best_triple_heads_its_three_genes_lists():
    theta, pr, P, _ = fixture_case("small", "K10_s1", 25)[:4]
    eng = engine(theta[None], pr[None])
    s, ids = eng.scan_top(1, None, sample=0)
    rows = eng.partners_top([int(g) for g in ids[0]], 4, sample=0)
    eng.close()
    for ps, pids in rows:
        np.testing.assert_array_equal(pids[0], ids[0])
        np.testing.assert_allclose(ps[0], s[0], rtol=RTOL, atol=0)


# ------------------------------------------------------------------ 8. errors
def test_errors():
    from trigenicinteractionpredictor_amd import _lib
    th, pr = scan_ref.random_params(3, 20, 5)
    eng = engine(th, pr)
    cap = eng.lib.mmsbm_partners_max_n()
    assert cap >= 1024
    assert len(eng.partners_top([3], cap)[0][0]) == min(cap, candidates(20))
    with pytest.raises(_lib.MMSBMError) as e:
        eng.partners_top([3], cap + 1)
    assert e.value.code == _lib.MMSBM_ERR_UNSUPPORTED
    with pytest.raises(_lib.MMSBMError) as e:
        eng.partners_top([3], 0)
    assert e.value.code == _lib.MMSBM_ERR_INVALID
    for bad in ([20], [-1], [0, 5, 20]):
        with pytest.raises(_lib.MMSBMError) as e:
            eng.partners_top(bad, 8)
        assert e.value.code == _lib.MMSBM_ERR_INVALID
    off = np.array([0, 2, 4], dtype=np.int64)
    with pytest.raises(ValueError):
        eng.partners_top([1, 2], 8, (off, np.array([5, 4, 7, 9])))       # unsorted slice
    with pytest.raises(ValueError):
        eng.partners_top([1, 2], 8, (off, np.array([4, 5, 9, 9])))       # a repeated key
    with pytest.raises(ValueError):
        eng.partners_top([1, 2], 8, (off[:2], np.array([4, 5])))         # offsets of another Q
    # a key may fall from one query's slice to the next: slices are sorted on their own
    assert len(eng.partners_top([1, 2], 8, (off, np.array([4, 9, 5, 7])))) == 2
    eng.close()


# ------------------------------------------------------------------ 9, 10. Model
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


def model_check(m, rows, gene_id, n, exclude):
    from trigenicinteractionpredictor_amd.scan import partner_known
    theta, pr = np.array(m.theta, dtype=np.float64), np.array(m.pr, dtype=np.float64)
    (known,) = slices(partner_known(m, [gene_id], exclude))
    want_s, want_ids, gap = ref.want_list(theta, pr, gene_id, n, known)
    assert gap > 1e-9
    assert [r[1] for r in rows] == ["_".join(str(int(g)) for g in row) for row in want_ids]
    np.testing.assert_allclose([r[0] for r in rows], want_s, rtol=RTOL, atol=0)
    for p, key, names in rows:
        i, j, k = key.split("_")
        assert sorted([i, j, k]) == [i, j, k] and len({i, j, k}) == 3     # the reference's key order
        assert str(gene_id) in (i, j, k)
        assert names == sorted(m.id_gene[int(x)] for x in (i, j, k))
        if "train" in exclude:
            assert key not in m.links
        if "test" in exclude:
            assert key not in m.test_links


def test_model_predict_partners():
    m = fitted_model()
    g = 5
    rows = m.predict_partners(g, 20)
    assert len(rows) == 20
    model_check(m, rows, g, 20, ("train", "test"))
    assert m.predict_partners(m.id_gene[g], 20) == rows        # by name
    assert m.predict_partners(str(g), 20) == rows
    np.testing.assert_allclose(rows[0][0], m.do_prediction(*rows[0][1].split("_")), rtol=RTOL)
    for exclude in (("train",), ("test",), ()):
        model_check(m, m.predict_partners(g, 20, exclude=exclude), g, 20, exclude)
    assert m.predict_partners(g, 20, exclude=())[0][0] >= rows[0][0]
    for bad in (m.P, -m.P - 1):
        with pytest.raises(IndexError):
            m.predict_partners(bad, 5)
    with pytest.raises(KeyError):
        m.predict_partners("no-such-gene", 5)


def test_model_predict_third():
    m = fitted_model()
    g1, g2 = 5, 12
    rows = m.predict_third(g1, g2, m.P, exclude=())
    assert len(rows) == m.P - 2
    probs = [r[0] for r in rows]
    assert probs == sorted(probs, reverse=True)
    thirds = set()
    for p, key, names in rows:
        parts = key.split("_")
        assert sorted(parts) == parts and str(g1) in parts and str(g2) in parts
        (t,) = [x for x in parts if x not in (str(g1), str(g2))]
        thirds.add(int(t))
        np.testing.assert_allclose(p, m.do_prediction(*parts), rtol=RTOL, atol=0)
        assert names == sorted(m.id_gene[int(x)] for x in parts)
    assert thirds == set(range(m.P)) - {g1, g2}
    assert m.predict_third(m.id_gene[g1], str(g2), 7, exclude=()) == rows[:7]
    novel = m.predict_third(g1, g2, m.P)
    assert [r for r in rows if r[1] not in m.links and r[1] not in m.test_links] == novel
    with pytest.raises(ValueError):
        m.predict_third(g1, g1, 3)
    with pytest.raises(IndexError):
        m.predict_third(g1, m.P, 3)


# ------------------------------------------------------------------ 11. the driver
def run_driver(tmp_path, name, extra):
    from trigenicinteractionpredictor_amd import scan
    g = os.path.join(GOLDEN, "tiny")
    out = str(tmp_path / name)
    rc = scan.main(["-t", os.path.join(g, "train.dat"), "-e", os.path.join(g, "test.dat"), "-k", "3",
                    "-n", "2", "-i", "5", "--seed", "1", "--top", "10", "-o", out] + extra,
                   out=lambda *a: None)
    assert rc == 0
    with open(out, encoding="utf-8") as f:
        return f.read()


def parse_table(text):
    lines = text.rstrip("\n").split("\n")
    assert lines[0].split("\t") == ["query", "rank", "probability", "ids", "names"]
    return [ln.split("\t") for ln in lines[1:]]


def test_driver_gene_tables(tmp_path):
    from trigenicinteractionpredictor_amd import Model
    m = Model()
    m.get_traintest(os.path.join(GOLDEN, "tiny", "train.dat"), os.path.join(GOLDEN, "tiny", "test.dat"))
    genes = [m.id_gene[7], "3", m.id_gene[11]]
    texts = [run_driver(tmp_path, n, ["--gene", genes[0], "--gene", ",".join(genes[1:])]) for n in ("a.tsv", "b.tsv")]
    assert texts[0] == texts[1]                              # reproducible with --seed
    rows = parse_table(texts[0])
    assert len(rows) == 30
    assert [r[0] for r in rows] == [m.id_gene[7]] * 10 + [m.id_gene[3]] * 10 + [m.id_gene[11]] * 10
    assert [int(r[1]) for r in rows] == list(range(1, 11)) * 3
    for i in range(3):
        probs = [float(r[2]) for r in rows[10 * i:10 * i + 10]]
        assert probs == sorted(probs, reverse=True)
    for r, gid in zip(rows, [7] * 10 + [3] * 10 + [11] * 10):
        assert str(gid) in r[3].split("_") and len(set(r[3].split("_"))) == 3
        assert r[4].split("_") == sorted(m.id_gene[int(x)] for x in r[3].split("_"))
        assert r[3] not in m.links and r[3] not in m.test_links
    # --all-genes: every gene in id order, and the same rows for the genes asked for above
    every = parse_table(run_driver(tmp_path, "c.tsv", ["--all-genes"]))
    assert [r[0] for r in every] == [m.id_gene[g] for g in range(m.P) for _ in range(10)]
    for gid in (7, 3, 11):
        assert [r for r in every if r[0] == m.id_gene[gid]] == [r for r in rows if r[0] == m.id_gene[gid]]


def test_driver_gene_table_equals_predict_partners(tmp_path):
    """One restart, --best: the driver's engine holds what a Model fitted from the same seed holds."""
    from trigenicinteractionpredictor_amd import Model, scan
    g = os.path.join(GOLDEN, "tiny")
    out = str(tmp_path / "one.tsv")
    argv = ["-t", os.path.join(g, "train.dat"), "-e", os.path.join(g, "test.dat"), "-k", "3", "-n", "1",
            "-i", "5", "--seed", "1", "--top", "10", "--gene", "7", "-o", out]
    assert scan.main(argv, out=lambda *a: None) == 0
    with open(out, encoding="utf-8") as f:
        rows = parse_table(f.read())
    m = Model()
    m.get_traintest(os.path.join(g, "train.dat"), os.path.join(g, "test.dat"))
    random.seed(1)
    m.initialize_parameters(3)
    m.make_iterations(5)
    want = m.predict_partners(7, 10)
    assert [[r[3], r[4].split("_")] for r in rows] == [[k, names] for _, k, names in want]
    np.testing.assert_allclose([float(r[2]) for r in rows], [p for p, _, _ in want], rtol=RTOL)


def test_driver_without_gene_options_is_unchanged(tmp_path):
    """The genome-wide table: same header, same rows as EMEngine.scan_top on the same fit."""
    from trigenicinteractionpredictor_amd import scan
    text = run_driver(tmp_path, "plain.tsv", [])
    lines = text.rstrip("\n").split("\n")
    assert lines[0].split("\t") == ["rank", "probability", "ids", "names"]
    rows = [ln.split("\t") for ln in lines[1:]]
    assert len(rows) == 10 and [int(r[0]) for r in rows] == list(range(1, 11))
    probs = [float(r[1]) for r in rows]
    assert probs == sorted(probs, reverse=True)
    assert all(len(r) == 4 and len(r[2].split("_")) == 3 and len(r[3].split("_")) == 3 for r in rows)
    # byte for byte what run() and the four-column writer give
    import io
    g = os.path.join(GOLDEN, "tiny")
    cfg = scan.parse(["-t", os.path.join(g, "train.dat"), "-e", os.path.join(g, "test.dat"), "-k", "3",
                      "-n", "2", "-i", "5", "--seed", "1", "--top", "10"])
    buf = io.StringIO()
    buf.write("rank\tprobability\tids\tnames\n")
    for rank, p, key, names in scan.run(cfg, out=lambda *a: None):
        buf.write("%d\t%r\t%s\t%s\n" % (rank, p, key, "_".join(names)))
    assert buf.getvalue() == text
