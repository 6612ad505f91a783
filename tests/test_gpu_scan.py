"""Genome-wide scan (include/mmsbm.h mmsbm_scan_topn, EMEngine.scan_top, Model.predict_novel, the
scan driver) against a numpy float64 reference scorer, which is itself tied to the pinned C oracle.

The result is the exact top N under a total order (score descending, packed key ascending), so the
tests demand the identical ordered id list.  Each first asserts, on the reference alone, that every
adjacent relative gap inside the reference's top N + 1 exceeds 1e-9 (the project's RTOL; the
kernel's re-association error is about K^3 2^-53 <= 4e-12), so the order is determined.
"""
import itertools
import os

import numpy as np
import pytest

import scan_ref
from golden_util import GOLDEN, load
from scan_gpu import engine, fixture_case

pytestmark = pytest.mark.gpu

RTOL = scan_ref.RTOL


def check(got_scores, got_ids, scores, keys, n, P, known=None):
    want_s, want_k = scan_ref.top(scores, keys, n, known)
    scan_ref.assert_gaps(want_s)
    want_s, want_k = want_s[:n], want_k[:n]
    assert got_ids.dtype == np.int32 and got_scores.dtype == np.float64
    assert got_ids.shape == (want_k.size, 3)
    np.testing.assert_array_equal(got_ids, scan_ref.keys_to_ids(want_k, P))
    np.testing.assert_allclose(got_scores, want_s, rtol=RTOL, atol=0)
    if known is not None and len(known):
        assert not np.isin(scan_ref.packed(got_ids, P), known).any()


# ------------------------------------------------------------------ the reference vs the oracle
def test_reference_scorer_matches_the_c_oracle():
    from oracle import c_oracle
    theta, pr, P, _, _, scores, keys = fixture_case("small", "K10_s1", 5)
    assert scores.size == 4455100
    pick = np.random.default_rng(0).choice(scores.size, 2000, replace=False)
    ids = scan_ref.keys_to_ids(keys[pick], P).astype(np.int32)
    np.testing.assert_allclose(scores[pick], c_oracle.predict(ids, theta, pr), rtol=RTOL, atol=0)


# ------------------------------------------------------------------ 1. exact list on fixtures
CASES = [("tiny", "K10_s1", 25, n) for n in (1, 64, 1000)] + \
        [("small", "K10_s1", 5, n) for n in (100, 4096)] + \
        [("multi", "K3_s4", 25, n) for n in (16, 100)]


@pytest.mark.parametrize("exclude", [False, True], ids=["all", "novel"])
@pytest.mark.parametrize("fold,name,it,n", CASES, ids=["%s-%s-N%d" % (c[0], c[1], c[3]) for c in CASES])
def test_exact_list_on_reference_parameters(fold, name, it, n, exclude):
    theta, pr, P, _, known, scores, keys = fixture_case(fold, name, it)
    known = known["train", "test"]
    eng = engine(theta[None], pr[None])
    got_s, got_ids = eng.scan_top(n, known if exclude else None, sample=0)
    check(got_s, got_ids, scores, keys, n, P, known if exclude else None)
    eng.close()


# ------------------------------------------------------------------ 2. ties
def test_ties_resolve_by_packed_key():
    K, P, N = 5, 37, 50
    th, pr = scan_ref.random_params(K, 1, 7)
    th = np.repeat(th, P, axis=1)                       # every gene the same row
    eng = engine(th, pr)
    first = np.array(list(itertools.combinations(range(P), 3))[:N + 10])
    first_keys = (first[:, 0] * P + first[:, 1]) * P + first[:, 2]
    s, ids = eng.scan_top(N)
    assert np.unique(s.view(np.int64)).size == 1        # all scores share their bits
    np.testing.assert_array_equal(ids, scan_ref.keys_to_ids(first_keys[:N], P))
    s2, ids2 = eng.scan_top(N, known=first_keys[:10])
    np.testing.assert_array_equal(ids2, scan_ref.keys_to_ids(first_keys[10:N + 10], P))
    np.testing.assert_array_equal(s2.view(np.int64), s.view(np.int64))
    eng.close()


# ------------------------------------------------------------------ 3. ensemble and slots
def test_ensemble_and_slots():
    from trigenicinteractionpredictor_amd._lib import MMSBMError
    _, vec, _, _ = load("tiny", "K10_s1")
    thetas = np.stack([vec["theta_%d" % it] for it in (1, 5, 25)])
    prs = np.stack([vec["pr_%d" % it] for it in (1, 5, 25)])
    P, N = thetas.shape[1], 64
    per = [scan_ref.ref_scores(thetas[b], prs[b]) for b in range(3)]
    keys = per[0][1]
    eng = engine(thetas, prs)
    # the mean over the active prefix, added in slot order
    mean3 = ((per[0][0] + per[1][0]) + per[2][0]) / 3
    s, ids = eng.scan_top(N, sample=None)
    check(s, ids, mean3, keys, N, P)
    # N = 4096 keeps the candidate buffer in the workspace instead of the LDS
    s, ids = eng.scan_top(4096, sample=None)
    check(s, ids, mean3, keys, 4096, P)
    # one slot of the batch = an engine holding only that sample, bit for bit
    s1, ids1 = eng.scan_top(N, sample=1)
    solo = engine(thetas[1:2], prs[1:2])
    t1, jds1 = solo.scan_top(N, sample=0)
    np.testing.assert_array_equal(s1.view(np.int64), t1.view(np.int64))
    np.testing.assert_array_equal(ids1, jds1)
    t1, jds1 = solo.scan_top(N, sample=None)            # an ensemble of one is that sample
    np.testing.assert_array_equal(s1.view(np.int64), t1.view(np.int64))
    np.testing.assert_array_equal(ids1, jds1)
    check(s1, ids1, per[1][0], keys, N, P)
    solo.close()
    # a shorter active prefix
    eng.set_active(2)
    s, ids = eng.scan_top(N, sample=None)
    check(s, ids, (per[0][0] + per[1][0]) / 2, keys, N, P)
    with pytest.raises((ValueError, MMSBMError)):
        eng.scan_top(N, sample=2)
    eng.close()


# ------------------------------------------------------------------ 4. edges
def test_fewer_eligible_than_n():
    import torch
    th, pr = scan_ref.random_params(4, 5, 3)
    eng = engine(th, pr)
    scores, keys = scan_ref.ref_scores(th[0], pr[0])
    assert scores.size == 10
    s, ids = eng.scan_top(64)
    check(s, ids, scores, keys, 64, 5)
    sd, idd, count = eng.scan_top_async(64)
    torch.cuda.synchronize()
    assert int(count.cpu()[0]) == 10
    assert np.isnan(sd.cpu().numpy()[10:]).all() and not np.isnan(sd.cpu().numpy()[:10]).any()
    assert (idd.cpu().numpy()[10:] == -1).all()
    # everything excluded
    s, ids = eng.scan_top(64, known=np.sort(keys))
    assert s.size == 0 and ids.shape == (0, 3)
    eng.close()


@pytest.mark.parametrize("P", [1, 2, 3, 16, 17])
def test_small_gene_counts(P):
    th, pr = scan_ref.random_params(3, P, 11 + P)
    eng = engine(th, pr)
    scores, keys = scan_ref.ref_scores(th[0], pr[0])
    assert scores.size == P * (P - 1) * (P - 2) // 6
    s, ids = eng.scan_top(32)
    check(s, ids, scores, keys, 32, P)
    eng.close()


def test_n_above_the_cap_is_unsupported():
    from trigenicinteractionpredictor_amd import _lib
    th, pr = scan_ref.random_params(3, 20, 5)
    eng = engine(th, pr)
    cap = eng.lib.mmsbm_scan_max_n()
    assert cap >= 4096
    with pytest.raises(_lib.MMSBMError) as e:
        eng.scan_top(cap + 1)
    assert e.value.code == _lib.MMSBM_ERR_UNSUPPORTED
    with pytest.raises(_lib.MMSBMError) as e:
        eng.scan_top(0)
    assert e.value.code == _lib.MMSBM_ERR_INVALID
    eng.close()


def test_scan_leaves_parameters_untouched_and_repeats_bitwise():
    theta, pr, P, _, known, _, _ = fixture_case("tiny", "K10_s1", 25)
    known = known["train", "test"]
    eng = engine(theta[None], pr[None])
    th0, p0 = eng.theta.cpu().numpy().copy(), eng.pr.cpu().numpy().copy()
    a = eng.scan_top(1000, known)
    b = eng.scan_top(1000, known)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    assert eng.theta.cpu().numpy().tobytes() == th0.tobytes()
    assert eng.pr.cpu().numpy().tobytes() == p0.tobytes()
    eng.close()


# ------------------------------------------------------------------ 5. larger K
@pytest.mark.parametrize("K,B", [(30, 1), (13, 1), (30, 4), (30, 8), (32, 2)],
                         ids=["K30", "K13", "K30xB4", "K30xB8", "K32xB2"])
def test_larger_k(K, B):
    """K padding, the large-K LDS sizing and (B = 4, 8 at K = 30) the narrower row blocks."""
    P, N = 50, 64
    th, pr = scan_ref.random_params(K, P, 100 + K + B, B)
    per = [scan_ref.ref_scores(th[b], pr[b]) for b in range(B)]
    total = per[0][0]
    for b in range(1, B):
        total = total + per[b][0]
    eng = engine(th, pr)
    s, ids = eng.scan_top(N)
    check(s, ids, total / B, per[0][1], N, P)
    eng.close()


# ------------------------------------------------------------------ 6. Model and driver
def test_model_predict_novel():
    from trigenicinteractionpredictor_amd import Model
    import random
    m = Model()
    m.get_traintest(os.path.join(GOLDEN, "tiny", "train.dat"), os.path.join(GOLDEN, "tiny", "test.dat"))
    random.seed(1)
    m.initialize_parameters(10)
    for _ in range(5):
        m.make_iteration()
    rows = m.predict_novel(20)
    assert len(rows) == 20
    probs = [r[0] for r in rows]
    assert probs == sorted(probs, reverse=True)
    for p, key, names in rows:
        i, j, k = key.split("_")
        assert sorted([i, j, k]) == [i, j, k] and len({i, j, k}) == 3     # the reference's key order
        np.testing.assert_allclose(p, m.do_prediction(i, j, k), rtol=RTOL)
        assert names == sorted(names)
        assert sorted(m.gene_id[g] for g in names) == sorted(int(x) for x in (i, j, k))
        assert key not in m.links and key not in m.test_links
    # without exclusion measured triples may come back; the list is still the global top
    every = m.predict_novel(20, exclude=())
    assert every[0][0] >= rows[0][0]


def test_driver_writes_a_sorted_reproducible_table(tmp_path):
    from trigenicinteractionpredictor_amd import scan
    g = os.path.join(GOLDEN, "tiny")
    texts = []
    for name in ("a.tsv", "b.tsv"):
        out = str(tmp_path / name)
        rc = scan.main(["-t", os.path.join(g, "train.dat"), "-e", os.path.join(g, "test.dat"), "-k", "3",
                        "-n", "2", "-i", "5", "--seed", "1", "--top", "10", "-o", out], out=lambda *a: None)
        assert rc == 0
        with open(out, encoding="utf-8") as f:
            texts.append(f.read())
    assert texts[0] == texts[1]
    lines = texts[0].rstrip("\n").split("\n")
    assert lines[0].split("\t") == ["rank", "probability", "ids", "names"]
    rows = [ln.split("\t") for ln in lines[1:]]
    assert len(rows) == 10
    assert [int(r[0]) for r in rows] == list(range(1, 11))
    probs = [float(r[1]) for r in rows]
    assert probs == sorted(probs, reverse=True)
    assert all(len(r[2].split("_")) == 3 and len(r[3].split("_")) == 3 for r in rows)
