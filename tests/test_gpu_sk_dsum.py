"""The small-K E-step's d sums (csrc/sk.h phase 1): the products of four consecutive chunks of a
block are reduced in one butterfly (csrc/mmsbm.hip row16_merge), so a chunk's d depends on where
the chunk sits in its group of four, on the stretch changes inside the group and on how many of
the group's chunks exist.  Folds that put stretch ends on every position of a group and leave
last groups of 1, 2 and 3 chunks, in the fused family (SK_U + SK_LL) and the two-pass one
(SK_A + SK_B), against the C oracle at the suite's tolerance (tests/test_gpu_parity.py), after
1 and 5 iterations; one bitwise comparison of a sample alone with the same sample in a batch.
"""
import functools

import numpy as np
import pytest

import ratings_ref as ref

pytestmark = pytest.mark.gpu

RTOL = 1e-9
ATOL = 1e-300
ENV = ("MMSBM_SK", "MMSBM_SK_Y", "MMSBM_SK_FUSED", "MMSBM_UNITS", "MMSBM_GRAPH", "MMSBM_SK_RHO")

# name -> (P, E, MMSBM_UNITS).  "sparse": 60 genes with a few links each, so a unit carries as
# many stretches as it may (8, or 4 from K = 11) and their ends fall anywhere in a group.
# "long": 20 genes in nearly every triple they can form, with two or three units asked for per
# group of streams: a unit then closes only at its stretch cap, or at 128 chunks, so units run
# over several 16-chunk blocks and end inside one.
FOLDS = {"sparse": (60, 260, None), "long": (20, 1100, "2,3")}


@pytest.fixture(autouse=True)
def plain_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


@functools.lru_cache(maxsize=None)
def fold(name, R):
    P, E, _ = FOLDS[name]
    ids, counts = ref.links(P, E, R, 40 + R + len(name))
    tids, tcounts = ref.links(P, 80, R, 7 + R)
    for a in (ids, counts, tids, tcounts):
        a.setflags(write=False)
    return ids, counts, tids, tcounts


@functools.lru_cache(maxsize=None)
def start(name, K, R, sample=0):
    th, pr = ref.params(FOLDS[name][0], K, R, 1000 * sample + 10 * K + R)
    for a in (th, pr):
        a.setflags(write=False)
    return th, pr


@functools.lru_cache(maxsize=None)
def oracle(name, K, R):
    """{iterations: (theta, p, train L, test L)} of the C oracle after 1 and 5 iterations; one
    run per (fold, K, R), shared by the kernel families."""
    from oracle import c_oracle
    ids, counts, tids, tcounts = fold(name, R)
    th, pr = start(name, K, R)
    out = {}
    for it in range(1, 6):
        th, pr = c_oracle.make_iteration(ids, counts, th, pr, 1e-10)
        if it in (1, 5):
            out[it] = (th, pr, c_oracle.loglik(ids, counts, th, pr, 1e-10),
                       c_oracle.loglik(tids, tcounts, th, pr, 1e-10))
    return out


def engine(name, K, R, monkeypatch, B=1, family=None):
    from trigenicinteractionpredictor_amd import EMEngine
    P, _, units = FOLDS[name]
    if units is not None:
        monkeypatch.setenv("MMSBM_UNITS", units)
    ids, counts, tids, tcounts = fold(name, R)
    eng = EMEngine(K, P, B=B, R=R, family=family)
    eng.set_links(0, ids, counts)
    eng.set_links(1, tids, tcounts)
    return eng


def test_folds_have_the_shapes_they_are_named_for():
    """(host only, but it describes the GPU cases) sparse: most (slot, gene, rating) runs have 1-4
    links; long: the slot-0 runs of genes 0 and 1, neighbours in a unit, together exceed one
    16-chunk block for every rating."""
    for R in (2, 3):
        ids, counts, _, _ = fold("sparse", R)
        runs = []
        for s in range(3):
            for r in range(R):
                runs += np.bincount(ids[counts[:, r] > 0, s], minlength=60).tolist()
        runs = np.array([x for x in runs if x])
        assert np.median(runs) <= 4 and (runs <= 4).mean() > 0.5
        ids, counts, _, _ = fold("long", R)
        for r in range(R):
            run = np.bincount(ids[counts[:, r] > 0, 0], minlength=20)
            assert run[0] + run[1] > 64


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "two-pass"])
@pytest.mark.parametrize("name", sorted(FOLDS))
@pytest.mark.parametrize("R", [2, 3])
@pytest.mark.parametrize("K", [2, 3, 9, 10, 12])
def test_d_sums_match_oracle(monkeypatch, K, R, name, fused):
    if not fused:
        monkeypatch.setenv("MMSBM_SK_FUSED", "0")
    eng = engine(name, K, R, monkeypatch)
    assert eng.plan_info()["small_k"] == (2 if fused else 1)
    th0, pr0 = start(name, K, R)
    eng.upload(th0[None], pr0[None])
    want = oracle(name, K, R)
    done = 0
    for it in (1, 5):
        eng.iterate(it - done)
        done = it
        th, pr = eng.download()
        L, LT = eng.loglik(0)[0], eng.loglik(1)[0]
        th_o, pr_o, L_o, LT_o = want[it]
        print("K=%d R=%d %s %s it=%d max rel err theta %.2e p %.2e L %.2e LT %.2e"
              % (K, R, name, "fused" if fused else "two-pass", it, ref.max_rel(th[0], th_o),
                 ref.max_rel(pr[0], pr_o), ref.max_rel(L, L_o), ref.max_rel(LT, LT_o)))
        np.testing.assert_allclose(th[0], th_o, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(pr[0], pr_o, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(L, L_o, rtol=RTOL)
        np.testing.assert_allclose(LT, LT_o, rtol=RTOL)
    eng.close()


def test_one_sample_equals_its_slot_of_a_batch_bitwise(monkeypatch):
    """K = 10 on the many-stretch fold, SK_U: sample 1 run alone (B = 1) and as slot 1 of B = 3."""
    K, R, B = 10, 2, 3
    samples = [start("sparse", K, R, s) for s in range(B)]
    big = engine("sparse", K, R, monkeypatch, B=B, family="sku")
    assert big.plan_info()["small_k"] == 2
    big.upload(np.stack([s[0] for s in samples]), np.stack([s[1] for s in samples]))
    big.iterate(5)
    th_b, pr_b = big.download()
    L_b = big.loglik(0)
    one = engine("sparse", K, R, monkeypatch, B=1, family="sku")
    one.upload(samples[1][0][None], samples[1][1][None])
    one.iterate(5)
    th1, pr1 = one.download()
    np.testing.assert_array_equal(th1[0], th_b[1])
    np.testing.assert_array_equal(pr1[0], pr_b[1])
    assert one.loglik(0)[0] == L_b[1]
    big.close()
    one.close()
