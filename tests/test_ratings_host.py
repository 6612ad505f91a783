"""R = 2..8 rating classes, unobserved ratings included, on the CPU: the test oracles
(oracle/mmsbm_oracle.c, oracle/shard_oracle.py) against the direct numpy.longdouble restatement of
the formulas (tests/ratings_ref.py), and the engine's host work plan (csrc/plan.h through
tests/plan_check.cpp) at R > 2 and with empty (stream, rating) sections.

Tolerance: rtol 1e-12 against the longdouble values rounded to float64 (the C oracle sums up to
E K^3 = 137,200 float64 terms here, in the reference's order; the worst error measured on these
cases was 4.1e-15), and exactly 0 wherever a rating has no observation.
"""
import numpy as np
import pytest

import ratings_ref as ref
from oracle import c_oracle
from test_plan import _check, plan_check  # noqa: F401  (plan_check: the compiled driver, a fixture)

RTOL = 1e-12
P, E = 40, 400

# (R, K, empty ratings)
CASES = [(3, 4, ()), (3, 4, (1,)), (5, 7, ()), (5, 7, (4,)), (8, 3, ()), (8, 3, (0,)), (2, 5, (1,))]
IDS = ["R%d-K%d-%s" % (R, K, "empty" + "".join(map(str, e)) if e else "full") for R, K, e in CASES]


def close(got, want, empty=(), axis=-1):
    """got (float64) against want (longdouble) at RTOL; the `empty` ratings' slices exactly 0."""
    got = np.asarray(got)
    np.testing.assert_allclose(got, ref.f64(want), rtol=RTOL, atol=0)
    for r in empty:
        assert not np.take(got, r, axis=axis).any()


def case(R, K, empty, seed=0):
    ids, counts = ref.links(P, E, R, seed=10 * R + K + seed, empty=empty)
    th, pr = ref.params(P, K, R, seed=R + K + seed)
    return ids, counts, th, pr


def test_generator_covers_what_it_promises():
    ids, counts = ref.links(P, E, 5, seed=3, empty=(1, 3))
    assert ids.dtype == np.int32 and counts.dtype == np.int32 and counts.shape == (E, 5)
    assert np.unique(ids).size == P and len({tuple(t) for t in ids.tolist()}) == E
    assert not counts[:, [1, 3]].any() and (counts[:, [0, 2, 4]].sum(axis=0) > 0).all()
    assert (counts.max(axis=1) > 1).any() and ((counts > 0).sum(axis=1) == 2).any()
    assert any(len(set(t)) < 3 for t in ids.tolist())               # a repeated gene
    assert all(list(t) == sorted(t, key=str) for t in ids.tolist())  # the keys' slot order
    th, pr = ref.params(P, 4, 5, seed=1)
    np.testing.assert_allclose(th.sum(axis=1), 1, rtol=1e-14)
    np.testing.assert_allclose(pr.sum(axis=-1), 1, rtol=1e-14)
    m = pr.mean(axis=(0, 1, 2))
    assert (m[:-1] > 1.2 * m[1:]).all()                             # every rating its own scale


@pytest.mark.parametrize("R,K,empty", CASES, ids=IDS)
def test_c_oracle_accumulate_matches_direct_formula(R, K, empty):
    ids, counts, th, pr = case(R, K, empty)
    nth, npr = c_oracle.accumulate(ids, counts, th, pr)
    want_nth, want_npr = ref.accumulate(ids, counts, th, pr)
    close(nth, want_nth)
    close(npr, want_npr, empty)


@pytest.mark.parametrize("R,K,empty", CASES, ids=IDS)
def test_c_oracle_iterations_loglik_and_predict_match_direct_formula(R, K, empty):
    """Two iterations, each from the oracle's own state (the second starts from a lattice whose
    empty slices are 0: d = eps there), then the likelihood and the rating-1 prediction."""
    ids, counts, th, pr = case(R, K, empty)
    tids, tcounts = ref.links(P, 60, R, seed=77 + R)           # a test set: every rating observed
    for _ in range(2):
        want_th, want_pr = ref.iteration(ids, counts, th, pr)
        th, pr = c_oracle.make_iteration(ids, counts, th, pr)
        close(th, want_th)
        close(pr, want_pr, empty)
    for a, b in ((ids, counts), (tids, tcounts)):
        L = c_oracle.loglik(a, b, th, pr)
        assert np.isfinite(L)
        close(L, ref.loglik(a, b, th, pr))
    close(c_oracle.predict(tids, th, pr), ref.predict(tids, th, pr))
    if 1 in empty:
        assert not c_oracle.predict(tids, th, pr).any()


@pytest.mark.parametrize("eps", [1e-3, 1e-30])
def test_c_oracle_uses_eps_like_the_direct_formula(eps):
    ids, counts, th, pr = case(3, 4, (2,))
    want_th, want_pr = ref.iteration(ids, counts, th, pr, eps)
    got_th, got_pr = c_oracle.make_iteration(ids, counts, th, pr, eps)
    close(got_th, want_th)
    close(got_pr, want_pr, (2,))
    close(c_oracle.loglik(ids, counts, got_th, got_pr, eps), ref.loglik(ids, counts, got_th, got_pr, eps))


@pytest.mark.parametrize("R,K,empty2,empty3", [(3, 4, (), ()), (3, 4, (0,), ()), (8, 3, (), ()),
                                               (8, 3, (), (7,))],
                         ids=["R3", "R3-pairs-empty0", "R8", "R8-triplets-empty7"])
def test_c_oracle_joint_model_matches_direct_formula(R, K, empty2, empty3):
    ids3, counts3 = ref.links(P - 4, 300, R, seed=R, empty=empty3)      # 4 pair-only genes
    ids2, counts2 = ref.pair_links(P, 200, R, seed=R + 1, empty=empty2)
    th, pr = ref.params(P, K, R, seed=R + 2)
    _, qr = ref.params(P, K, R, seed=R + 3, pairs=True)
    for _ in range(2):
        want = ref.joint_iteration(ids3, counts3, ids2, counts2, th, pr, qr)
        th, pr, qr = c_oracle.joint_make_iteration(ids3, counts3, ids2, counts2, th, pr, qr)
        close(th, want[0])
        close(pr, want[1], empty3)
        close(qr, want[2], empty2)
    L = c_oracle.joint_loglik(ids3, counts3, ids2, counts2, th, pr, qr)
    close(L, ref.loglik(ids3, counts3, th, pr) + ref.loglik(ids2, counts2, th, qr))
    close(c_oracle.pair_predict(ids2, th, qr), ref.predict(ids2, th, qr))
    close(c_oracle.predict(ids3, th, pr), ref.predict(ids3, th, pr))


@pytest.mark.parametrize("empty", [(), (2,)], ids=["full", "empty2"])
def test_shard_oracle_halves_match_direct_formula_at_three_ratings(empty):
    """shard_oracle.accumulate leaves theta / p unapplied (n theta = theta nth, n p_r = p_r S_r);
    two link blocks summed, then mstep, are the direct iteration."""
    from oracle import shard_oracle
    R, K = 3, 4
    ids, counts, th, pr = case(R, K, empty, seed=5)
    half = E // 2
    parts = [shard_oracle.accumulate(ids[lo:hi], counts[lo:hi], th, pr) for lo, hi in ((0, half), (half, E))]
    nth, S = parts[0][0] + parts[1][0], parts[0][1] + parts[1][1]
    assert S.shape == (R, K ** 3)
    want_nth, want_npr = ref.accumulate(ids, counts, th, pr)
    close(th * nth, want_nth)
    close(pr * S.T.reshape(K, K, K, R), want_npr, empty)
    for r in empty:
        assert not S[r].any()
    got_th, got_pr = shard_oracle.mstep(th, pr, nth, S, ref.degree(P, ids))
    want_th, want_pr = ref.iteration(ids, counts, th, pr)
    close(got_th, want_th)
    close(got_pr, want_pr, empty)


# ------------------------------------------------------------------------------ the work plan
# (P, E, units, gcap, sp_rows, env): one plan of each kind tests/test_plan.py parametrises
PLANS = {
    "large": (40, 600, (1, 1), 33, 16, {}),
    "gene-capped": (200, 3000, (3, 5), 4, 16, {}),
    "merged": (300, 5000, (64, 64), 13, 120, {"PLAN_MERGE": "1"}),
    "fill8": (300, 5000, (1, 1), -1, 1024, {}),
    "fill4": (300, 5000, (1, 1), -2, 1024, {}),
    "sky": (300, 5000, (64, 64), -4, 1024, {}),
    "nw4": (300, 5000, (64, 64), 4, 128, {"PLAN_NW": "4", "PLAN_MERGE": "1"}),
}
# (R, empty ratings): first, middle and last rating empty; two of five; seven of eight; R = 2
# with no positive observation
RATINGS = [(3, ()), (3, (0,)), (3, (1,)), (3, (2,)), (5, ()), (5, (1, 3)), (8, ()),
           (8, (0, 1, 2, 3, 4, 5, 6)), (8, (1, 2, 3, 4, 5, 6, 7)), (2, (1,))]


@pytest.mark.parametrize("kind", list(PLANS))
@pytest.mark.parametrize("R,empty", RATINGS, ids=["R%d-empty%s" % (R, "".join(map(str, e)) or "-none")
                                                  for R, e in RATINGS])
def test_plan_invariants_with_more_ratings_and_empty_sections(plan_check, kind, R, empty):  # noqa: F811
    Pp, Ee, units, gcap, sp_rows, env = PLANS[kind]
    ids, counts = ref.links(Pp, Ee, R, seed=Pp + R, empty=empty, both=0.1)
    rows = np.concatenate([ids, counts], axis=1).astype(np.int64)
    out = _check(plan_check, Pp, Ee, units, gcap, sp_rows, 0.0, env=env, R=R, links=rows)
    if kind == "nw4":
        assert int(out[2]) == 4 * int(out[3])


def test_plan_links_helper_is_unchanged_at_two_ratings_and_valid_above():
    from test_plan import _links
    a = _links(50, 400, seed=3, both=0.5)
    assert a.shape == (400, 5) and ((a[:, 3:] > 0).sum(axis=1) == 2).any()
    b = _links(50, 400, seed=3, R=5, both=0.5)
    assert b.shape == (400, 8) and (b[:, 3:] >= 0).all() and ((b[:, 3:] > 0).sum(axis=1) == 2).any()


# ------------------------------------------------------------------ the newest scan families' references
def newest_params():
    from test_gpu_ratings import SCAN_PARAMS
    return SCAN_PARAMS


@pytest.mark.parametrize("R,K,B", newest_params(), ids=["R%d-K%d-B%d" % c for c in newest_params()])
def test_the_newest_families_references_tell_the_rating_slices_apart(R, K, B):
    """The preconditions of tests/test_gpu_ratings.py (f3), on the reference alone: newest_case asserts,
    for the dispute scan, the pair vote census, the partner statistics and every masked entry, that
    ratings 0 and 2 in rating 1's place give another answer, that the lists' gaps determine their
    order and that the thresholds are clear of every score.  Here also: nothing is empty."""
    from test_gpu_ratings import NEWEST_N, newest_case, newest_samples
    c = newest_case(R, K, B)
    assert 0 < c["blocked"].size and c["mask"].any()
    for i in range(len(c["queries"])):
        assert c["merged"][0][i + 1] > c["merged"][0][i]         # every query loses candidates to the mask
    assert len(c["partners_stat"]) == 5 * 2 * len(c["stat_calls"]) and len(c["stat_calls"]) == (3 if B == 2 else 1)
    for want_s, want_ids, bound in c["partners_stat"].values():
        assert want_s.shape == (NEWEST_N,) and want_ids.shape == (NEWEST_N, 3)
    families = 0
    for sample in newest_samples(B):
        for tab in ("all", "masked"):
            e = c[sample, tab]
            assert ("spread" in e) == (B == 2 and sample is None)
            assert e["pair_votes"][2].any() and len(e["pair_votes"][1]) == e["ns"]
            if tab == "masked":
                assert {"scan_top", "census", "scan_above", "votes", "quorum", "partners"} <= set(e)
                assert e["census"][1].max() > 0 and e["votes"][1][1:].sum() > 0
            families += len(e) - 1
    print("R %d K %d B %d: %d references, every one differs from ratings 0 and 2" % (R, K, B, families + len(c["partners_stat"])))
