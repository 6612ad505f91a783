"""Every kernel family on CONVERGED fits (tests/golden/converged/, tests/converged_ref.py), the
regime the engine is used in: half of p exactly 0, entries of p in the subnormal range, theta over
30 to 230 decades, a train likelihood that is a sum of logs of values next to 1, and top scores
that saturate at 1 - O(eps), so that hundreds of adjacent gaps of a top-4096 list lie below 1e-9.

The checkpoints are uploaded, never iterated to.  EM, likelihood and prediction: against the C
oracle at the suite's rtol 1e-9, atol 1e-300, which tests/test_converged_host.py justifies on the
reference alone.  Scan families: lists by SET at a clear cut (converged_ref.check_set_cut: the
order inside is not determined by the reference there, the list's own order is checked on its own
bits), counts exactly at thresholds clear of every reference score.
"""

import numpy as np
import pytest

import census_ref
import converged_ref as cr
import masked_ref
import pair_census_ref
import partners_ref
import quorum_ref
import scan_ref
import votes_ref
from scan_ref import bits
from test_gpu_ratings import ATOL, ENV, RTOL, engine, joint_engine

pytestmark = pytest.mark.gpu

WORST = {}      # label -> largest relative error against the oracle seen in this run
SCAN_ENV = ("MMSBM_SCAN_QUORUM_GRID", "MMSBM_SCAN_QUORUM_EARLY")


@pytest.fixture(autouse=True)
def plain_env(monkeypatch):
    for k in ENV + SCAN_ENV:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module", autouse=True)
def worst_errors():
    yield
    for label in sorted(WORST):
        print("max relative error vs oracle  %-16s %.3e" % (label, WORST[label]))


def close(label, got, want):
    WORST[label] = max(WORST.get(label, 0.0), cr.deviation(got, want))
    assert np.isfinite(got).all()
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)


def same(x, y):
    if isinstance(x, (tuple, list)):
        assert len(x) == len(y)
        for u, v in zip(x, y):
            same(u, v)
    else:
        assert x.dtype == y.dtype and x.shape == y.shape and bits(x) == bits(y)


def em_engine(cks, family=None, test=True):
    c = cks[0]
    return engine(c.K, c.P, c.R, c.ids, c.counts, [k.theta for k in cks], [k.pr for k in cks], B=len(cks),
                  family=family, test=c.test() if test else None)


def predict_ids(c):
    rng = np.random.default_rng(c.K + c.P)
    return np.concatenate([c.test_ids, rng.integers(0, c.P, (200, 3)).astype(np.int32)])


# ------------------------------------------------------------- (a) EM, likelihood, prediction
def run_em(label, names, family=None, small_k=None):
    """iterate(1), then iterate(2), from the uploaded checkpoints: theta and p after step 1 and
    after step 3, both likelihoods and the predictions against the oracle; exact zeros of p stay
    exact zeros."""
    from oracle import c_oracle
    cks = [cr.load(n) for n in names]
    c = cks[0]
    eng = em_engine(cks, family)
    if small_k is not None:
        assert eng.plan_info()["small_k"] == small_k, (eng.plan_info()["small_k"], small_k)
    eng.iterate(1)
    th1, pr1 = eng.download()
    eng.iterate(2)
    th3, pr3 = eng.download()
    L, LT = eng.loglik(0), eng.loglik(1)
    pids = predict_ids(c)
    pred = eng.predict(pids)
    for s, k in enumerate(cks):
        want = cr.steps(k, 3)
        for got, (th_o, pr_o) in (((th1[s], pr1[s]), want[0]), ((th3[s], pr3[s]), want[2])):
            close(label, got[0], th_o)
            close(label, got[1], pr_o)
            np.testing.assert_array_equal(got[1][k.pr == 0], 0.0)
        th_o, pr_o = want[2]
        close(label + " L", L[s], c_oracle.loglik(c.ids, c.counts, th_o, pr_o))
        close(label + " L", LT[s], c_oracle.loglik(c.test_ids, c.test_counts, th_o, pr_o))
        close(label + " predict", pred[s], c_oracle.predict(pids, th_o, pr_o))
    eng.close()


AB = cr.EM_A + cr.EM_B
A_BY_T = {t: ["A_s%d_T%d" % (s, t) for s in cr.A_SEEDS] for t in cr.A_ITERS}
# (label, environment, family, plan_info "small_k", checkpoints of one engine)
EM_CASES = [("sku", {}, None, 2, [n]) for n in AB] + \
           [("sky", {}, "sky", 3, [n]) for n in AB] + \
           [("sky-B2", {}, None, 3, A_BY_T[t][:2]) for t in cr.A_ITERS] + \
           [("sky-B3", {}, None, 3, A_BY_T[t]) for t in cr.A_ITERS] + \
           [("pass-a+b", {"MMSBM_SK_FUSED": "0"}, None, 1, [n]) for n in AB] + \
           [("large-forced", {"MMSBM_SK": "0"}, None, 0, [n]) for n in AB] + \
           [("units-1,1", {"MMSBM_UNITS": "1,1"}, None, None, [n]) for n in AB] + \
           [("large", {}, None, 0, [n]) for n in cr.EM_C] + \
           [("ratings-sku", {}, None, 2, [cr.RATINGS]), ("ratings-sky", {}, "sky", 3, [cr.RATINGS])]


@pytest.mark.parametrize("label,env,family,small_k,names", EM_CASES,
                         ids=["%s-%s" % (c[0], "+".join(c[4])) for c in EM_CASES])
def test_em_from_a_converged_checkpoint_matches_oracle(monkeypatch, label, env, family, small_k, names):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    run_em(label, names, family, small_k)


@pytest.mark.parametrize("T", cr.A_ITERS)
def test_batch_and_iteration_count_keep_bits(T):
    """The three seeds as one batch = each seed alone; iterate(3) = three iterate(1) calls."""
    cks = [cr.load(n) for n in A_BY_T[T]]
    batch = em_engine(cks, "sky")
    batch.iterate(3)
    thB, prB = batch.download()
    LB = batch.loglik(0)
    batch.close()
    for s, k in enumerate(cks):
        one = em_engine([k], "sky")
        for _ in range(3):
            one.iterate(1)
        th, pr = one.download()
        np.testing.assert_array_equal(th[0], thB[s])
        np.testing.assert_array_equal(pr[0], prB[s])
        assert one.loglik(0)[0] == LB[s]
        one.close()


@pytest.mark.parametrize("name", ["A_s1_T80", "A_s1_T1000", "B_s1_T2000", "C20_s1_T300"])
def test_accumulate_then_mstep_is_one_iteration(name):
    import torch
    k = cr.load(name)
    one = em_engine([k], test=False)
    one.iterate(1)
    want = one.download()
    one.close()
    eng = em_engine([k], test=False)
    n = torch.zeros((1, k.P, k.K), dtype=torch.float64, device=eng.device)
    s = torch.zeros((1, k.R, k.K ** 3), dtype=torch.float64, device=eng.device)
    eng.accumulate(n, s)
    eng.mstep(n, s)
    got = eng.download()
    eng.close()
    th_o, pr_o = cr.steps(k, 1)[0]
    for g, w, o in zip(got, want, (th_o, pr_o)):
        np.testing.assert_allclose(g, w, rtol=RTOL, atol=ATOL)
        close("accumulate+mstep", g[0], o)
    np.testing.assert_array_equal(got[1][0][k.pr == 0], 0.0)


@pytest.mark.parametrize("mode", ["iterate", "iterate_unfused"])
def test_joint_engine_from_a_converged_checkpoint(mode):
    from oracle import c_oracle
    k = cr.load(cr.JOINT)
    eng = joint_engine(k.K, k.P, k.R, k.train(), k.theta, k.pr, k.qr)
    getattr(eng, mode)(1)
    first = eng.download()
    getattr(eng, mode)(2)
    third = eng.download()
    want = cr.steps(k, 3)
    label = "joint-" + mode
    for got, w in ((first, want[0]), (third, want[2])):
        for g, o, start in zip(got, w, k.state()):
            close(label, g[0], o)
            if start.ndim > 2:
                np.testing.assert_array_equal(g[0][start == 0], 0.0)
    close(label + " L", eng.loglik(0)[0], c_oracle.joint_loglik(*k.train(), *want[2]))
    rng = np.random.default_rng(k.K)
    pids3 = np.concatenate([k.test_ids, rng.integers(0, k.P, (200, 3)).astype(np.int32)])
    pids2 = np.concatenate([k.test_ids2, rng.integers(0, k.P, (200, 2)).astype(np.int32)])
    close(label + " predict", eng.predict(pids3)[0], c_oracle.predict(pids3, want[2][0], want[2][1]))
    close(label + " predict", eng.predict(pids2)[0], c_oracle.pair_predict(pids2, want[2][0], want[2][2]))
    eng.close()


def test_drift_over_a_whole_run():
    """300 iterations of fit A, seed 1, from its seeded start on the default family: the deviation
    from the C oracle is at most ten times the deviation between the oracle and
    pivot_model.iterate on the CPU (two reference-grade orders of the same sums; the GPU's is a
    third, and the amplification depends on the trajectory)."""
    d = cr.drift()
    ck = cr.load("A_s1_T300")
    eng = engine(ck.K, ck.P, 2, d.ids, d.counts, *d.start)
    eng.iterate(cr.DRIFT_ITERS)
    th, pr = eng.download()
    L = eng.loglik(0)[0]
    eng.close()
    got = (cr.deviation(th[0], d.oracle[0]), cr.deviation(pr[0], d.oracle[1]), abs(L - d.L) / abs(d.L))
    print("drift over %d iterations: GPU vs oracle theta %.3e p %.3e L %.3e; pivot model vs oracle "
          "theta %.3e p %.3e L %.3e" % ((cr.DRIFT_ITERS,) + got + (d.theta, d.pr, d.dL)))
    assert np.isfinite(th).all() and np.isfinite(pr).all() and np.isfinite(L)
    assert max(d.theta, d.pr, d.dL) <= 1e-6
    assert got[0] <= 10 * d.theta and got[1] <= 10 * d.pr and got[2] <= 10 * d.dL, (got, d[5:])


# ------------------------------------------------------------------------ (b) the scan families
def scan_engine(s, slots=None):
    from scan_gpu import engine as scan_engine_of
    if slots is None:
        return scan_engine_of(s.theta, s.pr)
    return scan_engine_of(s.theta[slots], s.pr[slots])


def samples_of(s):
    """Every slot, then the ensemble (None)."""
    return list(range(s.per.shape[0])) + [None]


def ref_of(s, sample):
    return s.mean if sample is None else s.per[sample]


SCAN_PARAMS = [(label, known) for label in cr.SCAN_SETS for known in cr.KNOWN]
scan_cases = pytest.mark.parametrize("label,known", SCAN_PARAMS, ids=["%s-%s" % c for c in SCAN_PARAMS])


def thresholds_for(scores):
    """census_ref.gap_thresholds(scores, 3) and those of 0.5, 0.9, 1 - 1e-6 clear of every score."""
    fixed = np.array([0.5, 0.9, 1 - 1e-6])
    t = np.concatenate([census_ref.gap_thresholds(scores, 3), fixed[census_ref.clear_of_scores(scores, fixed)]])
    census_ref.assert_clear(scores, t)
    return t


@scan_cases
def test_scan_top_above_and_census_at_clear_cuts(label, known):
    s = cr.scan_set(label)
    kn = s.known[known]
    eng = scan_engine(s)
    for sample in samples_of(s):
        ref = ref_of(s, sample)
        desc = cr.eligible_desc(ref, s.keys, kn)
        for n in cr.pick_cuts(desc):
            got = eng.scan_top(n, kn, sample=sample)
            cr.check_set_cut(got[0], got[1], ref, s.keys, n, kn, s.P)
            t = cr.mid_threshold(desc, n)
            same(eng.scan_above(t, kn, sample=sample), got)
            counts, total = eng.census([t], kn, sample=sample)
            assert counts.tolist() == [n] and total == desc.size
    if s.per.shape[0] > 1:          # a slot of the batch = an engine holding that sample alone
        n = cr.pick_cuts(cr.eligible_desc(s.per[1], s.keys, kn))[0]
        solo = scan_engine(s, slice(1, 2))
        same(eng.scan_top(n, kn, sample=1), solo.scan_top(n, kn, sample=0))
        solo.close()
    eng.close()


@scan_cases
def test_census_and_pair_census_counts(label, known):
    s = cr.scan_set(label)
    kn = s.known[known]
    eng = scan_engine(s)
    for sample in samples_of(s):
        ref = ref_of(s, sample)
        t = thresholds_for(ref)
        want, want_total = census_ref.ref_census(ref, s.keys, t, kn)
        assert 0 < want.max() and want.min() < want_total        # on the reference: hits and misses
        got, total = eng.census(t, kn, sample=sample)
        np.testing.assert_array_equal(got, want)
        assert total == want_total
        mat = eng.pair_census(t, kn, sample=sample)
        np.testing.assert_array_equal(mat, pair_census_ref.ref_pairs(ref, s.keys, s.P, t, kn)[1])
        np.testing.assert_array_equal(np.triu(mat.transpose(2, 0, 1), 1).sum(axis=(1, 2)), 3 * want)
    eng.close()


def vote_thresholds(per):
    flat = per.reshape(-1)
    return thresholds_for(flat)          # asserted clear of every slot's scores


def check_votes(eng, s, t, kn, mask=None, kn_ref=None):
    kw = {} if mask is None else {"mask": mask}
    ns = s.per.shape[0]
    kn_ref = kn if kn_ref is None else kn_ref
    votes_r, keys_r, mean_r, hist_r = votes_ref.ref_votes(s.per, s.keys, t, known=kn_ref)
    np.testing.assert_array_equal(eng.vote_census(t, kn, **kw), hist_r)
    for m in range(1, ns + 1):
        v, sc, ids = eng.consensus(t, m, kn, **kw)
        got = scan_ref.packed(ids, s.P)
        np.testing.assert_array_equal(np.sort(got), keys_r[votes_r >= m])      # keys_r ascends
        np.testing.assert_array_equal(ids, scan_ref.keys_to_ids(got, s.P))
        at = np.searchsorted(keys_r, got)
        np.testing.assert_array_equal(v, votes_r[at])
        np.testing.assert_allclose(sc, mean_r[at], rtol=scan_ref.RTOL, atol=0)
        dv, ds, dk = np.diff(v), np.diff(sc), np.diff(got)
        assert (dv <= 0).all() and (ds[dv == 0] <= 0).all() and (dk[(dv == 0) & (ds == 0)] > 0).all()
    return hist_r


@scan_cases
def test_vote_census_and_consensus(label, known):
    s = cr.scan_set(label)
    kn = s.known[known]
    eng = scan_engine(s)
    used = 0
    for t in vote_thresholds(s.per):
        hist = check_votes(eng, s, float(t), kn)
        used += int(hist[1:].sum() > 0 and hist[0] > 0)
    assert used >= 2
    eng.close()


def quorum_cut(s, m, kn):
    q = quorum_ref.quorum(s.per, m)
    return q, cr.pick_cuts(cr.eligible_desc(q, s.keys, kn))


@scan_cases
def test_quorum_top_at_clear_cuts(monkeypatch, label, known):
    s = cr.scan_set(label)
    kn = s.known[known]
    eng = scan_engine(s)
    for m in range(1, s.per.shape[0] + 1):
        q, cuts = quorum_cut(s, m, kn)
        for n in cuts:
            got = eng.quorum_top(n, m, kn)
            cr.check_set_cut(got[0], got[1], q, s.keys, n, kn, s.P)
            monkeypatch.setenv("MMSBM_SCAN_QUORUM_EARLY", "0")
            same(eng.quorum_top(n, m, kn), got)
            monkeypatch.delenv("MMSBM_SCAN_QUORUM_EARLY")
            monkeypatch.setenv("MMSBM_SCAN_QUORUM_GRID", "7")
            same(eng.quorum_top(n, m, kn), got)
            monkeypatch.delenv("MMSBM_SCAN_QUORUM_GRID")
    eng.close()


@scan_cases
def test_one_mask_on_every_masked_family(label, known):
    """A masked call = the unmasked call with the blocked triples' keys added to `known`: by set
    for the lists, exactly for the counts; and both against the reference."""
    s = cr.scan_set(label)
    kn = s.known[known]
    mask, blocked = cr.random_pair_mask(s.P)
    both = np.union1d(np.zeros(0, np.int64) if kn is None else kn, blocked).astype(np.int64)
    eng = scan_engine(s)
    ns = s.per.shape[0]
    t = thresholds_for(s.mean)
    want, want_total = census_ref.ref_census(s.mean, s.keys, t, both)
    got, total = eng.census(t, kn, mask=mask)
    np.testing.assert_array_equal(got, want)
    assert total == want_total
    same(eng.census(t, both)[0], got)
    mat = eng.pair_census(t, kn, mask=mask)
    same(mat, eng.pair_census(t, both))
    np.testing.assert_array_equal(mat, pair_census_ref.ref_pairs(s.mean, s.keys, s.P, t, both)[1])
    # the threshold scan at a clear cut of the masked list
    desc = cr.eligible_desc(s.mean, s.keys, both)
    for n in cr.pick_cuts(desc):
        got = eng.scan_above(cr.mid_threshold(desc, n), kn, mask=mask)
        cr.check_set_cut(got[0], got[1], s.mean, s.keys, n, both, s.P)
        same(eng.scan_above(cr.mid_threshold(desc, n), both), got)
    # the vote scan
    for tv in vote_thresholds(s.per)[:3]:
        check_votes(eng, s, float(tv), kn, mask=mask, kn_ref=both)
    # the quorum scan
    for m in range(1, ns + 1):
        q, cuts = quorum_cut(s, m, both)
        for n in cuts:
            got = eng.quorum_top(n, m, kn, mask=mask)
            cr.check_set_cut(got[0], got[1], q, s.keys, n, both, s.P)
            same(eng.quorum_top(n, m, both), got)
    eng.close()


# ----------------------------------------------------------------------------- (c) partners
def partner_cuts(scores):
    """(the smallest clear cut >= 8, the largest <= 256) of one query's descending list."""
    cuts = cr.clear_cuts(scores, 8, 256)
    assert cuts.size, "no clear cut in [8, 256]"
    return int(cuts[0]), int(cuts[-1])


@pytest.mark.parametrize("exclude", [False, True], ids=["all", "novel"])
def test_partners_top_of_every_query_at_clear_cuts(exclude):
    from trigenicinteractionpredictor_amd.scan import partner_known
    k = cr.load("A_s1_T300")
    P = k.P
    _, rank = scan_ref.rank_tables(P)
    from scan_gpu import engine as scan_engine_of
    eng = scan_engine_of(k.theta[None], k.pr[None])
    queries = np.arange(P)
    off, pairs = partner_known((P, k.ids, k.test_ids), queries) if exclude else (np.zeros(P + 1, np.int64), None)
    refs, by_n = {}, {}
    for g in queries:
        sc, tk, pk = partners_ref.ref_query(k.theta, k.pr, int(rank[g]))
        if exclude:
            keep = ~np.isin(pk, pairs[off[g]:off[g + 1]])
            sc, tk = sc[keep], tk[keep]
        at = np.argsort(tk)
        refs[g] = (sc[at], tk[at])
        for n in partner_cuts(np.sort(sc)[::-1]):
            by_n.setdefault(n, []).append(int(g))
    assert len(by_n) > 1
    tight = 0
    for n, genes in sorted(by_n.items()):
        genes = sorted(set(genes))
        known = partner_known((P, k.ids, k.test_ids), genes) if exclude else None
        rows = eng.partners_top(genes, n, known)
        for g, (got_s, got_ids) in zip(genes, rows):
            got_k = cr.check_set_cut(got_s, got_ids, refs[g][0], refs[g][1], n, None, P)
            assert (np.sort(rank[got_ids], axis=1) == rank[g]).any(axis=1).all()   # every row holds the query
            tight += cr.tight_gaps(np.sort(refs[g][0])[::-1], n)
            del got_k
    assert tight > 0        # on the reference: some list holds a gap the order rule could not take
    eng.close()
