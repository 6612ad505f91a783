"""The converged checkpoints (tests/golden/converged/, tests/golden/make_converged_golden.py) and
the rule tests/test_gpu_converged.py holds the scan families to, on the CPU: that every file is in
the regime it stands for, that it is what the generator writes, that the GPU tests' tolerance is
justified on the reference alone, that the checker rejects what it should and that every list the
GPU tests ask for has a clear cut and the close scores it is there for."""
import os

import numpy as np
import pytest

import census_ref
import converged_ref as cr
import partners_converged_ref as pc
import partners_ref
import partners_stat_ref
import pivot_model
import quorum_ref
import scan_ref
from oracle import c_oracle

# file -> lower bounds of (share of exact zeros in p, subnormal entries of p, -log10 of the
# smallest theta, adjacent gaps <= 1e-9 inside the reference top 4096).  A state after 25
# iterations has (0, 0, < 4, 0).
REGIME = {
    "A_s1_T80": (0.02, 3, 6, 0), "A_s1_T300": (0.45, 0, 20, 200), "A_s1_T1000": (0.5, 0, 70, 1000),
    "A_s2_T80": (0.02, 3, 6, 0), "A_s2_T300": (0.45, 1, 20, 30), "A_s2_T1000": (0.5, 0, 70, 1000),
    "A_s3_T80": (0.02, 3, 6, 0), "A_s3_T300": (0.45, 0, 20, 1000), "A_s3_T1000": (0.5, 0, 90, 2000),
    "B_s1_T300": (0.3, 2, 30, 5), "B_s1_T2000": (0.45, 2, 230, 3000),
    "C13_s1_T300": (0.45, 1, 45, 200), "C20_s1_T300": (0.45, 8, 35, 10),
    "D_s1_T300": (0.05, 1, 150, 500), "E_s1_T300": (0.45, 0, 70, 1000),
}
LARGEST_OTHER_FIXTURE = 158347


def test_the_files_are_the_expected_ones_and_small():
    assert cr.files() == sorted(cr.ALL) == sorted(REGIME)
    sizes = [os.path.getsize(os.path.join(cr.DIR, n + ".npz")) for n in cr.ALL]
    assert max(sizes) < LARGEST_OTHER_FIXTURE and sum(sizes) < 600_000, sizes


@pytest.mark.parametrize("name", cr.ALL)
def test_regime(name):
    k = cr.load(name)
    zeros, sub, decades, tight = REGIME[name]
    assert k.T >= 80 and k.theta.shape == (k.P, k.K) and k.pr.shape == (k.K,) * 3 + (k.R,)
    for a in k.state() + k.state(prev=True):
        assert np.isfinite(a).all() and (a >= 0).all()
    assert (k.pr == 0).mean() >= zeros
    assert cr.subnormals(k.pr) >= sub
    assert 0 < k.theta.min() <= 10.0 ** -decades
    desc = np.sort(scan_ref.ref_scores(k.theta, k.pr)[0])[::-1]
    assert cr.tight_gaps(desc, 4096) >= tight
    if name.startswith("A_") and k.T == 80:
        gen = cr.generator()
        assert gen.SUBNORMAL_T[k.seed] == 80 and cr.subnormals(k.pr) >= gen.SUBNORMAL_MIN


def test_a_25_iteration_state_is_not_in_the_regime():
    """The bounds above tell a converged state from what the other fixtures hold."""
    _, state, step = cr.generator().setup("A_s1")
    for _ in range(25):
        state = step(state)
    desc = np.sort(scan_ref.ref_scores(*state)[0])[::-1]
    got = ((state[1] == 0).mean(), cr.subnormals(state[1]), -np.log10(state[0].min()), cr.tight_gaps(desc, 4096))
    for name in cr.ALL:
        assert any(g < bound for g, bound in zip(got, REGIME[name])), name


@pytest.mark.parametrize("name", cr.EM_A + cr.EM_C)
def test_reference_scores_are_far_above_the_smallest_normal(name):
    """Why the scan lists are compared at atol 0."""
    k = cr.load(name)
    assert scan_ref.ref_scores(k.theta, k.pr)[0].min() > 1e-280


# ------------------------------------------------------------------------------ provenance
@pytest.mark.parametrize("fit,upto", [("B_s1", None), ("A_s1", 300)])
def test_the_generator_reproduces_the_files(fit, upto):
    seen = 0
    for T, out in cr.generator().checkpoints(fit, upto):
        k = cr.load("%s_T%d" % (fit, T))
        assert sorted(out) == sorted(key for key in k if key != "name")
        for key, want in out.items():
            got = k[key]
            if np.ndim(want) == 0:
                assert got == want.item(), key
            else:
                assert got.dtype == want.dtype and got.shape == want.shape and got.tobytes() == want.tobytes(), key
        seen += 1
    assert seen == 2


@pytest.mark.parametrize("name", cr.ALL)
def test_one_oracle_step_maps_the_stored_states(name):
    k = cr.load(name)
    for got, want in zip(cr.step(k, k.state(prev=True)), k.state()):
        assert got.tobytes() == want.tobytes()


# ------------------------------------------------------------------------------ conditioning
def near(got, want, rtol):
    np.testing.assert_allclose(got, want, rtol=rtol, atol=1e-300)


@pytest.mark.parametrize("name", cr.ALL)
def test_conditioning_gates(name):
    """Other orders of the same sums agree with the oracle step a thousand times closer than the
    GPU tests' rtol of 1e-9: the comparison there is well conditioned."""
    k = cr.load(name)
    for prev in (True, False):
        start = k.state(prev)
        want = cr.step(k, start)
        for got, w in zip(cr.step(k, start, reverse=True), want):
            near(got, w, 1e-12)
        if name == cr.JOINT:        # no pivot model of the joint fit: the reversed order is the gate
            tabs = [np.ascontiguousarray(t[::-1]) for t in k.train()]
            np.testing.assert_allclose(c_oracle.joint_loglik(*tabs, *want), c_oracle.joint_loglik(*k.train(), *want),
                                       rtol=1e-10)
            continue
        for model in (pivot_model.iterate, pivot_model.iterate_y):
            for got, w in zip(model(k.ids, k.counts, *start), want):
                near(got, w, 1e-12)
        for ids, counts in (k.train(), k.test()):
            np.testing.assert_allclose(pivot_model.loglik(ids, counts, *want), c_oracle.loglik(ids, counts, *want),
                                       rtol=1e-10)


def test_drift_of_two_reference_orders_over_a_whole_run():
    """What tests/test_gpu_converged.py multiplies by ten: below the north-star tolerance of 1e-6,
    so theta, p and L are all asserted there; and the oracle run ends in the stored checkpoint."""
    d = cr.drift()
    print("oracle vs pivot model over %d iterations: theta %.3e p %.3e L %.3e" % (cr.DRIFT_ITERS, d.theta, d.pr, d.dL))
    assert 0 < max(d.theta, d.pr, d.dL) <= 1e-6
    k = cr.load("A_s1_T300")
    assert d.oracle[0].tobytes() == k.theta.tobytes() and d.oracle[1].tobytes() == k.pr.tobytes()


# ------------------------------------------------------------------------------ the checker
def a_list(n=300):
    s = cr.scan_set("A300")
    ref = s.per[0]
    n = int(cr.clear_cuts(cr.eligible_desc(ref, s.keys), n, 4096)[0])
    top_s, top_k = scan_ref.top(ref, s.keys, n + 1)
    return s, ref, n, top_s, top_k


def good(top_s, top_k, n, P):
    return top_s[:n].copy(), scan_ref.keys_to_ids(top_k[:n], P)


def test_check_set_cut_accepts_the_reference_and_any_order_inside_close_scores():
    s, ref, n, top_s, top_k = a_list()
    sc, ids = good(top_s, top_k, n, s.P)
    cr.check_set_cut(sc, ids, ref, s.keys, n, None, s.P)
    # scores moved by less than RTOL and sorted again: another order inside the close ones
    assert cr.tight_gaps(top_s, n) > 0
    moved = top_s[:n] * (1 + 4e-10 * np.random.default_rng(0).uniform(-1, 1, n))
    at = np.lexsort((top_k[:n], -moved))
    assert not np.array_equal(at, np.arange(n))
    cr.check_set_cut(moved[at], scan_ref.keys_to_ids(top_k[:n][at], s.P), ref, s.keys, n, None, s.P)


def test_check_set_cut_rejects_planted_errors():
    s, ref, n, top_s, top_k = a_list()
    # not a clear cut: on the reference alone
    desc = cr.eligible_desc(ref, s.keys)
    unclear = next(m for m in range(n, 4096) if not cr.clear_cuts(desc, m, m).size)
    us, uk = scan_ref.top(ref, s.keys, unclear)
    with pytest.raises(AssertionError, match="not a clear cut"):
        cr.check_set_cut(us[:unclear].copy(), scan_ref.keys_to_ids(uk[:unclear], s.P), ref, s.keys, unclear, None, s.P)
    # one key swapped for the (n + 1)-th
    sc, keys = top_s[:n].copy(), top_k[:n].copy()
    sc[-1], keys[-1] = top_s[n], top_k[n]
    with pytest.raises(AssertionError, match="missing"):
        cr.check_set_cut(sc, scan_ref.keys_to_ids(keys, s.P), ref, s.keys, n, None, s.P)
    # one score off by 1e-8, the order kept
    sc, ids = good(top_s, top_k, n, s.P)
    sc[0] *= 1 + 1e-8
    with pytest.raises(AssertionError, match="Not equal to tolerance"):
        cr.check_set_cut(sc, ids, ref, s.keys, n, None, s.P)
    # two bit-equal scores in descending key order
    sc, keys = top_s[:n].copy(), top_k[:n].copy()
    i = int(np.argmin((top_s[:n - 1] - top_s[1:n]) / top_s[:n - 1]))
    assert (sc[i] - sc[i + 1]) <= 1e-9 * sc[i]
    sc[i + 1] = sc[i]
    if keys[i] < keys[i + 1]:
        keys[[i, i + 1]] = keys[[i + 1, i]]
    with pytest.raises(AssertionError, match="not in the scan's order"):
        cr.check_set_cut(sc, scan_ref.keys_to_ids(keys, s.P), ref, s.keys, n, None, s.P)
    # a repeated key, and a known key
    sc, keys = top_s[:n].copy(), top_k[:n].copy()
    keys[1], sc[1] = keys[0], sc[0]
    with pytest.raises(AssertionError, match="repeated keys"):
        cr.check_set_cut(sc, scan_ref.keys_to_ids(keys, s.P), ref, s.keys, n, None, s.P)
    sc, ids = good(top_s, top_k, n, s.P)
    with pytest.raises(AssertionError):
        cr.check_set_cut(sc, ids, ref, s.keys, n, top_k[3:4], s.P)


def test_clear_cuts_on_a_small_list():
    s = np.array([1.0, 1.0 - 1e-12, 0.9, 0.9, 0.5, 0.5 * (1 - 5e-8)])
    assert cr.clear_cuts(s, 1, 10).tolist() == [2, 4]
    assert cr.clear_cuts(s, 3, 3).size == 0 and cr.clear_cuts(s[:1], 1, 4).size == 0
    assert 0.5 < cr.mid_threshold(s, 4) == (0.9 + 0.5) / 2 < 0.9


# ------------------------------------------------------------------------------ cut supply
@pytest.mark.parametrize("label", list(cr.SCAN_SETS))
def test_every_scan_list_has_its_cuts_and_its_close_scores(label):
    """Per known table: every slot, the ensemble and every q_m have a clear cut in (512, 4096] and
    one in [64, 512] (converged_ref.pick_cuts asserts it), and the lists of the family hold
    adjacent reference gaps at or below 1e-9: the regime the test is written for."""
    s = cr.scan_set(label)
    ns = s.per.shape[0]
    refs = {"slot %d" % b: s.per[b] for b in range(ns)}
    refs["ensemble"] = s.mean
    refs.update({"q_%d" % m: quorum_ref.quorum(s.per, m) for m in range(1, ns + 1)})
    blocked = cr.random_pair_mask(s.P)[1]
    for known in cr.KNOWN:
        kn = s.known[known]
        both = np.union1d(np.zeros(0, np.int64) if kn is None else kn, blocked)
        for tab in (kn, both):
            for name, ref in refs.items():
                desc = cr.eligible_desc(ref, s.keys, tab)
                big, small = cr.pick_cuts(desc)
                assert 512 < big <= 4096 and 64 <= small <= 512
                assert cr.tight_gaps(desc, big) > 0, (known, name)
                assert cr.tight_gaps(desc, small) > 0, (known, name)
    # thresholds: the census's own set is whole, and the fixed ones admitted are clear
    for ref in list(refs.values())[:ns + 1] + [s.per.reshape(-1)]:
        t = census_ref.gap_thresholds(ref, 3)
        assert t.size >= 6
        census_ref.assert_clear(ref, t)


def test_half_is_a_clear_threshold_for_most_fits():
    fixed = np.array([0.5])
    clear = [bool(census_ref.clear_of_scores(s, fixed)[0]) for label in cr.SCAN_SETS
             for s in cr.scan_set(label).per]
    assert sum(clear) >= len(clear) - 1, clear


def test_every_partner_query_has_clear_cuts():
    k = cr.load("A_s1_T300")
    tight = 0
    for q in range(k.P):
        sc = np.sort(partners_ref.ref_query(k.theta, k.pr, q)[0])[::-1]
        cuts = cr.clear_cuts(sc, 8, 256)
        assert cuts.size and cuts[0] <= 64, (q, cuts[:3])
        tight += cr.tight_gaps(sc, int(cuts[-1]))
    assert tight > 0


@pytest.mark.parametrize("label", pc.SETS)
def test_every_partner_list_has_both_cuts_and_a_crowded_top(label):
    """The preconditions of tests/test_gpu_partners_converged.py, on the reference alone, for every
    gene as a query, both `known` tables, with and without the shared pair mask, and for the ensemble,
    every slot, every quorum score and the spread: a clear cut in [8, 256] and one in [257, 1024]
    (partners_converged_ref.plan asserts them, and that enough tops crowd), and the facts the exact
    check builds on: every query keeps and loses candidates under the mask, and its chunks of at most
    1024 candidates are disjoint and cover them."""
    B = len(cr.SCAN_SETS[label])
    stats = pc.lists_of(B) + (partners_stat_ref.stat_calls(B) if label in pc.STAT_SETS else [])
    if label in pc.STAT_SETS:
        assert partners_stat_ref.stat_calls(B) == [("quorum", 1), ("quorum", 2), ("quorum", 3), ("spread", 0)]
    for known in pc.KNOWN:
        whole = pc.case(label, known, False)
        assert whole.P == (60 if label in pc.STAT_SETS else 80) and whole.genes == list(range(whole.P))
        for masked in (False, True):
            c = pc.case(label, known, masked)
            for stat in stats:
                p = pc.plan(label, known, masked, stat)
                print("%s %s %s %-14s %2d N, %2d of %d queries crowded" % (label, known, "masked" if masked else "all   ",
                                                                        stat, len(p.by_n), p.crowded, c.P))
                assert sum(len(v) for v in p.by_n.values()) == 2 * c.P
                if label in pc.STAT_SETS and not masked and stat[0] != "slot":
                    assert p.crowded >= 57
            for r, w in zip(c.refs, whole.refs):
                assert w.total == (c.P - 1) * (c.P - 2) // 2 and (known == "fold" or w.tkeys.size == w.total)
                assert 0 < r.tkeys.size <= w.tkeys.size and (r.tkeys.size < w.tkeys.size) == masked
                ch = pc.chunks(r)
                assert all(0 < x.size <= pc.FULL for x in ch) and len(ch) == -(-r.tkeys.size // pc.FULL)
                assert np.array_equal(np.concatenate(ch), np.sort(r.pkeys)) and np.unique(r.pkeys).size == r.pkeys.size
            assert max(r.tkeys.size for r in c.refs) > pc.FULL
