"""The dispute scan on converged fits: the ensembles of converged_ref.SCAN_SETS (three seeds each;
the single-sample set has no spread), tests/golden/converged/.

On a converged fit the restarts sit in different optima and hundreds of triples have a spread of
1 - O(eps): the top of the list crowds, adjacent gaps of the reference's top 4096 lie below the 4e-9
two spreads can move against each other, and the ORDER of a top-N list is not determined by the
reference.  Its SET is, wherever the reference's absolute gap between the N-th and the (N + 1)-th
spread exceeds census_ref.GAP (1e-7, 25 times that): the lists are compared there, as
converged_ref.check_set_cut compares, with the spread's absolute tolerance RTOL (hi + lo)
(tests/spread_ref.py).  Then exactly, without a tolerance, against the slots' own threshold scans.
"""
from math import comb

import numpy as np
import pytest

import converged_ref as cr
import scan_ref
import spread_ref
from scan_gpu import engine
from scan_ref import bits, packed

pytestmark = pytest.mark.gpu

GRID = "MMSBM_SCAN_SPREAD_GRID"
SETS = [label for label, names in cr.SCAN_SETS.items() if len(names) >= 2]
PARAMS = [(label, known) for label in SETS for known in cr.KNOWN]
cases = pytest.mark.parametrize("label,known", PARAMS, ids=["%s-%s" % c for c in PARAMS])


@pytest.fixture(autouse=True)
def no_grid_override(monkeypatch):
    monkeypatch.delenv(GRID, raising=False)


def same(x, y):
    assert len(x) == len(y)
    for u, v in zip(x, y):
        assert u.dtype == v.dtype and u.shape == v.shape and bits(u) == bits(v)


clear_cuts, check_set_cut = cr.clear_cuts_abs, cr.check_set_cut_abs     # the set rule with absolute gaps and bounds


def pick_cuts(desc):
    """The two N: the largest clear cut <= 4096 and the middle one of [64, 512]."""
    big, small = clear_cuts(desc, 513, 4096), clear_cuts(desc, 64, 512)
    assert big.size and small.size
    return int(big[-1]), int(small[small.size // 2])


@cases
def test_spread_top_at_clear_cuts(monkeypatch, label, known):
    s = cr.scan_set(label)
    kn = s.known[known]
    eng = engine(s.theta, s.pr)
    trims = eng.spread_trims()
    assert trims == spread_ref.legal(s.per.shape[0])
    for t in trims:
        d, tol = spread_ref.spread(s.per, t), spread_ref.atol(s.per, t)
        desc = cr.eligible_desc(d, s.keys, kn)
        # the order inside is not determined: the reason for comparing sets
        assert int(np.count_nonzero(desc[:4095] - desc[1:4096] <= 4 * spread_ref.RTOL)) > 0
        for n in pick_cuts(desc):
            got = eng.spread_top(n, t, kn)
            check_set_cut(got[0], got[1], d, tol, s.keys, n, kn, s.P)
            monkeypatch.setenv(GRID, "7")
            same(eng.spread_top(n, t, kn), got)
            monkeypatch.delenv(GRID)
    eng.close()


@pytest.mark.parametrize("label", SETS)
def test_exact_against_the_slots_threshold_scans(label):
    """No tolerance, crowded or not: sorted[B - 1 - t] - sorted[t] per key of the slots' own
    scan_above lists under the total order is spread_top's list in bits and ids, with and without a
    pair mask."""
    s = cr.scan_set(label)
    B, P = s.per.shape[0], s.P
    eng = engine(s.theta, s.pr)
    keys, per = None, []
    for slot in range(B):
        sc, ids = eng.scan_above(0.0, sample=slot)                  # every triple, whatever its score
        assert sc.size == comb(P, 3)
        k = packed(ids, P)
        at = np.argsort(k)
        assert keys is None or np.array_equal(keys, k[at])
        keys = k[at]
        per.append(sc[at])
    per = np.sort(np.stack(per), axis=0)
    mask, blocked = cr.random_pair_mask(P)
    for name in cr.KNOWN:
        kn = s.known[name]
        both = np.union1d(np.zeros(0, np.int64) if kn is None else kn, blocked).astype(np.int64)
        for t in eng.spread_trims():
            for known, kw in ((kn, {}), (both, {"mask": mask})):
                keep = np.ones(keys.size, bool) if known is None else ~np.isin(keys, known)
                d = (per[B - 1 - t] - per[t])[keep]
                order = np.lexsort((keys[keep], -d))
                want_s, want_k = d[order], keys[keep][order]
                for n in (64, 4096):
                    got_s, got_ids = eng.spread_top(n, t, kn, **kw)
                    assert got_s.size == n
                    assert bits(got_s) == bits(want_s[:n])
                    np.testing.assert_array_equal(got_ids, scan_ref.keys_to_ids(want_k[:n], P))
    eng.close()
