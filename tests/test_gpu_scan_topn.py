"""The pass loop the three top-N scans share (csrc/scan_topn.h run_passes: the published bound's
reset, prep, the seeding pass, the full pass, the merge levels) at its edges, for the scan, the
quorum scan and the dispute scan alike: K = 3, two slots, P in {2, 3, 17, 199, 200} and N in
{1, 5, 4096}.

P = 2 has no triple: only the merge runs, and it must write count 0, NaN scores and -1 ids.  P = 3
has one.  P = 199 is the last gene count without the seeding pass, P = 200 the first with it.
N = 4096 keeps the candidate buffers in the workspace.  MMSBM_SCAN_*_GRID = 1 gives one list and
one merge level, 33 the fewest lists with two levels; the lists must not depend on it.

Every list is compared in bits with the product's own threshold scan (every triple's score, ranked
here under the total order), and, wherever the reference's gaps decide the order (N <= 5, or fewer
triples than N), with the numpy references of the families' own tests under those tests' tolerances
(scan_ref, quorum_ref, spread_ref).  An engine keeps one workspace per family, so each engine below
runs N = 4096, 1, 5 on one buffer: after N = 1 the bound word holds the best score of all, and the
next call finds its five rows only if it starts from zero.
"""
import functools

import numpy as np
import pytest

import quorum_ref
import scan_ref
import spread_ref
from scan_gpu import engine
from scan_ref import packed

pytestmark = pytest.mark.gpu

K, B, SEED = 3, 2, 11
PS = (2, 3, 17, 199, 200)
NS = (4096, 1, 5)                                # in this order on one workspace (see above)
FAMILIES = {"scan": (None,), "scan_quorum": (1, 2), "scan_spread": (0,)}     # min_votes; trim
GRID = {"scan_quorum": "MMSBM_SCAN_QUORUM_GRID", "scan_spread": "MMSBM_SCAN_SPREAD_GRID"}


@pytest.fixture(autouse=True)
def no_grid_override(monkeypatch):
    for name in GRID.values():
        monkeypatch.delenv(name, raising=False)


@functools.lru_cache(maxsize=None)
def case(P):
    return quorum_ref.case(K, P, SEED, B)


def run(eng, family, arg, n, known):
    """-> host (scores f64[n], ids int32[n][3], count)"""
    if family == "scan":
        out = eng.scan_top_async(n, known)
    elif family == "scan_quorum":
        out = eng.quorum_top_async(n, arg, known)
    else:
        out = eng.spread_top_async(n, arg, known)
    scores, ids, count = (x.cpu().numpy() for x in out)
    return scores, ids, int(count[0])


def values(family, arg, per):
    """What the family ranks by, per triple, from the slots' scores."""
    if family == "scan":
        return scan_ref.prefix_mean(per, B)
    if family == "scan_quorum":
        return quorum_ref.quorum(per, arg)
    return spread_ref.spread(per, arg)


def own_scores(eng, P):
    """Every slot's score of every triple in the product's own bits (the threshold scan), and the
    ensemble mean's: -> (keys ascending, per f64[B][T], mean f64[T])."""
    rows = []
    for sample in (0, 1, None):
        s, ids = eng.scan_above(1e-300, sample=sample)          # below every score
        k = packed(ids, P)
        at = np.argsort(k)
        rows.append((k[at], s[at]))
    assert all(np.array_equal(k, rows[0][0]) for k, _ in rows)
    return rows[0][0], np.stack([rows[0][1], rows[1][1]]), rows[2][1]


def against_the_reference(family, arg, c, n, known, scores, ids, P):
    if family == "scan_spread":
        want_s, want_k = spread_ref.ref_top(c.per, c.keys, arg, n, known)      # asserts the gaps
    else:
        want_s, want_k = scan_ref.top(values(family, arg, c.per), c.keys, n, known)
        scan_ref.assert_gaps(want_s)
    want_s, want_k = want_s[:n], want_k[:n]
    np.testing.assert_array_equal(ids, scan_ref.keys_to_ids(want_k, P))
    if family == "scan_spread":
        atol = spread_ref.atol(c.per, arg)[np.searchsorted(c.keys, want_k)]
        assert (np.abs(scores - want_s) <= atol).all()
    else:
        np.testing.assert_allclose(scores, want_s, rtol=scan_ref.RTOL, atol=0)


@pytest.mark.parametrize("P", PS)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_pass_loop_edges(family, P, monkeypatch):
    c = case(P)
    triples = P * (P - 1) * (P - 2) // 6
    assert c.keys.size == triples
    eng = engine(c.theta, c.pr)
    if triples:
        keys, per, mean = own_scores(eng, P)
        assert np.array_equal(keys, c.keys)
    knowns = (c.keys[1::9].copy(),) if P >= 199 else (None, c.keys[1::9].copy())
    ws = None
    for arg in FAMILIES[family]:
        for known in knowns:
            eligible = triples - (0 if known is None else known.size)
            for n in NS:
                scores, ids, count = run(eng, family, arg, n, known)
                if ws is None:
                    ws = eng.scan_workspace(family, max(NS))
                assert eng.scan_workspace(family, n) is ws                   # one buffer for every N
                assert scores.shape == (n,) and ids.shape == (n, 3)
                assert count == min(n, eligible)
                assert np.isnan(scores[count:]).all() and (ids[count:] == -1).all()     # the NaN / -1 tail
                if not triples:
                    continue
                # the product's own bits, ranked here
                own = mean if family == "scan" else values(family, arg, per)
                want_s, want_k = scan_ref.top(own, keys, n, known)
                assert scores[:count].tobytes() == want_s[:count].tobytes()
                np.testing.assert_array_equal(ids[:count], scan_ref.keys_to_ids(want_k[:count], P))
                if n <= 5 or triples < n:
                    against_the_reference(family, arg, c, n, known, scores[:count], ids[:count], P)
                if family in GRID:
                    for grid in ("1", "33"):
                        monkeypatch.setenv(GRID[family], grid)
                        got = run(eng, family, arg, n, known)
                        assert got[2] == count and got[0].tobytes() == scores.tobytes()
                        assert got[1].tobytes() == ids.tobytes()
                    monkeypatch.delenv(GRID[family])
    eng.close()
