"""The scan families over their whole kernel matrix: scan (mmsbm_scan_topn), partners
(mmsbm_partners_topn), census (mmsbm_scan_census), pair census (mmsbm_pair_census) and threshold scan
(mmsbm_scan_above), each at every KS = ceil(K / 4) = 1..8, single sample and ensemble (ENS), and the
ensemble at each row-block width WB = 4, 2, 1 that csrc/scan_host.h pick_wb chooses, up to the last
supported ensemble and the first refused one.

References: the numpy float64 scorers of tests/census_ref.py, tests/pair_census_ref.py and
tests/partners_ref.py.  The ensemble reference is the per-slot reference scores added in slot order
and divided by the count.  Preconditions, asserted on the reference alone before any comparison:
census_ref.assert_clear for thresholds (every threshold more than 1e-7 relative from every reference
score) and every adjacent relative gap in the reference's top N + 1 above 1e-9 for ordered lists.
Tolerances are the project's: rtol 1e-9 on scores, equality on counts, ids and sets.

Every case takes the width it is meant to hit from the Python mirror of pick_wb (tests/scan_rule.py,
held against the C++ by tests/test_scan_rule_host.py) and asserts it, so a retuned rule fails here
loudly instead of quietly testing another layout.

At the end the module prints, per family and per (KS, ENS, WB) cell, the largest relative score
error against the reference it saw (the census and the pair census return integers only: their
cells show the number of exact count comparisons).  These numbers are reported, not asserted.
"""
import collections
import functools
from math import comb

import numpy as np
import pytest

import census_ref
import pair_census_ref as ref
import partners_ref
import scan_ref
import scan_rule
from scan_gpu import Raw, engine
from scan_ref import bits, packed, prefix_mean

pytestmark = pytest.mark.gpu

RTOL = scan_ref.RTOL
P_MATRIX = 70       # 5 b-tiles: 2, 3 and 5 row blocks per a at WB = 4, 2 and 1
N_TOP = 64
N_PARTNERS = 50

WORST = {}          # (family, KS, ENS, WB) -> largest relative score error seen
COUNTED = collections.Counter()     # (family, KS, ENS, WB) -> exact integer comparisons made


@pytest.fixture(scope="module", autouse=True)
def matrix_report():
    yield
    print()
    for cell in sorted(set(WORST) | set(COUNTED)):
        family, ks, ens, wb = cell
        what = "max rel err %.3e" % WORST[cell] if cell in WORST else "integers only"
        print("scan matrix  %-11s KS=%d %-8s WB=%d  %s, %d comparisons"
              % (family, ks, "ensemble" if ens else "single", wb, what, COUNTED[cell]))


def record(cell, got=None, want=None):
    if got is not None and np.size(want):
        err = float(np.max(np.abs(np.asarray(got) - want) / np.abs(want))) if np.shape(got) == np.shape(want) else np.inf
        WORST[cell] = max(WORST.get(cell, 0.0), err)
    COUNTED[cell] += 1


# ------------------------------------------------------------------------------ cases, reference
Case = collections.namedtuple("Case", "K B P th pr per scores keys")


@functools.lru_cache(maxsize=None)
def case(K, B, P, seed):
    """Random parameters of B samples with the reference scores of every slot and of the ensemble
    (added in slot order, divided by B); computed once and read-only."""
    th, pr = scan_ref.random_params(K, P, seed, B)
    per = [scan_ref.ref_scores(th[b], pr[b]) for b in range(B)]
    keys = per[0][1]
    assert (np.diff(keys) > 0).all()
    per = [s for s, _ in per]
    scores = prefix_mean(per, B)
    for a in per + [scores, keys, th, pr]:
        a.setflags(write=False)
    return Case(K, B, P, th, pr, per, scores, keys)


def cell_of(family, K, ns):
    """The (family, KS, ENS, WB) cell a call with ns samples runs in, by the mirror."""
    rule = scan_rule.PARTNERS if family == "partners" else scan_rule.CENSUS_LIKE
    wb = scan_rule.width(K, ns, rule)
    assert wb in (1, 2, 4), (family, K, ns)
    return (family, (K + 3) // 4, ns > 1, wb)


EDGE = [(0, 1, 2), (0, 1, 15), (-3, -2, -1), (0, -2, -1), (5, 33, 34), (15, 16, 17), (16, 17, 18), (31, 32, 47),
        (47, 48, 63), (63, 64, -1), (0, 15, 16), (17, 20, 31)]


def known_keys(keys, P):
    """Every fourth reference key plus known keys in the first, the last and diagonal tiles (the
    edge triples of test_gpu_census, those that exist at this P): sorted packed keys."""
    edge = []
    for t in EDGE:
        a, b, c = (v + P if v < 0 else v for v in t)
        if 0 <= a < b < c < P:
            edge.append((a * P + b) * P + c)
    return np.union1d(keys[::4], np.array(edge, dtype=np.int64)).astype(np.int64)


def threshold_near(scores, q):
    """The midpoint of the wide gap (census_ref.gap_thresholds' kind) nearest the q-quantile."""
    s = np.unique(scores)
    wide = np.flatnonzero((s[1:] - s[:-1]) > 4 * 1e-7 * np.abs(s[1:]))
    at = np.searchsorted(s, np.quantile(scores, q))
    i = wide[np.argmin(np.abs(wide - at))]
    return float((s[i] + s[i + 1]) / 2)


# ------------------------------------------------------------------------------ the five checks
def check_scan(eng, c, scores, known, sample, cell, n=N_TOP):
    want_s, want_k = scan_ref.top(scores, c.keys, n, known)
    assert scan_ref.min_gap(want_s) > 1e-9          # the precondition, reference alone
    want_s, want_k = want_s[:n], want_k[:n]
    got_s, got_ids = eng.scan_top(n, known, sample=sample)
    record(cell, got_s, want_s)
    assert got_ids.dtype == np.int32 and got_s.dtype == np.float64
    assert got_ids.shape == (want_k.size, 3)
    np.testing.assert_array_equal(got_ids, scan_ref.keys_to_ids(want_k, c.P))
    np.testing.assert_allclose(got_s, want_s, rtol=RTOL, atol=0)
    return got_s, got_ids


def check_census(eng, c, scores, known, sample, cell, thresholds=None):
    if thresholds is None:
        thresholds = census_ref.gap_thresholds(scores, 40)
    census_ref.assert_clear(scores, thresholds)         # the precondition, reference alone
    want, want_total = census_ref.ref_census(scores, c.keys, thresholds, known)
    got, got_total = eng.census(thresholds, known, sample=sample)
    record(cell)
    assert got.dtype == np.int64 and got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    assert got_total == want_total == comb(c.P, 3) - (0 if known is None else int(np.isin(c.keys, known).sum()))
    return thresholds


def check_pair_census(eng, c, scores, known, sample, cell, thresholds=None):
    if thresholds is None:
        thresholds = census_ref.gap_thresholds(scores, 40)[:8]
    census_ref.assert_clear(scores, thresholds)
    _, want = ref.ref_pairs(scores, c.keys, c.P, thresholds, known)
    got = eng.pair_census(thresholds, known, sample=sample)
    record(cell)
    assert got.dtype == np.int32 and got.shape == (c.P, c.P, len(thresholds))
    np.testing.assert_array_equal(got, want)


def check_scan_above(eng, c, scores, known, sample, cell, t):
    census_ref.assert_clear(scores, [t])
    s, ids = eng.scan_above(t, known, sample=sample)
    assert s.dtype == np.float64 and ids.dtype == np.int32 and ids.shape == (s.size, 3)
    got = packed(ids, c.P)
    want = scores >= t
    if known is not None and len(known):
        want &= ~np.isin(c.keys, known)
    at = np.minimum(np.searchsorted(c.keys, got), c.keys.size - 1)
    real = c.keys[at] == got                            # rows that name a triple (all, asserted below)
    record(cell, s[real], scores[at[real]])
    np.testing.assert_array_equal(np.sort(got), c.keys[want])               # the reference's set
    np.testing.assert_allclose(s, scores[np.searchsorted(c.keys, got)], rtol=RTOL, atol=0)
    assert (np.diff(s) <= 0).all() and (np.diff(got)[np.diff(s) == 0] > 0).all()   # the scan's total order
    counts, _ = eng.census([t], known, sample=sample)
    assert s.size == counts[0]                                               # the census, exactly
    return s, ids


def partner_queries(P):
    """The genes at the first, the middle and the last rank position."""
    order, _ = scan_ref.rank_tables(P)
    return [int(order[q]) for q in (0, P // 2, P - 1)]


def check_partners(eng, c, n_slots, known, sample, cell, n=N_PARTNERS):
    """Three queries against the reference mean of the first n_slots slots; `known` (packed triple
    keys) becomes each query's known pairs."""
    _, rank = scan_ref.rank_tables(c.P)
    queries = partner_queries(c.P)
    per_query, off, pairs = [], [0], []
    for g in queries:
        q = int(rank[g])
        _, tk, pk = partners_ref.ref_query(c.th[0], c.pr[0], q)
        per = [partners_ref.ref_query(c.th[b], c.pr[b], q)[0] for b in range(n_slots)]
        mine = np.sort(pk[np.isin(tk, known)]) if known is not None else np.zeros(0, np.int64)
        per_query.append((prefix_mean(per, n_slots), mine))
        pairs.append(mine)
        off.append(off[-1] + mine.size)
    kn = None if known is None else (np.array(off, dtype=np.int64), np.concatenate(pairs))
    rows = eng.partners_top(queries, n, kn, sample=sample)
    assert len(rows) == len(queries)
    for g, row, (scores, mine) in zip(queries, rows, per_query):
        want_s, _, gap = partners_ref.want_list(c.th[0], c.pr[0], g, n, mine, scores)
        assert gap > 1e-9                               # the precondition, reference alone
        record(cell, row[0], want_s)
        partners_ref.check_query(row, c.th[0], c.pr[0], g, n, mine, scores)
    return rows


# ------------------------------------------------------------------ (a) every KS, single sample
SINGLE_K = [3, 7, 10, 14, 18, 22, 26, 30]       # one per KS, none a multiple of 4: the padding is live


def single(K):
    assert K % 4 and (K + 3) // 4 == 1 + SINGLE_K.index(K)
    return case(K, 1, P_MATRIX, 300 + K)


@pytest.mark.parametrize("K", SINGLE_K)
def test_single_scan(K):
    c = single(K)
    eng = engine(c.th.copy(), c.pr.copy())
    for known in (None, known_keys(c.keys, c.P)):
        check_scan(eng, c, c.scores, known, 0, cell_of("scan", K, 1))
    eng.close()


@pytest.mark.parametrize("K", SINGLE_K)
def test_single_partners(K):
    c = single(K)
    eng = engine(c.th.copy(), c.pr.copy())
    for known in (None, known_keys(c.keys, c.P)):
        check_partners(eng, c, 1, known, 0, cell_of("partners", K, 1))
    eng.close()


@pytest.mark.parametrize("K", SINGLE_K)
def test_single_census(K):
    c = single(K)
    eng = engine(c.th.copy(), c.pr.copy())
    for known in (None, known_keys(c.keys, c.P)):
        check_census(eng, c, c.scores, known, 0, cell_of("census", K, 1))
    eng.close()


@pytest.mark.parametrize("K", SINGLE_K)
def test_single_pair_census(K):
    c = single(K)
    eng = engine(c.th.copy(), c.pr.copy())
    for known in (None, known_keys(c.keys, c.P)):
        check_pair_census(eng, c, c.scores, known, 0, cell_of("pair_census", K, 1))
    eng.close()


@pytest.mark.parametrize("K", SINGLE_K)
def test_single_scan_above(K):
    c = single(K)
    eng = engine(c.th.copy(), c.pr.copy())
    t = threshold_near(c.scores, 0.99)
    for known in (None, known_keys(c.keys, c.P)):
        s, _ = check_scan_above(eng, c, c.scores, known, 0, cell_of("scan_above", K, 1), t)
        assert 0.005 * c.keys.size < s.size < 0.015 * c.keys.size
    eng.close()


# ------------------------------------------------------------------ (b) every KS under ENS, each WB
ENSEMBLES = [(3, 22, 2), (7, 3, 4), (10, 10, 2), (10, 19, 1), (14, 7, 4), (14, 13, 2), (18, 6, 2), (18, 12, 1),
             (22, 5, 2), (22, 10, 1), (26, 4, 4), (26, 9, 1), (30, 4, 2), (30, 8, 1), (32, 15, 1)]
PARTNER_ENSEMBLES = [(3, 22, 2), (7, 3, 4), (10, 7, 2), (10, 14, 1), (14, 11, 1), (18, 5, 2), (22, 8, 1), (26, 3, 4),
                     (26, 7, 1), (30, 3, 2), (30, 6, 1), (32, 11, 1)]
ens_ids = ["K%dxB%d-WB%d" % e for e in ENSEMBLES]
partner_ens_ids = ["K%dxB%d-WB%d" % e for e in PARTNER_ENSEMBLES]


def ensemble(K, B, WB, family, P=P_MATRIX):
    cell = cell_of(family, K, B)
    assert cell[3] == WB, "the row-block rule moved: this case no longer runs at WB = %d" % WB
    return case(K, B, P, 500 + K + B), cell


def test_the_ensemble_cases_cover_the_matrix():
    """Every KS under ENS; every width at several KS; the last supported ensemble of each rule."""
    for cases, rule in ((ENSEMBLES, scan_rule.CENSUS_LIKE), (PARTNER_ENSEMBLES, scan_rule.PARTNERS)):
        assert all(scan_rule.width(K, B, rule) == WB for K, B, WB in cases)
        for WB in (4, 2, 1):
            assert len({(K + 3) // 4 for K, _, wb in cases if wb == WB}) >= 2
        assert (32, scan_rule.last_supported(32, rule), 1) in cases
        assert {(K + 3) // 4 for K, _, _ in cases} == set(range(1, 9))


@pytest.mark.parametrize("K,B,WB", ENSEMBLES, ids=ens_ids)
def test_ensemble_scan(K, B, WB):
    c, cell = ensemble(K, B, WB, "scan")
    eng = engine(c.th.copy(), c.pr.copy())
    for known in (None, known_keys(c.keys, c.P)):
        check_scan(eng, c, c.scores, known, None, cell)
    eng.close()


@pytest.mark.parametrize("K,B,WB", ENSEMBLES, ids=ens_ids)
def test_ensemble_census(K, B, WB):
    c, cell = ensemble(K, B, WB, "census")
    eng = engine(c.th.copy(), c.pr.copy())
    for known in (None, known_keys(c.keys, c.P)):
        check_census(eng, c, c.scores, known, None, cell)
    eng.close()


@pytest.mark.parametrize("K,B,WB", ENSEMBLES, ids=ens_ids)
def test_ensemble_pair_census(K, B, WB):
    c, cell = ensemble(K, B, WB, "pair_census")
    eng = engine(c.th.copy(), c.pr.copy())
    for known in (None, known_keys(c.keys, c.P)):
        check_pair_census(eng, c, c.scores, known, None, cell)
    eng.close()


@pytest.mark.parametrize("K,B,WB", ENSEMBLES, ids=ens_ids)
def test_ensemble_scan_above(K, B, WB):
    c, cell = ensemble(K, B, WB, "scan_above")
    eng = engine(c.th.copy(), c.pr.copy())
    t = threshold_near(c.scores, 0.99)
    for known in (None, known_keys(c.keys, c.P)):
        s, _ = check_scan_above(eng, c, c.scores, known, None, cell, t)
        assert 0.005 * c.keys.size < s.size < 0.015 * c.keys.size
    eng.close()


@pytest.mark.parametrize("K,B,WB", PARTNER_ENSEMBLES, ids=partner_ens_ids)
def test_ensemble_partners(K, B, WB):
    c, cell = ensemble(K, B, WB, "partners")
    eng = engine(c.th.copy(), c.pr.copy())
    for known in (None, known_keys(c.keys, c.P)):
        check_partners(eng, c, B, known, None, cell)
    eng.close()


# ------------------------------------------------------------------ (c) tile edges at narrow row blocks
EDGES = [(10, 10, 2, P) for P in (31, 32, 33, 65)] + [(10, 19, 1, P) for P in (17, 33, 47)]
edge_ids = ["K%dxB%d-WB%d-P%d" % e for e in EDGES]


@pytest.mark.parametrize("family", ["census", "pair_census", "scan_above"])
@pytest.mark.parametrize("K,B,WB,P", EDGES, ids=edge_ids)
def test_tile_edges_at_narrow_row_blocks(K, B, WB, P, family):
    """P below, at and above one 32-row item and two, and around the 16-row items of WB = 1: padded
    rows and columns, items that start mid-triangle and items with no triple."""
    c, cell = ensemble(K, B, WB, family, P)
    eng = engine(c.th.copy(), c.pr.copy())
    for known in (None, known_keys(c.keys, P)):
        if family == "census":
            check_census(eng, c, c.scores, known, None, cell)
        elif family == "pair_census":
            check_pair_census(eng, c, c.scores, known, None, cell)
        else:
            below_all = float(c.scores.min() * (1 - 1e-3))          # every lane of every tile appends
            s, _ = check_scan_above(eng, c, c.scores, known, None, cell, below_all)
            assert s.size == comb(P, 3) - (0 if known is None else known.size)
            check_scan_above(eng, c, c.scores, known, None, cell, threshold_near(c.scores, 0.5))
    eng.close()


@pytest.mark.parametrize("K,B,WB", [(10, 10, 2), (10, 19, 1)], ids=["WB2", "WB1"])
def test_everything_known_counts_nothing_at_narrow_row_blocks(K, B, WB):
    P = 33
    cells = [ensemble(K, B, WB, f, P)[1] for f in ("census", "pair_census", "scan_above")]
    c = ensemble(K, B, WB, "census", P)[0]
    eng = engine(c.th.copy(), c.pr.copy())
    thresholds = census_ref.gap_thresholds(c.scores, 20)
    every = c.keys.copy()
    check_census(eng, c, c.scores, every, None, cells[0], thresholds)
    counts, total = eng.census(thresholds, every)
    assert total == 0 and not counts.any()
    check_pair_census(eng, c, c.scores, every, None, cells[1], thresholds[:8])
    assert not eng.pair_census(thresholds[:8], every).any()
    s, ids = check_scan_above(eng, c, c.scores, every, None, cells[2], float(c.scores.min() * (1 - 1e-3)))
    assert s.size == 0 and ids.shape == (0, 3)
    eng.close()


# ------------------------------------------------------------------ (d) the families' identities
NARROW = [(10, 10, 2), (10, 19, 1)]
narrow_ids = ["WB2", "WB1"]


@pytest.mark.parametrize("K,B,WB", NARROW, ids=narrow_ids)
def test_identities_at_narrow_row_blocks(K, B, WB):
    """Product against product, exact, no precondition: the consumers of the shared sweep see the
    scan's score bits and the scan's triples at WB < 4 too."""
    c, _ = ensemble(K, B, WB, "census")
    P, N = c.P, 50
    eng = engine(c.th.copy(), c.pr.copy())
    upper = np.triu(np.ones((P, P), dtype=bool), k=1)
    for kn in (None, known_keys(c.keys, P)):
        scores, ids = eng.scan_top(N, kn)
        assert scores.size == N
        # the census at the scores of a scan list numbers the list
        counts, total = eng.census(scores, kn)
        np.testing.assert_array_equal(counts, (scores[None, :] >= scores[:, None]).sum(axis=1))
        assert total == comb(P, 3) - (0 if kn is None else kn.size)
        assert eng.census(np.nextafter(scores[:1], np.inf), kn)[0].tolist() == [0]
        # the pair census summed over x < y is three times the census
        thresholds = scores[np.linspace(0, N - 1, 8).astype(int)]
        census, _ = eng.census(thresholds, kn)
        assert census.tolist() == (scores[None, :] >= thresholds[:, None]).sum(axis=1).tolist()
        pairs = eng.pair_census(thresholds, kn)
        np.testing.assert_array_equal(pairs[upper].sum(axis=0, dtype=np.int64), 3 * census)
        # the threshold scan at the list's last score: the census's rows, headed by the list
        s2, ids2 = eng.scan_above(scores[-1], kn)
        assert s2.size == eng.census([scores[-1]], kn)[0][0] >= N
        np.testing.assert_array_equal(ids2[:N], ids)
        assert bits(s2[:N]) == bits(scores) and (s2[N:] == scores[-1]).all()
    eng.close()


@pytest.mark.parametrize("K,B,WB", NARROW, ids=narrow_ids)
def test_a_slot_of_a_wide_batch_equals_a_batch_of_one(K, B, WB):
    """sample = k takes the single-sample kernels at WB = 4 whatever the batch: bit for bit what a
    B = 1 engine holding that sample gives."""
    c, _ = ensemble(K, B, WB, "census")
    assert scan_rule.width(K, 1) == 4 and scan_rule.width(K, 1, scan_rule.PARTNERS) == 4
    known = known_keys(c.keys, c.P)
    eng = engine(c.th.copy(), c.pr.copy())
    queries = partner_queries(c.P)
    for k in (1, B - 1):
        solo_case = Case(K, 1, c.P, c.th[k:k + 1], c.pr[k:k + 1], [c.per[k]], c.per[k], c.keys)
        solo = engine(solo_case.th.copy(), solo_case.pr.copy())
        t = threshold_near(c.per[k], 0.99)
        for e, sample in ((eng, k), (solo, 0)):
            check_census(e, solo_case, c.per[k], known, sample, cell_of("census", K, 1))
        mine, theirs = [], []
        for out, (e, sample) in ((mine, (eng, k)), (theirs, (solo, 0))):
            out.extend(e.scan_top(N_TOP, known, sample=sample))
            out.extend(e.census(census_ref.gap_thresholds(c.per[k], 40), known, sample=sample))
            out.append(e.pair_census([t], known, sample=sample))
            out.extend(e.scan_above(t, known, sample=sample))
            for row in e.partners_top(queries, N_PARTNERS, sample=sample):
                out.extend(row)
        assert len(mine) == len(theirs) == 13
        for x, y in zip(mine, theirs):
            assert bits(x) == bits(y) if isinstance(x, np.ndarray) else x == y
        solo.close()
    eng.close()


@pytest.mark.parametrize("K,B,WB", NARROW, ids=narrow_ids)
def test_repeats_and_grids_at_narrow_row_blocks(K, B, WB, monkeypatch):
    c, _ = ensemble(K, B, WB, "census")
    assert scan_rule.width(K, B, scan_rule.PARTNERS) == WB      # the partner scan narrows here too
    known = known_keys(c.keys, c.P)
    thresholds = census_ref.gap_thresholds(c.scores, 40)
    t = threshold_near(c.scores, 0.9)
    eng = engine(c.th.copy(), c.pr.copy())
    th0, p0 = bits(eng.theta.cpu().numpy()), bits(eng.pr.cpu().numpy())

    def everything():
        rows = eng.partners_top(partner_queries(c.P), N_PARTNERS)
        return [*eng.scan_top(N_TOP, known), *eng.census(thresholds, known), eng.pair_census(thresholds[:8], known),
                *eng.scan_above(t, known), *[a for row in rows for a in row]]

    want = everything()
    assert 0.05 * c.keys.size < want[5].size < 0.15 * c.keys.size
    for grid in (None, "1", "7"):           # None: a repeated ensemble call repeats its bits
        for name in ("MMSBM_CENSUS_GRID", "MMSBM_PAIR_CENSUS_GRID", "MMSBM_SCAN_ABOVE_GRID"):
            if grid is not None:
                monkeypatch.setenv(name, grid)
        got = everything()
        assert len(got) == len(want)
        for x, y in zip(got, want):
            assert bits(x) == bits(y) if isinstance(x, np.ndarray) else x == y
    for name in ("MMSBM_CENSUS_GRID", "MMSBM_PAIR_CENSUS_GRID", "MMSBM_SCAN_ABOVE_GRID"):
        monkeypatch.delenv(name)
    assert bits(eng.theta.cpu().numpy()) == th0 and bits(eng.pr.cpu().numpy()) == p0
    eng.close()


# ------------------------------------------------------------------ (e) the active prefix moves the width
def test_the_active_prefix_moves_the_width():
    K, B = 10, 19
    c, _ = ensemble(K, B, 1, "census")
    eng = engine(c.th.copy(), c.pr.copy())
    for n, WB in ((19, 1), (10, 2), (9, 4), (1, 4)):
        assert scan_rule.width(K, n) == WB
        eng.set_active(n)
        scores = prefix_mean(c.per, n)
        for known in (None, known_keys(c.keys, c.P)):
            check_census(eng, c, scores, known, None, cell_of("census", K, n))
            check_scan(eng, c, scores, known, None, cell_of("scan", K, n))
    eng.close()


# ------------------------------------------------------------------ (f) the refusal boundary
def raw_call(raw, sample):
    """The family's C call at a small size into sentinel-filled outputs -> the return code."""
    torch, P = raw.torch, raw.eng.P
    f64, i32, i64 = torch.float64, torch.int32, torch.int64
    if raw.family == "scan":
        return raw.call((8,), [raw.full((8,), f64), raw.full((8, 3), i32), raw.full((1,), i64)], sample)
    if raw.family == "partners":
        queries = np.array(partner_queries(P), dtype=np.int32)
        Q = queries.size
        return raw.call((8,), [raw.full((Q, 8), f64), raw.full((Q, 8, 3), i32), raw.full((Q,), i64)], sample,
                        queries=queries)
    if raw.family == "scan_above":
        return raw.call((0.6, 64), [raw.full((64,), f64), raw.full((64,), i64), raw.full((1,), i64)], sample)
    thr = raw.upload(np.array([0.4, 0.6]))
    out = raw.full((3,), i64) if raw.family == "census" else raw.full((P, P, 2), i32)
    return raw.call((thr.data_ptr(), 2), [out], sample)


RAW_SIZES = {"scan": (8,), "partners": (3, 8), "census": (2,), "pair_census": (2,), "scan_above": ()}


def binding_call(eng, family, c, scores, n_slots, sample, cell):
    """The family's call through the binding, checked against `scores` (the reference of what
    `sample` names)."""
    if family == "scan":
        check_scan(eng, c, scores, None, sample, cell)
    elif family == "partners":
        check_partners(eng, c, n_slots, None, sample, cell)
    elif family == "census":
        check_census(eng, c, scores, None, sample, cell)
    elif family == "pair_census":
        check_pair_census(eng, c, scores, None, sample, cell)
    else:
        check_scan_above(eng, c, scores, None, sample, cell, threshold_near(scores, 0.99))


@pytest.mark.parametrize("family", ["scan", "partners", "census", "pair_census", "scan_above"])
@pytest.mark.parametrize("K", [10, 32])
def test_the_first_refused_ensemble_and_the_last_supported(K, family):
    from trigenicinteractionpredictor_amd import _lib
    rule = scan_rule.PARTNERS if family == "partners" else scan_rule.CENSUS_LIKE
    B = scan_rule.last_supported(K, rule) + 1
    assert B == {(10, False): 37, (32, False): 16, (10, True): 28, (32, True): 12}[(K, family == "partners")]
    assert scan_rule.width(K, B, rule) == 0 and scan_rule.width(K, B - 1, rule) == 1
    c = case(K, B, 40, 800 + K + B)
    eng = engine(c.th.copy(), c.pr.copy())
    # the full prefix: refused through the binding, and through the C call with its outputs untouched
    with pytest.raises(_lib.MMSBMError) as e:
        binding_call(eng, family, c, c.scores, B, None, None)
    assert e.value.code == _lib.MMSBM_ERR_UNSUPPORTED and "one by one" in str(e.value)
    raw = Raw(eng, family, *RAW_SIZES[family])       # the workspace follows the shape, not the prefix
    assert raw_call(raw, -1) == _lib.MMSBM_ERR_UNSUPPORTED and raw.intact()
    # one slot of the refused engine is a single-sample call
    binding_call(eng, family, c, c.per[0], 1, 0, cell_of(family, K, 1))
    assert raw_call(raw, 0) == _lib.MMSBM_OK and not raw.intact()
    # one slot fewer: the last supported ensemble
    eng.set_active(B - 1)
    binding_call(eng, family, c, prefix_mean(c.per, B - 1), B - 1, None, cell_of(family, K, B - 1))
    assert raw_call(raw, -1) == _lib.MMSBM_OK and not raw.intact()
    eng.close()


# ------------------------------------------------------------------ (g) the launch stream
@pytest.mark.parametrize("sample", [0, None], ids=["sample", "ensemble"])
@pytest.mark.parametrize("family", ["scan", "partners", "census", "pair_census", "scan_above"])
def test_a_side_stream_returns_the_bytes_of_the_current_stream(family, sample):
    """Two valid calls, plain equality: every tensor of a call belongs to its launch stream.  P = 40
    has three b-tiles, the last one ragged; B = 2 takes the ensemble path."""
    import torch
    from trigenicinteractionpredictor_amd.scan import partner_known
    c = case(5, 2, 40, 900)
    known = c.keys[::4].copy()
    queries = partner_queries(c.P)
    pairs = partner_known((c.P, scan_ref.keys_to_ids(known, c.P), None), queries)
    scores = c.per[0] if sample == 0 else c.scores
    thresholds = census_ref.gap_thresholds(scores, 40)      # unsorted, one duplicate
    eng = engine(c.th.copy(), c.pr.copy())
    call = {"scan": lambda s: eng.scan_top_async(N_TOP, known, sample, s),
            "partners": lambda s: eng.partners_top_async(queries, N_PARTNERS, pairs, sample, s),
            "census": lambda s: eng.census_async(thresholds, known, sample, s),
            "pair_census": lambda s: (eng.pair_census_async(thresholds[:12], known, sample, s),),
            "scan_above": lambda s: eng.scan_above_async(threshold_near(scores, 0.99), known, sample, s)}[family]
    here = [x.cpu().numpy() for x in call(None)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    out = call(side)
    side.synchronize()
    there = [x.cpu().numpy() for x in out]
    assert len(here) == len(there) and sum(x.size for x in here) > 0
    for x, y in zip(here, there):
        assert x.dtype == y.dtype and x.shape == y.shape and bits(x) == bits(y)
    eng.close()
