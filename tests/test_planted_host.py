"""The planted block model of tests/planted_ref.py against the all-triples references the suite
already has (scan_ref, census_ref, votes_ref, pair_census_ref, pair_votes_ref) at sizes where numpy
scores every triple, its exactness claims, and every precondition of tests/test_gpu_scale.py, on the
reference alone.  No GPU."""
from math import comb

import numpy as np
import pytest

import census_ref
import masked_ref
import pair_census_ref
import pair_votes_ref
import planted_ref as pl
import scan_ref
import votes_ref

SMALL = [(33, 1, 12), (33, 3, 12), (90, 1, 16), (90, 3, 16), (120, 1, 20), (120, 3, 20)]   # (P, B, E)


def small_model(P, B, E):
    return pl.build(P, B=B, E=E, seed=P + B, small=6)


def all_triples(model):
    """Per slot the scores of scan_ref.ref_scores on the full theta, and the keys."""
    per, keys = [], None
    for s in range(model.B):
        scores, keys = scan_ref.ref_scores(model.theta[s], model.pr[s])
        per.append(scores)
    return np.stack(per), keys


def known_of(model, keys):
    """Known keys of every kind: common, mixed and elite ones, the best elites among them."""
    rng = np.random.default_rng(7)
    best = model.keys[np.argsort(-pl.elite_values(model))[:5]]
    return np.unique(np.concatenate([keys[rng.random(keys.size) < 0.2], best]))


# ------------------------------------------------------------------ the structure and its exactness
@pytest.mark.parametrize("P,B,E", SMALL)
def test_structure_and_the_bands(P, B, E):
    m = small_model(P, B, E)
    order, _ = scan_ref.rank_tables(P)
    assert set(pl.edge_positions(P)[:E].tolist()) <= set(m.elite_pos.tolist()) and m.elite_pos.size == E
    assert {0, 1, 15, 16, 17, P - 2, P - 1} <= set(m.elite_pos.tolist())
    assert (m.label[m.elite_pos] == m.Kc).all() and (m.label < m.Kc).sum() == P - E
    sizes = np.bincount(m.label, minlength=m.Kc + 1)[:m.Kc]
    assert np.unique(sizes).size >= 3 and sizes.min() >= 2               # unequal, none empty
    for s in range(B):
        th = m.theta[s][order]                                           # by position
        np.testing.assert_allclose(th.sum(axis=1), 1.0, rtol=1e-12)
        common = m.label < m.Kc
        assert (th[common].max(axis=1) == 1.0).all() and ((th[common] == 0) | (th[common] == 1)).all()
        assert (th[common].argmax(axis=1) == m.Ke + m.label[common]).all()
        assert (th[~common][:, m.Ke:] == 0).all() and (th[~common][:, :m.Ke] > 0).all()
        p1 = m.pr[s][..., 1]
        assert (m.pr[s][..., 0] == 1.0 - p1).all()
        assert ((p1[:m.Ke, :m.Ke, :m.Ke] >= pl.ELITE_LO) & (p1[:m.Ke, :m.Ke, :m.Ke] <= pl.ELITE_HI)).all()
        cv = p1[m.Ke:, m.Ke:, m.Ke:]
        assert cv.tobytes() == m.cv[s].tobytes() and np.unique(cv).size == m.Kc ** 3
        assert cv.min() >= pl.COMMON_LO * (1 - 1e-12) and cv.max() <= pl.COMMON_HI * (1 + 1e-12)
        mixed = np.ones_like(p1, dtype=bool)
        mixed[:m.Ke, :m.Ke, :m.Ke] = False
        mixed[m.Ke:, m.Ke:, m.Ke:] = False
        assert (p1[mixed] == pl.MIXED).all()
    # the all-triples reference falls into the three bands the closed forms assume
    per, keys = all_triples(m)
    kind, cls, at = pl.classify(m, keys)
    assert (kind == 2).sum() == comb(E, 3) == m.keys.size and (kind == 1).sum() == pl.n_mixed(m)
    np.testing.assert_array_equal(keys[kind == 2], m.keys)
    for s in range(B):
        np.testing.assert_allclose(per[s][kind == 2], m.per[s], rtol=scan_ref.RTOL, atol=0)
        assert per[s][kind == 2].min() >= pl.ELITE_LO * (1 - 1e-12)
        assert per[s][kind == 1].max() <= pl.MIXED_TOP and per[s][kind == 1].min() > pl.BELOW_ALL
        c0 = kind == 0
        np.testing.assert_allclose(per[s][c0], m.cv[s][cls[0][c0], cls[1][c0], cls[2][c0]], rtol=1e-14, atol=0)
    assert per[:, kind != 2].max() <= pl.COMMON_HI * (1 + 1e-12)


def kernel_order_score(th_a, th_b, th_c, p1):
    """One triple's score in the order of csrc/scan_score.h: T_a[y][z] by a chain over x from zero,
    W[z] by a chain over y, S by a chain over z.  Every step is v = t * p + v in float64; for a
    one-hot row the product is exact (0 or the other factor), so the rounding of a fused
    multiply-add and of a multiply then add agree and plain arithmetic reproduces the bits."""
    K = th_a.size
    T = np.zeros((K, K))
    for x in range(K):
        T = th_a[x] * p1[x] + T
    W = np.zeros(K)
    for y in range(K):
        W = th_b[y] * T[y] + W
    S = 0.0
    for z in range(K):
        S = W[z] * th_c[z] + S
    return S


@pytest.mark.parametrize("P,B,E", [(33, 3, 12), (120, 1, 20)])
def test_a_common_triple_scores_its_class_value_bit_for_bit(P, B, E):
    m = small_model(P, B, E)
    order, _ = scan_ref.rank_tables(P)
    rng = np.random.default_rng(1)
    common = np.flatnonzero(m.label < m.Kc)
    for _ in range(60):
        a, b, c = np.sort(rng.choice(common, 3, replace=False))
        per = []
        for s in range(B):
            th = m.theta[s][order]
            got = kernel_order_score(th[a], th[b], th[c], m.pr[s][..., 1])
            want = m.pr[s][m.Ke + m.label[a], m.Ke + m.label[b], m.Ke + m.label[c], 1]
            assert np.float64(got).tobytes() == np.float64(want).tobytes()
            per.append(got)
        mean = scan_ref.prefix_mean(np.array(per)[:, None], B)[0]
        want = pl.class_values(m)[m.label[a], m.label[b], m.label[c]]
        assert np.float64(mean).tobytes() == np.float64(want).tobytes()
    # a mixed triple in the same order: below MIXED_TOP
    e = m.elite_pos
    for pos in ((e[0], common[3], common[9]), (common[0], e[3], common[9]), (e[1], e[2], common[-1]),
                (common[1], common[2], e[-1])):
        a, b, c = np.sort(pos)
        th = m.theta[0][order]
        assert 0 < kernel_order_score(th[a], th[b], th[c], m.pr[0][..., 1]) <= pl.MIXED_TOP


@pytest.mark.parametrize("P,B,E", SMALL)
def test_class_counts_against_a_loop_over_every_triple(P, B, E):
    m = small_model(P, B, E)
    _, keys = all_triples(m)
    a, b, c = pl.positions(keys, P)
    G = m.Kc + 1
    want = np.bincount((m.label[a] * G + m.label[b]) * G + m.label[c], minlength=G ** 3).reshape(G, G, G)
    np.testing.assert_array_equal(m.N, want)
    assert m.N.dtype == np.int64 and m.N.sum() == comb(P, 3)
    assert m.N[m.Kc, m.Kc, m.Kc] == comb(E, 3)


# ------------------------------------------------------------------ the closed forms
def modes(B):
    return [dict(sample=0)] if B == 1 else [dict(), dict(sample=1), dict(ns=2)]


@pytest.mark.parametrize("P,B,E", SMALL)
def test_census_counts(P, B, E):
    m = small_model(P, B, E)
    per, keys = all_triples(m)
    known = known_of(m, keys)
    for mode in modes(B):
        sl = pl.slots_of(m, **mode)
        scores = scan_ref.prefix_mean(per[sl], len(sl))
        t = pl.thresholds(m, **mode)
        assert t.size == 8 and (t < pl.COMMON_HI).sum() == 4 and (t > pl.ELITE_LO).sum() == 3
        census_ref.assert_clear(scores, t)
        for kn in (None, known):
            counts, total = pl.census(m, t, kn, **mode)
            want, want_total = census_ref.ref_census(scores, keys, t, kn)
            np.testing.assert_array_equal(counts, want)
            assert total == want_total and counts.dtype == np.int64
            assert counts[0] == total                   # the threshold below everything
        assert 0 < counts[1] < counts[2] < total        # both bands are cut inside


@pytest.mark.parametrize("P,B,E", SMALL)
def test_vote_histogram(P, B, E):
    m = small_model(P, B, E)
    per, keys = all_triples(m)
    known = known_of(m, keys)
    for ns in sorted({1, B}):
        checked = []
        for t in list(pl.vote_thresholds(m)) + pl.thresholds(m, ns=ns)[1:].tolist():
            if any(not census_ref.clear_of_scores(np.concatenate([m.cv[s].reshape(-1), m.per[s]]), [t]).all()
                   for s in range(ns)):
                continue
            checked.append(t)
            for kn in (None, known):
                want = votes_ref.ref_votes(per, keys, t, ns, kn)[3]
                np.testing.assert_array_equal(pl.votes(m, t, ns, kn), want)
        assert sum(pl.COMMON_LO < t < pl.COMMON_HI for t in checked) >= 2      # the common band was checked


@pytest.mark.parametrize("P,B,E", SMALL)
def test_pair_matrices_and_gene_counts(P, B, E):
    m = small_model(P, B, E)
    per, keys = all_triples(m)
    known = known_of(m, keys)
    mode = modes(B)[0]
    sl = pl.slots_of(m, **mode)
    scores = scan_ref.prefix_mean(per[sl], len(sl))
    t = pl.thresholds(m, **mode)
    for kn in (None, known):
        got = pl.pair_census(m, t, kn, **mode)
        np.testing.assert_array_equal(got, pair_census_ref.ref_pairs_rank(scores, keys, P, t, kn))
        assert got.dtype == np.int32
        np.testing.assert_array_equal(pl.gene_counts(got), pair_census_ref.ref_gene_counts(scores, keys, P, t, kn))
        np.testing.assert_array_equal(pair_votes_ref.upper_sums(got), 3 * pl.census(m, t, kn, **mode)[0])
    thr = [x for x in pl.thresholds(m, ns=B)[2:]
           if all(census_ref.clear_of_scores(np.concatenate([m.cv[s].reshape(-1), m.per[s]]), [x]).all()
                  for s in range(B))]
    assert len(thr) >= 2
    levels = list(range(1, B + 1))
    for x in (thr[0], thr[-1]):                         # one in the common band, one in the elite band
        for kn in (None, known):
            got = pl.pair_votes(m, x, levels, known=kn)
            np.testing.assert_array_equal(got, pair_votes_ref.ref_rank(per, keys, P, x, levels, known=kn))


@pytest.mark.parametrize("P,B", [(33, 1), (90, 3), (120, 3)])
def test_first_keys_is_the_top_of_an_all_common_model(P, B):
    m = pl.build(P, B=B, E=0, seed=5, small=6, best=(2, 3, 4))
    assert m.keys.size == 0 and m.N[m.Kc].sum() == 0
    per, keys = all_triples(m)
    scores = scan_ref.prefix_mean(per, B)
    cls, value = pl.best_class(m)
    assert cls == (2, 3, 4) and value == scores.max()
    n = min(40, int(m.N[cls]) // 2)                     # what the known keys leave holds n
    rng = np.random.default_rng(2)
    for kn in (None, np.sort(keys[scores == value][rng.random(int(m.N[cls])) < 0.3])):
        s, k = scan_ref.top(scores, keys, n, kn)
        np.testing.assert_array_equal(pl.first_keys(m, cls, n, kn), k[:n])
        assert (s[:n] == value).all()


@pytest.mark.parametrize("P,B,E", [(90, 3, 16), (120, 1, 20)])
def test_top_reference_is_the_top_of_all_triples(P, B, E):
    m = small_model(P, B, E)
    per, keys = all_triples(m)
    known = known_of(m, keys)
    n = 64
    cases = [("mean", None, scan_ref.prefix_mean(per, B))]
    if B > 1:
        srt = np.sort(per, axis=0)
        cases += [("quorum", 2, srt[B - 2]), ("spread", 0, srt[-1] - srt[0])]
    for what, arg, values in cases:
        for kn in (None, known):
            s, k = pl.top_reference(m, n, what, arg, kn)
            ws, wk = scan_ref.top(values, keys, n, kn)
            np.testing.assert_array_equal(k, wk[:n])
            np.testing.assert_allclose(s, ws[:n], rtol=0, atol=2e-9)


@pytest.mark.parametrize("P", [33, 90, 203])
def test_confined_mask_against_the_bool_matrix_packer(P):
    rng = np.random.default_rng(P)
    universe = np.unique(np.concatenate([[0, 31, 32, P - 1], rng.choice(P, P // 3, replace=False)]))
    blocked = [(universe[0], universe[3]), (universe[2], universe[-1]), (universe[1], universe[2])]
    sel = np.ones((P, P), dtype=bool)
    sel[np.ix_(universe, universe)] = False
    for i, j in blocked:
        sel[i, j] = True
    got = pl.confined_mask(P, universe, blocked)
    want = masked_ref.position_mask(P, sel)
    assert got.dtype == np.uint32 and got.shape == masked_ref.shape(P)
    np.testing.assert_array_equal(got, want)


# ------------------------------------------------------------------ what test_gpu_scale.py relies on
def test_scale_models_hold_their_preconditions():
    """The seeds of planted_ref.SCALE_SEEDS give lists of 64 and 4096 whose order is determined and
    whose last entry lies above everything a triple with a common gene can reach; the counts pass
    2^32; the known keys hold one work item's 100,000 and the best elites."""
    active = pl.SCALE_ACTIVE
    m = pl.scale_model("mean")
    assert m.P == 3001 and comb(m.P, 3) == 4499999500 > 2 ** 32 and m.B == 8
    sizes = np.sort(np.bincount(m.label, minlength=m.Kc + 1)[:m.Kc])
    assert 150 <= sizes[0] <= sizes[1] <= 250 and sizes[2] > 300
    stats = [pl.stat(m, ns=active), pl.stat(m, sample=0)]
    known = pl.scale_known(m, stats)
    assert known.size >= 299000 and (np.diff(known) > 0).all()
    a, b, _ = pl.positions(known, m.P)
    item = (a == pl.ITEM_A) & (b // 64 == pl.item_block(m.P) // 64)
    assert item.sum() >= 100000
    for st in stats:
        assert np.isin(m.keys[np.argsort(-st, kind="stable")[:50]], known).all()
    kind = pl.classify(m, known)[0]
    assert all((kind == k).sum() >= 50 for k in (0, 1, 2))
    for which in ("all", "known", "sample"):               # the lists of tests/test_gpu_scale.py
        for n in (64, 4096):
            for P in (3001, 6007):
                mm = pl.scale_model("mean", P)
                kn, _, kw = pl.scale_case(mm, which)
                pl.top_reference(mm, n, "mean", None, kn, **kw)
            for q in ((1,) if which == "sample" else (1, 3, 5)):
                mq = pl.scale_model("quorum")
                kn, _, kw = pl.scale_case(mq, which, "quorum", q)
                pl.top_reference(mq, n, "quorum", q, kn, **kw)
            for trim in (() if which == "sample" else (0, 1)):
                ms = pl.scale_model("spread")
                kn, _, kw = pl.scale_case(ms, which, "spread", trim)
                pl.top_reference(ms, n, "spread", trim, kn, **kw)
    for mode in (dict(ns=active), dict(sample=0)):
        t = pl.thresholds(m, **mode)
        counts, total = pl.census(m, t, known, **mode)
        assert total == comb(m.P, 3) - known.size and counts[0] == total
        assert counts[0] > 2 ** 32 > counts[2] > 2 ** 31 and counts[-1] > 0  # past 2^32, and past 2^31 in the common band
    mid, high = pl.vote_thresholds(m)
    hist = pl.votes(m, mid, active, known)
    assert (hist > 0).all() and hist.sum() == comb(m.P, 3) - known.size
    assert pl.votes(m, high, active, known)[0] > 2 ** 32             # one histogram bin past 2^32


def test_partner_lists_hold_their_preconditions():
    """tests/test_gpu_scale_partners.py: the elite queries' lists of 8 and 1024 under every statistic
    it runs, and the common query's tie; at P = 3001 the elite list equals tests/partners_ref.py on
    the full theta (at P = 6007 that numpy reference takes five seconds of CPU time a query)."""
    import partners_ref
    active, sample = pl.SCALE_ACTIVE, pl.SCALE_SAMPLE
    for P, ns in ((pl.SMALL_P, (8, 64)), (6007, (8, 1024))):
        m = pl.scale_model("mean", P)
        common = np.flatnonzero(m.label < m.Kc)
        for n in ns:
            for q in (int(m.elite_pos[0]), int(m.elite_pos[m.E // 2]), int(m.elite_pos[-1])):
                pl.partner_elite_list(m, q, n, sample=sample)
                pl.partner_elite_list(m, q, n, ns=active)
                pl.partner_elite_list(m, q, n, "quorum", (active + 1) // 2, ns=active)
                pl.partner_elite_list(m, q, n, "spread", 0, ns=active)
        for n in (8, ns[-1]) if P != pl.SMALL_P else (8,):
            pl.partner_common_list(m, int(common[common.size // 2]), n, ns=active)
            pl.partner_common_list(m, int(common[common.size // 2]), n, sample=sample)
    m = pl.scale_model("mean", 3001)
    order, _ = scan_ref.rank_tables(3001)
    q = int(m.elite_pos[m.E // 2])
    s, k = pl.partner_elite_list(m, q, 1024, sample=sample)
    ws, wids, gap = partners_ref.want_list(m.theta[sample], m.pr[sample], int(order[q]), 1024)
    assert gap > 1e-9
    np.testing.assert_array_equal(scan_ref.keys_to_ids(k, 3001), wids)
    np.testing.assert_allclose(s, ws, rtol=scan_ref.RTOL, atol=0)
    assert pl.partner_plan(6007, 1, 256) == (1024, 2) and pl.partner_plan(6007, 3, 256) == (683, 2)
    assert pl.partner_plan(6007, 100, 256) == (21, 1) and pl.partner_plan(20, 1, 256) == (4, 1)


@pytest.mark.parametrize("K,P,B", pl.CONFINED_CASES)
def test_confined_cases_hold_their_preconditions(K, P, B):
    """tests/test_gpu_scale_masked.py: the universe and its mask, and on the reference alone the
    gaps of every list of 64, a determined cut above the scan's cap and hits at two votes."""
    import quorum_ref
    import spread_ref
    th, pr, U, mask, per, keys = pl.confined_case(K, P, B)
    edge = 1 << (int(P - 1).bit_length() - 1)
    assert U.size == pl.CONFINED_UNIVERSE and {0, 31, 32, 63, 64, edge - 1, edge, P - 1} <= set(U.tolist())
    assert mask.shape == masked_ref.shape(P) and (mask[P:] == 0).all()
    inside = np.zeros(P, dtype=bool)
    inside[U] = True
    rng = np.random.default_rng(0)
    x, y = rng.integers(0, P, 4000), rng.integers(0, P, 4000)
    x, y = x[x != y], y[x != y]
    outside = ~(inside[x] & inside[y])
    assert (masked_ref.bit(mask, x, y)[outside] == 1).all()         # every pair that leaves the universe
    ux, uy = np.triu_indices(U.size, k=1)
    assert masked_ref.bit(mask, U[ux], U[uy]).sum() == 5             # inside it, the five blocked pairs
    assert not pl.blocked_keys(keys, mask, P).any()
    if P <= 203:                                        # the bool-matrix packer and a loop over every triple
        sel = np.ones((P, P), dtype=bool)
        sel[np.ix_(U, U)] = False
        for i, j in ((0, P - 1), (edge - 1, edge), (31, 32), (U[20], U[150]), (U[77], U[78])):
            sel[i, j] = True
        np.testing.assert_array_equal(mask, masked_ref.position_mask(P, sel))
        every = masked_ref.all_keys(P)
        np.testing.assert_array_equal(keys, every[~masked_ref.blocked(every, mask, P)])
    mean = scan_ref.prefix_mean(per, B)
    t = census_ref.gap_thresholds(mean, 5)
    census_ref.assert_clear(mean, t)
    scan_ref.assert_gaps(scan_ref.top(mean, keys, 64)[0])
    assert 4096 < pl.any_length(mean, keys, 4096) <= 4096 + 1500
    for m in sorted({1, (B + 1) // 2, B}):
        quorum_ref.ref_top(per, keys, m, 64)
    spread_ref.ref_top(per, keys, 0, 64)
    thr = votes_ref.at_quantile(per, votes_ref.clear_thresholds(per, 33), 0.9)
    assert votes_ref.ref_votes(per, keys, thr)[3][2] > 0
    a, b, c = pl.positions(keys, P)
    for q in (int(U[0]), int(U[U.size // 2]), int(U[-1])):
        has = (a == q) | (b == q) | (c == q)
        scan_ref.assert_gaps(scan_ref.top(mean[has], keys[has], 64)[0])
