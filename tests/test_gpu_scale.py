"""The triangle-sweep scan families at genome scale (P = 3001, and 6007 for the top-N scan) against
the closed forms of tests/planted_ref.py: counts past 2^32, one work item with 100,000 known keys,
top-N lists whose winners sit wherever the elites were planted and lists in which every candidate
ties.  The planted model's answers are exact (counts, keys) or come from a brute-force list of its
C(96, 3) elite triples (scores, at scan_ref.RTOL); tests/test_planted_host.py holds the closed forms
to the all-triples references and asserts every precondition used here.  Each case also runs at
P = 90, where planted_ref's ref_* functions form the same answer from all C(P, 3) scores as well.
The pair matrices are in tests/test_gpu_scale_pairs.py."""
from math import comb

import numpy as np
import pytest

import planted_ref as pl
import scan_gpu
import scan_ref
from scan_gpu import check_list, known_of, planted_engine
from scan_ref import packed

pytestmark = pytest.mark.gpu

ACTIVE = pl.SCALE_ACTIVE
MODES = {"single": dict(sample=0), "prefix": dict(ns=ACTIVE)}


# ------------------------------------------------------------------ 1. counts past 2^32
SENTINEL_ROWS = 64


def above_call(raw, threshold, capacity, known):
    """mmsbm_scan_above as C sees it, SENTINEL_ROWS sentinel rows behind `capacity`."""
    torch = raw.torch
    scores = raw.full((capacity + SENTINEL_ROWS,), torch.float64, float(scan_gpu.SENTINEL))
    keys = raw.full((capacity + SENTINEL_ROWS,), torch.int64, scan_gpu.SENTINEL)
    count = raw.full((1,), torch.int64, -1)
    rc = raw.call((float(threshold), capacity), [scores, keys, count], -1, known)
    return rc, scores.cpu().numpy(), keys.cpu().numpy(), int(count.cpu()[0])


@pytest.mark.parametrize("with_known", [False, True], ids=["all", "known"])
@pytest.mark.parametrize("mode", ["single", "prefix"])
@pytest.mark.parametrize("P", [pl.SMALL_P, 3001])
def test_counts(P, mode, with_known):
    """The census, the vote histogram and the threshold scan's count: int64 and exact.  At P = 3001
    the threshold below everything counts C(P, 3) - n_known = 4,499,999,500 - n_known > 2^32
    triples, and with the known keys one work item skips 100,000 of them."""
    m = pl.scale_model("mean", P)
    kw = MODES[mode]
    ns = 1 if mode == "single" else ACTIVE
    known = known_of(m, with_known)
    eng = planted_engine(m, mode)
    n_known = 0 if known is None else known.size
    # the census at thresholds of both bands, between them and below everything
    t = pl.thresholds(m, **kw)
    want, total = pl.ref_census(m, t, known, **kw)
    counts, eligible = eng.census(t, known)
    assert counts.dtype == np.int64
    np.testing.assert_array_equal(counts, want)
    assert eligible == total == comb(P, 3) - n_known == counts[0]
    if P == 3001:
        assert total > 2 ** 32 and (want[1:] < 2 ** 32).all() and want[2] > 2 ** 31
    # the vote histogram at two common-band thresholds: every bin filled; one bin past 2^32
    for thr in pl.vote_thresholds(m):
        want_hist = pl.ref_votes(m, thr, ns, known)
        hist = eng.vote_census(thr, known)
        assert hist.dtype == np.int64
        np.testing.assert_array_equal(hist, want_hist)
        assert hist.sum() == total
    if P == 3001:
        assert want_hist[0] > 2 ** 32
    # the threshold scan below everything with room for 1000 rows: the full count, exactly 1000
    # rows written, every one an eligible triple with the score its class or the elite list gives
    cap = 1000
    raw = scan_gpu.Raw(eng, "scan_above")
    rc, s, k, n = above_call(raw, pl.BELOW_ALL, cap, known)
    assert rc == 0 and n == total
    assert (s[cap:] == scan_gpu.SENTINEL).all() and (k[cap:] == scan_gpu.SENTINEL).all()
    s, k = s[:cap], k[:cap]
    assert np.unique(k).size == cap
    a, b, c = pl.positions(k, P)
    assert ((0 <= a) & (a < b) & (b < c) & (c < P)).all()
    if known is not None:
        assert not np.isin(k, known).any()
    kind = pl.classify(m, k)[0]
    ref = pl.key_values(m, k, pl.class_values(m, **kw), pl.elite_values(m, **kw))
    assert s[kind == 0].tobytes() == ref[kind == 0].tobytes()               # a class value: bit for bit
    np.testing.assert_allclose(s[kind == 2], ref[kind == 2], rtol=scan_ref.RTOL, atol=0)
    assert ((s[kind == 1] > pl.BELOW_ALL) & (s[kind == 1] <= pl.MIXED_TOP)).all()
    eng.close()


# ------------------------------------------------------------------ 2. top-N lists
LISTS = [(pl.SMALL_P, 64), (3001, 64), (3001, 4096)]
VARIANTS = ["all", "known", "sample"]


@pytest.mark.parametrize("which", VARIANTS)
@pytest.mark.parametrize("P,n", LISTS + [(6007, 64), (6007, 4096)])
def test_scan_top(P, n, which):
    """The winners are the planted elites: at positions 0, 1, 15..17, the block edges, P - 2, P - 1,
    the ragged last tile and in between, so the pruning bound is live from the first item on and the
    last items of the triangle still have to enter the list."""
    m = pl.scale_model("mean", P)
    known, sample, kw = pl.scale_case(m, which)
    eng = planted_engine(m)
    check_list(eng.scan_top(n, known, sample=sample), pl.ref_top(m, n, "mean", None, known, **kw), P)
    eng.close()


@pytest.mark.parametrize("which", VARIANTS)
@pytest.mark.parametrize("P,n", LISTS)
def test_quorum_top(P, n, which):
    m = pl.scale_model("quorum", P)
    eng = planted_engine(m)
    for votes in ((1,) if which == "sample" else (1, (ACTIVE + 1) // 2, ACTIVE)):
        known, sample, kw = pl.scale_case(m, which, "quorum", votes)
        want = pl.ref_top(m, n, "quorum", votes, known, **kw)
        check_list(eng.quorum_top(n, votes, known, sample=sample), want, P)
    eng.close()


@pytest.mark.parametrize("which", VARIANTS[:2])
@pytest.mark.parametrize("P,n", LISTS)
def test_spread_top(P, n, which):
    """A spread is one subtraction of two slot scores, each within RTOL relative and below 1: the
    bound is 2 RTOL absolute (tests/spread_ref.py)."""
    m = pl.scale_model("spread", P)
    eng = planted_engine(m)
    for trim in (0, 1):
        known, _, kw = pl.scale_case(m, which, "spread", trim)
        want = pl.ref_top(m, n, "spread", trim, known, **kw)
        check_list(eng.spread_top(n, trim, known), want, P, atol=2 * scan_ref.RTOL)
    eng.close()


@pytest.mark.parametrize("P,n", [(pl.SMALL_P, 16), (3001, 4096)])
def test_a_list_in_which_every_candidate_ties(P, n):
    """An all-common model: the best class holds more than 10^7 triples with one score, bit for bit,
    so the top n are that class's first n keys: the key tie-break decides every row.  With known
    keys that take every third of them, the next ones move up."""
    small = P == pl.SMALL_P
    m = pl.build(P, B=pl.SCALE_SLOTS, E=0, seed=11, small=6 if small else 200, best=(3, 4, 5))
    cls, value = pl.best_class(m, ns=ACTIVE)
    assert cls == (3, 4, 5) and (small or m.N[cls] > 10 ** 7) and m.N[cls] >= 2 * n
    others = np.sort(pl.class_values(m, ns=ACTIVE).reshape(-1))
    assert others[-1] == value and others[-2] < value * (1 - 1e-6)
    eng = planted_engine(m)
    first = pl.first_keys(m, cls, 2 * n)
    for known in (None, first[::3].copy()):
        want_k = pl.first_keys(m, cls, n, known)
        if small:
            values, keys = pl.brute_stat(m, ns=ACTIVE)
            np.testing.assert_array_equal(scan_ref.top(values, keys, n, known)[1][:n], want_k)
        s, ids = eng.scan_top(n, known)
        np.testing.assert_array_equal(ids, scan_ref.keys_to_ids(want_k, P))
        assert s.tobytes() == np.full(n, value).tobytes()                # the ensemble mean's bits
        s, ids = eng.quorum_top(n, (ACTIVE + 1) // 2, known)
        np.testing.assert_array_equal(ids, scan_ref.keys_to_ids(want_k, P))
        assert s.tobytes() == np.full(n, m.cv[0][cls]).tobytes()         # one slot's own bits
    eng.close()


@pytest.mark.parametrize("P,n", [(pl.SMALL_P, 300), (3001, 6000)])
def test_scan_top_any_brackets_past_the_list_cap(P, n):
    """n above mmsbm_scan_max_n(): censuses bracket a threshold (their counts run from the list's
    cap to the 4.5e9 eligible triples), scan_above fetches and the list is cut.  Lists this long
    have neighbours closer than any tolerance, so beyond the gap at the cut (asserted on the
    reference) the check is free of order: the set of keys, each score against its key's, and the
    order on the product's own values."""
    m = pl.scale_model("mean", P)
    eng = planted_engine(m)
    if P == 3001:
        assert n > int(eng.lib.mmsbm_scan_max_n())
    values = pl.stat(m, ns=ACTIVE)
    want_s, want_k = scan_ref.top(values, m.keys, n)
    assert want_s.size == n + 1 and (want_s[n - 1] - want_s[n]) > 1e-7 * want_s[n - 1] and want_s[n] > pl.COMMON_HI
    if P == pl.SMALL_P:
        bv, bk = pl.brute_stat(m, ns=ACTIVE)
        np.testing.assert_array_equal(np.sort(scan_ref.top(bv, bk, n)[1][:n]), np.sort(want_k[:n]))
    s, ids = eng.scan_top_any(n)
    keys = packed(ids, P)
    assert s.size == n and (np.diff(s) <= 0).all() and (np.diff(keys)[np.diff(s) == 0] > 0).all()
    np.testing.assert_array_equal(ids, scan_ref.keys_to_ids(keys, P))
    np.testing.assert_array_equal(np.sort(keys), np.sort(want_k[:n]))
    at = np.searchsorted(m.keys, keys)
    np.testing.assert_allclose(s, values[at], rtol=scan_ref.RTOL, atol=0)
    eng.close()
