"""Threshold scan (include/mmsbm.h mmsbm_scan_above, EMEngine.scan_above / scan_top_any,
Model.predict_network / predict_novel_any, the scan driver's --network) against the numpy float64
reference scorer of tests/census_ref.py over all C(P, 3) triples.

Lists of thousands have adjacent scores closer than any tolerance, so the reference check is free of
order: a threshold is first shown, on the reference alone, to lie more than 1e-7 relative from every
reference score (census_ref.assert_clear); then the SET of returned keys must equal the reference's
and every returned score must lie within RTOL = 1e-9 of the reference score of its key.  The order
is checked on the product's own values (score descending, equal scores by key ascending) and, bit
for bit, against the product's other kernels: the census's counts and the scan's top-N list.
"""
import ctypes
import os
from math import comb

import numpy as np
import pytest

import census_ref as ref
import scan_gpu
import scan_ref
from golden_util import GOLDEN, load
from scan_gpu import engine, random_case
from scan_ref import packed

pytestmark = pytest.mark.gpu


def assert_list_properties(s, ids, P):
    """The list itself: dtypes, unique keys, the scan's total order, ids = keys_to_ids(keys)."""
    assert s.dtype == np.float64 and ids.dtype == np.int32
    assert s.ndim == 1 and ids.shape == (s.size, 3)
    keys = packed(ids, P)
    assert np.unique(keys).size == keys.size
    assert (np.diff(s) <= 0).all()                                   # scores do not increase
    assert (np.diff(keys)[np.diff(s) == 0] > 0).all()                # equal scores: keys increase
    np.testing.assert_array_equal(ids, scan_ref.keys_to_ids(keys, P))    # key order, no slot swapped
    return keys


def thresholds_of(scores, n=3):
    """Below every score, above every score and up to n mid-distribution gap thresholds."""
    return np.unique(ref.gap_thresholds(scores, n))


def check(eng, scores, keys, thresholds, known=None, sample=0):
    """The precondition on the reference alone; then, per threshold, the reference set, each score
    against the reference score of its key, the list's own order, and the census's count."""
    P = eng.P
    ref.assert_clear(scores, thresholds)
    counts, _ = eng.census(thresholds, known, sample=sample)
    out = []
    for t, count in zip(thresholds, counts):
        s, ids = eng.scan_above(t, known, sample=sample)
        got = assert_list_properties(s, ids, P)
        assert s.size == count                                       # the census, exactly
        want = scores >= t
        if known is not None and len(known):
            want &= ~np.isin(keys, known)
        np.testing.assert_array_equal(np.sort(got), keys[want])
        np.testing.assert_allclose(s, scores[np.searchsorted(keys, got)], rtol=scan_ref.RTOL, atol=0)
        assert (s >= t).all()
        out.append((s, ids))
    return out


# ------------------------------------------------------------------ 1., 2. shapes and the list
@pytest.mark.parametrize("P", [0, 1, 2, 3, 4, 15, 16, 17, 33, 65, 70])
def test_gene_counts(P):
    """Every tile edge, one and several row blocks, an empty triangle.  P = 0 is no shape of the
    engine (mmsbm_set_shape refuses P < 1): the case asserts that refusal."""
    from trigenicinteractionpredictor_amd import _lib
    if P == 0:
        from trigenicinteractionpredictor_amd.engine import EMEngine
        with pytest.raises(_lib.MMSBMError) as e:
            EMEngine(3, 0)
        assert e.value.code == _lib.MMSBM_ERR_INVALID
        return
    theta, pr, scores, keys = random_case(3, P, 11 + P)
    eng = engine(theta[None], pr[None])
    if P < 3:
        for t in (1e-300, 0.5):
            s, ids = eng.scan_above(t)
            assert s.shape == (0,) and ids.shape == (0, 3) and s.dtype == np.float64 and ids.dtype == np.int32
    else:
        thresholds = thresholds_of(scores)
        lists = check(eng, scores, keys, thresholds)
        assert lists[0][0].size == comb(P, 3)           # below all: every lane of every tile appends
        assert lists[-1][0].size == 0                   # above all
        if P >= 15:                                     # at least three in mid-distribution
            assert len(thresholds) >= 5 and all(0 < s.size < comb(P, 3) for s, _ in lists[1:-1])
    eng.close()


@pytest.mark.parametrize("K", [1, 4, 5, 10, 13, 32])
def test_group_counts(K):
    """KS = 1, 2, 3, 4 and 8, and K that is no multiple of 4 (K = 1: every score the same)."""
    P = 40
    theta, pr, scores, keys = random_case(K, P, 100 + K)
    eng = engine(theta[None], pr[None])
    thresholds = thresholds_of(scores)
    lists = check(eng, scores, keys, thresholds)
    assert lists[0][0].size == comb(P, 3) and lists[-1][0].size == 0
    if K > 1:
        assert len(thresholds) >= 5 and all(0 < s.size < comb(P, 3) for s, _ in lists[1:-1])
    eng.close()


# ------------------------------------------------------------------ 3. the family's bits
@pytest.mark.parametrize("mode", ["sample", "ensemble"])
def test_list_starts_with_the_scan_list_bit_for_bit(mode):
    """Product against product, no tolerance: with t the last score of scan_top(n), the first n
    rows of scan_above(t) are that list and its length is the census's count at t."""
    K, P = 10, 33
    th, pr = scan_ref.random_params(K, P, 31, B=3)
    eng = engine(th, pr)
    sample = 1 if mode == "sample" else None
    known = random_case(K, P, 32)[3][::4].copy()
    for kn in (None, known):
        for n in (1, 16, 500):
            s, ids = eng.scan_top(n, kn, sample=sample)
            assert s.size == n
            s2, ids2 = eng.scan_above(s[-1], kn, sample=sample)
            assert_list_properties(s2, ids2, P)
            counts, _ = eng.census([s[-1]], kn, sample=sample)
            assert s2.size == counts[0] >= n
            np.testing.assert_array_equal(ids2[:n], ids)
            assert s2[:n].tobytes() == s.tobytes()
            assert (s2[n:] == s[-1]).all()                          # what follows ties with the last
    eng.close()


# ------------------------------------------------------------------ 4. exclusion
def test_exclusion():
    K, P = 3, 70
    theta, pr, scores, keys = random_case(K, P, 51)
    thresholds = thresholds_of(scores)
    eng = engine(theta[None], pr[None])
    a, b, c = keys // (P * P), (keys // P) % P, keys % P
    pick = np.random.default_rng(5).random(keys.size) < 0.3
    pick |= a == 5                                      # whole rows of one a
    pick |= (b >= 64) & (c >= 64)                       # the last tile
    pick |= (a == 20) & (b == 21)                       # one whole row b
    known = keys[pick].copy()
    assert known.size >= 0.3 * keys.size
    for s, ids in check(eng, scores, keys, thresholds, known):
        assert not np.isin(packed(ids, P), known).any()
    # keys of no triple are ignored
    junk = np.unique(np.concatenate([known, [(5 * P + 5) * P + 9, (9 * P + 4) * P + 2, P ** 3 + 7]]))
    check(eng, scores, keys, thresholds, junk)
    # everything known: nothing is left at any threshold
    s, ids = eng.scan_above(float(thresholds[0]), keys.copy())
    assert s.size == 0 and ids.shape == (0, 3)
    eng.close()


# ------------------------------------------------------------------ 5. ensemble and slots
def test_ensemble_and_slots():
    K, P = 10, 40
    th, pr = scan_ref.random_params(K, P, 41, B=3)
    per = [scan_ref.ref_scores(th[b], pr[b]) for b in range(3)]
    keys = per[0][1]
    known = keys[1::5].copy()
    eng = engine(th, pr)
    mean3 = ((per[0][0] + per[1][0]) + per[2][0]) / 3              # added in slot order
    check(eng, mean3, keys, thresholds_of(mean3), known, sample=None)
    # one slot is bitwise what a B = 1 engine holding its parameters gives
    t = float(thresholds_of(per[1][0])[2])
    s, ids = eng.scan_above(t, known, sample=1)
    solo = engine(th[1:2], pr[1:2])
    for sample in (0, None):                                        # an ensemble of one is that sample
        s1, ids1 = solo.scan_above(t, known, sample=sample)
        np.testing.assert_array_equal(ids1, ids)
        assert s1.tobytes() == s.tobytes() and s.size > 0
    solo.close()
    # a shrunken active prefix means over 2
    eng.set_active(2)
    mean2 = (per[0][0] + per[1][0]) / 2
    check(eng, mean2, keys, thresholds_of(mean2), known, sample=None)
    eng.close()


# ------------------------------------------------------------------ 6. grid
def test_the_sorted_list_does_not_depend_on_the_grid(monkeypatch):
    K, P = 3, 65
    theta, pr, scores, keys = random_case(K, P, 61)
    t = float(np.quantile(scores, 0.9))                             # about 10 % hits
    eng = engine(theta[None], pr[None])
    known = keys[2::7].copy()
    want_s, want_ids = eng.scan_above(t, known)
    assert 0.05 * keys.size < want_s.size < 0.15 * keys.size
    for grid in ("1", "7"):
        monkeypatch.setenv("MMSBM_SCAN_ABOVE_GRID", grid)
        s, ids = eng.scan_above(t, known)
        assert s.tobytes() == want_s.tobytes() and ids.tobytes() == want_ids.tobytes()
    monkeypatch.delenv("MMSBM_SCAN_ABOVE_GRID")
    s, ids = eng.scan_above(t, known)                                # a repeated call
    assert s.tobytes() == want_s.tobytes() and ids.tobytes() == want_ids.tobytes()
    eng.close()


# ------------------------------------------------------------------ 7. the C call
SENTINEL_ROWS = 64
SENTINEL_SCORE, SENTINEL_KEY = -7.0, -7


def above_call(raw, threshold, capacity, null=False, sample=0, known=None, ws_ptr=None, ws_bytes=None, rows=None):
    """mmsbm_scan_above as C sees it (scan_gpu.Raw), its outputs with SENTINEL_ROWS sentinel rows
    behind `capacity`: -> (return code, scores, keys, count)."""
    torch = raw.torch
    rows = max(capacity, 0) if rows is None else rows
    scores = raw.full((rows + SENTINEL_ROWS,), torch.float64, SENTINEL_SCORE)
    keys = raw.full((rows + SENTINEL_ROWS,), torch.int64, SENTINEL_KEY)
    count = raw.full((1,), torch.int64, -1)
    ws = (raw.ws.data_ptr() if ws_ptr is None else ws_ptr, raw.ws.numel() if ws_bytes is None else ws_bytes)
    rc = raw.call((float(threshold), capacity), [None if null else scores, None if null else keys, count],
                  sample, known, ws=ws)
    return rc, scores.cpu().numpy(), keys.cpu().numpy(), int(count.cpu()[0])


def test_c_call_and_its_capacity_guard():
    K, P = 5, 40
    theta, pr, scores, keys = random_case(K, P, 71)
    eng = engine(theta[None], pr[None])
    t = float(np.quantile(scores, 0.7))                             # about 30 % hits
    want_s, want_ids = eng.scan_above(t)
    want = dict(zip(packed(want_ids, P).tolist(), want_s.tolist()))
    count = len(want)
    assert count > 1000 and count == eng.census([t])[0][0]
    raw = scan_gpu.Raw(eng, "scan_above")
    # (a) capacity = count: the whole set, the sentinels intact
    rc, s, k, n = above_call(raw, t, count)
    assert rc == 0 and n == count
    assert dict(zip(k[:count].tolist(), s[:count].tolist())) == want
    assert (s[count:] == SENTINEL_SCORE).all() and (k[count:] == SENTINEL_KEY).all()
    # (b) capacity = count // 3: the full count, distinct members of the set, the sentinels intact
    cap = count // 3
    rc, s, k, n = above_call(raw, t, cap)
    assert rc == 0 and n == count
    assert np.unique(k[:cap]).size == cap
    assert all(want.get(key) == score for key, score in zip(k[:cap].tolist(), s[:cap].tolist()))
    assert (s[cap:] == SENTINEL_SCORE).all() and (k[cap:] == SENTINEL_KEY).all()
    # (c) capacity = 0 with null arrays: the count alone
    rc, _, _, n = above_call(raw, t, 0, null=True)
    assert rc == 0 and n == count
    # capacity = 0 with arrays: nothing is written
    rc, s, k, n = above_call(raw, t, 0)
    assert rc == 0 and n == count and (s == SENTINEL_SCORE).all() and (k == SENTINEL_KEY).all()
    # (d) the same workspace again, at another threshold and back: the cursor starts from zero
    t2 = float(np.quantile(scores, 0.95))
    rc, _, _, n2 = above_call(raw, t2, 0, null=True)
    assert rc == 0 and n2 == eng.census([t2])[0][0] and 0 < n2 < count
    rc, _, _, n = above_call(raw, t, 0, null=True)
    assert rc == 0 and n == count
    # (e) a threshold above every score: nothing is written
    rc, s, k, n = above_call(raw, float(scores.max()) * 1.001, 0, rows=count)
    assert rc == 0 and n == 0 and (s == SENTINEL_SCORE).all() and (k == SENTINEL_KEY).all()
    rc, s, k, n = above_call(raw, float(scores.max()) * 1.001, count)
    assert rc == 0 and n == 0 and (s == SENTINEL_SCORE).all() and (k == SENTINEL_KEY).all()
    eng.close()


# ------------------------------------------------------------------ 8. refusals
def test_refusals_leave_the_context_usable():
    from trigenicinteractionpredictor_amd import _lib
    from trigenicinteractionpredictor_amd.scan import LimitError
    K, P = 5, 40
    theta, pr, scores, keys = random_case(K, P, 71)
    th3, pr3 = scan_ref.random_params(K, P, 72, B=3)
    eng = engine(th3, pr3)
    eng.set_active(2)
    raw = scan_gpu.Raw(eng, "scan_above")
    t = float(np.quantile(scores, 0.7))
    INVALID = _lib.MMSBM_ERR_INVALID
    for bad in (float("nan"), float("inf"), float("-inf")):
        with pytest.raises(ValueError):
            eng.scan_above(bad)
        with pytest.raises(ValueError):
            eng.scan_above_async(bad)
        assert above_call(raw, bad, 16)[0] == INVALID
    assert above_call(raw, t, -1, rows=16)[0] == INVALID                                   # negative capacity
    assert above_call(raw, t, 16, null=True)[0] == INVALID                                 # null arrays, capacity > 0
    assert above_call(raw, t, 16, ws_bytes=raw.ws.numel() - 1)[0] == INVALID               # too small
    assert above_call(raw, t, 16, ws_ptr=raw.ws.data_ptr() + 8, ws_bytes=raw.ws.numel() - 8)[0] == INVALID  # misaligned
    assert above_call(raw, t, 16, ws_ptr=0)[0] == INVALID                                  # missing
    for sample in (2, 3, -2):                                                       # outside the active prefix
        assert above_call(raw, t, 16, sample=sample)[0] == INVALID
    for sample in (2, 3, -1):
        with pytest.raises(ValueError):
            eng.scan_above(t, sample=sample)
    assert above_call(raw, t, 16, known=np.array([5, 3], dtype=np.int64)[:0])[0] == 0      # an empty table is none
    count = raw.full((1,), raw.torch.int64, -1)
    assert raw.call((t, 0), [None, None, count], n_known=3) == INVALID              # keys announced, none given
    with pytest.raises(ValueError):
        eng.scan_above(t, known=np.array([5, 3], dtype=np.int64))                   # unsorted
    with pytest.raises(ValueError):
        eng.scan_above(t, known=np.array([3, 3], dtype=np.int64))                   # repeated
    # null pointers
    nbytes = ctypes.c_int64()
    assert eng.lib.mmsbm_scan_above_workspace_bytes(None, ctypes.byref(nbytes)) == INVALID
    assert eng.lib.mmsbm_scan_above_workspace_bytes(eng.ctx, None) == INVALID
    assert raw.call((t, 0), [None, None, None]) == INVALID                          # no out_count
    # a limit below the count: the message holds the count, and nothing was launched for the list
    count = int(eng.census([t], sample=0)[0][0])
    assert count > 100
    with pytest.raises(ValueError, match=str(count)) as e:
        eng.scan_above(t, sample=0, limit=count - 1)
    assert isinstance(e.value, LimitError) and (e.value.count, e.value.limit) == (count, count - 1)
    # after all of it the context answers a valid call, through the C call and the binding
    rc, s, k, n = above_call(raw, t, count)
    assert rc == 0 and n == count
    s2, ids2 = eng.scan_above(t, sample=0, limit=count)
    assert s2.size == count and sorted(packed(ids2, P).tolist()) == sorted(k[:count].tolist())
    eng.close()


# ------------------------------------------------------------------ 9. scan_top_any
def test_scan_top_any():
    K, P = 5, 40
    theta, pr, scores, keys = random_case(K, P, 91)
    total = comb(P, 3)
    assert total == 9880
    eng = engine(theta[None], pr[None])
    assert eng.lib.mmsbm_scan_max_n() == 4096
    s, ids = eng.scan_top_any(100)
    s0, ids0 = eng.scan_top(100)
    assert s.tobytes() == s0.tobytes() and ids.tobytes() == ids0.tobytes()
    n = 5000
    s, ids = eng.scan_top_any(n)
    assert s.size == n
    got = assert_list_properties(s, ids, P)
    s0, ids0 = eng.scan_top(4096)
    assert s[:4096].tobytes() == s0.tobytes() and ids[:4096].tobytes() == ids0.tobytes()
    # against the reference, around its n-th score
    star = np.sort(scores)[::-1][n - 1]
    assert (np.abs(scores - star) <= 1e-7 * star).sum() <= 8        # the precondition, reference alone
    assert np.isin(keys[scores > star * (1 + 1e-7)], got).all()     # everything clearly above is listed
    assert (scores[np.searchsorted(keys, got)] >= star * (1 - 1e-7)).all()
    np.testing.assert_allclose(s, scores[np.searchsorted(keys, got)], rtol=scan_ref.RTOL, atol=0)
    # n above the eligible total: everything, with and without exclusion
    s, ids = eng.scan_top_any(20000)
    assert s.size == total
    assert_list_properties(s, ids, P)
    known = keys[::2].copy()
    s, ids = eng.scan_top_any(6000, known)
    assert s.size == total - known.size and not np.isin(packed(ids, P), known).any()
    s, ids = eng.scan_top_any(4500, known)
    assert s.size == 4500 and not np.isin(packed(ids, P), known).any()
    s0, _ = eng.scan_top(4096, known)
    assert s[:4096].tobytes() == s0.tobytes()
    with pytest.raises(ValueError):
        eng.scan_top_any(0)
    eng.close()


# ------------------------------------------------------------------ 10. Model and driver
@pytest.mark.parametrize("name", ["K2_s1", "K10_s1"])
def test_model_predict_network_and_novel_any(name):
    from trigenicinteractionpredictor_amd import Model
    _, vec, train, test = load("small", name)
    m = Model()
    m.get_traintest(train, test)
    m.initialize_parameters(vec["theta_5"].shape[1])
    m.theta, m.pr = vec["theta_5"].tolist(), vec["pr_5"].tolist()
    top = m.predict_novel(50)
    long = m.predict_novel(3000)
    t = long[-1][0]                                                  # a threshold that is a score
    rows = m.predict_network(t)
    counts, total = m.novel_census([t])
    assert len(rows) == counts[0] >= 3000
    assert rows[:50] == top and rows[:3000] == long
    probs = [r[0] for r in rows]
    assert probs == sorted(probs, reverse=True) and probs[-1] >= t
    for p, key, names in rows[::97]:
        assert key not in m.links and key not in m.test_links
        assert names == sorted(m.id_gene[int(g)] for g in key.split("_"))
    with pytest.raises(ValueError, match=str(int(counts[0]))):
        m.predict_network(t, limit=100)
    # without exclusion the measured triples may come back
    assert len(m.predict_network(t, exclude=())) >= len(rows)
    # predict_novel without the cap
    assert m.predict_novel_any(50) == top
    any5000 = m.predict_novel_any(5000)
    assert len(any5000) == 5000 and any5000[:3000] == long
    assert [r[0] for r in any5000] == sorted((r[0] for r in any5000), reverse=True)
    assert len({r[1] for r in any5000}) == 5000


def test_driver_writes_the_network_table(tmp_path):
    from trigenicinteractionpredictor_amd import scan
    g = os.path.join(GOLDEN, "small")
    base = ["-t", os.path.join(g, "train.dat"), "-e", os.path.join(g, "test.dat"), "-k", "3", "-n", "2", "-i", "5",
            "--seed", "1", "--top", "10"]

    def census_rows(path):
        lines = open(path, encoding="utf-8").read().rstrip("\n").split("\n")
        return [(float(ln.split("\t")[0]), int(ln.split("\t")[1])) for ln in lines[2:]]

    # a first run finds a threshold with a list of modest length: the smallest census count >= 100
    grid = ",".join("%.2f" % v for v in np.arange(99, 0, -1) / 100)
    files = [str(tmp_path / f) for f in ("top0.tsv", "census0.tsv")]
    assert scan.main(base + ["-o", files[0], "--census", files[1], "--thresholds", grid], out=lambda *a: None) == 0
    T, want = min((row for row in census_rows(files[1]) if row[1] >= 100), key=lambda row: row[1])
    # the run under test
    files = [str(tmp_path / f) for f in ("top.tsv", "census.tsv", "network.tsv")]
    rc = scan.main(base + ["-o", files[0], "--census", files[1], "--thresholds", repr(T), "--network", files[2],
                           "--network-threshold", repr(T)], out=lambda *a: None)
    assert rc == 0
    assert census_rows(files[1]) == [(T, want)]
    top, net = (open(f, encoding="utf-8").read().rstrip("\n").split("\n") for f in (files[0], files[2]))
    assert net[0].split("\t") == ["rank", "probability", "ids", "names"]
    rows = [ln.split("\t") for ln in net[1:]]
    assert len(rows) == want
    assert [int(r[0]) for r in rows] == list(range(1, want + 1))
    probs = [float(r[1]) for r in rows]
    assert probs == sorted(probs, reverse=True) and probs[-1] >= T
    assert all(len(r) == 4 and len(r[2].split("_")) == 3 and len(r[3].split("_")) == 3 for r in rows)
    assert len({r[2] for r in rows}) == want
    assert net[:11] == top[:11]                                      # the main table is its head
    # a count above --network-limit is refused, with the count, before anything is written
    out = str(tmp_path / "refused.tsv")
    rc = scan.main(base + ["-o", out, "--network", str(tmp_path / "refused.net.tsv"), "--network-threshold", repr(T),
                           "--network-limit", str(want - 1)], out=lambda *a: None)
    assert rc == 2 and not os.path.exists(out) and not os.path.exists(str(tmp_path / "refused.net.tsv"))
