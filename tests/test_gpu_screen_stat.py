"""Screen statistics (include/mmsbm.h mmsbm_screen_stat_topn / mmsbm_screen_stat_scores,
EMEngine.screen_quorum_* / screen_spread_*, the scan driver's --screen-quorum / --screen-disputed)
against the slots' own rows and a numpy reference (tests/screen_stat_ref.py).

A quorum score is one slot's word and a spread one IEEE subtraction of two, so the rows are compared
bit for bit with what numpy forms from screen_scores(sample=s), and a list with the lexsort of the
call's own row: no tolerance is involved.  Only the comparison with the independent reference
(screen_ref.ref_row) has one, which follows from RTOL: an order statistic is 1-Lipschitz in the sup
norm over the slots.
"""
import ctypes
import os
import random

import numpy as np
import pytest

import converged_ref
import scan_ref
import screen_ref
import screen_stat_ref as ref
from golden_util import GOLDEN
from scan_gpu import SENTINEL
from scan_ref import bits

pytestmark = pytest.mark.gpu

RTOL = scan_ref.RTOL
Q = 17      # two query tiles of 16, the second ragged


def params(K, P, B, seed, R=2):
    rng = np.random.default_rng(seed)
    th = rng.random((B, P, K))
    th /= th.sum(axis=2, keepdims=True)
    pr = rng.random((B, K, K, K, R))
    pr /= pr.sum(axis=4, keepdims=True)
    return th, pr


def make_engine(th, pr, active=None):
    from trigenicinteractionpredictor_amd.engine import EMEngine
    B, P, K = th.shape
    eng = EMEngine(K, P, B=B, R=pr.shape[-1])
    eng.upload(th, pr)
    if active is not None:
        eng.set_active(active)
    return eng


def to_ids(P, position_pairs):
    order, _ = scan_ref.rank_tables(P)
    return order[np.asarray(position_pairs, dtype=np.int64).reshape(-1, 2)].astype(np.int32)


def rank_rows(P, rows):
    """[Q][gene id] -> [Q][rank position]."""
    order, _ = scan_ref.rank_tables(P)
    return rows[:, order]


def csr(slices):
    off = np.zeros(len(slices) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(s) for s in slices])
    flat = np.concatenate([np.asarray(s, dtype=np.int32) for s in slices]) if slices else np.zeros(0, np.int32)
    return off, flat.astype(np.int32)


def queries(P, seed, extra=()):
    """Q rank-position pairs: `extra`, screen_ref.three_queries(P) and random pairs."""
    rng = np.random.default_rng(seed + 100)
    pos = [tuple(p) for p in extra] + screen_ref.three_queries(P)
    while len(pos) < Q:
        a, b = sorted(int(v) for v in rng.choice(P, 2, replace=False))
        pos.append((a, b))
    return pos[:Q]


def words(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def same_words(got, want, what):
    """NaN at exactly the same places, every other word identical."""
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want), err_msg=str(what))
    ok = ~np.isnan(want)
    np.testing.assert_array_equal(words(got[ok]), words(want[ok]), err_msg=str(what))


def slot_rows(eng, pairs, known=None, mask=None):
    """The active slots' own rows in rank positions -> f64[ns][Q][P], read-only."""
    per = np.stack([rank_rows(eng.P, eng.screen_scores(pairs, known, sample=s, mask=mask)) for s in range(eng.active)])
    per.setflags(write=False)
    return per


def stat_calls(ns):
    """Every legal (name, argument) within the caps."""
    return [("quorum", m) for m in ref.legal_votes(ns)] + [("spread", t) for t in ref.legal_trims(ns)]


def stat_rows(eng, pairs, what, arg, known=None, mask=None):
    f = eng.screen_quorum_scores if what == "quorum" else eng.screen_spread_scores
    return rank_rows(eng.P, f(pairs, arg, known, mask=mask))


def stat_top(eng, pairs, n, what, arg, known=None, mask=None):
    f = eng.screen_quorum_top if what == "quorum" else eng.screen_spread_top
    return f(pairs, n, arg, known, mask=mask)


def want_rows(per, what, arg):
    """The reference statistic of per f64[ns][Q][P] -> f64[Q][P]."""
    f = ref.quorum if what == "quorum" else ref.spread
    return np.stack([f(per[:, i], arg) for i in range(per.shape[1])])


def check_rows_against_slots(eng, pairs, known=None, mask=None):
    """Check 1 for every legal argument; -> {(what, arg): the call's rows in rank positions}."""
    per = slot_rows(eng, pairs, known, mask)
    out = {}
    for what, arg in stat_calls(eng.active):
        got = stat_rows(eng, pairs, what, arg, known, mask)
        assert got.shape == (len(pairs), eng.P) and got.dtype == np.float64
        same_words(got, want_rows(per, what, arg), (what, arg))
        if what == "spread":
            assert not np.signbit(got[~np.isnan(got)]).any()        # d_t >= +0
        out[what, arg] = got
    return per, out


def check_lists_against_rows(eng, pairs, pos, rows, n, what, arg, known=None, mask=None):
    """Check 2: ids and score words are the reference lexsort of the call's own rows; the counts
    and the NaN / -1 tail through the device tensors."""
    import torch
    f = eng.screen_quorum_top_async if what == "quorum" else eng.screen_spread_top_async
    sd, idd, cd = f(pairs, n, arg, known, mask=mask)
    torch.cuda.synchronize()
    sd, idd, cd = sd.cpu().numpy(), idd.cpu().numpy(), cd.cpu().numpy()
    assert sd.shape == (len(pairs), n) and idd.shape == (len(pairs), n, 3) and cd.dtype == np.int64
    lists = stat_top(eng, pairs, n, what, arg, known, mask)
    for i, (x, y) in enumerate(pos):
        want_s, want_ids = ref.top_list(rows[i], eng.P, x, y, n)
        c = int(cd[i])
        assert c == want_s.size == min(n, int((~np.isnan(rows[i])).sum())), (what, arg, i)
        np.testing.assert_array_equal(idd[i, :c], want_ids, err_msg=str((what, arg, i)))
        np.testing.assert_array_equal(words(sd[i, :c]), words(want_s), err_msg=str((what, arg, i)))
        assert np.isnan(sd[i, c:]).all() and (idd[i, c:] == -1).all()
        assert bits(lists[i][0]) == bits(sd[i, :c]) and bits(lists[i][1]) == bits(idd[i, :c])
        assert lists[i][1].dtype == np.int32 and lists[i][1].shape == (c, 3)


# ------------------------------------------------------------------ 1. rows against the slots' own rows
SHAPES = [(3, 50, 3, None, 2), (10, 50, 8, None, 2), (13, 64, 2, None, 2), (32, 35, 4, None, 2), (10, 50, 8, 5, 2),
          (5, 50, 3, None, 3)]      # (K, P, B, active, R)
SHAPE_IDS = ["K%d-P%d-B%d-act%s-R%d" % c for c in SHAPES]


@pytest.mark.parametrize("K,P,B,active,R", SHAPES, ids=SHAPE_IDS)
def test_rows_are_the_order_statistics_of_the_slots_own_rows(K, P, B, active, R):
    th, pr = params(K, P, B, 7 + K, R)
    pos = queries(P, K)
    assert len(pos) == Q
    pairs = to_ids(P, pos)
    eng = make_engine(th, pr, active)
    ns = eng.active
    assert ns == (active or B)
    per, rows = check_rows_against_slots(eng, pairs)
    assert len(rows) == len(ref.legal_votes(ns)) + len(ref.legal_trims(ns)) >= 3
    for i, (x, y) in enumerate(pos):        # NaN exactly at the query's own genes
        assert np.flatnonzero(np.isnan(rows["quorum", 1][i])).tolist() == [x, y]
    # the restarts differ: the statistics are not one slot's row
    assert np.nanmax(rows["quorum", 1] - rows["quorum", ns]) > 0 and np.nanmax(rows["spread", 0]) > 0
    # lists of the same calls
    for what, arg in stat_calls(ns):
        check_lists_against_rows(eng, pairs, pos, rows[what, arg], 7, what, arg)
    eng.close()


def blocked_pair(mask, P):
    bx, by = np.nonzero(np.triu(np.unpackbits(mask.view(np.uint8), axis=1, bitorder="little")[:P, :P], 1))
    assert bx.size
    return int(bx[0]), int(by[0])


@pytest.mark.parametrize("variant", ["known", "mask", "both"])
@pytest.mark.parametrize("K,P,B", [(3, 50, 3), (10, 50, 8)], ids=["K3-B3", "K10-B8"])
def test_rows_under_a_known_slice_and_a_pair_mask(K, P, B, variant):
    th, pr = params(K, P, B, 21 + K)
    mask = converged_ref.random_pair_mask_words(P) if variant != "known" else None
    own = [blocked_pair(mask, P)] if mask is not None else []       # a query whose own pair is blocked
    pos = queries(P, 3 + K, own)
    pairs = to_ids(P, pos)
    rng = np.random.default_rng(9)
    slices = [np.sort(rng.choice(P, int(rng.integers(0, 7)), replace=False)) for _ in range(Q)]
    known = csr(slices) if variant != "mask" else None
    eng = make_engine(th, pr)
    per, rows = check_rows_against_slots(eng, pairs, known, mask)
    for i, (x, y) in enumerate(pos):
        ok = screen_ref.eligible(P, x, y, slices[i] if known is not None else None, mask)
        for row in rows.values():
            np.testing.assert_array_equal(np.isnan(row[i]), ~ok)
    if own:
        assert all(np.isnan(row[0]).all() for row in rows.values())
    for what, arg in (("quorum", B), ("quorum", 2), ("spread", 0), ("spread", (B - 2) // 2)):
        check_lists_against_rows(eng, pairs, pos, rows[what, arg], 9, what, arg, known, mask)
        check_lists_against_rows(eng, pairs, pos, rows[what, arg], P, what, arg, known, mask)
    eng.close()


# ------------------------------------------------------------------ 2. lists against the rows
@pytest.mark.parametrize("P", [2, 3, 20, 50])
def test_lists_are_the_lexsort_of_the_calls_own_rows(P):
    K, B = 4, 5
    th, pr = params(K, P, B, 60 + P)
    if P < 20:
        pos = [(x, y) for x in range(P) for y in range(x + 1, P)]
    else:
        pos = queries(P, P)
    pairs = to_ids(P, pos)
    eng = make_engine(th, pr)
    _, rows = check_rows_against_slots(eng, pairs)
    for what, arg in stat_calls(B):
        if P == 2:
            assert np.isnan(rows[what, arg]).all()
        for n in (1, 7, max(P - 2, 1), P + 3):
            check_lists_against_rows(eng, pairs, pos, rows[what, arg], n, what, arg)
    eng.close()


def test_a_wide_row_runs_the_select_kernels_overflow_path():
    """P = 1100, N = 512: 1098 candidates pass a buffer of 1024."""
    K, P, B, N = 3, 1100, 3, 512
    assert screen_ref.cap_of(N) < P - 2
    th, pr = params(K, P, B, 77)
    pos = screen_ref.three_queries(P) + [(211, 402)]
    pairs = to_ids(P, pos)
    eng = make_engine(th, pr)
    per = slot_rows(eng, pairs)
    for what, arg in (("quorum", 2), ("quorum", 3), ("spread", 0)):
        rows = stat_rows(eng, pairs, what, arg)
        same_words(rows, want_rows(per, what, arg), (what, arg))
        check_lists_against_rows(eng, pairs, pos, rows, N, what, arg)
    eng.close()


# ------------------------------------------------------------------ 3. independence
def test_a_query_does_not_depend_on_the_call(monkeypatch):
    K, P, B = 10, 50, 8
    th, pr = params(K, P, B, 5)
    rng = np.random.default_rng(2)
    others = np.array([rng.choice(P, 2, replace=False) for _ in range(40)], dtype=np.int32)
    q = np.array([[7, 31]], dtype=np.int32)
    N = 16
    eng = make_engine(th, pr)
    th0, p0 = bits(eng.theta.cpu().numpy()), bits(eng.pr.cpu().numpy())
    calls = [(np.concatenate([others[:at], q, others[at:]]), at) for at in (0, 17, 40)]
    calls.append((np.concatenate([q[:, ::-1], others]), 0))        # given as (g2, g1)
    for what, arg in (("quorum", 8), ("quorum", 3), ("quorum", 6), ("spread", 0), ("spread", 2)):
        monkeypatch.delenv("MMSBM_SCREEN_CHUNK", raising=False)
        (solo,) = stat_top(eng, q, N, what, arg)
        solo_row = stat_rows(eng, q, what, arg)[0]
        assert solo[0].size == N
        for chunk in (None, 1, 16):
            if chunk is None:
                monkeypatch.delenv("MMSBM_SCREEN_CHUNK", raising=False)
            else:
                monkeypatch.setenv("MMSBM_SCREEN_CHUNK", str(chunk))    # read at every call
            for pairs, at in calls:
                lists = stat_top(eng, pairs, N, what, arg)
                rows = stat_rows(eng, pairs, what, arg)
                assert bits(lists[at][0]) == bits(solo[0]) and bits(lists[at][1]) == bits(solo[1]), (what, arg, chunk, at)
                assert bits(rows[at]) == bits(solo_row), (what, arg, chunk, at)
    monkeypatch.delenv("MMSBM_SCREEN_CHUNK", raising=False)
    assert bits(eng.theta.cpu().numpy()) == th0 and bits(eng.pr.cpu().numpy()) == p0
    eng.close()


# ------------------------------------------------------------------ 4. degenerate ensembles
def test_identical_slots_give_slot_0_and_a_zero_spread():
    K, P, B, N = 6, 40, 4, 12
    th1, pr1 = params(K, P, 1, 31)
    th, pr = np.repeat(th1, B, axis=0), np.repeat(pr1, B, axis=0)
    pos = queries(P, 1)
    pairs = to_ids(P, pos)
    eng = make_engine(th, pr)
    slot0 = rank_rows(P, eng.screen_scores(pairs, sample=0))
    for m in range(1, B + 1):
        same_words(stat_rows(eng, pairs, "quorum", m), slot0, m)
    for t in (0, 1):
        rows = stat_rows(eng, pairs, "spread", t)
        np.testing.assert_array_equal(np.isnan(rows), np.isnan(slot0))
        assert (words(rows[~np.isnan(rows)]) == 0).all()            # +0, the sign bit clear
        lists = eng.screen_spread_top(pairs, N, t)
        for (x, y), (s, ids) in zip(pos, lists):
            keys = np.sort(screen_ref.row_keys(P, x, y)[screen_ref.eligible(P, x, y)])[:N]
            assert s.size == N and (words(s) == 0).all()
            np.testing.assert_array_equal(ids, scan_ref.keys_to_ids(keys, P))
    eng.close()


def test_one_slot():
    K, P = 5, 33
    th, pr = params(K, P, 1, 8)
    pos = queries(P, 2)
    pairs = to_ids(P, pos)
    eng = make_engine(th, pr)
    assert bits(eng.screen_quorum_scores(pairs, 1)) == bits(eng.screen_scores(pairs, sample=0))
    assert bits(eng.screen_quorum_scores(pairs)) == bits(eng.screen_scores(pairs, sample=0))     # the default: every slot
    for a, b in zip(eng.screen_quorum_top(pairs, 9), eng.screen_top(pairs, 9, sample=0)):
        assert bits(a[0]) == bits(b[0]) and bits(a[1]) == bits(b[1])
    eng.close()
    # one ACTIVE slot of several
    th, pr = params(K, P, 3, 8)
    eng = make_engine(th, pr, active=1)
    assert bits(eng.screen_quorum_scores(pairs, 1)) == bits(eng.screen_scores(pairs, sample=0))
    with pytest.raises(ValueError):
        eng.screen_spread_scores(pairs)
    eng.close()


# ------------------------------------------------------------------ 5. an independent reference
@pytest.mark.parametrize("K,P,B", [(3, 50, 3), (10, 50, 8), (13, 64, 2)], ids=["K3-B3", "K10-B8", "K13-B2"])
def test_against_the_numpy_reference(K, P, B):
    """|got - want| <= RTOL max_s |score_s| for the quorum score, twice that for the spread: each
    slot's row is within RTOL of screen_ref.ref_row (tests/test_gpu_screen.py) and an order statistic
    moves by no more than the largest move of a slot."""
    th, pr = params(K, P, B, 40 + K)
    pos = queries(P, 11)
    pairs = to_ids(P, pos)
    eng = make_engine(th, pr)
    want_per = np.stack([[screen_ref.ref_row(th[b], pr[b], x, y) for (x, y) in pos] for b in range(B)])
    scale = np.abs(want_per).max(axis=0)
    for what, arg in stat_calls(B):
        got = stat_rows(eng, pairs, what, arg)
        want = want_rows(want_per, what, arg)
        np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
        ok = ~np.isnan(want)
        bound = (1 if what == "quorum" else 2) * RTOL * scale[ok]
        assert (np.abs(got[ok] - want[ok]) <= bound).all(), (what, arg, float((np.abs(got[ok] - want[ok]) / scale[ok]).max()))
    eng.close()


# ------------------------------------------------------------------ 6. converged fits
@pytest.mark.parametrize("label", ["A300", "A1000"])
def test_converged_fits(label):
    """The three A seeds as B = 3: the regime in which the restarts really differ."""
    cks = [converged_ref.load(n) for n in converged_ref.SCAN_SETS[label]]
    th, pr = np.stack([c.theta for c in cks]), np.stack([c.pr for c in cks])
    P, B = th.shape[1], th.shape[0]
    assert B == 3
    pos = queries(P, 7)
    pairs = to_ids(P, pos)
    eng = make_engine(th, pr)
    per, rows = check_rows_against_slots(eng, pairs)
    assert sorted(rows) == [("quorum", 1), ("quorum", 2), ("quorum", 3), ("spread", 0)]
    ok = ~np.isnan(per[0])
    assert (per.max(axis=0)[ok] - per.min(axis=0)[ok]).max() > 0.05        # on the slots' rows: the seeds disagree
    for key, row in rows.items():
        for n in (8, P):
            check_lists_against_rows(eng, pairs, pos, row, n, *key)
    eng.close()


# ------------------------------------------------------------------ 7. refusals
class RawStat:
    """mmsbm_screen_stat_topn / mmsbm_screen_stat_scores as C sees them, on sentinel-filled outputs."""

    def __init__(self, eng, nq, N):
        import torch
        self.eng, self.torch, self.Q, self.N = eng, torch, nq, N
        self.ws = eng.scan_workspace("screen", nq, N)
        full = lambda shape, dtype: torch.full(shape, SENTINEL, dtype=dtype, device=eng.device)
        self.lists = [full((nq, N), torch.float64), full((nq, N, 3), torch.int32), full((nq,), torch.int64)]
        self.rows = [full((nq, eng.P), torch.float64)]

    def args(self, pairs, stat, arg, lists=True):
        eng = self.eng
        self.pairs = np.ascontiguousarray(pairs, dtype=np.int32)
        outs = self.lists if lists else self.rows
        return [eng.ctx, eng.scan_order.data_ptr(), self.pairs.ctypes.data_as(ctypes.c_void_p), self.Q, None, None, None,
                eng.theta.data_ptr(), eng.pr.data_ptr(), stat, arg, *([self.N] if lists else []), self.ws.data_ptr(),
                self.ws.numel(), *[o.data_ptr() for o in outs], eng._stream()]

    def call(self, args, lists=True):
        rc = (self.eng.lib.mmsbm_screen_stat_topn if lists else self.eng.lib.mmsbm_screen_stat_scores)(*args)
        self.torch.cuda.synchronize(self.eng.device)
        return rc

    def intact(self):
        return all(bool((o == SENTINEL).all()) for o in self.lists + self.rows)


def test_refusals_leave_the_outputs_alone():
    from trigenicinteractionpredictor_amd import _lib
    INVALID, UNSUPPORTED = _lib.MMSBM_ERR_INVALID, _lib.MMSBM_ERR_UNSUPPORTED
    QUORUM, SPREAD = _lib.MMSBM_SCREEN_STAT_QUORUM, _lib.MMSBM_SCREEN_STAT_SPREAD
    P, nq, N, B = 20, 3, 8, 12
    th, pr = params(3, P, B, 5)
    eng = make_engine(th, pr)
    assert eng.screen_stat_max_depth == eng.lib.mmsbm_screen_stat_max_depth() == 4
    good = [[1, 2], [3, 19], [0, 7]]
    raw = RawStat(eng, nq, N)
    # in the argument lists: 0 ctx, 1 order, 2 pairs, 3 Q, 4 known_off, 5 known_thirds, 6 mask, 7 theta, 8 pr,
    # 9 stat, 10 arg; then N (lists only), ws, ws_bytes, the outputs, the stream
    for lists in (True, False):
        w = 12 if lists else 11
        n_out = 3 if lists else 1
        bad = [("unknown stat 2", good, QUORUM, 1, [(9, 2)], INVALID), ("unknown stat -1", good, QUORUM, 1, [(9, -1)], INVALID),
               ("unknown stat -2", good, QUORUM, 1, [(9, -2)], INVALID),
               ("m 0", good, QUORUM, 0, [], INVALID), ("m -1", good, QUORUM, -1, [], INVALID),
               ("m ns + 1", good, QUORUM, B + 1, [], INVALID),
               ("t -1", good, SPREAD, -1, [], INVALID), ("t leaves no two", good, SPREAD, 6, [], INVALID),
               ("depth 5 from the top", good, QUORUM, 5, [], UNSUPPORTED), ("depth 5 from the bottom", good, QUORUM, 8, [], UNSUPPORTED),
               ("depth 6", good, QUORUM, 6, [], UNSUPPORTED), ("trim 4", good, SPREAD, 4, [], UNSUPPORTED),
               ("trim 5", good, SPREAD, 5, [], UNSUPPORTED),
               ("null ctx", good, QUORUM, 1, [(0, None)], INVALID), ("null order", good, QUORUM, 1, [(1, None)], INVALID),
               ("null pairs", good, SPREAD, 0, [(2, None)], INVALID), ("null theta", good, QUORUM, 1, [(7, None)], INVALID),
               ("null pr", good, SPREAD, 0, [(8, None)], INVALID),
               ("known_off alone", good, QUORUM, 1, [(4, raw.ws.data_ptr())], INVALID),
               ("id P", [[1, 2], [3, P], [0, 7]], QUORUM, 1, [], INVALID), ("id -1", [[1, 2], [3, 4], [-1, 7]], SPREAD, 0, [], INVALID),
               ("equal ids", [[1, 2], [5, 5], [0, 7]], QUORUM, 1, [], INVALID), ("Q -1", good, QUORUM, 1, [(3, -1)], INVALID),
               ("Q 65536", good, QUORUM, 1, [(3, 65536)], INVALID), ("no ws", good, QUORUM, 1, [(w, None)], INVALID),
               ("misaligned ws", good, SPREAD, 0, [(w, raw.ws.data_ptr() + 8)], INVALID),
               ("small ws", good, QUORUM, 1, [(w + 1, raw.ws.numel() // 2)], INVALID)]
        bad += [("null output %d" % i, good, QUORUM, 1, [(w + 2 + i, None)], INVALID) for i in range(n_out)]
        if lists:
            bad += [("N 0", good, QUORUM, 1, [(11, 0)], UNSUPPORTED), ("N 1025", good, SPREAD, 0, [(11, 1025)], UNSUPPORTED),
                    ("N -1", good, QUORUM, 1, [(11, -1)], UNSUPPORTED)]
        for what, pairs, stat, arg, replace, code in bad:
            args = raw.args(pairs, stat, arg, lists)
            for i, v in replace:
                args[i] = v
            assert raw.call(args, lists) == code, (what, lists)
            assert raw.intact(), (what, lists)
            assert eng.lib.mmsbm_last_error()
    # one active slot: the spread is refused, the quorum takes m = 1 only
    eng.set_active(1)
    for lists in (True, False):
        for stat, arg in ((SPREAD, 0), (QUORUM, 2)):
            assert raw.call(raw.args(good, stat, arg, lists), lists) == INVALID and raw.intact()
    eng.set_active(B)
    # the context is usable afterwards, through the same scratch and outputs; the legal edge of every cap
    for stat, arg in ((QUORUM, 4), (QUORUM, 9), (SPREAD, 3)):
        assert raw.call(raw.args(good, stat, arg)) == 0 and raw.call(raw.args(good, stat, arg, False), False) == 0
    want = eng.screen_spread_top(good, N, 3)
    for i in range(nq):
        assert bits(raw.lists[0][i].cpu().numpy()) == bits(want[i][0])
        assert bits(raw.lists[1][i].cpu().numpy()) == bits(want[i][1])
    assert raw.lists[2].cpu().tolist() == [N] * nq
    assert bits(rank_rows(P, eng.screen_spread_scores(good, 3))) == bits(raw.rows[0].cpu().numpy())
    # Q = 0 returns OK and writes nothing
    raw = RawStat(eng, nq, N)
    for lists in (True, False):
        args = raw.args(good, QUORUM, 1, lists)
        args[3] = 0
        assert raw.call(args, lists) == 0 and raw.intact()
    # the workspace is the screen scan's: the rows-only plan fits every list plan
    nbytes = ctypes.c_int64(-7)
    assert eng.lib.mmsbm_screen_workspace_bytes(eng.ctx, nq, 0, ctypes.byref(nbytes)) == 0
    assert 0 < nbytes.value <= raw.ws.numel()
    eng.close()


def test_python_checks():
    th, pr = params(3, 20, 12, 5)
    eng = make_engine(th, pr)
    from trigenicinteractionpredictor_amd._lib import MMSBMError
    pairs = [(1, 2), (3, 4)]
    off = np.array([0, 2, 4], dtype=np.int64)
    for f in (eng.screen_quorum_top, eng.screen_spread_top):
        with pytest.raises(ValueError):
            f(pairs, 8, known=(off, np.array([5, 4, 7, 9])))       # an unsorted slice
        with pytest.raises(ValueError):
            f([(1, 1)], 8)
        with pytest.raises(IndexError):
            f([(1, 20)], 8)
    for m in (0, -1, 13):
        with pytest.raises(ValueError):
            eng.screen_quorum_top(pairs, 8, m)
        with pytest.raises(ValueError):
            eng.screen_quorum_scores(pairs, m)
    for t in (-1, 6):
        with pytest.raises(ValueError):
            eng.screen_spread_top(pairs, 8, t)
        with pytest.raises(ValueError):
            eng.screen_spread_scores(pairs, t)
    for m in (5, 8):
        with pytest.raises(MMSBMError):
            eng.screen_quorum_top(pairs, 8, m)
    with pytest.raises(MMSBMError):
        eng.screen_spread_scores(pairs, 4)
    assert eng.screen_quorum_top([], 8) == [] and eng.screen_spread_scores([]).shape == (0, 20)
    # the default votes: every active slot, the minimum
    assert bits(eng.screen_quorum_scores(pairs)) == bits(eng.screen_quorum_scores(pairs, 12))
    # positions equal to x or y, or beyond the table, are ignored
    got = eng.screen_spread_top(pairs, 20, known=(off, np.array([4, 99, 5, 7])))
    assert [g[0].size for g in got] == [17, 16]
    eng.close()


# ------------------------------------------------------------------ 8. the driver
def test_driver_writes_the_two_tables(tmp_path):
    from trigenicinteractionpredictor_amd import Model, _lib, scan
    from trigenicinteractionpredictor_amd.engine import EMEngine
    from trigenicinteractionpredictor_amd.restarts import stream_states
    g = os.path.join(GOLDEN, "tiny")
    train, test = os.path.join(g, "train.dat"), os.path.join(g, "test.dat")
    K, B, iters, seed, top = 3, 4, 5, 1, 6
    model = Model()
    model.get_traintest(train, test)
    qfile = tmp_path / "q.txt"
    qfile.write_text("# queries\n7\t3\n%s %s\n11 4\n" % (model.id_gene[4], model.id_gene[10]))
    pairs = [(7, 3), (4, 10), (11, 4)]
    allow = tmp_path / "allow.txt"
    genes = list(range(0, model.P, 2)) + [3, 7, 11]
    allow.write_text("\n".join(str(x) for x in genes) + "\n")
    files = {n: str(tmp_path / (n + ".tsv")) for n in ("out", "screen", "quorum", "disputed")}
    base = ["-t", train, "-e", test, "-k", str(K), "-n", str(B), "-i", str(iters), "--seed", str(seed), "-o", files["out"],
            "--query-pairs", str(qfile), "--screen-top", str(top), "--allow-genes", str(allow), "--exclude", "train"]
    rc = scan.main(base + ["--screen", files["screen"], "--screen-quorum", files["quorum"], "--screen-votes", "3",
                           "--screen-disputed", files["disputed"], "--screen-trim", "1"], out=lambda *a: None)
    assert rc == 0
    # the same fit
    random.seed(seed)
    eng = EMEngine(K, model.P, B=B, R=model.R, eps=model.eps)
    eng.set_links(_lib.SET_TRAIN, *model._link_arrays(0))
    for b, (_, theta, pr) in enumerate(stream_states(model, K, range(B))):
        eng.upload_slot(b, theta, pr)
    eng.iterate(iters)
    mask = model.pair_mask(genes=genes)
    known = scan.screen_known(model, pairs, ("train",))
    assert known[1].size
    for name, label, column, lists in (("quorum", "votes", "quorum", eng.screen_quorum_top(pairs, top, 3, known, mask=mask)),
                                       ("disputed", "trim", "spread", eng.screen_spread_top(pairs, top, 1, known, mask=mask))):
        lines = open(files[name], encoding="utf-8").read().rstrip("\n").split("\n")
        assert lines[0] == "# samples\t%d" % B and lines[1] == "# screen %s\t%d" % (label, 3 if name == "quorum" else 1)
        assert lines[2].split("\t") == ["query", "rank", column, "mean", "min", "max", "ids", "names"]
        rows = [ln.split("\t") for ln in lines[3:]]
        assert len(rows) == sum(len(s) for s, _ in lists) > top
        at = 0
        for (g1, g2), (scores, ids) in zip(pairs, lists):
            a, b = sorted((g1, g2), key=str)
            probs = eng.predict(ids)[:B]
            mean = (((probs[0] + probs[1]) + probs[2]) + probs[3]) / B
            desc = -np.sort(-probs, axis=0)
            for rank, (v, row) in enumerate(zip(scores, ids), 1):
                r = rows[at]
                at += 1
                assert r[0] == "%s_%s" % (model.id_gene[a], model.id_gene[b]) and int(r[1]) == rank
                assert r[2] == repr(float(v)) and r[6] == "_".join(str(int(x)) for x in row)      # the engine call's value
                assert r[7] == "_".join(sorted(model.id_gene[int(x)] for x in row))
                assert all(int(x) in genes for x in row)                                           # --allow-genes applies
                i = rank - 1
                assert [r[3], r[4], r[5]] == [repr(float(mean[i])), repr(float(probs[:, i].min())), repr(float(probs[:, i].max()))]
                assert float(r[4]) <= float(r[3]) <= float(r[5])
                # consistent with predict: the value lies within RTOL of predict's own order statistic
                stat = desc[2, i] if name == "quorum" else desc[1, i] - desc[2, i]
                scale = 1 if name == "quorum" else 2
                assert abs(v - stat) <= scale * RTOL * np.abs(probs[:, i]).max()
    # the --screen table of the same run is what it is without the new tables
    plain = str(tmp_path / "plain.tsv")
    assert scan.main(base + ["--screen", plain], out=lambda *a: None) == 0
    assert open(plain).read() == open(files["screen"]).read()
    # without --screen, from --screen-best
    q2 = str(tmp_path / "q2.tsv")
    assert scan.main(base[:14] + ["--screen-best", "2", "--screen-quorum", q2], out=lambda *a: None) == 0
    lines = open(q2, encoding="utf-8").read().rstrip("\n").split("\n")
    assert lines[1] == "# screen votes\t%d" % B
    best = eng.pairs_top(2, 0.5, scan.known_keys(model, ("train", "test")))[2]
    want = eng.screen_quorum_top(best, 20, None, scan.screen_known(model, best, ("train", "test")))
    assert [ln.split("\t")[2] for ln in lines[3:]] == [repr(float(v)) for s, _ in want for v in s] and len(lines) > 3 + 20
    eng.close()
    # --best is refused before anything is written
    refused = str(tmp_path / "refused.tsv")
    assert scan.main(base + ["--screen-quorum", refused, "--best"], out=lambda *a: None) == 2
    assert not os.path.exists(refused)
