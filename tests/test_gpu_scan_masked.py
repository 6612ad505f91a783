"""The pair-masked census and threshold scan (include/mmsbm.h mmsbm_scan_census_masked,
mmsbm_scan_above_masked) on the GPU, through EMEngine's mask= keyword, the raw C calls, Model,
joint.Model and the scan driver.

Two oracles.  The existing kernels: a mask stands for the key table of every triple that contains a
blocked pair (masked_ref.expand), so a masked call must return exactly what the unmasked call
returns under known + expand(mask): counts equal, sorted rows equal in keys and score BYTES.  And
numpy (scan_ref / census_ref over masked_ref.blocked), with the project's preconditions asserted on
the reference alone (census_ref.assert_clear for thresholds, scan_ref.min_gap > 1e-9 for ordered
lists) and its tolerances: equality on counts, ids, keys and sets, rtol 1e-9 on scores.

The masks come from tests/masked_ref.py, never from the code under test.  P = 70 (54,740 triples) is
the largest shape."""
import ctypes
import functools
import os
import random
from math import comb

import numpy as np
import pytest

import census_ref
import masked_ref
import scan_ref
import scan_rule
from golden_util import GOLDEN, joint_load
from scan_gpu import SENTINEL, Raw, engine
from scan_ref import bits, packed, prefix_mean

pytestmark = pytest.mark.gpu

RTOL = scan_ref.RTOL
P_MATRIX = 70
EMPTY = np.zeros(0, np.int64)


@functools.lru_cache(maxsize=None)
def case(K, B, P, seed):
    """(th [B][P][K], pr, per-slot reference scores, ensemble scores, keys), computed once, read-only."""
    th, pr = scan_ref.random_params(K, P, seed, B)
    per = [scan_ref.ref_scores(th[b], pr[b]) for b in range(B)]
    keys = per[0][1]
    per = [s for s, _ in per]
    scores = prefix_mean(per, B)
    for a in per + [scores, keys, th, pr]:
        a.setflags(write=False)
    return th, pr, per, scores, keys


MASKS = {"random": masked_ref.random_mask, "allowed": masked_ref.allowed_mask, "block": masked_ref.block_mask,
         "single": masked_ref.single_pair_mask, "last_tile": masked_ref.last_tile_mask, "tiles": masked_ref.tiles_mask,
         "full": masked_ref.full_mask, "zero": lambda P: masked_ref.naive_mask(P, [])}


@functools.lru_cache(maxsize=None)
def mask_case(name, P):
    """(mask, expand(mask)) of one of the shared masks, computed once, read-only."""
    mask = np.ascontiguousarray(MASKS[name](P))
    assert mask.dtype == np.uint32 and mask.shape == masked_ref.shape(P)
    keys = masked_ref.expand(mask, P)
    mask.setflags(write=False)
    keys.setflags(write=False)
    return mask, keys


def some_known(keys):
    return np.ascontiguousarray(keys[::4])


def threshold_near(scores, q):
    """The midpoint of the wide gap (census_ref.gap_thresholds' kind) nearest the q-quantile."""
    s = np.unique(scores)
    wide = np.flatnonzero((s[1:] - s[:-1]) > 4 * 1e-7 * np.abs(s[1:]))
    at = np.searchsorted(s, np.quantile(scores, q))
    i = wide[np.argmin(np.abs(wide - at))]
    return float((s[i] + s[i + 1]) / 2)


def same(x, y):
    assert type(x) is type(y)
    if isinstance(x, np.ndarray):
        assert x.dtype == y.dtype and x.shape == y.shape and bits(x) == bits(y)
    else:
        assert x == y


def check_identity(eng, P, name, known, sample, thresholds, t):
    """Mask = keys: the masked calls against the unmasked calls under known + expand(mask).
    -> the number of rows of the list."""
    mask, blocked_keys = mask_case(name, P)
    union = np.union1d(EMPTY if known is None else known, blocked_keys).astype(np.int64)
    counts, total = eng.census(thresholds, known, sample, mask=mask)
    want, want_total = eng.census(thresholds, union, sample)
    same(counts, want)
    assert total == want_total == comb(P, 3) - union.size
    s, ids = eng.scan_above(t, known, sample, mask=mask)
    s0, ids0 = eng.scan_above(t, union, sample)
    same(s, s0)
    same(ids, ids0)
    assert s.size == eng.census([t], known, sample, mask=mask)[0][0]
    return s.size


# ------------------------------------------------------------------ 1. an all-zero mask
@pytest.mark.parametrize("B,sample", [(1, 0), (3, None), (3, 1)], ids=["single", "ensemble", "slot"])
def test_an_all_zero_mask_is_the_unmasked_call(B, sample):
    K, P = 10, P_MATRIX
    th, pr, per, scores, keys = case(K, B, P, 41)
    ref = per[sample] if sample is not None else scores
    zero, none = mask_case("zero", P)
    assert not zero.any() and none.size == 0
    eng = engine(th.copy(), pr.copy())
    thresholds = census_ref.gap_thresholds(ref, 12)
    t = threshold_near(ref, 0.9)
    for known in (None, some_known(keys)):
        got, want = eng.census(thresholds, known, sample, mask=zero), eng.census(thresholds, known, sample)
        same(got[0], want[0])
        assert got[1] == want[1]
        got, want = eng.scan_above(t, known, sample, mask=zero), eng.scan_above(t, known, sample)
        assert got[0].size > 1000
        same(got[0], want[0])
        same(got[1], want[1])
    eng.close()


# ------------------------------------------------------------------ 2. mask = keys
@pytest.mark.parametrize("name", ["random", "allowed", "block", "single", "last_tile"])
@pytest.mark.parametrize("K,P", [(3, 50), (10, 70)])
def test_a_mask_is_the_key_table_it_stands_for(K, P, name):
    th, pr, per, scores, keys = case(K, 1, P, 5)
    eng = engine(th.copy(), pr.copy())
    thresholds = census_ref.gap_thresholds(scores, 12)
    lowest = float(scores.min() * (1 - 1e-3))
    for known in (None, some_known(keys)):
        check_identity(eng, P, name, known, 0, thresholds, threshold_near(scores, 0.9))
        n = check_identity(eng, P, name, known, 0, thresholds, lowest)      # every eligible triple is a row
        assert n == comb(P, 3) - np.union1d(EMPTY if known is None else known, mask_case(name, P)[1]).size
    eng.close()


def test_the_masks_block_what_they_were_chosen_for():
    P = P_MATRIX
    assert comb(P, 3) == 54740
    assert 0.2 * 54740 < mask_case("random", P)[1].size < 0.35 * 54740
    assert 54740 - mask_case("allowed", P)[1].size == comb(24, 3)
    assert mask_case("block", P)[1].size == 13568
    assert mask_case("single", P)[1].size == P - 2


# ------------------------------------------------------------------ 3. against numpy
@pytest.mark.parametrize("name", ["random", "allowed", "block"])
def test_against_numpy(name):
    K, P = 10, P_MATRIX
    th, pr, per, scores, keys = case(K, 1, P, 5)
    mask, _ = mask_case(name, P)
    eng = engine(th.copy(), pr.copy())
    thresholds = census_ref.gap_thresholds(scores, 12)
    census_ref.assert_clear(scores, thresholds)                 # the precondition, reference alone
    for known in (None, some_known(keys)):
        out = masked_ref.blocked(keys, mask, P)
        if known is not None:
            out |= np.isin(keys, known)
        live_s, live_k = scores[~out], keys[~out]
        want, want_total = census_ref.ref_census(live_s, live_k, thresholds)
        got, total = eng.census(thresholds, known, 0, mask=mask)
        np.testing.assert_array_equal(got, want)
        assert total == want_total == live_k.size
        # the set of keys at a threshold
        t = threshold_near(scores, 0.8)
        census_ref.assert_clear(scores, [t])
        s, ids = eng.scan_above(t, known, 0, mask=mask)
        got_k = packed(ids, P)
        np.testing.assert_array_equal(np.sort(got_k), live_k[live_s >= t])
        np.testing.assert_allclose(s, scores[np.searchsorted(keys, got_k)], rtol=RTOL, atol=0)
        # the top 64 of the masked candidates
        want_s, want_k = scan_ref.top(live_s, live_k, 64)
        assert scan_ref.min_gap(want_s) > 1e-9                  # the precondition, reference alone
        s, ids = eng.scan_top_any(64, known, 0, mask=mask)
        np.testing.assert_array_equal(ids, scan_ref.keys_to_ids(want_k[:64], P))
        np.testing.assert_allclose(s, want_s[:64], rtol=RTOL, atol=0)
    # n above the masked total returns all of them, best first
    out = masked_ref.blocked(keys, mask, P)
    s, ids = eng.scan_top_any(60000, None, 0, mask=mask)
    assert s.size == int((~out).sum()) and (np.diff(s) <= 0).all()
    np.testing.assert_array_equal(np.sort(packed(ids, P)), keys[~out])
    with pytest.raises(ValueError):
        eng.scan_top_any(0, mask=mask)
    with pytest.raises(ValueError):
        eng.census([0.5], mask=mask.astype(np.int64))
    eng.close()


# ------------------------------------------------------------------ 4. the kernel matrix at P = 70
SINGLE_K = [3, 7, 10, 14, 18, 22, 26, 30]
ENSEMBLES = [(3, 22, 2), (7, 3, 4), (10, 10, 2), (10, 19, 1), (26, 4, 4), (32, 15, 1)]
EDGES = [(10, 10, 2, P) for P in (17, 31, 32, 33, 47, 65)] + [(10, 19, 1, P) for P in (17, 31, 32, 33, 47, 65)]


@pytest.mark.parametrize("K", SINGLE_K)
def test_every_ks_single_sample(K):
    assert (K + 3) // 4 == 1 + SINGLE_K.index(K) and scan_rule.width(K, 1) == 4
    th, pr, per, scores, keys = case(K, 1, P_MATRIX, 300 + K)
    eng = engine(th.copy(), pr.copy())
    thresholds = census_ref.gap_thresholds(scores, 12)
    for known in (None, some_known(keys)):
        assert check_identity(eng, P_MATRIX, "random", known, 0, thresholds, threshold_near(scores, 0.9)) > 500
    eng.close()


@pytest.mark.parametrize("K,B,WB", ENSEMBLES, ids=["K%dxB%d-WB%d" % e for e in ENSEMBLES])
def test_ensembles_at_every_width(K, B, WB):
    assert scan_rule.width(K, B) == WB, "the row-block rule moved: this case no longer runs at WB = %d" % WB
    th, pr, per, scores, keys = case(K, B, P_MATRIX, 500 + K + B)
    eng = engine(th.copy(), pr.copy())
    thresholds = census_ref.gap_thresholds(scores, 12)
    for known in (None, some_known(keys)):
        assert check_identity(eng, P_MATRIX, "random", known, None, thresholds, threshold_near(scores, 0.9)) > 500
    eng.close()


@pytest.mark.parametrize("K,B,WB,P", EDGES, ids=["K%dxB%d-WB%d-P%d" % e for e in EDGES])
def test_tile_edges(K, B, WB, P):
    """P below, at and above one and two tiles and row blocks, under a mask that blocks every pair of
    one whole b-tile and one whole c-tile (dead items, dead waves, dead tiles) and under the random one."""
    assert scan_rule.width(K, B) == WB
    th, pr, per, scores, keys = case(K, B, P, 500 + K + B)
    eng = engine(th.copy(), pr.copy())
    thresholds = census_ref.gap_thresholds(scores, 12)
    lowest = float(scores.min() * (1 - 1e-3))
    for name in ("tiles", "random"):
        for known in (None, some_known(keys)):
            check_identity(eng, P, name, known, None, thresholds, lowest)
        check_identity(eng, P, name, None, 0, thresholds, lowest)       # and the single-sample kernels
    eng.close()


# ------------------------------------------------------------------ 5., 6. raw C calls
class MaskedRaw(Raw):
    """scan_gpu.Raw for the masked entries: the mask pointer goes behind n_known."""
    MASKED = {"census": "mmsbm_scan_census_masked", "scan_above": "mmsbm_scan_above_masked"}

    def call(self, mask_ptr, mid, outs, sample=0, known=None):
        eng = self.eng
        known_d = None if known is None else self.upload(known)
        self.outs = outs
        rc = getattr(eng.lib, self.MASKED[self.family])(
            eng.ctx, eng.scan_order.data_ptr(), None if known is None else known_d.data_ptr(),
            0 if known is None else int(known.size), mask_ptr, eng.theta.data_ptr(), eng.pr.data_ptr(), sample, *mid,
            self.ws.data_ptr(), self.ws.numel(), *[None if o is None else o.data_ptr() for o in outs], eng._stream())
        self.torch.cuda.synchronize(eng.device)
        return rc


def device_mask(raw, mask):
    return raw.upload(np.array(mask).view(np.int32))       # a copy: the shared masks are read-only


def test_a_full_mask_counts_and_writes_nothing():
    import torch
    from trigenicinteractionpredictor_amd import _lib
    K, P = 10, P_MATRIX
    th, pr, per, scores, keys = case(K, 3, P, 41)
    full, every = mask_case("full", P)
    assert every.size == comb(P, 3)
    eng = engine(th.copy(), pr.copy())
    thresholds = np.sort(census_ref.gap_thresholds(scores, 12))
    lowest = float(scores.min() * (1 - 1e-3))
    for sample in (0, None):
        counts, total = eng.census(thresholds, None, sample, mask=full)
        assert total == 0 and not counts.any()
        s, ids = eng.scan_above(lowest, None, sample, mask=full)
        assert s.size == 0 and ids.shape == (0, 3)
    raw = MaskedRaw(eng, "scan_above")
    m = device_mask(raw, full)
    for sample in (0, -1):
        outs = [raw.full((64,), torch.float64), raw.full((64,), torch.int64), raw.full((1,), torch.int64)]
        assert raw.call(m.data_ptr(), (lowest, 64), outs, sample) == _lib.MMSBM_OK
        assert int(outs[2].cpu()[0]) == 0                                   # *out_count
        assert bool((outs[0] == SENTINEL).all()) and bool((outs[1] == SENTINEL).all())     # no row written
    raw = MaskedRaw(eng, "census", thresholds.size)
    out = raw.full((thresholds.size + 1,), torch.int64)
    assert raw.call(m.data_ptr(), (raw.upload(thresholds).data_ptr(), thresholds.size), [out]) == _lib.MMSBM_OK
    assert not out.cpu().numpy().any()
    eng.close()


def test_raw_calls_null_mask_and_capacity():
    import torch
    from trigenicinteractionpredictor_amd import _lib
    K, P = 10, P_MATRIX
    th, pr, per, scores, keys = case(K, 1, P, 5)
    mask, blocked_keys = mask_case("random", P)
    eng = engine(th.copy(), pr.copy())
    f64, i64 = torch.float64, torch.int64
    # the shape
    rows, words = ctypes.c_int32(), ctypes.c_int32()
    assert eng.lib.mmsbm_pair_mask_shape(eng.ctx, ctypes.byref(rows), ctypes.byref(words)) == _lib.MMSBM_OK
    assert (rows.value, words.value) == masked_ref.shape(P) == (80, 3)
    assert eng.lib.mmsbm_pair_mask_shape(eng.ctx, None, ctypes.byref(words)) == _lib.MMSBM_ERR_INVALID
    # a NULL mask: refused, outputs intact
    raw = MaskedRaw(eng, "scan_above")
    t = threshold_near(scores, 0.9)
    outs = [raw.full((64,), f64), raw.full((64,), i64), raw.full((1,), i64)]
    assert raw.call(None, (t, 64), outs) == _lib.MMSBM_ERR_INVALID and raw.intact()
    assert b"mask" in eng.lib.mmsbm_last_error()
    rawc = MaskedRaw(eng, "census", 2)
    thr = rawc.upload(np.array([0.4, 0.6]))
    assert rawc.call(None, (thr.data_ptr(), 2), [rawc.full((3,), i64)]) == _lib.MMSBM_ERR_INVALID and rawc.intact()
    # capacity below the count: the full count, `capacity` distinct hits, nothing at or past it
    m = device_mask(raw, mask)
    want = int(eng.census([t], None, 0, mask=mask)[0][0])
    live = ~masked_ref.blocked(keys, mask, P)
    assert want == int((scores[live] >= t).sum()) > 600
    capacity = 500
    outs = [raw.full((capacity + 300,), f64), raw.full((capacity + 300,), i64), raw.full((1,), i64)]
    assert raw.call(m.data_ptr(), (t, capacity), outs) == _lib.MMSBM_OK
    assert int(outs[2].cpu()[0]) == want
    s, k = outs[0].cpu().numpy(), outs[1].cpu().numpy()
    assert (s[capacity:] == SENTINEL).all() and (k[capacity:] == SENTINEL).all()           # the sentinel tail
    assert np.unique(k[:capacity]).size == capacity and np.isin(k[:capacity], keys[live & (scores >= t)]).all()
    # a count-only call with NULL arrays
    outs = [None, None, raw.full((1,), i64)]
    assert raw.call(m.data_ptr(), (t, 0), outs) == _lib.MMSBM_OK and int(outs[2].cpu()[0]) == want
    eng.close()


def test_p_above_the_cap_is_refused():
    """P = 16385 on a scratch context without links: the shape call and both masked calls return
    UNSUPPORTED before any device call; every buffer has its full size all the same."""
    import torch
    from trigenicinteractionpredictor_amd import _lib
    lib = _lib.load()
    K, P = 2, 16385
    dev = torch.device("cuda", torch.cuda.current_device())
    ctx = ctypes.c_void_p()
    _lib.check(lib.mmsbm_create(dev.index, ctypes.byref(ctx)))
    try:
        _lib.check(lib.mmsbm_set_shape(ctx, K, 2, 1, P, 1e-10))
        rows, words = ctypes.c_int32(-1), ctypes.c_int32(-1)
        assert lib.mmsbm_pair_mask_shape(ctx, ctypes.byref(rows), ctypes.byref(words)) == _lib.MMSBM_ERR_UNSUPPORTED
        assert (rows.value, words.value) == (-1, -1) and b"16384" in lib.mmsbm_last_error()
        nbytes = ctypes.c_int64()
        _lib.check(lib.mmsbm_scan_above_workspace_bytes(ctx, ctypes.byref(nbytes)))
        ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
        order = torch.arange(P, dtype=torch.int32, device=dev)
        theta = torch.full((1, P, K), 0.5, dtype=torch.float64, device=dev)
        pr = torch.full((1, 2, K ** 3), 0.5, dtype=torch.float64, device=dev)
        mask = torch.zeros((16400, 513), dtype=torch.int32, device=dev)
        count = torch.full((1,), SENTINEL, dtype=torch.int64, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = lib.mmsbm_scan_above_masked(ctx, order.data_ptr(), None, 0, mask.data_ptr(), theta.data_ptr(),
                                         pr.data_ptr(), 0, 0.5, 0, ws.data_ptr(), ws.numel(), None, None,
                                         count.data_ptr(), stream)
        assert rc == _lib.MMSBM_ERR_UNSUPPORTED
        _lib.check(lib.mmsbm_census_workspace_bytes(ctx, 0, ctypes.byref(nbytes)))
        ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
        rc = lib.mmsbm_scan_census_masked(ctx, order.data_ptr(), None, 0, mask.data_ptr(), theta.data_ptr(),
                                          pr.data_ptr(), 0, None, 0, ws.data_ptr(), ws.numel(), count.data_ptr(), stream)
        assert rc == _lib.MMSBM_ERR_UNSUPPORTED
        torch.cuda.synchronize(dev)
        assert int(count.cpu()[0]) == SENTINEL
        # at the cap itself the shape is served
        _lib.check(lib.mmsbm_set_shape(ctx, K, 2, 1, 16384, 1e-10))
        _lib.check(lib.mmsbm_pair_mask_shape(ctx, ctypes.byref(rows), ctypes.byref(words)))
        assert (rows.value, words.value) == (16384, 512)
    finally:
        lib.mmsbm_destroy(ctx)


# ------------------------------------------------------------------ 7. grid and repeats
@pytest.mark.parametrize("B,sample", [(1, 0), (10, None)], ids=["single", "ensemble"])
def test_results_do_not_depend_on_the_grid_or_on_repeats(B, sample, monkeypatch):
    K, P = 10, P_MATRIX
    th, pr, per, scores, keys = case(K, B, P, 500 + K + B if B > 1 else 5)
    mask, _ = mask_case("random", P)
    known = some_known(keys)
    eng = engine(th.copy(), pr.copy())
    thresholds = census_ref.gap_thresholds(scores, 12)
    t = threshold_near(scores, 0.9)

    def everything():
        return [*eng.census(thresholds, known, sample, mask=mask), *eng.scan_above(t, known, sample, mask=mask)]

    want = everything()
    assert want[2].size > 500
    for grid in (None, "1", "7"):
        for name in ("MMSBM_CENSUS_GRID", "MMSBM_SCAN_ABOVE_GRID"):
            if grid is not None:
                monkeypatch.setenv(name, grid)
        for x, y in zip(everything(), want):
            same(x, y)
    eng.close()


# ------------------------------------------------------------------ 8. joint.Model
def joint_model(case_name, name, it=5):
    from trigenicinteractionpredictor_amd.joint import DataType, Model
    meta, vec, train, test = joint_load(case_name, name)
    m = Model()
    m.get_train_test(train, test)
    random.seed(meta["seed"])
    m.initialize_parameters(meta["K"], getattr(DataType, meta["interaction"]))
    m.theta, m.pr, m.qr = vec["theta_%d" % it].tolist(), vec["pr_%d" % it].tolist(), vec["qr_%d" % it].tolist()
    return m, vec["theta_%d" % it], vec["pr_%d" % it], vec["qr_%d" % it]


@pytest.mark.parametrize("case_name,name", [("tiny", "K10_s1"), ("small", "K10_s1")])
def test_joint_digenic_mask_and_trigenic_scan(case_name, name):
    m, theta, pr, qr = joint_model(case_name, name)
    P = m.P
    assert P == {"tiny": 40, "small": 200}[case_name]
    order, rank = scan_ref.rank_tables(P)
    x, y = np.triu_indices(P, 1)
    i, j = order[x], order[y]                                   # every pair as its key spells it
    pred = np.einsum("nx,ny,xy->n", theta[i], theta[j], np.asarray(qr)[..., 1])
    # a threshold at the midpoint of the widest gap of the middle half of the host predictions
    s = np.sort(pred)
    lo, hi = s.size // 4, 3 * s.size // 4
    g = lo + int(np.argmax(s[lo + 1:hi] - s[lo:hi - 1]))
    threshold = float((s[g] + s[g + 1]) / 2)
    near = int((np.abs(pred - threshold) <= 1e-9 * threshold).sum())
    assert near == 0                                            # nothing to exclude from the comparison
    over = pred >= threshold
    assert 0 < over.sum() < over.size
    measured = [[int(v) for v in key.split("_")] for table in (m.dlinks, m.dtest_links)
                for key, n in table.items() if n[1]]
    want = masked_ref.naive_mask(P, list(zip(x[over], y[over])) + [(rank[a], rank[b]) for a, b in measured if a != b])
    np.testing.assert_array_equal(m.digenic_mask(threshold), want)
    predicted_only = masked_ref.naive_mask(P, list(zip(x[over], y[over])))
    np.testing.assert_array_equal(m.digenic_mask(threshold, measured=False), predicted_only)
    # the trigenic scan under that mask against numpy
    measured3 = [[int(v) for v in key.split("_")] for table in (m.links, m.test_links) for key in table
                 if key.count("_") == 2]                        # test_links holds the test pairs too
    known = np.unique(packed(np.array([t for t in measured3 if len(set(t)) == 3]), P))
    scores, keys = scan_ref.ref_scores(theta, pr)
    live = ~(masked_ref.blocked(keys, want, P) | np.isin(keys, known))
    assert 64 < live.sum() < keys.size
    want_s, want_k = scan_ref.top(scores[live], keys[live], 64)
    assert scan_ref.min_gap(want_s) > 1e-9                      # the precondition, reference alone
    rows = m.predict_novel_trigenic(64, threshold)
    ids = scan_ref.keys_to_ids(want_k[:64], P)
    assert [r[1] for r in rows] == ["_".join(str(int(v)) for v in row) for row in ids]
    np.testing.assert_allclose([r[0] for r in rows], want_s[:64], rtol=RTOL, atol=0)
    assert rows[0][2] == sorted(m.id_gene[int(v)] for v in ids[0])
    thresholds = census_ref.gap_thresholds(scores, 12)
    census_ref.assert_clear(scores, thresholds)
    counts, total = m.novel_trigenic_census(thresholds, threshold)
    ref_counts, ref_total = census_ref.ref_census(scores[live], keys[live], thresholds)
    np.testing.assert_array_equal(counts, ref_counts)
    assert total == ref_total


# ------------------------------------------------------------------ 9. Model and the driver
def test_model_mask_keyword():
    from trigenicinteractionpredictor_amd import Model
    from golden_util import load
    _, vec, train, test = load("tiny", "K10_s1")
    m = Model()
    m.get_traintest(train, test)
    m.initialize_parameters(vec["theta_5"].shape[1])
    m.theta, m.pr = vec["theta_5"].tolist(), vec["pr_5"].tolist()
    genes = [m.id_gene[g] for g in range(0, m.P, 2)]
    mask = m.pair_mask(genes=genes, pairs=[(0, 2)])
    rows = m.predict_novel_any(30, mask=mask)
    allowed = set(genes)
    assert len(rows) == 30 and all(set(r[2]) <= allowed for r in rows)
    assert all(not {"0", "2"} <= set(r[1].split("_")) for r in rows)
    t = rows[-1][0]
    net = m.predict_network(t, mask=mask)
    counts, total = m.novel_census([t], mask=mask)
    assert net[:30] == rows and len(net) == counts[0] and total < m.novel_census([t])[1]
    assert m.predict_novel_any(30) != rows


def test_the_driver_under_a_mask(tmp_path):
    """--allow-genes and --block-pairs on the main table, --census and --network against numpy over
    the parameters the same fit gives (the EM is deterministic: same seed, same batch, same bits)."""
    from trigenicinteractionpredictor_amd import Model, _lib, scan
    from trigenicinteractionpredictor_amd.engine import EMEngine
    from trigenicinteractionpredictor_amd.restarts import stream_states
    g = os.path.join(GOLDEN, "tiny")
    train, test = os.path.join(g, "train.dat"), os.path.join(g, "test.dat")
    K, B, iters, seed, top = 3, 2, 5, 1, 40
    m = Model()
    m.get_traintest(train, test)
    P = m.P
    genes = [gid for gid in range(P) if gid % 4 != 1]
    pairs = [(0, 2), (3, 4), (10, 12)]
    allow, block = tmp_path / "allow.txt", tmp_path / "block.txt"
    allow.write_text("".join("%s\n" % (m.id_gene[v] if v % 3 else v) for v in genes))
    block.write_text("".join("%d\t%s\n" % (a, m.id_gene[b]) for a, b in pairs))
    # the reference: the same fit, downloaded
    random.seed(seed)
    eng = EMEngine(K, P, B=B, R=m.R, eps=m.eps)
    eng.set_links(_lib.SET_TRAIN, *m._link_arrays(0))
    for b, (_, theta, pr) in enumerate(stream_states(m, K, range(B))):
        eng.upload_slot(b, theta, pr)
    eng.iterate(iters)
    th, pr = eng.download()
    eng.close()
    per = [scan_ref.ref_scores(th[b], pr[b]) for b in range(B)]
    keys = per[0][1]
    scores = prefix_mean([s for s, _ in per], B)
    mask = masked_ref.naive_from_ids(P, pairs, genes)
    live = ~(masked_ref.blocked(keys, mask, P) | np.isin(keys, scan.known_keys(m)))
    live_s, live_k = scores[live], keys[live]
    want_s, want_k = scan_ref.top(live_s, live_k, top)
    assert scan_ref.min_gap(want_s) > 1e-9                      # the precondition, reference alone
    T = threshold_near(live_s, 0.9)
    thresholds = [T, threshold_near(live_s, 0.5)]
    census_ref.assert_clear(scores, thresholds)
    files = [str(tmp_path / f) for f in ("top.tsv", "census.tsv", "network.tsv")]
    rc = scan.main(["-t", train, "-e", test, "-k", str(K), "-n", str(B), "-i", str(iters), "--seed", str(seed),
                    "--top", str(top), "-o", files[0], "--census", files[1], "--thresholds",
                    ",".join(repr(v) for v in thresholds), "--network", files[2], "--network-threshold", repr(T),
                    "--allow-genes", str(allow), "--block-pairs", str(block)], out=lambda *a: None)
    assert rc == 0

    def table(path):
        return [ln.split("\t") for ln in open(path, encoding="utf-8").read().rstrip("\n").split("\n")]

    def key_text(ks):
        return ["_".join(str(int(v)) for v in row) for row in scan_ref.keys_to_ids(ks, P)]

    rows = table(files[0])[1:]
    assert [r[2] for r in rows] == key_text(want_k[:top])
    np.testing.assert_allclose([float(r[1]) for r in rows], want_s[:top], rtol=RTOL, atol=0)
    cen = table(files[1])
    assert cen[0] == ["# total", str(live_k.size)]
    assert [int(r[1]) for r in cen[2:]] == [int((live_s >= v).sum()) for v in sorted(thresholds, reverse=True)]
    net = table(files[2])[1:]
    order = np.lexsort((live_k[live_s >= T], -live_s[live_s >= T]))
    assert scan_ref.min_gap(live_s[live_s >= T][order]) > 1e-9  # the precondition, reference alone
    assert [r[2] for r in net] == key_text(live_k[live_s >= T][order])
    np.testing.assert_allclose([float(r[1]) for r in net], live_s[live_s >= T][order], rtol=RTOL, atol=0)
