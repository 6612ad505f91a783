"""The pair mask for the pair census, the vote scan and the quorum scan (include/mmsbm.h
mmsbm_pair_census_masked, mmsbm_scan_votes_masked, mmsbm_scan_quorum_topn_masked) on the GPU, through
EMEngine's mask= keyword, the raw C calls, Model and joint.Model.

The oracle throughout is the existing unmasked call: a mask stands for the key table of every triple
that contains a blocked pair (masked_ref.expand), so a masked call must return exactly what the
unmasked call returns under known + expand(mask), a few further known keys included so that both
tables are live: integer outputs equal, score BYTES equal, the vote scan's rows equal as sorted sets
(EMEngine.consensus sorts them), the quorum list equal row by row.  The Python surface is held
against numpy over scan_ref's scores (tests/pair_census_ref.py) with the project's preconditions
asserted on the reference alone.

The masks come from tests/masked_ref.py, never from the code under test.  P = 70 (54,740 triples) is
the shape of the matrices; P = 203 is the smallest at which the quorum scan runs its seeding pass."""
import ctypes
import functools
import random
from math import comb

import numpy as np
import pytest

import census_ref
import masked_ref
import pair_census_ref
import scan_ref
import scan_rule
from golden_util import joint_load
from scan_gpu import SENTINEL, Raw, engine
from scan_ref import bits, packed, prefix_mean

pytestmark = pytest.mark.gpu

P_MATRIX = 70
EMPTY = np.zeros(0, np.int64)
GRID_VARS = ("MMSBM_PAIR_CENSUS_GRID", "MMSBM_SCAN_VOTES_GRID", "MMSBM_SCAN_QUORUM_GRID")


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


def union_of(known, blocked_keys):
    return np.union1d(EMPTY if known is None else known, blocked_keys).astype(np.int64)


def levels(scores, qs=(0.5, 0.9, 0.99)):
    """Thresholds at the quantiles qs of the reference scores, ascending: hits at every level."""
    return np.array([float(np.quantile(scores, q)) for q in qs])


LEVELS8 = (0.3, 0.5, 0.7, 0.8, 0.9, 0.95, 0.99, 0.995)


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
    elif isinstance(x, (tuple, list)):
        assert len(x) == len(y)
        for u, v in zip(x, y):
            same(u, v)
    else:
        assert x == y


def quorum_votes(eng, sample, depths=None):
    """The min_votes the quorum scan is asked for: all of them up to 3 slots, else the two ends and
    what `depths` adds."""
    ns = eng.active if sample is None else 1
    ms = set(range(1, ns + 1)) if ns <= 3 else {1, ns}
    ms |= set(m for m in depths or () if m <= ns)
    return sorted(m for m in ms if eng.quorum_depth(m, sample) <= eng.quorum_max_depth)


def families(eng, known, sample, mask, thr, t, n=64, depths=None):
    """Every output of the three families for one (known, sample, mask): a flat list for same()."""
    kw = {} if mask is None else {"mask": mask}
    ns = eng.active if sample is None else 1
    out = [eng.pair_census(thr[-1:], known, sample, **kw),              # M = 1
           eng.pair_census(thr, known, sample, **kw),                   # M = len(thr)
           eng.vote_census(t, known, sample, **kw)]                     # histogram-only
    for m in sorted({1, ns}):
        out.append(eng.consensus(t, m, known, sample, **kw))            # listing
    for m in quorum_votes(eng, sample, depths):
        out.append(eng.quorum_top(n, m, known, sample, **kw))
    return out


def check_identity(eng, P, name, known, sample, ref, n=64, depths=None):
    """Mask = keys: the masked calls against the unmasked calls under known + expand(mask).
    -> the masked outputs."""
    mask, blocked_keys = mask_case(name, P)
    thr = levels(ref, LEVELS8)
    t = float(np.quantile(ref, 0.9))
    got = families(eng, known, sample, mask, thr, t, n, depths)
    want = families(eng, union_of(known, blocked_keys), sample, None, thr, t, n, depths)
    same(got, want)
    return got


# ------------------------------------------------------------------ 1. mask = keys
@pytest.mark.parametrize("name", ["random", "allowed", "block", "single", "last_tile"])
@pytest.mark.parametrize("K,P", [(3, 50), (10, 70)])
@pytest.mark.parametrize("B,sample", [(1, 0), (3, None), (3, 1)], ids=["single", "ensemble", "slot"])
def test_a_mask_is_the_key_table_it_stands_for(B, sample, K, P, name):
    th, pr, per, scores, keys = case(K, B, P, 5)
    ref = per[sample] if sample is not None else scores
    eng = engine(th.copy(), pr.copy())
    for known in (None, some_known(keys)):
        got = check_identity(eng, P, name, known, sample, ref)
        mat1, mat8, hist = got[0], got[1], got[2]
        assert mat1.shape == (P, P, 1) and mat8.shape == (P, P, 8)
        assert mat8[:, :, 0].any()
        if name != "allowed":                                           # a third of the genes: few triples
            assert mat8[:, :, -1].any(), "no hit at the highest level"
        assert hist.sum() == comb(P, 3) - union_of(known, mask_case(name, P)[1]).size
        assert got[-1][0].size > 0                                      # a quorum list with rows
    eng.close()


# ------------------------------------------------------------------ 2. the all-zero and the full mask
@pytest.mark.parametrize("B,sample", [(1, 0), (3, None), (3, 1)], ids=["single", "ensemble", "slot"])
def test_an_all_zero_mask_is_the_unmasked_call(B, sample):
    K, P = 10, P_MATRIX
    th, pr, per, scores, keys = case(K, B, P, 41)
    ref = per[sample] if sample is not None else scores
    zero, none = mask_case("zero", P)
    assert not zero.any() and none.size == 0
    eng = engine(th.copy(), pr.copy())
    thr, t = levels(ref, LEVELS8), float(np.quantile(ref, 0.9))
    for known in (None, some_known(keys)):
        got = families(eng, known, sample, zero, thr, t)
        same(got, families(eng, known, sample, None, thr, t))
        assert got[1].any() and got[3][0].size > 1000 and got[-1][0].size == 64
    eng.close()


class MaskedRaw(Raw):
    """scan_gpu.Raw for the masked entries: the mask pointer goes behind n_known."""
    MASKED = {"pair_census": "mmsbm_pair_census_masked", "scan_votes": "mmsbm_scan_votes_masked",
              "scan_quorum": "mmsbm_scan_quorum_topn_masked"}

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


def votes_outs(raw, ns, rows):
    """mmsbm_scan_votes' outputs, full of the sentinel: hist, scores, keys, votes, count."""
    t = raw.torch
    return [raw.full((ns + 1,), t.int64), raw.full((rows,), t.float64), raw.full((rows,), t.int64),
            raw.full((rows,), t.int32), raw.full((1,), t.int64)]


def quorum_outs(raw, n):
    t = raw.torch
    return [raw.full((n,), t.float64), raw.full((n, 3), t.int32), raw.full((1,), t.int64)]


def test_a_full_mask_counts_and_lists_nothing():
    from trigenicinteractionpredictor_amd import _lib
    K, P, B = 10, P_MATRIX, 3
    th, pr, per, scores, keys = case(K, B, P, 41)
    full, every = mask_case("full", P)
    assert every.size == comb(P, 3)
    eng = engine(th.copy(), pr.copy())
    thr = levels(scores, LEVELS8)
    lowest = float(min(s.min() for s in per) * (1 - 1e-3))
    for sample in (0, None):
        ns = 1 if sample is not None else B
        assert not eng.pair_census(thr, None, sample, mask=full).any()
        assert not eng.gene_census(thr, None, sample, mask=full).any()
        hist = eng.vote_census(lowest, None, sample, mask=full)
        assert hist.shape == (ns + 1,) and not hist.any()
        votes, s, ids = eng.consensus(lowest, 1, None, sample, mask=full)
        assert votes.size == s.size == 0 and ids.shape == (0, 3)
        s, ids = eng.quorum_top(64, 1, None, sample, mask=full)
        assert s.size == 0 and ids.shape == (0, 3)
    # the raw calls: no row written, the quorum's tail NaN / -1 from row 0 on
    raw = MaskedRaw(eng, "scan_votes")
    m = device_mask(raw, full)
    for sample in (0, -1):
        ns = 1 if sample >= 0 else B
        outs = votes_outs(raw, ns, 64)
        assert raw.call(m.data_ptr(), (lowest, 1, 64), outs, sample) == _lib.MMSBM_OK
        assert not outs[0].cpu().numpy().any() and int(outs[4].cpu()[0]) == 0
        assert all(bool((o == SENTINEL).all()) for o in outs[1:4])
    raw = MaskedRaw(eng, "scan_quorum", 64)
    for sample, votes in ((0, 1), (-1, 2)):
        outs = quorum_outs(raw, 64)
        assert raw.call(m.data_ptr(), (votes, 64), outs, sample) == _lib.MMSBM_OK
        assert int(outs[2].cpu()[0]) == 0
        assert np.isnan(outs[0].cpu().numpy()).all() and (outs[1].cpu().numpy() == -1).all()
    raw = MaskedRaw(eng, "pair_census", 8)
    out = raw.full((P, P, 8), raw.torch.int32)
    assert raw.call(m.data_ptr(), (raw.upload(thr).data_ptr(), 8), [out], -1) == _lib.MMSBM_OK
    assert not out.cpu().numpy().any()
    eng.close()


# ------------------------------------------------------------------ 3. across the families
@pytest.mark.parametrize("name", ["random", "allowed", "tiles"])
def test_the_families_agree_under_one_mask(name):
    K, P, B = 10, P_MATRIX, 3
    th, pr, per, scores, keys = case(K, B, P, 41)
    mask, blocked_keys = mask_case(name, P)
    known = some_known(keys)
    eng = engine(th.copy(), pr.copy())
    thr = levels(scores, LEVELS8)
    for sample in (None, 1):
        ns = B if sample is None else 1
        counts, total = eng.census(thr, known, sample, mask=mask)
        mat = eng.pair_census(thr, known, sample, mask=mask)
        x, y = np.triu_indices(P, 1)
        np.testing.assert_array_equal(mat[x, y].sum(axis=0, dtype=np.int64), 3 * counts)
        t = float(np.quantile(per[sample or 0], 0.9))
        hist = eng.vote_census(t, known, sample, mask=mask)
        assert hist.sum() == total == comb(P, 3) - union_of(known, blocked_keys).size
        # a blocked pair's row of the matrix is zero (gene ids -> rank positions)
        _, rank = scan_ref.rank_tables(P)
        bx, by = np.nonzero(np.triu(np.unpackbits(mask.view(np.uint8), axis=1, bitorder="little")[:P, :P], 1))
        inv = np.argsort(rank)
        assert bx.size and not mat[inv[bx], inv[by]].any()
        # votes >= m at t exactly when the masked q_m >= t; t at the 99 % quantile of the reference's
        # q_m, so that 4096 rows hold every triple at or above it (1 % of 54,740)
        slots = np.stack(per if sample is None else [per[sample]])
        for m in range(1, ns + 1):
            t = float(np.quantile(np.sort(slots, axis=0)[ns - m], 0.99))
            votes, s, ids = eng.consensus(t, m, known, sample, mask=mask)
            qs, qids = eng.quorum_top(4096, m, known, sample, mask=mask)
            assert qs.size < 4096 or qs[-1] < t, "the quorum list does not hold every row at or above t"
            want = np.sort(packed(qids[qs >= t], P))
            assert want.size > 0 or name == "allowed"
            np.testing.assert_array_equal(np.sort(packed(ids, P)), want)
            assert (votes >= m).all()
    # pairs_top's eligible column: the masked pair census at a threshold every score passes
    n = comb(P, 2)
    counts, eligible, ids = eng.pairs_top(n, 0.0, known, 0, mask=mask)
    assert counts.size == n
    np.testing.assert_array_equal(counts, eligible)
    mat0 = eng.pair_census([0.0], known, 0, mask=mask)[:, :, 0]
    np.testing.assert_array_equal(mat0[ids[:, 0], ids[:, 1]], eligible)
    assert (eligible == 0).any() and eligible.sum() == 3 * (comb(P, 3) - union_of(known, blocked_keys).size)
    eng.close()


# ------------------------------------------------------------------ 4. the kernel matrix
SINGLE_K = [3, 7, 10, 14, 18, 22, 26, 30]
ENSEMBLES = [(3, 22, 2), (7, 3, 4), (10, 10, 2), (10, 19, 1), (26, 4, 4), (32, 15, 1)]
EDGE_P = (17, 31, 32, 33, 47, 65)


@pytest.mark.parametrize("K", SINGLE_K)
def test_every_ks_single_sample(K):
    assert (K + 3) // 4 == 1 + SINGLE_K.index(K) and scan_rule.width(K, 1) == 4
    th, pr, per, scores, keys = case(K, 1, P_MATRIX, 300 + K)
    eng = engine(th.copy(), pr.copy())
    for known in (None, some_known(keys)):
        got = check_identity(eng, P_MATRIX, "tiles", known, 0, scores)
        assert got[1].any() and got[3][0].size > 100 and got[-1][0].size == 64
    eng.close()


@pytest.mark.parametrize("K,B,WB", ENSEMBLES, ids=["K%dxB%d-WB%d" % e for e in ENSEMBLES])
def test_ensembles_at_every_width(K, B, WB):
    assert scan_rule.width(K, B) == WB, "the row-block rule moved: this case no longer runs at WB = %d" % WB
    th, pr, per, scores, keys = case(K, B, P_MATRIX, 500 + K + B)
    eng = engine(th.copy(), pr.copy())
    for known in (None, some_known(keys)):
        got = check_identity(eng, P_MATRIX, "tiles", known, None, scores)
        assert got[1].any() and got[-1][0].size == 64
    eng.close()


@pytest.mark.parametrize("K", [3, 10, 18, 30])
def test_quorum_depths_three_and_four_in_both_directions(K):
    """B = 8: m = 4 keeps the 4 largest, m = 5 the 4 smallest, m = 3 and 6 lists of depth 3."""
    B = 8
    th, pr, per, scores, keys = case(K, B, P_MATRIX, 700 + K)
    eng = engine(th.copy(), pr.copy())
    assert [eng.quorum_depth(m) for m in (3, 4, 5, 6)] == [3, 4, 4, 3]
    mask, blocked_keys = mask_case("tiles", P_MATRIX)
    for known in (None, some_known(keys)):
        union = union_of(known, blocked_keys)
        for m in (3, 4, 5, 6):
            got = eng.quorum_top(64, m, known, mask=mask)
            same(got, eng.quorum_top(64, m, union))
            assert got[0].size == 64
    eng.close()


@pytest.mark.parametrize("P", EDGE_P)
def test_tile_edges(P):
    """P below, at and above one and two tiles and row blocks, under a mask that blocks every pair of
    one whole b-tile and one whole c-tile (dead items, dead waves, dead tiles)."""
    K, B = 10, 10
    assert scan_rule.width(K, B) == 2
    th, pr, per, scores, keys = case(K, B, P, 500 + K + B)
    eng = engine(th.copy(), pr.copy())
    for known in (None, some_known(keys)):
        check_identity(eng, P, "tiles", known, None, scores, depths=(4, 7))
    check_identity(eng, P, "tiles", None, 0, per[0])                    # and the single-sample kernels
    eng.close()


# ------------------------------------------------------------------ 5. the quorum scan
@functools.lru_cache(maxsize=None)
def seeded_case():
    """K = 3, P = 203, 3 slots in a batch of 4: the seeding pass, with a partial last tile."""
    K, P, B = 3, 203, 4
    th, pr = scan_ref.random_params(K, P, 77, B)
    th.setflags(write=False)
    pr.setflags(write=False)
    return K, P, th, pr


@pytest.mark.parametrize("name", ["allowed", "random"])
def test_quorum_with_the_seeding_pass(name, monkeypatch):
    K, P, th, pr = seeded_case()
    assert P >= 200 and P % 16
    mask, blocked_keys = mask_case(name, P)
    for var in ("MMSBM_SCAN_QUORUM_GRID", "MMSBM_SCAN_QUORUM_EARLY"):
        monkeypatch.delenv(var, raising=False)
    three = engine(th[:3].copy(), pr[:3].copy())
    wide = engine(th.copy(), pr.copy())
    wide.set_active(3)
    known = np.ascontiguousarray(masked_ref.all_keys(P)[5::11])
    union = union_of(known, blocked_keys)
    for m in (1, 2, 3):
        for n in (64, 1000):
            want = three.quorum_top(n, m, union)
            assert want[0].size == n
            same(three.quorum_top(n, m, known, mask=mask), want)
            same(wide.quorum_top(n, m, known, mask=mask), want)          # the slots inside a larger batch
        monkeypatch.setenv("MMSBM_SCAN_QUORUM_EARLY", "0")
        same(three.quorum_top(64, m, known, mask=mask), three.quorum_top(64, m, union))
        monkeypatch.delenv("MMSBM_SCAN_QUORUM_EARLY")
        for grid in ("1", "7"):
            monkeypatch.setenv("MMSBM_SCAN_QUORUM_GRID", grid)
            same(three.quorum_top(64, m, known, mask=mask), three.quorum_top(64, m, union))
        monkeypatch.delenv("MMSBM_SCAN_QUORUM_GRID")
    same(three.quorum_top(64, 1, known, 2, mask=mask), three.quorum_top(64, 1, union, 2))   # one slot
    three.close()
    wide.close()


def test_quorum_asked_for_more_rows_than_the_mask_leaves():
    K, P, B = 10, P_MATRIX, 3
    th, pr, per, scores, keys = case(K, B, P, 41)
    mask, blocked_keys = mask_case("allowed", P)
    left = comb(P, 3) - blocked_keys.size
    assert left == comb(24, 3) < 4096
    eng = engine(th.copy(), pr.copy())
    for m in (1, 2, 3):
        s, ids = eng.quorum_top(4096, m, None, mask=mask)
        assert s.size == left
        same((s, ids), eng.quorum_top(4096, m, blocked_keys.copy()))
        np.testing.assert_array_equal(np.sort(packed(ids, P)), keys[~masked_ref.blocked(keys, mask, P)])
        scores_d, ids_d, count = eng.quorum_top_async(4096, m, mask=mask)
        assert int(count.cpu()[0]) == left
        assert np.isnan(scores_d.cpu().numpy()[left:]).all() and (ids_d.cpu().numpy()[left:] == -1).all()
    eng.close()


@pytest.mark.parametrize("m", [1, 2, 3])
def test_quorum_when_the_mask_blocks_most_of_the_unmasked_list(m):
    """Every pair among the positions of the unmasked top 64, but those of its last rows, is blocked:
    a pruning bound seeded from blocked candidates would cut the masked list short."""
    K, P, th, pr = seeded_case()
    eng = engine(th[:3].copy(), pr[:3].copy())
    s0, ids0 = eng.quorum_top(64, m)
    _, rank = scan_ref.rank_tables(P)
    pos = np.unique(rank[ids0[:60]])
    sel = np.zeros((P, P), dtype=bool)
    sel[np.ix_(pos, pos)] = True
    mask = masked_ref.position_mask(P, sel)
    union = masked_ref.expand(mask, P)
    want = eng.quorum_top(64, m, union)                                 # the reference first
    unmasked = set(packed(ids0, P).tolist())
    differ = sum(int(k) not in unmasked for k in packed(want[1], P))
    assert want[0].size == 64 and differ > 32, "the mask leaves most of the unmasked list in place"
    assert want[0][-1] < s0[-1]                                         # below the unmasked N-th best
    same(eng.quorum_top(64, m, None, mask=mask), want)
    same(eng.quorum_top(1000, m, None, mask=mask), eng.quorum_top(1000, m, union))
    eng.close()


# ------------------------------------------------------------------ 6. raw C calls
def test_raw_calls_null_mask_and_capacity():
    import torch
    from trigenicinteractionpredictor_amd import _lib
    K, P, B = 10, P_MATRIX, 3
    th, pr, per, scores, keys = case(K, B, P, 41)
    mask, blocked_keys = mask_case("random", P)
    eng = engine(th.copy(), pr.copy())
    t = float(np.quantile(scores, 0.5))                         # low enough for rows that every slot votes for
    # a NULL mask: refused, outputs intact
    rawp = MaskedRaw(eng, "pair_census", 2)
    thr = rawp.upload(np.array([0.4, 0.6]))
    assert rawp.call(None, (thr.data_ptr(), 2), [rawp.full((P, P, 2), torch.int32)], -1) == _lib.MMSBM_ERR_INVALID
    assert rawp.intact() and b"mask" in eng.lib.mmsbm_last_error()
    rawv = MaskedRaw(eng, "scan_votes")
    assert rawv.call(None, (t, 1, 64), votes_outs(rawv, B, 64), -1) == _lib.MMSBM_ERR_INVALID
    assert rawv.intact() and b"mask" in eng.lib.mmsbm_last_error()
    rawq = MaskedRaw(eng, "scan_quorum", 64)
    assert rawq.call(None, (1, 64), quorum_outs(rawq, 64), -1) == _lib.MMSBM_ERR_INVALID
    assert rawq.intact() and b"mask" in eng.lib.mmsbm_last_error()
    # the workspaces are the unmasked calls': the masked calls above ran on them, and they have not grown
    # capacity below the count: the full count, `capacity` distinct hits, nothing at or past it
    m = device_mask(rawv, mask)
    for sample, min_votes in ((-1, 1), (-1, B), (0, 1)):
        ns = B if sample < 0 else 1
        hist = eng.vote_census(t, None, None if sample < 0 else sample, mask=mask)
        want = int(hist[min_votes:].sum())
        votes, s, ids = eng.consensus(t, min_votes, None, None if sample < 0 else sample, mask=mask)
        assert votes.size == want > 300
        capacity = want - 200
        outs = votes_outs(rawv, ns, capacity + 300)
        assert rawv.call(m.data_ptr(), (t, min_votes, capacity), outs, sample) == _lib.MMSBM_OK
        np.testing.assert_array_equal(outs[0].cpu().numpy(), hist)
        assert int(outs[4].cpu()[0]) == want                               # always the full count
        sc, k, v = (o.cpu().numpy() for o in outs[1:4])
        assert (sc[capacity:] == SENTINEL).all() and (k[capacity:] == SENTINEL).all() and (v[capacity:] == SENTINEL).all()
        assert np.unique(k[:capacity]).size == capacity and np.isin(k[:capacity], packed(ids, P)).all()
        assert not masked_ref.blocked(k[:capacity], mask, P).any()
        # a histogram-only call with NULL arrays
        outs = [rawv.full((ns + 1,), torch.int64), None, None, None, rawv.full((1,), torch.int64)]
        assert rawv.call(m.data_ptr(), (t, min_votes, 0), outs, sample) == _lib.MMSBM_OK
        assert int(outs[4].cpu()[0]) == want
    eng.close()


def test_p_above_the_cap_is_refused():
    """P = 16400 on a scratch context without links: the three masked calls return UNSUPPORTED before
    any device call."""
    import torch
    from trigenicinteractionpredictor_amd import _lib
    lib = _lib.load()
    K, P = 2, 16400
    dev = torch.device("cuda", torch.cuda.current_device())
    ctx = ctypes.c_void_p()
    _lib.check(lib.mmsbm_create(dev.index, ctypes.byref(ctx)))
    try:
        _lib.check(lib.mmsbm_set_shape(ctx, K, 2, 1, P, 1e-10))
        order = torch.arange(P, dtype=torch.int32, device=dev)
        theta = torch.full((1, P, K), 0.5, dtype=torch.float64, device=dev)
        pr = torch.full((1, 2, K ** 3), 0.5, dtype=torch.float64, device=dev)
        mask = torch.zeros((16400, 513), dtype=torch.int32, device=dev)
        outs = [torch.full((64,), SENTINEL, dtype=d, device=dev)
                for d in (torch.int64, torch.float64, torch.int64, torch.int32, torch.int64)]
        ids = torch.full((8, 3), SENTINEL, dtype=torch.int32, device=dev)
        thr = torch.full((1,), 0.5, dtype=torch.float64, device=dev)
        stream = torch.cuda.current_stream(dev).cuda_stream
        head = (ctx, order.data_ptr(), None, 0, mask.data_ptr(), theta.data_ptr(), pr.data_ptr(), 0)
        nbytes = ctypes.c_int64()
        _lib.check(lib.mmsbm_scan_votes_workspace_bytes(ctx, ctypes.byref(nbytes)))
        ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
        rc = lib.mmsbm_scan_votes_masked(*head, 0.5, 1, 8, ws.data_ptr(), ws.numel(), outs[0].data_ptr(),
                                         outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(),
                                         outs[4].data_ptr(), stream)
        assert rc == _lib.MMSBM_ERR_UNSUPPORTED and b"16384" in lib.mmsbm_last_error()
        _lib.check(lib.mmsbm_scan_quorum_workspace_bytes(ctx, 8, ctypes.byref(nbytes)))
        ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
        rc = lib.mmsbm_scan_quorum_topn_masked(*head, 1, 8, ws.data_ptr(), ws.numel(), outs[1].data_ptr(),
                                               ids.data_ptr(), outs[4].data_ptr(), stream)
        assert rc == _lib.MMSBM_ERR_UNSUPPORTED and b"16384" in lib.mmsbm_last_error()
        # the pair census has the same cap of its own; the output is never touched, so a small one will do
        rc = lib.mmsbm_pair_census_masked(*head, thr.data_ptr(), 1, ws.data_ptr(), ws.numel(), outs[3].data_ptr(),
                                          stream)
        assert rc == _lib.MMSBM_ERR_UNSUPPORTED and b"16384" in lib.mmsbm_last_error()
        torch.cuda.synchronize(dev)
        assert all(bool((o == SENTINEL).all()) for o in outs + [ids])
    finally:
        lib.mmsbm_destroy(ctx)


@pytest.mark.parametrize("B,sample", [(1, 0), (10, None)], ids=["single", "ensemble"])
def test_results_do_not_depend_on_the_grid_or_on_repeats(B, sample, monkeypatch):
    K, P = 10, P_MATRIX
    th, pr, per, scores, keys = case(K, B, P, 500 + K + B if B > 1 else 5)
    mask, _ = mask_case("random", P)
    known = some_known(keys)
    eng = engine(th.copy(), pr.copy())
    thr, t = levels(scores, LEVELS8), float(np.quantile(scores, 0.9))
    for var in GRID_VARS:
        monkeypatch.delenv(var, raising=False)
    want = families(eng, known, sample, mask, thr, t, depths=(4, 7))
    assert want[1].any() and want[3][0].size > 500
    for grid in (None, "1", "7"):
        for var in GRID_VARS:
            if grid is not None:
                monkeypatch.setenv(var, grid)
        same(families(eng, known, sample, mask, thr, t, depths=(4, 7)), want)
    eng.close()


# ------------------------------------------------------------------ 7. the Python surface
def test_model_mask_keywords_against_numpy():
    from trigenicinteractionpredictor_amd import Model
    from trigenicinteractionpredictor_amd.scan import known_keys, pair_eligible
    from golden_util import load
    _, vec, train, test = load("tiny", "K10_s1")
    m = Model()
    m.get_traintest(train, test)
    m.initialize_parameters(vec["theta_5"].shape[1])
    m.theta, m.pr = vec["theta_5"].tolist(), vec["pr_5"].tolist()
    P = m.P
    scores, keys = scan_ref.ref_scores(vec["theta_5"], vec["pr_5"])
    genes = list(range(0, P, 2))
    pairs = [(0, 2), (4, 8)]
    mask = m.pair_mask(genes=[m.id_gene[g] for g in genes], pairs=pairs)
    np.testing.assert_array_equal(mask, masked_ref.naive_from_ids(P, pairs, genes))
    known = known_keys(m)
    union = union_of(known, masked_ref.expand(mask, P))
    thresholds = census_ref.gap_thresholds(scores, 5)
    census_ref.assert_clear(scores, thresholds)                 # the precondition, reference alone
    t = float(np.sort(thresholds)[2])
    rank_mat, gene_mat = pair_census_ref.ref_pairs(scores, keys, P, thresholds, union)
    np.testing.assert_array_equal(m.novel_pair_counts(thresholds, mask=mask), gene_mat)
    got = m.novel_gene_counts(thresholds, mask=mask)
    assert got.dtype == np.int64 and got.shape == (P, thresholds.size)
    np.testing.assert_array_equal(got, pair_census_ref.ref_gene_counts(scores, keys, P, thresholds, union))
    assert got.any() and not got[1::2].any()                    # nothing for a gene outside the universe
    rows = m.predict_query_pairs(7, t, mask=mask)
    want_counts, want_ids = pair_census_ref.top_pairs(
        pair_census_ref.ref_pairs_rank(scores, keys, P, [t], union)[:, :, 0], 7)
    el = pair_eligible(P, known, mask)
    np.testing.assert_array_equal(el, pair_census_ref.to_gene_ids(
        pair_census_ref.ref_pairs_rank(scores, keys, P, [-1.0], union))[:, :, 0])
    assert len(rows) == 7 and want_counts[0] > 0
    for (count, eligible, key, names), n, (i, j) in zip(rows, want_counts, want_ids):
        assert key == "%d_%d" % (i, j) and names == sorted([m.id_gene[int(i)], m.id_gene[int(j)]])
        assert count == n and eligible == el[i, j] and count <= eligible
    assert m.predict_query_pairs(7, t) != rows
    assert m.predict_query_pairs(7, t, mask=None) == m.predict_query_pairs(7, t)


def joint_model(case_name, name, it=5):
    from trigenicinteractionpredictor_amd.joint import DataType, Model
    meta, vec, train, test = joint_load(case_name, name)
    m = Model()
    m.get_train_test(train, test)
    random.seed(meta["seed"])
    m.initialize_parameters(meta["K"], getattr(DataType, meta["interaction"]))
    m.theta, m.pr, m.qr = vec["theta_%d" % it].tolist(), vec["pr_%d" % it].tolist(), vec["qr_%d" % it].tolist()
    return m, vec["theta_%d" % it], vec["pr_%d" % it], vec["qr_%d" % it]


def test_joint_trigenic_query_pairs():
    from trigenicinteractionpredictor_amd.scan import pair_eligible
    m, theta, pr, qr = joint_model("tiny", "K10_s1")
    P = m.P
    order, rank = scan_ref.rank_tables(P)
    x, y = np.triu_indices(P, 1)
    pred = np.einsum("nx,ny,xy->n", theta[order[x]], theta[order[y]], np.asarray(qr)[..., 1])
    s = np.sort(pred)
    lo, hi = s.size // 4, 3 * s.size // 4
    g = lo + int(np.argmax(s[lo + 1:hi] - s[lo:hi - 1]))
    threshold = float((s[g] + s[g + 1]) / 2)                    # the widest gap of the middle half
    assert int((np.abs(pred - threshold) <= 1e-9 * threshold).sum()) == 0
    mask = m.digenic_mask(threshold)
    measured3 = [[int(v) for v in key.split("_")] for table in (m.links, m.test_links) for key in table
                 if key.count("_") == 2]
    known = np.unique(packed(np.array([t for t in measured3 if len(set(t)) == 3]), P))
    union = union_of(known, masked_ref.expand(mask, P))
    scores, keys = scan_ref.ref_scores(theta, pr)
    assert 64 < keys.size - union.size < keys.size
    t = threshold_near(scores[~np.isin(keys, union)], 0.7)
    census_ref.assert_clear(scores, [t])                        # the precondition, reference alone
    rows = m.predict_trigenic_query_pairs(9, t, threshold)
    want_counts, want_ids = pair_census_ref.top_pairs(
        pair_census_ref.ref_pairs_rank(scores, keys, P, [t], union)[:, :, 0], 9)
    el = pair_eligible(P, known, mask)
    assert len(rows) == 9 and want_counts[0] > 0
    for (count, eligible, key, names), n, (i, j) in zip(rows, want_counts, want_ids):
        assert key == "%d_%d" % (i, j) and names == sorted([m.id_gene[int(i)], m.id_gene[int(j)]])
        assert count == n and eligible == el[i, j] and count <= eligible


def test_async_calls_return_device_tensors():
    import torch
    K, P, B = 10, P_MATRIX, 3
    th, pr, per, scores, keys = case(K, B, P, 41)
    mask, _ = mask_case("random", P)
    eng = engine(th.copy(), pr.copy())
    t = float(np.quantile(scores, 0.9))
    stream = torch.cuda.Stream(eng.device)
    for st in (None, stream):
        sync = (stream if st is not None else torch.cuda.current_stream(eng.device)).synchronize
        mat = eng.pair_census_async([t], stream=st, mask=mask)
        hist = eng.vote_census_async(t, stream=st, mask=mask)
        votes, s, ids = eng.consensus_async(t, 2, stream=st, mask=mask)
        qs, qids, count = eng.quorum_top_async(64, 2, stream=st, mask=mask)
        sync()
        assert all(x.is_cuda for x in (mat, hist, votes, s, ids, qs, qids, count))
        same(mat.cpu().numpy(), eng.pair_census([t], stream=st, mask=mask))
        same(hist.cpu().numpy(), eng.vote_census(t, stream=st, mask=mask))
        same((votes.cpu().numpy(), s.cpu().numpy(), ids.cpu().numpy()), eng.consensus(t, 2, stream=st, mask=mask))
        same((qs.cpu().numpy(), qids.cpu().numpy()), eng.quorum_top(64, 2, stream=st, mask=mask))
    with pytest.raises(ValueError):
        eng.pair_census([t], mask=mask.astype(np.int64))        # before anything is uploaded
    with pytest.raises(ValueError):
        eng.quorum_top(5, 1, mask=mask[:-1])
    with pytest.raises(ValueError):
        eng.vote_census(t, mask=np.asfortranarray(mask))
    eng.close()
