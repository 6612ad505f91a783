"""The pair mask in the genome-wide top-N scan (include/mmsbm.h mmsbm_scan_topn_masked) on the GPU,
through EMEngine.scan_top(mask=), the raw C call, scan_top_any, Model, joint.Model and the driver.

The oracle, as in tests/test_gpu_scan_masked_families.py, is the unmasked call: a mask stands for the
key table of every triple that contains a blocked pair (masked_ref.expand), so the masked scan_top
must return what the unmasked scan_top returns under known + expand(mask), row for row: ids equal,
score BYTES equal (both sides run one score phase, so there is no tolerance), with `known` empty and
with a live `known`.  One case per mask is held against numpy over scan_ref's scores, with the
project's gap precondition asserted on the reference alone.

The masks come from tests/masked_ref.py, never from the code under test.  P = 70 (54,740 triples) is
the shape of the matrix; P = 203 is the smallest at which the seeding pass runs with a third of the
genes allowed leaving it fewer than N eligible triples."""
import functools
import itertools
import os
import random
from math import comb

import numpy as np
import pytest

import converged_ref
import masked_ref
import scan_ref
import scan_rule
from golden_util import GOLDEN, joint_load, load
from scan_gpu import Raw, engine
from scan_ref import RTOL, bits, packed, prefix_mean

pytestmark = pytest.mark.gpu

P_MATRIX = 70
EMPTY = np.zeros(0, np.int64)
NS = (1, 64, 1000, 4096)        # 1 sorts constantly; 4096 keeps the candidate buffer in the workspace
MASKS = {"random": masked_ref.random_mask, "allowed": masked_ref.allowed_mask, "block": masked_ref.block_mask,
         "single": masked_ref.single_pair_mask, "last_tile": masked_ref.last_tile_mask, "tiles": masked_ref.tiles_mask,
         "full": masked_ref.full_mask, "zero": lambda P: masked_ref.naive_mask(P, [])}


@pytest.fixture(autouse=True)
def no_grid_override(monkeypatch):
    monkeypatch.delenv("MMSBM_SCAN_GRID", raising=False)


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


@functools.lru_cache(maxsize=None)
def params(K, B, P, seed):
    """The parameters alone, where no numpy reference is needed (P = 203)."""
    th, pr = scan_ref.random_params(K, P, seed, B)
    th.setflags(write=False)
    pr.setflags(write=False)
    return th, pr


@functools.lru_cache(maxsize=None)
def mask_case(name, P):
    """(mask, expand(mask)) of one of the shared masks, computed once, read-only."""
    mask = np.ascontiguousarray(MASKS[name](P))
    assert mask.dtype == np.uint32 and mask.shape == masked_ref.shape(P)
    keys = masked_ref.expand(mask, P)
    mask.setflags(write=False)
    keys.setflags(write=False)
    return mask, keys


@functools.lru_cache(maxsize=None)
def every_key(P):
    keys = masked_ref.all_keys(P)
    keys.setflags(write=False)
    return keys


def some_known(keys):
    return np.ascontiguousarray(keys[::4])


def union_of(known, blocked_keys):
    return np.union1d(EMPTY if known is None else known, blocked_keys).astype(np.int64)


def same_list(got, want):
    assert got[0].dtype == np.float64 and got[1].dtype == np.int32
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape
    assert bits(got[0]) == bits(want[0])
    np.testing.assert_array_equal(got[1], want[1])


def check_identity(eng, P, name, known, sample, ns=NS):
    """Mask = keys, for every N: -> the rows of the longest list."""
    mask, blocked_keys = mask_case(name, P)
    rows = 0
    for n in ns:
        got = eng.scan_top(n, known, sample, mask=mask)
        same_list(got, eng.scan_top(n, union_of(known, blocked_keys), sample))
        eligible = comb(P, 3) - union_of(known, blocked_keys).size
        assert got[0].size == min(n, eligible)
        rows = max(rows, got[0].size)
    return rows


# ------------------------------------------------------------------ 1. the kernel matrix at P = 70
SINGLE_K = [1, 2, 4, 5, 10, 13, 20, 22, 26, 30, 32]      # KS = 1, 1, 1, 2, 3, 4, 5, 6, 7, 8, 8
# the issue's ensembles (all at WB = 4) and two more, so that every width pick_wb returns is run
ENSEMBLES = [(10, 2, 4), (10, 4, 4), (10, 8, 4), (30, 3, 4), (10, 10, 2), (10, 19, 1)]


@pytest.mark.parametrize("K", SINGLE_K)
def test_every_ks_single_sample(K):
    assert sorted(set((k + 3) // 4 for k in SINGLE_K)) == list(range(1, 9))
    th, pr, per, scores, keys = case(K, 1, P_MATRIX, 300 + K)
    eng = engine(th.copy(), pr.copy())
    for name in ("random", "tiles"):
        for known in (None, some_known(keys)):
            assert check_identity(eng, P_MATRIX, name, known, 0) == 4096
    eng.close()


@pytest.mark.parametrize("K,B,WB", ENSEMBLES, ids=["K%dxB%d-WB%d" % e for e in ENSEMBLES])
def test_ensembles_at_every_width(K, B, WB):
    assert scan_rule.width(K, B) == WB, "the row-block rule moved: this case no longer runs at WB = %d" % WB
    th, pr, per, scores, keys = case(K, B, P_MATRIX, 500 + K + B)
    eng = engine(th.copy(), pr.copy())
    for name in ("random", "tiles"):
        for known in (None, some_known(keys)):
            assert check_identity(eng, P_MATRIX, name, known, None) == 4096
    check_identity(eng, P_MATRIX, "random", some_known(keys), 1, ns=(64,))      # a slot of the batch
    eng.close()


@pytest.mark.parametrize("name", sorted(set(MASKS) - {"full", "zero"}))
def test_a_mask_is_the_key_table_it_stands_for(name):
    th, pr, per, scores, keys = case(10, 1, P_MATRIX, 5)
    eng = engine(th.copy(), pr.copy())
    for known in (None, some_known(keys)):
        assert check_identity(eng, P_MATRIX, name, known, 0) >= 1000
    eng.close()


def test_the_masks_block_what_they_were_chosen_for():
    P = P_MATRIX
    assert comb(P, 3) == 54740
    assert 0.2 * 54740 < mask_case("random", P)[1].size < 0.35 * 54740
    assert 54740 - mask_case("allowed", P)[1].size == comb(24, 3)
    assert mask_case("single", P)[1].size == P - 2
    assert mask_case("full", P)[1].size == 54740 and mask_case("zero", P)[1].size == 0
    # P = 203: every 61st item of a third of the genes holds fewer than 1000 eligible triples
    assert comb(203, 3) - mask_case("allowed", 203)[1].size == comb(68, 3) < 61 * 1000


# ------------------------------------------------------------------ 2. the seeding pass
@pytest.mark.parametrize("name", ["allowed", "random"])
@pytest.mark.parametrize("K,B", [(10, 1), (3, 2)], ids=["K10", "K3xB2"])
def test_the_seeding_pass_under_a_mask(K, B, name):
    """P = 203 >= 200: the seeding pass runs.  Under `allowed` it finds fewer than N eligible triples
    (its bound then must stay unpublished or low); under `random` it finds its N among the eligible
    ones only: a bound formed from a blocked triple would cut the masked list short."""
    P = 203
    th, pr = params(K, B, P, 77)
    mask, blocked_keys = mask_case(name, P)
    eng = engine(th.copy(), pr.copy())
    sample = 0 if B == 1 else None
    for known in (None, np.ascontiguousarray(every_key(P)[::5])):
        for n in (1000, 4096):
            got = eng.scan_top(n, known, sample, mask=mask)
            same_list(got, eng.scan_top(n, union_of(known, blocked_keys), sample))
            assert got[0].size == n
    eng.close()


# ------------------------------------------------------------------ 3. small gene counts
@pytest.mark.parametrize("P", [3, 4, 16, 17, 33])
def test_small_gene_counts(P):
    th, pr, per, scores, keys = case(3, 2, P, 11 + P)
    eng = engine(th.copy(), pr.copy())
    for sample in (0, None):
        plain = eng.scan_top(64, None, sample)
        assert plain[0].size == min(64, comb(P, 3))
        same_list(eng.scan_top(64, None, sample, mask=mask_case("zero", P)[0]), plain)
        s, ids = eng.scan_top(64, None, sample, mask=mask_case("full", P)[0])
        assert s.size == 0 and ids.shape == (0, 3)
        for known in (None, keys[::3].copy()):
            rows = check_identity(eng, P, "single", known, sample, ns=(1, 64))
            assert rows == min(64, comb(P, 3) - union_of(known, mask_case("single", P)[1]).size)
    eng.close()


def test_a_full_mask_writes_an_empty_result():
    import torch
    th, pr, per, scores, keys = case(10, 3, P_MATRIX, 41)
    eng = engine(th.copy(), pr.copy())
    full, every = mask_case("full", P_MATRIX)
    assert every.size == comb(P_MATRIX, 3)
    for sample in (0, None):
        for n in (64, 4096):
            s, ids, count = eng.scan_top_async(n, None, sample, mask=full)
            torch.cuda.synchronize()
            assert int(count.cpu()[0]) == 0
            assert np.isnan(s.cpu().numpy()).all() and (ids.cpu().numpy() == -1).all()
    eng.close()


@pytest.mark.parametrize("B,sample", [(1, 0), (3, None), (3, 1)], ids=["single", "ensemble", "slot"])
def test_an_all_zero_mask_is_the_unmasked_call(B, sample):
    th, pr, per, scores, keys = case(10, B, P_MATRIX, 41)
    zero, none = mask_case("zero", P_MATRIX)
    assert not zero.any() and none.size == 0
    eng = engine(th.copy(), pr.copy())
    for known in (None, some_known(keys)):
        for n in NS:
            got = eng.scan_top(n, known, sample, mask=zero)
            same_list(got, eng.scan_top(n, known, sample))
            assert got[0].size == n
    eng.close()


# ------------------------------------------------------------------ 4. the grid and repeats
@pytest.mark.parametrize("B,sample", [(1, 0), (10, None)], ids=["single", "ensemble"])
def test_the_list_does_not_depend_on_the_grid_or_on_repeats(B, sample, monkeypatch):
    th, pr, per, scores, keys = case(10, B, P_MATRIX, 500 + 10 + B if B > 1 else 5)
    mask, _ = mask_case("random", P_MATRIX)
    known = some_known(keys)
    eng = engine(th.copy(), pr.copy())
    for n in (64, 4096):
        want = eng.scan_top(n, known, sample, mask=mask)
        assert want[0].size == n
        for grid in (None, "1", "7", "33"):
            if grid is not None:
                monkeypatch.setenv("MMSBM_SCAN_GRID", grid)
            same_list(eng.scan_top(n, known, sample, mask=mask), want)
        monkeypatch.delenv("MMSBM_SCAN_GRID")
    eng.close()


# ------------------------------------------------------------------ 5. ties
def test_ties_resolve_by_packed_key_under_a_mask():
    """Every gene the same theta row: every score shares its bits and the list is the first eligible
    keys.  The mask blocks the pairs (0, 1) and (2, 5) of rank positions."""
    K, P, N = 5, 37, 50
    th, pr = scan_ref.random_params(K, 1, 7)
    th = np.repeat(th, P, axis=1)
    eng = engine(th, pr)
    mask = masked_ref.naive_mask(P, [(0, 1), (2, 5)])
    triples = np.array(list(itertools.combinations(range(P), 3)))
    all_keys = (triples[:, 0] * P + triples[:, 1]) * P + triples[:, 2]
    live = all_keys[~masked_ref.blocked(all_keys, mask, P)]
    assert live.size == all_keys.size - 2 * (P - 2) and live[0] == (0 * P + 2) * P + 3
    s, ids = eng.scan_top(N, mask=mask)
    assert np.unique(s.view(np.int64)).size == 1        # all scores share their bits
    np.testing.assert_array_equal(ids, scan_ref.keys_to_ids(live[:N], P))
    s2, ids2 = eng.scan_top(N, known=live[:10].copy(), mask=mask)
    np.testing.assert_array_equal(ids2, scan_ref.keys_to_ids(live[10:N + 10], P))
    np.testing.assert_array_equal(s2.view(np.int64), s.view(np.int64))
    eng.close()


# ------------------------------------------------------------------ 6. against numpy
@pytest.mark.parametrize("name", sorted(set(MASKS) - {"full", "zero"}))
def test_against_numpy(name):
    K, P, N = 10, P_MATRIX, 64
    th, pr, per, scores, keys = case(K, 1, P, 5)
    mask, _ = mask_case(name, P)
    eng = engine(th.copy(), pr.copy())
    for known in (None, some_known(keys)):
        out = masked_ref.blocked(keys, mask, P)
        if known is not None:
            out |= np.isin(keys, known)
        want_s, want_k = scan_ref.top(scores[~out], keys[~out], N)
        assert scan_ref.min_gap(want_s) > 1e-9                  # the precondition, reference alone
        s, ids = eng.scan_top(N, known, 0, mask=mask)
        np.testing.assert_array_equal(ids, scan_ref.keys_to_ids(want_k[:N], P))
        np.testing.assert_allclose(s, want_s[:N], rtol=RTOL, atol=0)
        assert not masked_ref.blocked(packed(ids, P), mask, P).any()
    eng.close()


# ------------------------------------------------------------------ 7. scan_top_any
def test_scan_top_any_under_a_mask():
    K, P = 10, P_MATRIX
    th, pr, per, scores, keys = case(K, 1, P, 5)
    mask, _ = mask_case("random", P)
    out = masked_ref.blocked(keys, mask, P)
    eng = engine(th.copy(), pr.copy())
    same_list(eng.scan_top_any(64, None, 0, mask=mask), eng.scan_top(64, None, 0, mask=mask))
    # n above the cap and above the masked total: all of them, best first, from the bracket route
    s, ids = eng.scan_top_any(60000, None, 0, mask=mask)
    assert s.size == int((~out).sum()) > 4096 and (np.diff(s) <= 0).all()
    np.testing.assert_array_equal(np.sort(packed(ids, P)), keys[~out])
    assert bits(s[:4096]) == bits(eng.scan_top(4096, None, 0, mask=mask)[0])
    # n above the cap under a mask that leaves fewer than the cap: the masked scan_top(max) is all there is
    allowed, gone = mask_case("allowed", P)
    s, ids = eng.scan_top_any(5000, None, 0, mask=allowed)
    assert s.size == comb(24, 3) == keys.size - gone.size
    same_list((s, ids), eng.scan_top(4096, np.array(gone), 0))       # a copy: the shared keys are read-only
    with pytest.raises(ValueError):
        eng.scan_top_any(0, mask=mask)
    eng.close()


# ------------------------------------------------------------------ 8. errors
class MaskedRaw(Raw):
    """scan_gpu.Raw for mmsbm_scan_topn_masked: the mask pointer goes behind n_known."""

    def call(self, mask_ptr, mid, outs, sample=0, known=None):
        eng = self.eng
        known_d = None if known is None else self.upload(known)
        self.outs = outs
        rc = eng.lib.mmsbm_scan_topn_masked(
            eng.ctx, eng.scan_order.data_ptr(), None if known is None else known_d.data_ptr(),
            0 if known is None else int(known.size), mask_ptr, eng.theta.data_ptr(), eng.pr.data_ptr(), sample, *mid,
            self.ws.data_ptr(), self.ws.numel(), *[None if o is None else o.data_ptr() for o in outs], eng._stream())
        self.torch.cuda.synchronize(eng.device)
        return rc


def test_errors():
    import torch
    from trigenicinteractionpredictor_amd import _lib
    K, P = 10, P_MATRIX
    th, pr, per, scores, keys = case(K, 1, P, 5)
    mask, blocked_keys = mask_case("random", P)
    eng = engine(th.copy(), pr.copy())
    raw = MaskedRaw(eng, "scan", 64)

    def outs(n=64):
        return [raw.full((n,), torch.float64), raw.full((n, 3), torch.int32), raw.full((1,), torch.int64)]

    # a NULL mask: refused, outputs intact
    assert raw.call(None, (64,), outs()) == _lib.MMSBM_ERR_INVALID and raw.intact()
    assert b"mask" in eng.lib.mmsbm_last_error()
    # the raw call with a mask is the engine's list
    m = raw.upload(np.array(mask).view(np.int32))
    o = outs()
    assert raw.call(m.data_ptr(), (64,), o) == _lib.MMSBM_OK and int(o[2].cpu()[0]) == 64
    same_list((o[0].cpu().numpy(), o[1].cpu().numpy()), eng.scan_top(64, blocked_keys, 0))
    # N = 0 and N above the cap
    assert raw.call(m.data_ptr(), (0,), outs()) == _lib.MMSBM_ERR_INVALID and raw.intact()
    assert raw.call(m.data_ptr(), (4097,), outs()) == _lib.MMSBM_ERR_UNSUPPORTED and raw.intact()
    with pytest.raises(_lib.MMSBMError) as e:
        eng.scan_top(0, mask=mask)
    assert e.value.code == _lib.MMSBM_ERR_INVALID
    with pytest.raises(_lib.MMSBMError) as e:
        eng.scan_top(eng.lib.mmsbm_scan_max_n() + 1, mask=mask)
    assert e.value.code == _lib.MMSBM_ERR_UNSUPPORTED
    # a mask of the wrong dtype or shape through EMEngine
    for bad in (mask.astype(np.int64), mask.astype(np.int32), mask[:-1], mask[:, :-1], mask.T, mask.tolist()):
        with pytest.raises(ValueError):
            eng.scan_top(8, mask=bad)
        with pytest.raises(ValueError):
            eng.scan_top_async(8, mask=bad)
    eng.close()


# ------------------------------------------------------------------ 9. the converged regime
@pytest.mark.parametrize("name", ["A_s1_T300", "C20_s1_T300"])
def test_on_a_converged_fit(name):
    """Scores crowded near 0 and 1, many sharing their bits: the order is the key's, and the masked
    list is still the unmasked one under the expanded keys."""
    ck = converged_ref.load(name)
    theta, pr = np.asarray(ck.theta), np.asarray(ck.pr)
    P = theta.shape[0]
    if name.startswith("C20"):
        assert theta.shape[1] > 12
    eng = engine(theta[None].copy(), pr[None].copy())
    keys = every_key(P)
    for mname in ("random", "allowed"):
        for known in (None, some_known(keys)):
            check_identity(eng, P, mname, known, 0, ns=(64, 1000))
    eng.close()


# ------------------------------------------------------------------ 10. Model, joint.Model, the driver
def tiny_model():
    from trigenicinteractionpredictor_amd import Model
    _, vec, train, test = load("tiny", "K10_s1")
    m = Model()
    m.get_traintest(train, test)
    m.initialize_parameters(vec["theta_5"].shape[1])
    m.theta, m.pr = vec["theta_5"].tolist(), vec["pr_5"].tolist()
    return m


def test_model_predict_novel_mask():
    m = tiny_model()
    genes = [m.id_gene[g] for g in range(0, m.P, 2)]
    mask = m.pair_mask(genes=genes, pairs=[(0, 2)])
    rows = m.predict_novel(30, mask=mask)
    allowed = set(genes)
    assert len(rows) == 30 and all(set(r[2]) <= allowed for r in rows)
    assert all(not {"0", "2"} <= set(r[1].split("_")) for r in rows)
    assert all(r[1] not in m.links and r[1] not in m.test_links for r in rows)
    assert rows == m.predict_novel_any(30, mask=mask)
    assert rows == m.predict_network(rows[-1][0], mask=mask)[:30]         # the masked threshold scan's rows
    assert m.predict_novel(30) != rows
    assert m.predict_novel(30, exclude=(), mask=mask)[0][0] >= rows[0][0]
    with pytest.raises(ValueError):
        m.predict_novel(30, mask=mask.astype(np.int64))


def test_joint_predict_novel_trigenic_against_the_census_route():
    """predict_novel_trigenic now is one masked scan_top; the route it had (masked censuses bracket
    the cut from 1.0, the masked threshold scan lists above it) is called here directly."""
    from trigenicinteractionpredictor_amd.joint import DataType, Model
    from trigenicinteractionpredictor_amd.scan import bracket_threshold
    meta, vec, train, test = joint_load("small", "K10_s1")
    m = Model()
    m.get_train_test(train, test)
    random.seed(meta["seed"])
    m.initialize_parameters(meta["K"], getattr(DataType, meta["interaction"]))
    m.theta, m.pr, m.qr = vec["theta_5"].tolist(), vec["pr_5"].tolist(), vec["qr_5"].tolist()
    n, threshold = 200, 0.5
    rows = m.predict_novel_trigenic(n, threshold)
    assert len(rows) == n
    eng = m._push().tri
    mask, known = m.digenic_mask(threshold), m._trigenic_known(("train", "test"))
    assert mask.any()
    lo = bracket_threshold(n, 1.0, lambda t: eng.census(t, known, 0, mask=mask)[0])
    s, ids = eng.scan_above(lo, known, 0, mask=mask)
    assert s.size >= n
    assert [r[1] for r in rows] == ["_".join(str(int(g)) for g in row) for row in ids[:n]]
    assert bits(np.array([r[0] for r in rows])) == bits(s[:n])


def test_the_drivers_main_table_under_allow_genes(tmp_path):
    """One restart: the driver's engine holds what a Model fitted from the same seed holds."""
    from trigenicinteractionpredictor_amd import Model, scan
    g = os.path.join(GOLDEN, "tiny")
    train, test = os.path.join(g, "train.dat"), os.path.join(g, "test.dat")
    m = Model()
    m.get_traintest(train, test)
    genes = [gid for gid in range(m.P) if gid % 4 != 1]
    allow = tmp_path / "allow.txt"
    allow.write_text("".join("%s\n" % (m.id_gene[v] if v % 3 else v) for v in genes))
    out = str(tmp_path / "top.tsv")
    argv = ["-t", train, "-e", test, "-k", "3", "-n", "1", "-i", "5", "--seed", "1", "--top", "40", "-o", out,
            "--allow-genes", str(allow)]
    assert scan.main(argv, out=lambda *a: None) == 0
    lines = open(out, encoding="utf-8").read().rstrip("\n").split("\n")
    assert lines[0].split("\t") == ["rank", "probability", "ids", "names"]
    rows = [ln.split("\t") for ln in lines[1:]]
    random.seed(1)
    m.initialize_parameters(3)
    m.make_iterations(5)
    want = m.predict_novel_any(40, mask=m.pair_mask(genes=genes))
    assert len(rows) == len(want) == 40
    assert [[r[2], r[3].split("_")] for r in rows] == [[k, names] for _, k, names in want]
    np.testing.assert_allclose([float(r[1]) for r in rows], [p for p, _, _ in want], rtol=RTOL)
    assert all(set(int(x) for x in r[2].split("_")) <= set(genes) for r in rows)
