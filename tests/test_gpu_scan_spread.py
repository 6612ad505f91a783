"""Dispute scan (include/mmsbm.h mmsbm_scan_spread_topn, EMEngine.spread_top, the scan driver's
--disputed) against the numpy float64 reference of tests/spread_ref.py over all C(P, 3) triples of
every slot, and against the product's own threshold scan.

The result is the exact top N under a total order, so the tests demand the identical ordered id
list.  Each comparison with the reference first asserts, on the reference alone, that every adjacent
absolute gap inside the reference's top N + 1 exceeds spread_ref.SPREAD_GAP (1e-8 > 4 RTOL: scores
are <= 1, a spread moves by at most 2 RTOL), and compares a spread within RTOL (hi + lo) absolute of
the reference, hi and lo the two slot scores it subtracts.  Large N, where gaps close, is tested
against the product's own bits without a tolerance.
"""
import ctypes
import functools
import os
from math import comb

import numpy as np
import pytest

import masked_ref
import scan_gpu
import scan_ref
import scan_rule
import spread_ref
from golden_util import GOLDEN
from scan_gpu import engine
from scan_ref import packed

pytestmark = pytest.mark.gpu

GRID = "MMSBM_SCAN_SPREAD_GRID"


@pytest.fixture(autouse=True)
def no_grid_override(monkeypatch):
    monkeypatch.delenv(GRID, raising=False)


class Raw(scan_gpu.Raw):
    ENTRY = dict(scan_gpu.Raw.ENTRY, scan_spread="mmsbm_scan_spread_topn")


def same(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and g.tobytes() == w.tobytes() for g, w in zip(got, want))


def check(eng, per, keys, t, n, known=None):
    """spread_top(n, t) against the reference's list: equal ids, spreads within RTOL (hi + lo)."""
    P = eng.P
    want_s, want_k = spread_ref.ref_top(per, keys, t, n, known)    # asserts the gaps
    want_s, want_k = want_s[:n], want_k[:n]
    s, ids = eng.spread_top(n, t, known)
    assert ids.dtype == np.int32 and s.dtype == np.float64 and ids.shape == (want_k.size, 3)
    np.testing.assert_array_equal(ids, scan_ref.keys_to_ids(want_k, P))
    atol = spread_ref.atol(per, t)[np.searchsorted(keys, want_k)]
    assert (np.abs(s - want_s) <= atol).all(), float(np.max(np.abs(s - want_s) - atol))
    if known is not None and len(known):
        assert not np.isin(packed(ids, P), known).any()
    return s, ids


# ------------------------------------------------------------------ 1. the reference
@pytest.mark.parametrize("K,P,B,seed", spread_ref.reference_cases())
def test_against_the_reference(K, P, B, seed):
    """P = 53: interior tiles, boundary tiles and a ragged last tile; P = 20: boundary tiles only."""
    c = spread_ref.case(K, P, seed, B)
    eng = engine(c.theta, c.pr)
    assert eng.spread_max_trim == 3
    trims = eng.spread_trims()
    assert trims == spread_ref.legal(B) == spread_ref.trims(B)      # B <= 8: every legal trim
    for known in spread_ref.exclusions(c.keys, P):
        for t in trims:
            for n in spread_ref.NS:
                check(eng, c.per, c.keys, t, n, known)
    assert same(eng.spread_top(5), eng.spread_top(5, 0))            # the default trim: the range
    eng.close()


# ------------------------------------------------------------------ 2. exact, product against product
def slot_lists(eng, B, P, mask=None):
    """Every slot's full list from the threshold scan, aligned by key: -> (keys int64[T] ascending,
    per f64[B][T] with each slot's own bits)."""
    total = comb(P, 3)
    keys, per = None, []
    for s in range(B):
        sc, ids = eng.scan_above(1e-300, sample=s)      # below every score
        assert sc.size == total
        k = packed(ids, P)
        at = np.argsort(k)
        assert keys is None or np.array_equal(keys, k[at])
        keys = k[at]
        per.append(sc[at])
    return keys, np.stack(per)


def exact_lists(keys, per, t, known=None):
    """The slots' own bits -> (spreads, keys) of every eligible triple under the total order."""
    B = per.shape[0]
    keep = np.ones(keys.size, bool) if known is None else ~np.isin(keys, known)
    srt = np.sort(per, axis=0)
    d = (srt[B - 1 - t] - srt[t])[keep]
    order = np.lexsort((keys[keep], -d))
    return d[order], keys[keep][order]


@pytest.mark.parametrize("K,P,B,seed", spread_ref.EXACT_CASES)
def test_exact_against_the_slots_threshold_scans(K, P, B, seed):
    """No tolerance: sorted[B - 1 - t] - sorted[t] per key of the slots' own scan_above lists, sorted
    under the total order, is spread_top's list in bits and ids; N = 4096 puts the candidate buffer
    in the workspace; P = 211 runs the seeding pass."""
    c = spread_ref.case(K, P, seed, B)
    eng = engine(c.theta, c.pr)
    keys, per = slot_lists(eng, B, P)
    for known in (None, keys[1::9].copy()):
        for t in eng.spread_trims():
            want_s, want_k = exact_lists(keys, per, t, known)
            for n in (1, 5, 300, 4096):
                s, ids = eng.spread_top(n, t, known)
                assert s.size == n
                assert s.tobytes() == want_s[:n].tobytes()
                np.testing.assert_array_equal(ids, scan_ref.keys_to_ids(want_k[:n], P))
    eng.close()


# ------------------------------------------------------------------ 3. few triples
@pytest.mark.parametrize("P", [2, 3])
def test_one_triple_and_none(P):
    c = spread_ref.case(3, P, 11, 3)
    eng = engine(c.theta, c.pr)
    scores, ids, count = (x.cpu().numpy() for x in eng.spread_top_async(4, 0))
    assert int(count[0]) == (0 if P == 2 else 1)
    assert np.isnan(scores[int(count[0]):]).all() and (ids[int(count[0]):] == -1).all()
    s, ids = eng.spread_top(4, 0)
    if P == 2:
        assert s.shape == (0,) and ids.shape == (0, 3) and s.dtype == np.float64 and ids.dtype == np.int32
    else:
        assert ids.tolist() == scan_ref.keys_to_ids(c.keys, 3).tolist()
        assert (np.abs(s - spread_ref.spread(c.per, 0)) <= spread_ref.atol(c.per, 0)).all()
    eng.close()


def test_more_rows_asked_than_there_are_triples():
    K, P, B, seed = 3, 20, 3, 11
    c = spread_ref.case(K, P, seed, B)
    eng = engine(c.theta, c.pr)
    known = c.keys[1::9].copy()
    eligible = comb(P, 3) - known.size
    n = 2048
    assert eligible < n
    scores, ids, count = eng.spread_top_async(n, 0, known)
    scores, ids, count = scores.cpu().numpy(), ids.cpu().numpy(), int(count.cpu()[0])
    assert count == eligible
    assert np.isnan(scores[count:]).all() and (ids[count:] == -1).all()     # the NaN / -1 tail
    keep = ~np.isin(c.keys, known)
    got = packed(ids[:count], P)
    np.testing.assert_array_equal(np.sort(got), c.keys[keep])               # all of them, each once
    at = np.searchsorted(c.keys, got)
    assert (np.abs(scores[:count] - spread_ref.spread(c.per, 0)[at]) <= spread_ref.atol(c.per, 0)[at]).all()
    assert (np.diff(scores[:count]) <= 0).all()
    eng.close()


# ------------------------------------------------------------------ 4. schedule and batch
def test_nothing_depends_on_the_batch_or_the_grid(monkeypatch):
    K, P, B, seed = spread_ref.EXACT_CASES[1]                        # P = 211: the seeding pass
    theta, pr = scan_ref.random_params(K, P, seed, 4)
    known = spread_ref.case(K, P, seed, B).keys[2::7].copy()
    eng = engine(theta, pr)
    assert eng.spread_trims() == [0, 1]
    eng.set_active(3)
    assert eng.spread_trims() == [0]
    three = engine(theta[:3], pr[:3])
    for n in (5, 300, 4096):
        want = three.spread_top(n, 0, known)
        assert want[0].size == n
        assert same(eng.spread_top(n, 0, known), want)               # a prefix of a wider batch
        for grid in ("1", "7"):
            monkeypatch.setenv(GRID, grid)
            assert same(eng.spread_top(n, 0, known), want)
            assert same(three.spread_top(n, 0, known), want)
        monkeypatch.delenv(GRID)
        assert same(eng.spread_top(n, 0, known), want)               # the default again
    with pytest.raises(ValueError):
        eng.spread_top(5, 1)                                         # three slots keep no two scores at t = 1
    three.close()
    eng.close()


# ------------------------------------------------------------------ 5. the kernel matrix
@pytest.mark.parametrize("K,B,WB", spread_ref.matrix_cases(), ids=lambda v: str(v))
def test_kernel_matrix(K, B, WB):
    """KS = 1..8 x the row-block widths 4, 2, 1, every supported trim (held against the
    instantiations by tests/test_spread_host.py), N = 64 against the reference."""
    assert scan_rule.width(K, B) == WB
    c = spread_ref.matrix_case(K, B)
    eng = engine(c.theta, c.pr)
    known = c.keys[1::9].copy()
    assert eng.spread_trims() == spread_ref.trims(B)
    for t in eng.spread_trims():
        check(eng, c.per, c.keys, t, spread_ref.MATRIX_N, known)
    eng.close()


# ------------------------------------------------------------------ 6. the masked call
@functools.lru_cache(maxsize=None)
def mask_case(name, P):
    """(mask, the key table it stands for), read-only.  random: 10 % of the pairs of rank positions,
    made by the tests' own packer; allowed: about half the genes allowed, through scan.pair_mask;
    zero: no pair."""
    from trigenicinteractionpredictor_amd.scan import pair_mask
    if name == "random":
        mask = masked_ref.random_mask(P)
    elif name == "allowed":
        genes = np.sort(np.random.default_rng(P).permutation(P)[:(P + 1) // 2])
        mask = pair_mask(P, genes=genes)
        np.testing.assert_array_equal(mask, masked_ref.naive_from_ids(P, genes=genes.tolist()))
    else:
        mask = masked_ref.naive_mask(P, [])
    mask = np.ascontiguousarray(mask)
    assert mask.dtype == np.uint32 and mask.shape == masked_ref.shape(P)
    keys = masked_ref.expand(mask, P)
    mask.setflags(write=False)
    keys.setflags(write=False)
    return mask, keys


MASKED_SHAPES = [(10, 33, 4, 5), (10, 65, 4, 5), (3, 211, 4, 11)]      # (K, P, B, seed); B = 4: trims 0 and 1


@pytest.mark.parametrize("K,P,B,seed", MASKED_SHAPES)
def test_a_mask_is_the_key_table_it_stands_for(K, P, B, seed):
    """A masked call returns the unmasked call's list with every triple that contains a blocked pair
    added to `known`, bit for bit; an all-zero mask returns the unmasked list."""
    theta, pr = scan_ref.random_params(K, P, seed, B)
    eng = engine(theta, pr)
    all_keys = masked_ref.all_keys(P)
    ns = (5, 64, 1000) if P < 200 else (64, 4096)
    for known in (None, np.ascontiguousarray(all_keys[1::9])):
        empty = np.zeros(0, np.int64) if known is None else known
        zero, none = mask_case("zero", P)
        assert none.size == 0
        for t in eng.spread_trims():
            for n in ns:
                assert same(eng.spread_top(n, t, known, mask=zero), eng.spread_top(n, t, known))
        for name in ("random", "allowed"):
            mask, blocked = mask_case(name, P)
            assert 0 < blocked.size < all_keys.size
            union = np.union1d(empty, blocked).astype(np.int64)
            for t in eng.spread_trims():
                for n in ns:
                    got = eng.spread_top(n, t, known, mask=mask)
                    assert got[0].size == min(n, all_keys.size - union.size) > 0
                    assert same(got, eng.spread_top(n, t, union))
                    assert not masked_ref.blocked(packed(got[1], P), mask, P).any()
    eng.close()


def test_the_masked_list_does_not_depend_on_the_grid(monkeypatch):
    K, P, B, seed = MASKED_SHAPES[2]
    theta, pr = scan_ref.random_params(K, P, seed, B)
    eng = engine(theta, pr)
    mask, _ = mask_case("allowed", P)
    want = eng.spread_top(300, 1, None, mask=mask)
    for grid in ("1", "7"):
        monkeypatch.setenv(GRID, grid)
        assert same(eng.spread_top(300, 1, None, mask=mask), want)
    eng.close()


# ------------------------------------------------------------------ 7. refusals
def spread_outs(raw, n):
    """The three outputs of mmsbm_scan_spread_topn, full of the sentinel."""
    torch = raw.torch
    return [raw.full((n,), torch.float64), raw.full((n, 3), torch.int32), raw.full((1,), torch.int64)]


def intact(outs):
    return all(bool((o == scan_gpu.SENTINEL).all()) for o in outs if o is not None)


def test_refusals_leave_the_outputs_and_the_context_intact():
    from trigenicinteractionpredictor_amd import _lib
    K, P, B, N = 3, 20, 10, 16
    c = spread_ref.case(K, P, 11, B)
    eng = engine(c.theta, c.pr)
    cap = eng.spread_max_trim
    assert cap == int(eng.lib.mmsbm_scan_spread_max_trim()) == 3
    assert spread_ref.legal(B) == [0, 1, 2, 3, 4] and eng.spread_trims() == [0, 1, 2, 3]
    raw = Raw(eng, "scan_spread", N)
    INVALID, UNSUPPORTED = _lib.MMSBM_ERR_INVALID, _lib.MMSBM_ERR_UNSUPPORTED

    def refused(code=INVALID, trim=0, n=N, nulls=(), **kw):
        outs = spread_outs(raw, N)
        for i in nulls:
            outs[i] = None
        rc = raw.call((trim, n), outs, **dict({"sample": -1}, **kw))
        return rc == code and intact(outs)

    for i in (0, 1, 2):
        assert refused(nulls=(i,))                                   # out_scores, out_ids, out_count
    for i in (0, 1, 4, 5):                                           # ctx, order, theta, pr
        assert refused(replace=[(i, None)])
    for sample in (0, 1, B - 1):                                     # one restart has no spread
        assert refused(sample=sample)
        assert b"one restart has no spread" in eng.lib.mmsbm_last_error()
    for sample in (B, B + 1, -2):                                    # outside the active prefix
        assert refused(sample=sample)
    for t in (-1, -5, 5, 6, B, 1 << 30):                             # trim < 0, or fewer than two scores left
        assert refused(trim=t)
        assert b"trim" in eng.lib.mmsbm_last_error()
        with pytest.raises(ValueError):
            eng.spread_top(N, t)
    assert refused(UNSUPPORTED, trim=4)                              # legal (10 - 8 >= 2), above the cap
    assert b"mmsbm_scan_spread_max_trim" in eng.lib.mmsbm_last_error()
    with pytest.raises(_lib.MMSBMError) as e:
        eng.spread_top(N, 4)
    assert e.value.code == UNSUPPORTED
    assert refused(n=0) and refused(n=-1)                            # N < 1
    assert refused(UNSUPPORTED, n=int(eng.lib.mmsbm_scan_max_n()) + 1)
    assert refused(n_known=3) and refused(n_known=-1)                # keys announced, none given
    with pytest.raises(ValueError):
        eng.spread_top(N, 0, known=np.array([5, 3], dtype=np.int64))  # unsorted
    assert refused(ws=(raw.ws.data_ptr(), raw.ws.numel() - 1))       # too small
    assert refused(ws=(raw.ws.data_ptr() + 8, raw.ws.numel() - 8))   # misaligned
    assert refused(ws=(0, raw.ws.numel()))                           # missing
    nbytes = ctypes.c_int64()
    assert eng.lib.mmsbm_scan_spread_workspace_bytes(None, N, ctypes.byref(nbytes)) == INVALID
    assert eng.lib.mmsbm_scan_spread_workspace_bytes(eng.ctx, N, None) == INVALID
    assert eng.lib.mmsbm_scan_spread_workspace_bytes(eng.ctx, 0, ctypes.byref(nbytes)) == INVALID
    # one active slot
    eng.set_active(1)
    assert eng.spread_trims() == []
    assert refused()
    assert b"one restart has no spread" in eng.lib.mmsbm_last_error()
    with pytest.raises(ValueError):
        eng.spread_top(N)
    with pytest.raises(ValueError):
        eng.spread_top_async(N, 0)
    eng.set_active(B)
    # after all of it the context answers, through the C call and the binding
    outs = spread_outs(raw, N)
    assert raw.call((3, N), outs, sample=-1) == 0 and int(outs[2].cpu()[0]) == N
    s, ids = check(eng, c.per, c.keys, 3, 5)
    assert outs[0].cpu().numpy()[:5].tobytes() == s.tobytes()
    eng.close()


def test_an_ensemble_beyond_the_lds_is_refused():
    from trigenicinteractionpredictor_amd import _lib
    K, P, B = 30, 53, 16
    assert scan_rule.width(K, B) == 0 and scan_rule.last_supported(K) == 15
    th, pr = scan_ref.random_params(K, P, 331, B)
    eng = engine(th, pr)
    with pytest.raises(_lib.MMSBMError) as e:
        eng.spread_top(5, 0)                                         # trim 0: the LDS refuses, not the trim
    assert e.value.code == _lib.MMSBM_ERR_UNSUPPORTED
    raw = Raw(eng, "scan_spread", 8)
    outs = spread_outs(raw, 8)
    assert raw.call((0, 8), outs, sample=-1) == _lib.MMSBM_ERR_UNSUPPORTED and intact(outs)
    # the context stays usable: the largest ensemble that fits
    eng.set_active(15)
    assert eng.spread_top(64, 3)[0].size == 64
    eng.close()


class MaskedRaw(Raw):
    """scan_gpu.Raw for the masked entry: the mask pointer goes behind n_known."""

    def call(self, mask_ptr, mid, outs, sample=-1):
        eng = self.eng
        self.outs = outs
        rc = eng.lib.mmsbm_scan_spread_topn_masked(
            eng.ctx, eng.scan_order.data_ptr(), None, 0, mask_ptr, eng.theta.data_ptr(), eng.pr.data_ptr(), sample,
            *mid, self.ws.data_ptr(), self.ws.numel(), *[o.data_ptr() for o in outs], eng._stream())
        self.torch.cuda.synchronize(eng.device)
        return rc


def test_the_masked_call_refuses_a_null_mask_and_p_above_the_cap():
    import torch
    from trigenicinteractionpredictor_amd import _lib
    K, P, B, seed = spread_ref.CASES[2]
    c = spread_ref.case(K, P, seed, B)
    eng = engine(c.theta, c.pr)
    raw = MaskedRaw(eng, "scan_spread", 64)
    assert raw.call(None, (0, 64), spread_outs(raw, 64)) == _lib.MMSBM_ERR_INVALID
    assert raw.intact() and b"mask" in eng.lib.mmsbm_last_error()
    # the same call with a mask runs, on the unmasked call's workspace
    mask, blocked = mask_case("random", P)
    m = raw.upload(np.array(mask).view(np.int32))
    outs = spread_outs(raw, 64)
    assert raw.call(m.data_ptr(), (0, 64), outs) == _lib.MMSBM_OK
    assert outs[0].cpu().numpy().tobytes() == eng.spread_top(64, 0, blocked.copy())[0].tobytes()
    eng.close()
    # P = 16400 on a scratch context without links: UNSUPPORTED before any device call
    lib = _lib.load()
    K, P, B = 2, 16400, 2
    dev = torch.device("cuda", torch.cuda.current_device())
    ctx = ctypes.c_void_p()
    _lib.check(lib.mmsbm_create(dev.index, ctypes.byref(ctx)))
    try:
        _lib.check(lib.mmsbm_set_shape(ctx, K, 2, B, P, 1e-10))
        order = torch.arange(P, dtype=torch.int32, device=dev)
        theta = torch.full((B, P, K), 0.5, dtype=torch.float64, device=dev)
        pr = torch.full((B, 2, K ** 3), 0.5, dtype=torch.float64, device=dev)
        mask = torch.zeros((16400, 513), dtype=torch.int32, device=dev)
        outs = [torch.full(shape, scan_gpu.SENTINEL, dtype=d, device=dev)
                for shape, d in (((8,), torch.float64), ((8, 3), torch.int32), ((1,), torch.int64))]
        nbytes = ctypes.c_int64()
        _lib.check(lib.mmsbm_scan_spread_workspace_bytes(ctx, 8, ctypes.byref(nbytes)))
        ws = torch.empty(int(nbytes.value), dtype=torch.uint8, device=dev)
        rc = lib.mmsbm_scan_spread_topn_masked(ctx, order.data_ptr(), None, 0, mask.data_ptr(), theta.data_ptr(),
                                               pr.data_ptr(), -1, 0, 8, ws.data_ptr(), ws.numel(),
                                               outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(),
                                               torch.cuda.current_stream(dev).cuda_stream)
        assert rc == _lib.MMSBM_ERR_UNSUPPORTED and b"16384" in lib.mmsbm_last_error()
        torch.cuda.synchronize(dev)
        assert intact(outs)
    finally:
        lib.mmsbm_destroy(ctx)


# ------------------------------------------------------------------ 8. the async calls
def test_async_calls_return_device_tensors():
    import torch
    K, P, B, seed = spread_ref.CASES[2]
    c = spread_ref.case(K, P, seed, B)
    eng = engine(c.theta, c.pr)
    mask, _ = mask_case("random", P)
    stream = torch.cuda.Stream(eng.device)
    for st in (None, stream):
        for kw in ({}, {"mask": mask}):
            scores, ids, count = eng.spread_top_async(64, 0, stream=st, **kw)
            (stream if st is not None else torch.cuda.current_stream(eng.device)).synchronize()
            assert all(x.is_cuda for x in (scores, ids, count)) and int(count.cpu()[0]) == 64
            assert scores.dtype == torch.float64 and ids.dtype == torch.int32 and count.dtype == torch.int64
            assert same((scores.cpu().numpy(), ids.cpu().numpy()), eng.spread_top(64, 0, stream=st, **kw))
    eng.close()


# ------------------------------------------------------------------ 9. the driver
def test_driver_writes_the_disputed_table(tmp_path):
    import random
    from trigenicinteractionpredictor_amd import Model, _lib, scan
    from trigenicinteractionpredictor_amd.engine import EMEngine
    from trigenicinteractionpredictor_amd.restarts import stream_states
    g = os.path.join(GOLDEN, "tiny")
    train, test = os.path.join(g, "train.dat"), os.path.join(g, "test.dat")
    K, B, iters, seed, top = 3, 4, 5, 1, 20
    base = ["-t", train, "-e", test, "-k", str(K), "-n", str(B), "-i", str(iters), "--seed", str(seed), "--top",
            str(top)]
    model = Model()
    model.get_traintest(train, test)
    random.seed(seed)
    eng = EMEngine(K, model.P, B=B, R=model.R, eps=model.eps)
    eng.set_links(_lib.SET_TRAIN, *model._link_arrays(0))
    for b, (_, theta, pr) in enumerate(stream_states(model, K, range(B))):
        eng.upload_slot(b, theta, pr)
    eng.iterate(iters)
    known = scan.known_keys(model, ("train", "test"))
    allowed = sorted(range(model.P))[::2]                            # about half the genes
    allow_file = str(tmp_path / "allow.txt")
    with open(allow_file, "w", encoding="utf-8") as f:
        f.write("".join(model.id_gene[x] + "\n" for x in allowed))
    mask = scan.pair_mask(model.P, genes=allowed)
    for T, masked in ((None, False), (1, False), (None, True), (1, True)):      # the default T is 0
        files = [str(tmp_path / f) for f in ("top%s%s.tsv" % (T, masked), "disputed%s%s.tsv" % (T, masked))]
        argv = base + ["-o", files[0], "--disputed", files[1]] + ([] if T is None else ["--disputed-trim", str(T)])
        rc = scan.main(argv + (["--allow-genes", allow_file] if masked else []), out=lambda *a: None)
        assert rc == 0
        t = 0 if T is None else T
        lines = open(files[1], encoding="utf-8").read().rstrip("\n").split("\n")
        assert lines[0] == "# samples\t%d" % B and lines[1] == "# disputed trim\t%d" % t
        assert lines[2].split("\t") == ["rank", "spread", "mean", "min", "max", "ids", "names"]
        rows = [ln.split("\t") for ln in lines[3:]]
        # the rows are EMEngine.spread_top on the same engine state
        scores, ids = eng.spread_top(top, t, known, mask=mask if masked else None)
        assert len(rows) == scores.size == top and [int(r[0]) for r in rows] == list(range(1, top + 1))
        assert [[r[1], r[5]] for r in rows] == [[repr(float(q)), "_".join(str(int(x)) for x in row)]
                                                for q, row in zip(scores, ids)]
        assert all(r[6] == "_".join(sorted(model.id_gene[int(x)] for x in r[5].split("_"))) for r in rows)
        if masked:
            assert np.isin(ids, allowed).all()
        # mean, min and max are predict's bits on those ids; the spread column lies within the
        # tolerance of predict's own order statistics
        probs = eng.predict(ids)[:B]
        mean = (((probs[0] + probs[1]) + probs[2]) + probs[3]) / B
        assert [[r[2], r[3], r[4]] for r in rows] == [[repr(float(a)), repr(float(lo)), repr(float(hi))]
                                                      for a, lo, hi in zip(mean, probs.min(axis=0), probs.max(axis=0))]
        assert (np.abs(scores - spread_ref.spread(probs, t)) <= spread_ref.atol(probs, t)).all()
    eng.close()
    # --best has no spread: refused before anything is written
    out = str(tmp_path / "refused.tsv")
    assert scan.main(base + ["-o", out, "--disputed", str(tmp_path / "refused.d.tsv"), "--best"], out=lambda *a: None) == 2
    assert not os.path.exists(out) and not os.path.exists(str(tmp_path / "refused.d.tsv"))
