"""Quorum scan (include/mmsbm.h mmsbm_scan_quorum_topn, EMEngine.quorum_top, the scan driver's
--quorum) against the numpy float64 reference of tests/quorum_ref.py over all C(P, 3) triples of
every slot, and against the product's own threshold scan, scan and vote scan.

The result is the exact top N under a total order, so the tests demand the identical ordered id
list.  Each comparison with the reference first asserts, on the reference alone, that every adjacent
relative gap inside the reference's top N + 1 exceeds 1e-9 (scan_ref.assert_gaps; an order statistic
moves by at most what a slot's score moves, RTOL).  Large N, where gaps close, is tested against the
product's own bits without a tolerance.
"""
import ctypes
import os
from math import comb

import numpy as np
import pytest

import quorum_ref
import scan_gpu
import scan_ref
import scan_rule
from golden_util import GOLDEN
from scan_gpu import engine
from scan_ref import packed

pytestmark = pytest.mark.gpu

RTOL = scan_ref.RTOL


class Raw(scan_gpu.Raw):
    ENTRY = dict(scan_gpu.Raw.ENTRY, scan_quorum="mmsbm_scan_quorum_topn")


def same(got, want):
    return all(g.tobytes() == w.tobytes() for g, w in zip(got, want))


def check(eng, per, keys, m, n, known=None, sample=None):
    """quorum_top(n, m) against the reference's list: equal ids, scores within RTOL."""
    P = eng.P
    want_s, want_k = quorum_ref.ref_top(per, keys, m, n, known)    # asserts the gaps
    want_s, want_k = want_s[:n], want_k[:n]
    s, ids = eng.quorum_top(n, m, known, sample=sample)
    assert ids.dtype == np.int32 and s.dtype == np.float64 and ids.shape == (want_k.size, 3)
    np.testing.assert_array_equal(ids, scan_ref.keys_to_ids(want_k, P))
    np.testing.assert_allclose(s, want_s, rtol=RTOL, atol=0)
    if known is not None and len(known):
        assert not np.isin(packed(ids, P), known).any()
    return s, ids


# ------------------------------------------------------------------ 1. the reference
@pytest.mark.parametrize("K,P,B,seed", quorum_ref.reference_cases())
def test_against_the_reference(K, P, B, seed):
    """P = 53: interior tiles, boundary tiles and a ragged last tile; P = 20: boundary tiles only."""
    c = quorum_ref.case(K, P, seed, B)
    eng = engine(c.theta, c.pr)
    ms = quorum_ref.supported(B, eng.quorum_max_depth)
    assert {1, B} <= set(ms) and [eng.quorum_depth(m) for m in ms] == [quorum_ref.depth(m, B) for m in ms]
    for known in quorum_ref.exclusions(c.keys, P):
        for m in ms:
            for n in quorum_ref.NS:
                check(eng, c.per, c.keys, m, n, known)
    # None: every scored slot
    assert same(eng.quorum_top(5), eng.quorum_top(5, B))
    eng.close()


@pytest.mark.parametrize("P", [2, 3])
def test_one_triple_and_none(P):
    c = quorum_ref.case(3, P, 11, 3)
    eng = engine(c.theta, c.pr)
    for m, sample in ((1, None), (2, None), (3, None), (1, 1)):
        s, ids = eng.quorum_top(4, m, sample=sample)
        if P == 2:
            assert s.shape == (0,) and ids.shape == (0, 3) and s.dtype == np.float64 and ids.dtype == np.int32
        else:
            per = c.per if sample is None else c.per[sample:sample + 1]
            assert ids.tolist() == scan_ref.keys_to_ids(c.keys, 3).tolist()
            np.testing.assert_allclose(s, quorum_ref.quorum(per, m), rtol=RTOL, atol=0)
    eng.close()


def test_more_rows_asked_than_there_are_triples():
    K, P, B, seed = 3, 20, 3, 11
    c = quorum_ref.case(K, P, seed, B)
    eng = engine(c.theta, c.pr)
    known = c.keys[1::9].copy()
    eligible = comb(P, 3) - known.size
    n = 2048
    assert eligible < n
    scores, ids, count = eng.quorum_top_async(n, 2, known)
    scores, ids, count = scores.cpu().numpy(), ids.cpu().numpy(), int(count.cpu()[0])
    assert count == eligible
    assert np.isnan(scores[count:]).all() and (ids[count:] == -1).all()     # the NaN / -1 tail
    q = quorum_ref.quorum(c.per, 2)
    keep = ~np.isin(c.keys, known)
    got = packed(ids[:count], P)
    np.testing.assert_array_equal(np.sort(got), c.keys[keep])               # all of them, each once
    np.testing.assert_allclose(scores[:count], q[np.searchsorted(c.keys, got)], rtol=RTOL, atol=0)
    assert (np.diff(scores[:count]) <= 0).all()
    eng.close()


# ------------------------------------------------------------------ 2. exact, product against product
def slot_lists(eng, B, P):
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


@pytest.mark.parametrize("K,P,B,seed", quorum_ref.EXACT_CASES)
def test_exact_against_the_slots_threshold_scans(K, P, B, seed):
    """No tolerance: the m-th largest per key of the slots' own scan_above lists, sorted under the
    total order, is quorum_top's list in bits and ids; N = 4096 puts the candidate buffer in the
    workspace; P = 211 runs the seeding pass.  Then the vote identity at the N-th score."""
    c = quorum_ref.case(K, P, seed, B)
    eng = engine(c.theta, c.pr)
    keys, per = slot_lists(eng, B, P)
    for known in (None, keys[1::9].copy()):
        keep = np.ones(keys.size, bool) if known is None else ~np.isin(keys, known)
        for m in quorum_ref.supported(B, eng.quorum_max_depth):
            q = np.sort(per, axis=0)[B - m][keep]
            order = np.lexsort((keys[keep], -q))
            want_s, want_k = q[order], keys[keep][order]
            for n in (1, 5, 300, 4096):
                s, ids = eng.quorum_top(n, m, known)
                assert s.size == n
                assert s.tobytes() == want_s[:n].tobytes()
                np.testing.assert_array_equal(ids, scan_ref.keys_to_ids(want_k[:n], P))
                # votes(t) >= m exactly when q_m >= t
                t = float(s[-1])
                assert eng.vote_census(t, known)[m:].sum() >= n
                assert eng.vote_census(float(np.nextafter(t, np.inf)), known)[m:].sum() <= n - 1
    eng.close()


# ------------------------------------------------------------------ 3. one slot
def test_one_slot_is_the_scan():
    K, P, B, seed = quorum_ref.EXACT_CASES[0]
    c = quorum_ref.case(K, P, seed, B)
    known = c.keys[1::9].copy()
    eng = engine(c.theta, c.pr)
    for n in (1, 64, 4096):
        for s in range(B):
            assert same(eng.quorum_top(n, 1, known, sample=s), eng.scan_top(n, known, sample=s))
    s = 2
    solo = engine(c.theta[s:s + 1], c.pr[s:s + 1])
    want = eng.scan_top(300, known, sample=s)
    for sample in (None, 0):                                         # an ensemble of one is that sample
        assert same(solo.quorum_top(300, 1, known, sample=sample), want)
        assert same(solo.quorum_top(300, None, known, sample=sample), want)
    with pytest.raises(ValueError):
        solo.quorum_top(5, 2)
    solo.close()
    eng.close()


# ------------------------------------------------------------------ 4. schedule and batch
def test_nothing_depends_on_the_batch_the_grid_or_the_early_exit(monkeypatch):
    K, P, B, seed = quorum_ref.EXACT_CASES[1]                        # P = 211: the seeding pass
    theta, pr = scan_ref.random_params(K, P, seed, 4)
    known = quorum_ref.case(K, P, seed, B).keys[2::7].copy()
    eng = engine(theta, pr)
    eng.set_active(3)
    three = engine(theta[:3], pr[:3])
    for var in ("MMSBM_SCAN_QUORUM_GRID", "MMSBM_SCAN_QUORUM_EARLY"):
        monkeypatch.delenv(var, raising=False)
    for n in (5, 300, 4096):
        for m in (1, 2, 3):
            want = three.quorum_top(n, m, known)
            assert want[0].size == n
            assert same(eng.quorum_top(n, m, known), want)           # a prefix of a wider batch
            for grid in ("1", "7"):
                monkeypatch.setenv("MMSBM_SCAN_QUORUM_GRID", grid)
                assert same(eng.quorum_top(n, m, known), want)
            monkeypatch.delenv("MMSBM_SCAN_QUORUM_GRID")
            for early in ("0", "1"):
                monkeypatch.setenv("MMSBM_SCAN_QUORUM_EARLY", early)
                assert same(eng.quorum_top(n, m, known), want)
            monkeypatch.delenv("MMSBM_SCAN_QUORUM_EARLY")
            assert same(eng.quorum_top(n, m, known), want)           # the defaults again
    with pytest.raises(ValueError):
        eng.quorum_top(5, 4)                                         # more votes than scored slots
    three.close()
    eng.close()


# ------------------------------------------------------------------ 5. the kernel matrix
@pytest.mark.parametrize("K,B,WB", quorum_ref.matrix_cases(), ids=lambda v: str(v))
def test_kernel_matrix(K, B, WB):
    """KS = 1..8 x the row-block widths 4, 2, 1, every supported depth in both directions (held
    against the instantiations by tests/test_quorum_host.py), N = 64 against the reference."""
    assert scan_rule.width(K, B) == WB
    c = quorum_ref.matrix_case(K, B)
    eng = engine(c.theta, c.pr)
    known = c.keys[1::9].copy()
    for m in quorum_ref.supported(B, eng.quorum_max_depth):
        check(eng, c.per, c.keys, m, quorum_ref.MATRIX_N, known)
    eng.close()


def test_an_ensemble_beyond_the_lds_is_refused():
    from trigenicinteractionpredictor_amd import _lib
    K, P, B = 30, 53, 16
    assert scan_rule.width(K, B) == 0 and scan_rule.last_supported(K) == 15
    th, pr = scan_ref.random_params(K, P, 331, B)
    eng = engine(th, pr)
    with pytest.raises(_lib.MMSBMError) as e:
        eng.quorum_top(5, 1)                                         # depth 1: the LDS refuses, not the depth
    assert e.value.code == _lib.MMSBM_ERR_UNSUPPORTED
    raw = Raw(eng, "scan_quorum", 8)
    assert raw.call((1, 8), quorum_outs(raw, 8), sample=-1) == _lib.MMSBM_ERR_UNSUPPORTED and raw.intact()
    # the context stays usable: one slot, and the largest ensemble that fits
    assert same(eng.quorum_top(64, 1, sample=3), eng.scan_top(64, sample=3))
    eng.set_active(15)
    assert eng.quorum_top(64, 15)[0].size == 64
    eng.close()


# ------------------------------------------------------------------ 6. refusals
def quorum_outs(raw, n):
    """The three outputs of mmsbm_scan_quorum_topn, full of the sentinel."""
    torch = raw.torch
    return [raw.full((n,), torch.float64), raw.full((n, 3), torch.int32), raw.full((1,), torch.int64)]


def intact(outs):
    return all(bool((o == scan_gpu.SENTINEL).all()) for o in outs if o is not None)


def test_refusals_leave_the_outputs_and_the_context_intact():
    from trigenicinteractionpredictor_amd import _lib
    K, P, B, N = 3, 37, 9, 16
    c = quorum_ref.case(K, P, 11, B)
    eng = engine(c.theta, c.pr)
    cap = eng.quorum_max_depth
    assert cap == int(eng.lib.mmsbm_scan_quorum_max_depth()) and 2 * cap + 1 <= B
    raw = Raw(eng, "scan_quorum", N)
    INVALID, UNSUPPORTED = _lib.MMSBM_ERR_INVALID, _lib.MMSBM_ERR_UNSUPPORTED

    def refused(code=INVALID, min_votes=1, n=N, nulls=(), **kw):
        outs = quorum_outs(raw, N)
        for i in nulls:
            outs[i] = None
        rc = raw.call((min_votes, n), outs, **dict({"sample": -1}, **kw))
        return rc == code and intact(outs)

    for i in (0, 1, 2):
        assert refused(nulls=(i,))                                   # out_scores, out_ids, out_count
    for i in (0, 1, 4, 5):                                           # ctx, order, theta, pr
        assert refused(replace=[(i, None)])
    for m in (0, -1, B + 1):                                         # min_votes outside [1, ns]
        assert refused(min_votes=m)
        with pytest.raises(ValueError):
            eng.quorum_top(N, m)
        with pytest.raises(ValueError):
            eng.quorum_depth(m)
    assert refused(min_votes=2, sample=0)                            # one slot has one vote
    with pytest.raises(ValueError):
        eng.quorum_top(N, 2, sample=1)
    for m in range(cap + 1, B - cap + 1):                            # a depth above the cap
        assert eng.quorum_depth(m) > cap
        assert refused(UNSUPPORTED, min_votes=m)
        with pytest.raises(_lib.MMSBMError) as e:
            eng.quorum_top(N, m)
        assert e.value.code == UNSUPPORTED
    assert refused(n=0) and refused(n=-1)                            # N < 1
    assert refused(UNSUPPORTED, n=int(eng.lib.mmsbm_scan_max_n()) + 1)
    for sample in (B, B + 1, -2):                                    # outside the active prefix
        assert refused(sample=sample)
    with pytest.raises(ValueError):
        eng.quorum_top(N, 1, sample=B)
    assert refused(n_known=3) and refused(n_known=-1)                # keys announced, none given
    with pytest.raises(ValueError):
        eng.quorum_top(N, 1, known=np.array([5, 3], dtype=np.int64))  # unsorted
    assert refused(ws=(raw.ws.data_ptr(), raw.ws.numel() - 1))       # too small
    assert refused(ws=(raw.ws.data_ptr() + 8, raw.ws.numel() - 8))   # misaligned
    assert refused(ws=(0, raw.ws.numel()))                           # missing
    nbytes = ctypes.c_int64()
    assert eng.lib.mmsbm_scan_quorum_workspace_bytes(None, N, ctypes.byref(nbytes)) == INVALID
    assert eng.lib.mmsbm_scan_quorum_workspace_bytes(eng.ctx, N, None) == INVALID
    assert eng.lib.mmsbm_scan_quorum_workspace_bytes(eng.ctx, 0, ctypes.byref(nbytes)) == INVALID
    # after all of it the context answers, through the C call and the binding
    outs = quorum_outs(raw, N)
    assert raw.call((B, N), outs, sample=-1) == 0 and int(outs[2].cpu()[0]) == N
    s, ids = check(eng, c.per, c.keys, B, 5)
    assert outs[0].cpu().numpy()[:5].tobytes() == s.tobytes()
    eng.close()


def test_async_calls_return_device_tensors():
    import torch
    K, P, B, seed = quorum_ref.CASES[2]
    c = quorum_ref.case(K, P, seed, B)
    eng = engine(c.theta, c.pr)
    stream = torch.cuda.Stream(eng.device)
    for st in (None, stream):
        scores, ids, count = eng.quorum_top_async(64, 1, stream=st)
        (stream if st is not None else torch.cuda.current_stream(eng.device)).synchronize()
        assert all(x.is_cuda for x in (scores, ids, count)) and int(count.cpu()[0]) == 64
        assert same((scores.cpu().numpy(), ids.cpu().numpy()), eng.quorum_top(64, 1, stream=st))
    eng.close()


# ------------------------------------------------------------------ 7. the driver
def test_driver_writes_the_quorum_table(tmp_path):
    import random
    from trigenicinteractionpredictor_amd import Model, _lib, scan
    from trigenicinteractionpredictor_amd.engine import EMEngine
    from trigenicinteractionpredictor_amd.restarts import stream_states
    g = os.path.join(GOLDEN, "tiny")
    train, test = os.path.join(g, "train.dat"), os.path.join(g, "test.dat")
    K, B, iters, seed, top = 3, 3, 5, 1, 20
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
    for M in (None, 2):                                              # the default M is every restart
        files = [str(tmp_path / f) for f in ("top%s.tsv" % M, "quorum%s.tsv" % M)]
        rc = scan.main(base + ["-o", files[0], "--quorum", files[1]] + ([] if M is None else ["--quorum-votes", str(M)]),
                       out=lambda *a: None)
        assert rc == 0
        lines = open(files[1], encoding="utf-8").read().rstrip("\n").split("\n")
        assert lines[0] == "# samples\t%d" % B and lines[1] == "# quorum votes\t%d" % (B if M is None else M)
        assert lines[2].split("\t") == ["rank", "quorum", "mean", "min", "max", "ids", "names"]
        rows = [ln.split("\t") for ln in lines[3:]]
        assert len(rows) == top and [int(r[0]) for r in rows] == list(range(1, top + 1))
        # the rows are EMEngine.quorum_top on the same engine state
        scores, ids = eng.quorum_top(top, M, known)
        assert [[r[1], r[5]] for r in rows] == [[repr(float(q)), "_".join(str(int(x)) for x in row)]
                                                for q, row in zip(scores, ids)]
        assert all(r[6] == "_".join(sorted(model.id_gene[int(x)] for x in r[5].split("_"))) for r in rows)
        # mean, min and max are predict's bits on those ids; the quorum column lies within RTOL of
        # predict's own order statistic
        probs = eng.predict(ids)[:B]
        mean = ((probs[0] + probs[1]) + probs[2]) / B
        assert [[r[2], r[3], r[4]] for r in rows] == [[repr(float(a)), repr(float(lo)), repr(float(hi))]
                                                      for a, lo, hi in zip(mean, probs.min(axis=0), probs.max(axis=0))]
        np.testing.assert_allclose(scores, np.sort(probs, axis=0)[B - (B if M is None else M)], rtol=RTOL, atol=0)
    eng.close()
    # --best has no quorum: refused before anything is written
    out = str(tmp_path / "refused.tsv")
    assert scan.main(base + ["-o", out, "--quorum", str(tmp_path / "refused.q.tsv"), "--best"], out=lambda *a: None) == 2
    assert not os.path.exists(out) and not os.path.exists(str(tmp_path / "refused.q.tsv"))
