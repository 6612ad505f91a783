"""The pair mask in the partner scan (include/mmsbm.h mmsbm_partners_topn_masked) on the GPU, through
EMEngine.partners_top(mask=), the raw C call, Model.predict_partners / predict_third and
joint.Model.predict_trigenic_partners.

The oracle is the unmasked call: for a query at rank position q a mask stands for the pair keys
b P + c with any of {q, b}, {q, c}, (b, c) blocked (tests/partners_masked_ref.py, itself held against
a triple loop in tests/test_masked_topn_host.py), so the masked partners_top must return what the
unmasked partners_top returns with those keys merged into the query's slice of `known`: ids equal,
score BYTES equal (one score phase on both sides, no tolerance).  One case per region of the query
is held against numpy (tests/partners_ref.py) with the gap precondition asserted on the reference
alone.  The masks come from tests/masked_ref.py and tests/partners_masked_ref.py, never from the
code under test."""
import functools
import random

import numpy as np
import pytest

import masked_ref
import partners_masked_ref as pm
import partners_ref as ref
import scan_ref
from golden_util import joint_load, load
from scan_gpu import Raw, engine
from scan_ref import RTOL, bits

pytestmark = pytest.mark.gpu

NS = (1, 50, 1024)
MASKS = {"random": masked_ref.random_mask, "allowed": masked_ref.allowed_mask, "block": masked_ref.block_mask,
         "single": masked_ref.single_pair_mask, "last_tile": masked_ref.last_tile_mask, "tiles": masked_ref.tiles_mask,
         "full": masked_ref.full_mask, "zero": lambda P: masked_ref.naive_mask(P, [])}


@functools.lru_cache(maxsize=None)
def params(K, B, P, seed):
    th, pr = scan_ref.random_params(K, P, seed, B)
    th.setflags(write=False)
    pr.setflags(write=False)
    return th, pr


@functools.lru_cache(maxsize=None)
def shared_mask(name, P):
    mask = np.ascontiguousarray(MASKS[name](P))
    mask.setflags(write=False)
    return mask


def candidates(P):
    return (P - 1) * (P - 2) // 2 if P >= 3 else 0


def positions(P):
    """Rank positions of the queries: the first, a middle one, the last, and the first of the last,
    partial tile."""
    return sorted({0, P // 2, P - 1, (P - 1) // 16 * 16})


def genes_at(P, pos):
    order, _ = scan_ref.rank_tables(P)
    return [int(order[q]) for q in pos]


def some_known(P, queries, seed=1):
    """A third of every query's pairs, as (known_off, known_pairs)."""
    rng = np.random.default_rng(seed)
    off, parts = [0], []
    for q in pm.query_positions(P, queries):
        b, c = np.triu_indices(P, k=1)
        keep = (b != q) & (c != q)
        pk = (b[keep].astype(np.int64) * P + c[keep])
        drop = np.sort(pk[rng.random(pk.size) < 1 / 3])
        parts.append(drop)
        off.append(off[-1] + drop.size)
    return np.array(off, dtype=np.int64), (np.concatenate(parts) if parts else np.zeros(0, np.int64))


def same_rows(got, want):
    assert len(got) == len(want)
    for i, ((s, ids), (ws, wids)) in enumerate(zip(got, want)):
        assert s.dtype == np.float64 and ids.dtype == np.int32
        assert s.shape == ws.shape and ids.shape == wids.shape, i
        assert bits(s) == bits(ws), i
        np.testing.assert_array_equal(ids, wids, err_msg="query %d" % i)


def check_identity(eng, P, mask, queries, n, known=None, sample=None):
    """Mask = keys -> the masked rows."""
    got = eng.partners_top(queries, n, known, sample, mask=mask)
    want = eng.partners_top(queries, n, pm.merged_known(mask, P, queries, known), sample)
    same_rows(got, want)
    if known is None:
        for q, (s, _) in zip(pm.query_positions(P, queries), got):
            assert s.size == min(n, candidates(P) - pm.blocked_pairs(mask, P, q).size)
    return got


# ------------------------------------------------------------------ 1. mask = keys: shapes
@pytest.mark.parametrize("P", [3, 4, 16, 17, 33, 70])
def test_a_mask_is_the_key_table_it_stands_for(P):
    """Every shared mask; queries at the first, a middle and the last rank position and in the last,
    partial tile, each alone (Q = 1: the query spread over the device) and in one call with repeats;
    every gene (Q = P: a workgroup or two per query); N below and above the candidate count."""
    th, pr = params(3, 2, P, 40 + P)
    eng = engine(th.copy(), pr.copy())
    some = genes_at(P, positions(P))
    for name in sorted(MASKS):
        mask = shared_mask(name, P)
        for sample in (0, None):
            for n in NS if P == 70 else (1, 50):
                check_identity(eng, P, mask, some + some[:2], n, None, sample)           # repeated queries
            every = check_identity(eng, P, mask, list(range(P)), 50, None, sample)       # Q = P
            for g in some:                                                             # Q = 1
                (solo,) = check_identity(eng, P, mask, [g], 50, None, sample)
                same_rows([solo], [every[g]])
            check_identity(eng, P, mask, some, 50, some_known(P, some), sample)          # a live `known`
        if name == "full":
            assert all(s.size == 0 and ids.shape == (0, 3) for s, ids in every)
        if name == "zero":
            same_rows(every, eng.partners_top(list(range(P)), 50, None, None))
    eng.close()


def test_one_query_spread_over_the_device():
    """P = 300, Q = 1: hundreds of workgroups, ncc > 1 and two merge levels for the one query."""
    P, N = 300, 50
    th, pr = params(10, 1, P, 9)
    eng = engine(th.copy(), pr.copy())
    for name in ("random", "allowed", "tiles"):
        mask = shared_mask(name, P)
        every = eng.partners_top(list(range(P)), N, mask=mask)
        for g in genes_at(P, positions(P)):
            (solo,) = check_identity(eng, P, mask, [g], N, None, 0)
            same_rows([solo], [every[g]])
    eng.close()


# ------------------------------------------------------------------ 2. the kernel matrix
@pytest.mark.parametrize("K,B", [(1, 1), (2, 1), (10, 1), (13, 1), (30, 1), (32, 1), (10, 2), (10, 4), (30, 2), (30, 4)],
                         ids=lambda v: str(v))
def test_every_k_and_ensembles(K, B):
    P = 70
    th, pr = params(K, B, P, 100 + K + B)
    eng = engine(th.copy(), pr.copy())
    some = genes_at(P, positions(P))
    for name in ("random", "tiles"):
        mask = shared_mask(name, P)
        for n in NS:
            check_identity(eng, P, mask, some, n, None, None)
        check_identity(eng, P, mask, list(range(P)), 50, some_known(P, list(range(P))), None)
        if B > 1:
            check_identity(eng, P, mask, some, 50, None, 1)         # a slot of the batch
    eng.close()


# ------------------------------------------------------------------ 3. masks about the query
def test_masks_about_the_query():
    P, N = 70, 50
    th, pr = params(10, 1, P, 5)
    order, rank = scan_ref.rank_tables(P)
    eng = engine(th.copy(), pr.copy())
    everyone = list(range(P))
    plain = eng.partners_top(everyone, N)
    for q in positions(P):
        g = int(order[q])
        # every pair that contains the query: it has no candidate left, the others lose only the pairs with q
        mask = pm.query_all_mask(P, q)
        rows = check_identity(eng, P, mask, everyone, N)
        assert rows[g][0].size == 0 and rows[g][1].shape == (0, 3)
        sd, idd, cd = (x.cpu().numpy() for x in eng.partners_top_async([g, everyone[0] if g else 1], N, mask=mask))
        assert cd.tolist()[0] == 0 and np.isnan(sd[0]).all() and (idd[0] == -1).all()      # the NaN / -1 row
        assert cd.tolist()[1] == N
        for other in everyone:
            if other != g:
                assert rows[other][0].size == N
                assert not (rows[other][1] == g).any()
        # only pairs with the query
        mask = pm.only_with_query_mask(P, q)
        rows = check_identity(eng, P, mask, everyone, N)
        gone = set(int(order[x]) for x in [x for x in range(P) if x != q][::3])
        assert not (set(rows[g][1].ravel().tolist()) & gone)
        # only pairs without the query: queries inside no blocked pair see (b, c) bits alone
        mask = pm.only_without_query_mask(P, q)
        rows = check_identity(eng, P, mask, everyone, N)
        assert bits(rows[g][0]) != bits(plain[g][0])
    eng.close()


def test_an_all_zero_mask_is_the_unmasked_call():
    P = 70
    th, pr = params(10, 3, P, 41)
    zero = shared_mask("zero", P)
    assert not zero.any()
    eng = engine(th.copy(), pr.copy())
    everyone = list(range(P))
    for sample in (0, None, 1):
        for known in (None, some_known(P, everyone)):
            for n in NS:
                same_rows(eng.partners_top(everyone, n, known, sample, mask=zero),
                          eng.partners_top(everyone, n, known, sample))
    eng.close()


# ------------------------------------------------------------------ 4. invariants
def test_a_row_does_not_depend_on_the_other_queries():
    P, N = 70, 50
    th, pr = params(10, 1, P, 5)
    mask = shared_mask("random", P)
    eng = engine(th.copy(), pr.copy())
    everyone = list(range(P))
    known = some_known(P, everyone)
    every = eng.partners_top(everyone, N, known, mask=mask)
    same_rows(eng.partners_top(everyone, N, known, mask=mask), every)           # repeats
    for g in everyone:                                                          # one query per call
        sl = (np.array([0, known[0][g + 1] - known[0][g]], dtype=np.int64), known[1][known[0][g]:known[0][g + 1]])
        (solo,) = eng.partners_top([g], N, sl, mask=mask)
        same_rows([solo], [every[g]])
    shuffled = everyone[::-1] + everyone[::3] + [7, 7, 7]
    rows = eng.partners_top(shuffled, N, mask=mask)
    plain = eng.partners_top(everyone, N, mask=mask)
    same_rows(rows, [plain[g] for g in shuffled])
    eng.close()


# ------------------------------------------------------------------ 5. against numpy
@pytest.mark.parametrize("name", ["random", "block", "last_tile"])
def test_against_numpy(name):
    """One query per region structure: the first rank position (q < b < c only), a middle one (all
    three regions) and the last (b < c < q only)."""
    K, P, N = 10, 70, 50
    th, pr = params(K, 1, P, 5)
    mask = shared_mask(name, P)
    order, _ = scan_ref.rank_tables(P)
    eng = engine(th.copy(), pr.copy())
    for q in (0, P // 2, P - 1):
        g = int(order[q])
        gone = pm.blocked_pairs(mask, P, q)
        assert 0 < gone.size < candidates(P)
        (row,) = eng.partners_top([g], N, mask=mask)
        ref.check_query(row, th[0], pr[0], g, N, gone)           # asserts the gap on the reference alone
    eng.close()


# ------------------------------------------------------------------ 6. the genome-wide scan
def test_the_best_masked_triple_heads_its_three_genes_masked_lists():
    P = 70
    th, pr = params(10, 1, P, 5)
    eng = engine(th.copy(), pr.copy())
    for name in ("random", "allowed", "tiles"):
        mask = shared_mask(name, P)
        s, ids = eng.scan_top(1, None, 0, mask=mask)
        rows = eng.partners_top([int(g) for g in ids[0]], 4, sample=0, mask=mask)
        for ps, pids in rows:
            np.testing.assert_array_equal(pids[0], ids[0])
            np.testing.assert_allclose(ps[0], s[0], rtol=1e-9, atol=0)     # the header's bound between the two
    eng.close()


# ------------------------------------------------------------------ 7. ties
def test_ties_resolve_by_packed_triple_key_under_a_mask():
    K, P, N = 5, 37, 50
    order, rank = scan_ref.rank_tables(P)
    th, pr = scan_ref.random_params(K, 1, 7)
    th = np.repeat(th, P, axis=1)                       # every gene the same row
    eng = engine(th, pr)
    for q in (0, P - 1):          # one region each: one contraction, one score
        g = int(order[q])
        mask = masked_ref.naive_mask(P, [(q, 3), (1, 2), (4, 9)])
        gone = set(pm.blocked_pairs(mask, P, q).tolist())
        keys = sorted((lambda t: (t[0] * P + t[1]) * P + t[2])(sorted((q, b, c)))
                      for b in range(P) for c in range(b + 1, P) if q not in (b, c) and b * P + c not in gone)
        ((s, ids),) = eng.partners_top([g], N, mask=mask)
        assert np.unique(s.view(np.int64)).size == 1
        np.testing.assert_array_equal(ids, scan_ref.keys_to_ids(np.array(keys[:N], dtype=np.int64), P))
    eng.close()


# ------------------------------------------------------------------ 8. errors
def test_errors():
    import torch
    from trigenicinteractionpredictor_amd import _lib
    P = 70
    th, pr = params(10, 1, P, 5)
    mask = shared_mask("random", P)
    eng = engine(th.copy(), pr.copy())
    raw = Raw(eng, "partners", 2, 8)
    queries = np.array([3, 5], dtype=np.int32)

    def call(mask_ptr, n):
        outs = [raw.full((2, 8), torch.float64), raw.full((2, 8, 3), torch.int32), raw.full((2,), torch.int64)]
        raw.outs = outs
        rc = eng.lib.mmsbm_partners_topn_masked(
            eng.ctx, eng.scan_order.data_ptr(), queries.ctypes.data, 2, None, None, mask_ptr, eng.theta.data_ptr(),
            eng.pr.data_ptr(), 0, n, raw.ws.data_ptr(), raw.ws.numel(), *[o.data_ptr() for o in outs], eng._stream())
        torch.cuda.synchronize(eng.device)
        return rc, outs

    rc, _ = call(None, 8)                                   # a NULL mask: refused, outputs intact
    assert rc == _lib.MMSBM_ERR_INVALID and raw.intact() and b"mask" in eng.lib.mmsbm_last_error()
    m = raw.upload(np.array(mask).view(np.int32))
    rc, outs = call(m.data_ptr(), 8)
    assert rc == _lib.MMSBM_OK and outs[2].cpu().tolist() == [8, 8]
    want = eng.partners_top([3, 5], 8, pm.merged_known(mask, P, [3, 5]), 0)
    for i in range(2):
        assert bits(outs[0][i].cpu().numpy()) == bits(want[i][0])
        np.testing.assert_array_equal(outs[1][i].cpu().numpy(), want[i][1])
    rc, _ = call(m.data_ptr(), 0)
    assert rc == _lib.MMSBM_ERR_INVALID and raw.intact()
    rc, _ = call(m.data_ptr(), eng.lib.mmsbm_partners_max_n() + 1)
    assert rc == _lib.MMSBM_ERR_UNSUPPORTED and raw.intact()
    with pytest.raises(_lib.MMSBMError) as e:
        eng.partners_top([3], 0, mask=mask)
    assert e.value.code == _lib.MMSBM_ERR_INVALID
    with pytest.raises(_lib.MMSBMError) as e:
        eng.partners_top([3], 1025, mask=mask)
    assert e.value.code == _lib.MMSBM_ERR_UNSUPPORTED
    with pytest.raises(_lib.MMSBMError) as e:
        eng.partners_top([P], 8, mask=mask)
    assert e.value.code == _lib.MMSBM_ERR_INVALID
    for bad in (mask.astype(np.int64), mask.astype(np.int32), mask[:-1], mask[:, :-1], mask.T, mask.tolist()):
        with pytest.raises(ValueError):
            eng.partners_top([3], 8, mask=bad)
    assert eng.partners_top([], 8, mask=mask) == []
    eng.close()


# ------------------------------------------------------------------ 9. Model and joint.Model
def tiny_model():
    from trigenicinteractionpredictor_amd import Model
    _, vec, train, test = load("tiny", "K10_s1")
    m = Model()
    m.get_traintest(train, test)
    m.initialize_parameters(vec["theta_5"].shape[1])
    m.theta, m.pr = vec["theta_5"].tolist(), vec["pr_5"].tolist()
    return m, vec["theta_5"], vec["pr_5"]


def test_model_predict_partners_mask():
    from trigenicinteractionpredictor_amd.scan import partner_known
    m, theta, pr = tiny_model()
    P, g, n = m.P, 5, 20
    genes = [gid for gid in range(P) if gid % 5 != 1]
    pairs = [(5, 2), (3, 4)]
    mask = m.pair_mask(genes=genes, pairs=pairs)
    np.testing.assert_array_equal(mask, masked_ref.naive_from_ids(P, pairs, genes))
    rows = m.predict_partners(g, n, mask=mask)
    assert len(rows) == n and rows != m.predict_partners(g, n)
    _, rank = scan_ref.rank_tables(P)
    off, known = partner_known(m, [g], ("train", "test"))
    gone = np.union1d(known, pm.blocked_pairs(mask, P, int(rank[g])))
    want_s, want_ids, gap = ref.want_list(theta, pr, g, n, gone)
    assert gap > 1e-9                                               # the precondition, reference alone
    assert [r[1] for r in rows] == ["_".join(str(int(x)) for x in row) for row in want_ids]
    np.testing.assert_allclose([r[0] for r in rows], want_s, rtol=RTOL, atol=0)
    for p, key, names in rows:
        ids = [int(x) for x in key.split("_")]
        assert g in ids and set(ids) <= set(genes) and not {5, 2} <= set(ids) and not {3, 4} <= set(ids)
        assert names == sorted(m.id_gene[x] for x in ids)
    assert m.predict_partners(m.id_gene[g], n, mask=mask) == rows
    assert m.predict_partners(1, n, mask=mask) == []                # gene 1 is outside the allowed universe


def test_model_predict_third_mask():
    m, theta, pr = tiny_model()
    P, g1, g2 = m.P, 5, 12
    genes = [gid for gid in range(P) if gid % 5 != 1]
    mask = m.pair_mask(genes=genes, pairs=[(5, 2), (12, 3), (7, 8)])
    plain = m.predict_third(g1, g2, P, exclude=())
    rows = m.predict_third(g1, g2, P, exclude=(), mask=mask)
    thirds = lambda rs: [next(int(x) for x in r[1].split("_") if int(x) not in (g1, g2)) for r in rs]   # noqa: E731
    ok = set(genes) - {g1, g2, 2, 3}
    assert set(thirds(rows)) == ok and len(rows) == len(ok)
    assert rows == [r for r, t in zip(plain, thirds(plain)) if t in ok]            # the same rows, filtered
    assert m.predict_third(g1, g2, 7, mask=mask) == [r for r in rows if r[1] not in m.links
                                                      and r[1] not in m.test_links][:7]
    # the partner scan's masked list of g1 restricted to g2 is the same ranking
    part = [r for r in m.predict_partners(g1, 1024, exclude=(), mask=mask) if str(g2) in r[1].split("_")]
    assert sorted(r[1] for r in part) == sorted(r[1] for r in rows)
    assert m.predict_third(g1, g2, P, mask=m.pair_mask(pairs=[(g1, g2)])) == []     # a blocked query pair
    assert m.predict_third(g1, 1, P, mask=mask) == []                              # 1 is not allowed
    with pytest.raises(ValueError):
        m.predict_third(g1, g2, 3, mask=mask.astype(np.int64))


def test_joint_predict_trigenic_partners():
    from trigenicinteractionpredictor_amd.joint import DataType, Model
    from trigenicinteractionpredictor_amd.scan import partner_known
    meta, vec, train, test = joint_load("small", "K10_s1")
    m = Model()
    m.get_train_test(train, test)
    random.seed(meta["seed"])
    m.initialize_parameters(meta["K"], getattr(DataType, meta["interaction"]))
    m.theta, m.pr, m.qr = vec["theta_5"].tolist(), vec["pr_5"].tolist(), vec["qr_5"].tolist()
    P, n, threshold = m.P, 40, 0.5
    eng = m._push().tri
    mask = m.digenic_mask(threshold)
    assert mask.any()
    order, rank = scan_ref.rank_tables(P)
    novel = m.predict_novel_trigenic(1, threshold)
    for g in genes_at(P, positions(P)) + [int(x) for x in novel[0][1].split("_")]:
        rows = m.predict_trigenic_partners(g, n, threshold)
        known = partner_known(m._trigenic_tables(), [g], ("train", "test"))
        ((s, ids),) = eng.partners_top([g], n, pm.merged_known(mask, P, [g], known), 0)
        assert [r[1] for r in rows] == ["_".join(str(int(x)) for x in row) for row in ids]
        assert bits(np.array([r[0] for r in rows])) == bits(s)
        assert all(r[2] == sorted(m.id_gene[int(x)] for x in r[1].split("_")) for r in rows)
        assert m.predict_trigenic_partners(m.id_gene[g], n, threshold) == rows
    # the best novel trigenic triple heads its genes' lists
    for g in novel[0][1].split("_"):
        top = m.predict_trigenic_partners(int(g), 1, threshold)
        assert top[0][1] == novel[0][1]
        np.testing.assert_allclose(top[0][0], novel[0][0], rtol=1e-9, atol=0)
    with pytest.raises(IndexError):
        m.predict_trigenic_partners(P, 5)
