"""The partner scan at P = 6007 on the planted model of tests/planted_ref.py: with one and with three
queries a query gets several hundred workgroups, so its lists pass through both merge levels.  An
elite query's list comes from the brute-force list of the elite triples (every other partner pair
gives a triple below 1e-2); a common query's list ties throughout inside its best class and is that
class's first candidates by packed triple key.  At P = 90 the same lists are also held to
tests/partners_ref.py on the full theta."""
import numpy as np
import pytest

import partners_ref
import planted_ref as pl
import scan_ref
from scan_gpu import check_list, planted_engine

pytestmark = pytest.mark.gpu

ACTIVE = pl.SCALE_ACTIVE

WIDE_P = 6007


def elite_queries(m):
    """Rank positions: the first, a middle and the last elite (positions 0 and P - 1 among them)."""
    return [int(m.elite_pos[0]), int(m.elite_pos[m.E // 2]), int(m.elite_pos[-1])]


def common_query(m):
    common = np.flatnonzero(m.label < m.Kc)
    return int(common[common.size // 2])


def calls(eng, fn, genes, Q, *args, **kw):
    """One call with all the genes (Q = 3) or one call per gene (Q = 1) -> the lists in order."""
    if Q == 1:
        return [fn([g], *args, **kw)[0] for g in genes]
    assert len(genes) == Q
    return fn(genes, *args, **kw)


@pytest.mark.parametrize("Q", [1, 3])
@pytest.mark.parametrize("P,n", [(pl.SMALL_P, 8), (pl.SMALL_P, 64), (WIDE_P, 8), (WIDE_P, 1024)])
def test_elite_queries(P, n, Q):
    import torch
    m = pl.scale_model("mean", P)
    eng = planted_engine(m)
    order, _ = scan_ref.rank_tables(P)
    if P == WIDE_P:     # the plan of csrc/partners.hip: more than 32 workgroups a query, two merge levels
        ncu = torch.cuda.get_device_properties(eng.device).multi_processor_count
        gpq, levels = pl.partner_plan(P, Q, ncu)
        assert gpq > 32 and levels == 2, (ncu, gpq)
    pos = elite_queries(m)
    assert pos[0] == 0 and pos[-1] == P - 1
    genes = [int(order[q]) for q in pos]
    s = pl.SCALE_SAMPLE
    for q, got in zip(pos, calls(eng, eng.partners_top, genes, Q, n, sample=s)):
        check_list(got, pl.partner_elite_list(m, q, n, sample=s), P)
        if P == pl.SMALL_P:
            partners_ref.check_query(got, m.theta[s], m.pr[s], int(order[q]), n)
    for q, got in zip(pos, calls(eng, eng.partners_top, genes, Q, n)):
        check_list(got, pl.partner_elite_list(m, q, n, ns=ACTIVE), P)
    votes = (ACTIVE + 1) // 2
    for q, got in zip(pos, calls(eng, eng.partners_quorum_top, genes, Q, n, votes)):
        check_list(got, pl.partner_elite_list(m, q, n, "quorum", votes, ns=ACTIVE), P)
    for q, got in zip(pos, calls(eng, eng.partners_spread_top, genes, Q, n, 0)):
        check_list(got, pl.partner_elite_list(m, q, n, "spread", 0, ns=ACTIVE), P, atol=2 * scan_ref.RTOL)
    eng.close()


@pytest.mark.parametrize("P,n", [(pl.SMALL_P, 8), (WIDE_P, 8), (WIDE_P, 1024)])
def test_a_common_query_whose_list_ties(P, n):
    """Every row carries the class value, bit for bit, so the packed triple key decides the order
    across the hundreds of workgroups' lists and both merge levels."""
    m = pl.scale_model("mean", P)
    eng = planted_engine(m)
    order, _ = scan_ref.rank_tables(P)
    q = common_query(m)
    for kw, sample in ((dict(ns=ACTIVE), None), (dict(sample=pl.SCALE_SAMPLE), pl.SCALE_SAMPLE)):
        value, keys = pl.partner_common_list(m, q, n, **kw)
        if P == pl.SMALL_P:
            sl = pl.slots_of(m, **kw)
            per = [partners_ref.ref_query(m.theta[s], m.pr[s], q) for s in sl]
            mean = scan_ref.prefix_mean(np.stack([p[0] for p in per]), len(sl))
            np.testing.assert_array_equal(scan_ref.top(mean, per[0][1], n)[1][:n], keys)
        (s, ids), = eng.partners_top([int(order[q])], n, sample=sample)
        np.testing.assert_array_equal(ids, scan_ref.keys_to_ids(keys, P))
        assert s.tobytes() == np.full(n, value).tobytes()
    eng.close()
