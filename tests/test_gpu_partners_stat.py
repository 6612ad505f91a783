"""Partner statistics (include/mmsbm.h mmsbm_partners_stat_topn, EMEngine.partners_quorum_top /
partners_spread_top, the scan driver's --partners-quorum / --partners-disputed) on the GPU.

A quorum score is one slot's word and a spread one IEEE subtraction of two, so wherever a query has
at most 1024 eligible candidates the lists are compared bit for bit with what numpy forms from the
slots' own complete lists, partners_top(sample=s, n=1024): no tolerance is involved.  Only the
comparison with the independent reference (partners_ref.ref_query per slot) has one: scan_ref.RTOL
relative for a quorum score and spread_ref.atol for a spread (order statistics are 1-Lipschitz in the
sup norm over the slots), with the gap precondition asserted on the reference alone (and for every
case in tests/test_partners_stat_host.py)."""
import ctypes
import functools
import json
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import partners_converged_ref as pc
import partners_masked_ref as pm
import partners_stat_ref as ref
import quorum_ref
import scan_ref
import spread_ref
from golden_util import GOLDEN
from scan_gpu import SENTINEL
from scan_ref import RTOL, bits

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL = 1024     # mmsbm_partners_max_n(): a slot's list of this length is complete up to 1024 candidates
NS = (1, 7, FULL)


@functools.lru_cache(maxsize=None)
def params(K, P, B, seed):
    th, pr = scan_ref.random_params(K, P, seed, B)
    th.setflags(write=False)
    pr.setflags(write=False)
    return th, pr


def make_engine(th, pr, active=None):
    from trigenicinteractionpredictor_amd.engine import EMEngine
    B, P, K = th.shape
    eng = EMEngine(K, P, B=B)
    eng.upload(th.copy(), pr.copy())
    if active is not None:
        eng.set_active(active)
    return eng


def candidates(P):
    return (P - 1) * (P - 2) // 2 if P >= 3 else 0


def stat_top(eng, genes, n, what, arg, known=None, mask=None):
    f = eng.partners_quorum_top if what == "quorum" else eng.partners_spread_top
    return f(genes, n, arg, known, mask=mask)


def slot_tables(eng, genes, known=None, mask=None):
    """Per query (per f64[ns][n], triple keys ascending) from the active slots' own complete lists."""
    per_slot = [eng.partners_top(genes, FULL, known, sample=s, mask=mask) for s in range(eng.active)]
    out = []
    for i in range(len(genes)):
        lists = [per_slot[s][i] for s in range(eng.active)]
        assert all(sc.size < FULL or candidates(eng.P) <= FULL for sc, _ in lists)     # complete lists
        out.append(ref.from_slot_lists(lists, eng.P))
    return out


def same_list(got, want, what):
    (s, ids), (ws, wids) = got, want
    assert s.dtype == np.float64 and ids.dtype == np.int32, what
    assert s.shape == ws.shape and ids.shape == wids.shape, (what, s.shape, ws.shape)
    np.testing.assert_array_equal(ids, wids, err_msg=str(what))
    assert bits(s) == bits(ws), what


def check_against_slots(eng, genes, calls=None, ns=NS, known=None, mask=None):
    """Check 1: the stat call's ids and score words are numpy's order statistic and lexsort of the
    slots' own words; -> {(what, arg, n): lists}."""
    tables = slot_tables(eng, genes, known, mask)
    out = {}
    for what, arg in calls or ref.stat_calls(eng.active):
        want_v = [ref.stat(per, what, arg) for per, _ in tables]
        for n in ns:
            got = stat_top(eng, genes, n, what, arg, known, mask)
            assert len(got) == len(genes)
            for i, (per, keys) in enumerate(tables):
                same_list(got[i], ref.top_list(want_v[i], keys, eng.P, n), (what, arg, n, i))
                if what == "spread":
                    assert not np.signbit(got[i][0]).any()      # d_t >= +0
            out[what, arg, n] = got
    return out


# ------------------------------------------------------------------ 1. bit for bit against the slots
SHAPES = [(3, 37, 3), (13, 40, 4), (5, 33, 2), (10, 46, 8)]


@pytest.mark.parametrize("K,P,B", SHAPES, ids=lambda v: str(v))
def test_lists_are_the_order_statistics_of_the_slots_own_words(K, P, B):
    th, pr = params(K, P, B, 7 + K)
    assert candidates(P) <= FULL
    genes = ref.genes_at(P, ref.positions(P))
    assert len(genes) in (6, 7)     # P // 2 = 16 at P = 33
    eng = make_engine(th, pr)
    calls = ref.stat_calls(B)
    assert len(calls) == len(ref.legal_votes(B)) + len(ref.legal_trims(B))
    if B == 8:
        assert ("quorum", 4) in calls and ("quorum", 5) in calls and ("spread", 3) in calls   # depth 4, both directions
    got = check_against_slots(eng, genes, calls)
    # the restarts differ: the statistics are not one slot's list
    if B >= 2:
        assert bits(got["quorum", 1, 7][0][0]) != bits(got["quorum", B, 7][0][0])
        assert (got["spread", 0, 1][0][0] > 0).all()
    for (_, _, n), lists in got.items():
        assert all(s.size == min(n, candidates(P)) for s, _ in lists)
    eng.close()


def test_counts_and_tails_through_the_device_tensors():
    import torch
    K, P, B, n = 5, 33, 2, FULL
    th, pr = params(K, P, B, 7 + K)
    genes = ref.genes_at(P, ref.positions(P))
    eng = make_engine(th, pr)
    for f, arg in ((eng.partners_quorum_top_async, 2), (eng.partners_spread_top_async, 0)):
        sd, idd, cd = f(genes, n, arg)
        torch.cuda.synchronize()
        sd, idd, cd = sd.cpu().numpy(), idd.cpu().numpy(), cd.cpu().numpy()
        assert sd.shape == (len(genes), n) and idd.shape == (len(genes), n, 3) and cd.dtype == np.int64
        c = candidates(P)
        assert cd.tolist() == [c] * len(genes)
        assert np.isnan(sd[:, c:]).all() and (idd[:, c:] == -1).all() and not np.isnan(sd[:, :c]).any()
        for g, row in zip(genes, idd[:, :c]):
            assert (row == g).any(axis=1).all()         # every listed triple holds the query
    eng.close()


def test_an_active_prefix_a_repeated_query_and_no_query():
    K, P, B = 10, 46, 8
    th, pr = params(K, P, B, 7 + K)
    eng = make_engine(th, pr, active=5)
    assert eng.active == 5
    order, _ = scan_ref.rank_tables(P)
    genes = [int(order[3]), int(order[40]), int(order[3])]
    got = check_against_slots(eng, genes, ns=(7,))
    assert sorted(k[:2] for k in got) == sorted(ref.stat_calls(5))
    for lists in got.values():
        same_list(lists[0], lists[2], "repeat")
    # the default votes: every ACTIVE slot
    same_list(eng.partners_quorum_top(genes[:1], 7)[0], got["quorum", 5, 7][0], "default")
    assert eng.partners_quorum_top([], 7) == [] and eng.partners_spread_top([], 7) == []
    eng.close()


def test_one_slot_is_the_slots_own_list():
    K, P = 5, 33
    th, pr = params(K, P, 3, 8)
    genes = ref.genes_at(P, ref.positions(P))
    eng = make_engine(th[:1], pr[:1])
    for n in NS:
        for a, b in zip(eng.partners_quorum_top(genes, n, 1), eng.partners_top(genes, n, sample=0)):
            same_list(a, b, n)
    with pytest.raises(ValueError):
        eng.partners_spread_top(genes, 7)
    eng.close()
    eng = make_engine(th, pr, active=1)     # one ACTIVE slot of several
    for a, b in zip(eng.partners_quorum_top(genes, 7), eng.partners_top(genes, 7, sample=0)):
        same_list(a, b, "active 1")
    eng.close()


def test_two_genes_have_no_candidate():
    import torch
    th, pr = params(3, 2, 2, 1)
    eng = make_engine(th, pr)
    for f, arg in ((eng.partners_quorum_top_async, 1), (eng.partners_spread_top_async, 0)):
        sd, idd, cd = f([0, 1], 4, arg)
        torch.cuda.synchronize()
        assert cd.cpu().tolist() == [0, 0] and np.isnan(sd.cpu().numpy()).all() and (idd.cpu().numpy() == -1).all()
    eng.close()


def test_a_query_spread_over_many_workgroups_under_a_known_table():
    """P = 100, Q = 1: the query has 49 workgroups (7 row blocks of 16 x 7 column tiles) and the merge
    runs two levels; a random `known` table leaves about 900 survivors per query, so the slots' lists
    stay complete."""
    K, P, B = 7, 100, 5
    th, pr = params(K, P, B, 9)
    rng = np.random.default_rng(4)
    positions = ref.positions(P)
    genes = ref.genes_at(P, positions)
    eng = make_engine(th, pr)
    for g, q in zip(genes, positions):
        b, c = np.triu_indices(P, k=1)
        keep = (b != q) & (c != q)
        pk = b[keep].astype(np.int64) * P + c[keep]
        drop = np.sort(pk[rng.random(pk.size) >= 900 / pk.size])
        assert 800 < pk.size - drop.size < FULL
        known = (np.array([0, drop.size], dtype=np.int64), drop)
        got = check_against_slots(eng, [g], [("quorum", 1), ("quorum", 3), ("quorum", 5), ("spread", 0), ("spread", 1)],
                                  known=known)
        assert got["quorum", 3, FULL][0][0].size == pk.size - drop.size
    eng.close()


def test_identical_slots_give_a_positive_zero_spread_in_key_order():
    K, P, B, N = 6, 40, 4, 12
    th1, pr1 = params(K, P, 1, 31)
    th, pr = np.repeat(th1, B, axis=0), np.repeat(pr1, B, axis=0)
    positions = ref.positions(P)
    genes = ref.genes_at(P, positions)
    eng = make_engine(th, pr)
    for m in (1, 2, B):
        for a, b in zip(eng.partners_quorum_top(genes, N, m), eng.partners_top(genes, N, sample=0)):
            same_list(a, b, m)
    for t in (0, 1):
        for n in (N, FULL):
            for q, (s, ids) in zip(positions, eng.partners_spread_top(genes, n, t)):
                _, tk, _ = ref.ref_slots(th[:1], pr[:1], q)
                assert s.size == min(n, candidates(P)) and not s.view(np.int64).any()       # +0, the sign bit clear
                np.testing.assert_array_equal(ids, scan_ref.keys_to_ids(np.sort(tk)[:n], P))
    eng.close()


# ------------------------------------------------------------------ 2. the independent reference
@pytest.mark.parametrize("K,P,B,seed", ref.REF_CASES, ids=lambda v: str(v))
def test_against_the_numpy_reference(K, P, B, seed):
    """N far below the candidate count: the workgroups prune by their own and the query's bound."""
    th, pr = params(K, P, B, seed)
    positions = ref.positions(P)
    genes = ref.genes_at(P, positions)
    eng = make_engine(th, pr)
    slots = [ref.ref_slots(th, pr, q) for q in positions]
    for what, arg in ref.stat_calls(B):
        for n in ref.REF_NS:
            got = stat_top(eng, genes, n, what, arg)
            for i, (per, tk, _) in enumerate(slots):
                v = ref.stat(per, what, arg)
                ok, gap = ref.gap_ok(v, what, n)        # the precondition, on the reference alone
                assert ok, (positions[i], what, arg, n, gap)
                want_s, want_ids = ref.top_list(v, tk, P, n)
                s, ids = got[i]
                np.testing.assert_array_equal(ids, want_ids, err_msg=str((positions[i], what, arg, n)))
                if what == "quorum":
                    np.testing.assert_allclose(s, want_s, rtol=RTOL, atol=0)
                else:
                    bound, _ = ref.top_list(spread_ref.atol(per, arg), tk, P, n, order_by=v)   # per listed triple
                    assert (np.abs(s - want_s) <= bound).all(), (positions[i], what, arg, n)
    eng.close()


# ------------------------------------------------------------------ 3. the kernel matrix
@pytest.mark.parametrize("K", quorum_ref.MATRIX_K)
def test_every_ks(K):
    """One K per KS = ceil(K / 4) = 1..8 at 8 slots: depth 1 and 4 from the top and from the bottom,
    the range and the deepest trim."""
    P, B = 40, 8
    th, pr = params(K, P, B, 700 + K)
    genes = ref.genes_at(P, ref.positions(P))
    eng = make_engine(th, pr)
    check_against_slots(eng, genes, [("quorum", m) for m in (1, 4, 5, 8)] + [("spread", t) for t in (0, 3)])
    eng.close()


# ------------------------------------------------------------------ 4. masks
def test_an_all_zero_mask_is_the_unmasked_call():
    import masked_ref
    K, P, B = 10, 46, 8
    th, pr = params(K, P, B, 7 + K)
    zero = np.ascontiguousarray(masked_ref.naive_mask(P, []))
    assert not zero.any()
    genes = ref.genes_at(P, ref.positions(P))
    eng = make_engine(th, pr)
    for what, arg in (("quorum", 1), ("quorum", 5), ("quorum", 8), ("spread", 0), ("spread", 3)):
        for n in NS:
            for a, b in zip(stat_top(eng, genes, n, what, arg, mask=zero), stat_top(eng, genes, n, what, arg)):
                same_list(a, b, (what, arg, n))
    eng.close()


@pytest.mark.parametrize("K,P,B", [(3, 37, 3), (10, 46, 8)], ids=lambda v: str(v))
def test_a_mask_is_the_key_table_it_stands_for(K, P, B):
    import masked_ref
    th, pr = params(K, P, B, 7 + K)
    order, _ = scan_ref.rank_tables(P)
    positions = ref.positions(P)
    genes = ref.genes_at(P, positions)
    eng = make_engine(th, pr)
    calls = [("quorum", 1), ("quorum", B), ("quorum", (B + 1) // 2), ("spread", 0), ("spread", (B - 2) // 2)]
    masks = [np.ascontiguousarray(masked_ref.random_mask(P))]
    masks += [f(P, q) for q in (positions[0], positions[2], positions[-1])
              for f in (pm.query_all_mask, pm.only_with_query_mask, pm.only_without_query_mask)]
    for mask in masks:
        mask = np.ascontiguousarray(mask)
        merged = pm.merged_known(mask, P, genes)
        for what, arg in calls:
            for n in (7, FULL):
                got = stat_top(eng, genes, n, what, arg, mask=mask)
                want = stat_top(eng, genes, n, what, arg, merged)
                for i, (a, b) in enumerate(zip(got, want)):
                    same_list(a, b, (what, arg, n, i))
                    assert a[0].size == min(n, candidates(P) - pm.blocked_pairs(mask, P, positions[i]).size)
    # under a mask and a `known` table, against the slots' own masked lists
    rng = np.random.default_rng(2)
    off, parts = [0], []
    for q in positions:
        b, c = np.triu_indices(P, k=1)
        keep = (b != q) & (c != q)
        pk = b[keep].astype(np.int64) * P + c[keep]
        parts.append(np.sort(pk[rng.random(pk.size) < 0.3]))
        off.append(off[-1] + parts[-1].size)
    known = (np.array(off, dtype=np.int64), np.concatenate(parts))
    check_against_slots(eng, genes, calls, (7, FULL), known, masks[0])
    eng.close()


def test_a_query_whose_every_candidate_is_blocked():
    import torch
    K, P, B = 10, 46, 8
    th, pr = params(K, P, B, 7 + K)
    order, _ = scan_ref.rank_tables(P)
    eng = make_engine(th, pr)
    for q in (0, 16, P - 1):
        g, other = int(order[q]), int(order[(q + 5) % P])
        mask = np.ascontiguousarray(pm.query_all_mask(P, q))
        for f, arg in ((eng.partners_quorum_top_async, 5), (eng.partners_spread_top_async, 3)):
            sd, idd, cd = (x.cpu().numpy() for x in f([g, other], 9, arg, mask=mask))
            assert cd.tolist() == [0, 9] and np.isnan(sd[0]).all() and (idd[0] == -1).all()
            assert not (idd[1] == g).any() and not np.isnan(sd[1]).any()
    eng.close()


# ------------------------------------------------------------------ 5. the early exit
CHILD = r"""
import json, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
import scan_ref
from trigenicinteractionpredictor_amd.engine import EMEngine
K, P, B, seed = 7, 100, 5, 9
th, pr = scan_ref.random_params(K, P, seed, B)
eng = EMEngine(K, P, B=B)
eng.upload(th, pr)
order, _ = scan_ref.rank_tables(P)
genes = [int(order[q]) for q in (0, 16, 50, 99)]
out = {}
for m in (1, 2, 3, 4, 5):
    for n in (1, 5, 64):
        for q in (genes, genes[1:2]):
            lists = eng.partners_quorum_top(q, n, m)
            out["%d %d %d" % (m, n, len(q))] = [[s.tobytes().hex(), ids.tobytes().hex()] for s, ids in lists]
eng.close()
print("LISTS " + json.dumps(out))
"""


def run_child(early):
    env = dict(os.environ)
    env.pop("MMSBM_PARTNERS_STAT_EARLY", None)
    if early is not None:
        env["MMSBM_PARTNERS_STAT_EARLY"] = early
    p = subprocess.run([sys.executable, "-c", CHILD, os.path.dirname(os.path.abspath(__file__))], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=240)
    assert p.returncode == 0, p.stderr[-3000:]
    (line,) = [ln for ln in p.stdout.splitlines() if ln.startswith("LISTS ")]
    return json.loads(line[6:])


def test_the_early_exit_does_not_change_a_list():
    """MMSBM_PARTNERS_STAT_EARLY is read at the call: each setting runs in a child process of its
    own.  Every m of five slots (m = 1 and m = ns among them), N far below the candidate count, one
    query spread over the device and four in one call."""
    on, off = run_child(None), run_child("0")
    assert sorted(on) == sorted(off) and len(on) == 30
    assert on == off
    # and the lists are the ones this process gets
    th, pr = params(7, 100, 5, 9)
    eng = make_engine(th, pr)
    order, _ = scan_ref.rank_tables(100)
    genes = [int(order[q]) for q in (0, 16, 50, 99)]
    for m in (1, 5):
        here = eng.partners_quorum_top(genes, 5, m)
        assert [[s.tobytes().hex(), ids.tobytes().hex()] for s, ids in here] == on["%d 5 4" % m]
    eng.close()


# ------------------------------------------------------------------ 5b. long lists out of many candidates
@pytest.mark.parametrize("K,P,B,seed", pc.LONG_CASES, ids=lambda v: str(v))
def test_long_lists_out_of_many_candidates(K, P, B, seed):
    """N = 300 and 1024 where a query has 4851 (P = 100: 49 workgroups at Q = 1) and 44 551 candidates
    (P = 300: hundreds of workgroups, several column chunks, two merge levels): the statistic's
    candidate buffer fills and is cut back to the best N, per workgroup and again in the merge.
    Against the independent reference by the set rule at clear cuts (asserted on the reference alone;
    tests/test_partners_stat_host.py shows 300 and 1024 are clear for every query and statistic), the
    seven queries in one call and each alone, bit-equal.  At P = 100 also exactly: numpy's order
    statistic and lexsort of the slots' own words of every candidate, from 5 chunks x 5 slots of
    partners_top under a `known` table.  At P = 300 that would take 44 chunks per slot and is left
    out."""
    c = pc.long_case(K, P, B, seed)
    eng = make_engine(c.theta, c.pr)
    calls = ref.stat_calls(B)
    kept = {}
    for stat in calls:
        cuts = [pc.long_cuts(r, stat) for r in c.refs]         # the precondition
        for n in sorted({n for two in cuts for n in two}):
            idx = [i for i, two in enumerate(cuts) if n in two]
            got = stat_top(eng, [c.genes[i] for i in idx], n, *stat)
            for i, lst in zip(idx, got):
                pc.check_list(lst, c.refs[i], stat, n, P, c.genes[i])
                (solo,) = stat_top(eng, [c.genes[i]], n, *stat)
                same_list(solo, lst, ("alone", stat, n, i))
                kept[stat, n, i] = lst
    assert len(kept) == len(calls) * 2 * len(c.genes)
    if P == 100:
        parts = 5
        assert all(len(pc.chunks(r)) == parts for r in c.refs)
        words = []      # [slot][query]
        for s in range(B):
            by_part = [eng.partners_top(c.genes, FULL, pc.chunk_known(P, c.positions, c.refs, part), sample=s)
                       for part in range(parts)]
            words.append([pc.words_from_chunks([by_part[part][i] for part in range(parts)], r, P)
                          for i, r in enumerate(c.refs)])
        for (stat, n, i), lst in kept.items():
            v = ref.stat(np.stack([words[s][i] for s in range(B)]), *stat)
            same_list(lst, ref.top_list(v, c.refs[i].tkeys, P, n), (stat, n, i))
            if stat[0] == "spread":
                assert not np.signbit(lst[0]).any()
        # each query confined to ONE workgroup (eight queries per compute unit leave it no more): 4851
        # candidates go through its buffer of 2 N <= 2048 entries, which fills and is cut back to the best N
        genes, idx = confined(eng, c.genes)
        for stat in calls:
            for n in pc.LONG_NS:
                for i, lst in zip(idx, stat_top(eng, genes, n, *stat)):
                    same_list(lst, kept[stat, n, i], ("one workgroup", stat, n, i))
    eng.close()


def confined(eng, genes):
    """The queries repeated until the call has at least eight per compute unit -> (gene ids, the index
    of each into `genes`)."""
    import torch
    units = torch.cuda.get_device_properties(eng.device).multi_processor_count
    reps = -(-8 * units // len(genes)) + 1
    assert 8 * units <= reps * len(genes) <= 65535
    return list(genes) * reps, list(range(len(genes))) * reps


def test_total_ties_under_a_live_bound(monkeypatch):
    """Every candidate of a query has the same word in a slot (partners_converged_ref.tie_case: exact
    in any order of the sums), so every statistic ties all 1711 of them and the list is the N smallest
    triple keys.  A query confined to one workgroup overflows its buffer of 512 entries, which is cut
    back to N: from then on EVERY value sits exactly on the bound, while tiles still to come hold
    smaller keys than the bound's (a row block is walked tile by tile, not in key order).  A tile may
    end early only if no element can reach the bound; an element that equals it still can.  In bits
    and ids against the numpy reference, with the early exit and without it."""
    c = pc.tie_case()
    K, P, B = pc.TIE_SHAPE
    eng = make_engine(c.theta, c.pr)
    monkeypatch.delenv("MMSBM_PARTNERS_STAT_EARLY", raising=False)
    genes, idx = confined(eng, c.genes)
    for stat in ref.stat_calls(B):
        for n in pc.TIE_NS:
            want = [ref.top_list(ref.stat(r.per, *stat), r.tkeys, P, n) for r in c.refs]
            for q, i in ((c.genes, range(len(c.genes))), (genes, idx)):
                got = stat_top(eng, q, n, *stat)
                for j, lst in zip(i, got):
                    same_list(lst, want[j], (stat, n, j, len(q)))
                if stat[0] == "quorum":
                    monkeypatch.setenv("MMSBM_PARTNERS_STAT_EARLY", "0")
                    again = stat_top(eng, q, n, *stat)
                    monkeypatch.delenv("MMSBM_PARTNERS_STAT_EARLY")
                    for a, b in zip(got, again):
                        same_list(a, b, ("early exit", stat, n))
    eng.close()


def test_the_early_exit_keeps_a_long_list(monkeypatch):
    """N = 1024 out of 4851 candidates, every m of five slots, the seven queries in one call, one alone
    and each confined to one workgroup: MMSBM_PARTNERS_STAT_EARLY is read at every call."""
    K, P, B, seed = pc.LONG_CASES[0]
    c = pc.long_case(K, P, B, seed)
    eng = make_engine(c.theta, c.pr)
    monkeypatch.delenv("MMSBM_PARTNERS_STAT_EARLY", raising=False)
    for m in range(1, B + 1):
        for genes in (c.genes, c.genes[1:2], confined(eng, c.genes)[0]):       # the last: the buffer fills, the bound is set
            on = eng.partners_quorum_top(genes, FULL, m)
            monkeypatch.setenv("MMSBM_PARTNERS_STAT_EARLY", "0")
            off = eng.partners_quorum_top(genes, FULL, m)
            monkeypatch.delenv("MMSBM_PARTNERS_STAT_EARLY")
            assert len(on) == len(off) == len(genes)
            for a, b in zip(on, off):
                assert a[0].size == FULL
                same_list(a, b, (m, len(genes)))
    eng.close()


# ------------------------------------------------------------------ 6. independence
def test_a_query_does_not_depend_on_the_call_or_on_the_order_of_the_slots():
    K, P, B, N = 10, 50, 8, 16
    th, pr = params(K, P, B, 6)
    order, _ = scan_ref.rank_tables(P)
    rng = np.random.default_rng(2)
    g = int(order[17])
    others = [int(x) for x in rng.integers(0, P, 16)]
    eng = make_engine(th, pr)
    perm = rng.permutation(B)
    eng2 = make_engine(th[perm], pr[perm])
    th0, p0 = bits(eng.theta.cpu().numpy()), bits(eng.pr.cpu().numpy())
    for what, arg in (("quorum", 8), ("quorum", 3), ("quorum", 5), ("quorum", 1), ("spread", 0), ("spread", 2)):
        (solo,) = stat_top(eng, [g], N, what, arg)
        assert solo[0].size == N
        for at in (0, 9, 16):
            mixed = others[:at] + [g] + others[at:]
            assert len(mixed) == 17
            same_list(stat_top(eng, mixed, N, what, arg)[at], solo, (what, arg, at))
        same_list(stat_top(eng2, [g], N, what, arg)[0], solo, (what, arg, "slots permuted"))
    assert bits(eng.theta.cpu().numpy()) == th0 and bits(eng.pr.cpu().numpy()) == p0
    eng.close()
    eng2.close()


# ------------------------------------------------------------------ 7. refusals
class RawStat:
    """mmsbm_partners_stat_topn as C sees it, on sentinel-filled outputs."""

    def __init__(self, eng, nq, N):
        import torch
        self.eng, self.torch, self.Q, self.N = eng, torch, nq, N
        self.ws = eng.scan_workspace("partners", nq, N)
        full = lambda shape, dtype: torch.full(shape, SENTINEL, dtype=dtype, device=eng.device)
        self.outs = [full((nq, N), torch.float64), full((nq, N, 3), torch.int32), full((nq,), torch.int64)]

    def args(self, genes, stat, arg):
        eng = self.eng
        self.genes = np.ascontiguousarray(genes, dtype=np.int32)
        return [eng.ctx, eng.scan_order.data_ptr(), self.genes.ctypes.data_as(ctypes.c_void_p), self.Q, None, None, None,
                eng.theta.data_ptr(), eng.pr.data_ptr(), stat, arg, self.N, self.ws.data_ptr(), self.ws.numel(),
                *[o.data_ptr() for o in self.outs], eng._stream()]

    def call(self, args):
        rc = self.eng.lib.mmsbm_partners_stat_topn(*args)
        self.torch.cuda.synchronize(self.eng.device)
        return rc

    def intact(self):
        return all(bool((o == SENTINEL).all()) for o in self.outs)


def test_refusals_leave_the_outputs_alone():
    from trigenicinteractionpredictor_amd import _lib
    INVALID, UNSUPPORTED = _lib.MMSBM_ERR_INVALID, _lib.MMSBM_ERR_UNSUPPORTED
    QUORUM, SPREAD = _lib.MMSBM_PARTNERS_STAT_QUORUM, _lib.MMSBM_PARTNERS_STAT_SPREAD
    P, nq, N, B = 20, 3, 8, 12
    th, pr = params(3, P, B, 5)
    eng = make_engine(th, pr)
    assert eng.partners_stat_max_depth == eng.lib.mmsbm_partners_stat_max_depth() == 4
    good = [1, 19, 7]
    raw = RawStat(eng, nq, N)
    # in the argument list: 0 ctx, 1 order, 2 queries, 3 Q, 4 known_off, 5 known_pairs, 6 mask, 7 theta, 8 pr,
    # 9 stat, 10 arg, 11 N, 12 ws, 13 ws_bytes, 14-16 the outputs, 17 the stream
    bad = [("unknown stat 2", good, QUORUM, 1, [(9, 2)], INVALID), ("unknown stat -1", good, QUORUM, 1, [(9, -1)], INVALID),
           ("m 0", good, QUORUM, 0, [], INVALID), ("m -1", good, QUORUM, -1, [], INVALID),
           ("m ns + 1", good, QUORUM, B + 1, [], INVALID),
           ("t -1", good, SPREAD, -1, [], INVALID), ("t leaves no two", good, SPREAD, 6, [], INVALID),
           ("depth 5 from the top", good, QUORUM, 5, [], UNSUPPORTED), ("depth 5 from the bottom", good, QUORUM, 8, [], UNSUPPORTED),
           ("ns 12, m 6", good, QUORUM, 6, [], UNSUPPORTED), ("trim 4", good, SPREAD, 4, [], UNSUPPORTED),
           ("trim 5", good, SPREAD, 5, [], UNSUPPORTED),
           ("null ctx", good, QUORUM, 1, [(0, None)], INVALID), ("null order", good, QUORUM, 1, [(1, None)], INVALID),
           ("null queries", good, SPREAD, 0, [(2, None)], INVALID), ("null theta", good, QUORUM, 1, [(7, None)], INVALID),
           ("null pr", good, SPREAD, 0, [(8, None)], INVALID),
           ("known_off alone", good, QUORUM, 1, [(4, raw.ws.data_ptr())], INVALID),
           ("misaligned mask", good, QUORUM, 1, [(6, raw.ws.data_ptr() + 2)], INVALID),
           ("id P", [1, P, 7], QUORUM, 1, [], INVALID), ("id -1", [1, 19, -1], SPREAD, 0, [], INVALID),
           ("Q -1", good, QUORUM, 1, [(3, -1)], INVALID), ("Q 65536", good, QUORUM, 1, [(3, 65536)], INVALID),
           ("no ws", good, QUORUM, 1, [(12, None)], INVALID),
           ("misaligned ws", good, SPREAD, 0, [(12, raw.ws.data_ptr() + 8)], INVALID),
           ("small ws", good, QUORUM, 1, [(13, raw.ws.numel() // 2)], INVALID),
           ("N 0", good, QUORUM, 1, [(11, 0)], INVALID), ("N -1", good, QUORUM, 1, [(11, -1)], INVALID),
           ("N 1025", good, SPREAD, 0, [(11, 1025)], UNSUPPORTED)]
    bad += [("null output %d" % i, good, QUORUM, 1, [(14 + i, None)], INVALID) for i in range(3)]
    for what, genes, stat, arg, replace, code in bad:
        args = raw.args(genes, stat, arg)
        for i, v in replace:
            args[i] = v
        assert raw.call(args) == code, what
        assert raw.intact(), what
        assert eng.lib.mmsbm_last_error()
    # one active slot: the spread is refused, the quorum takes m = 1 only
    eng.set_active(1)
    for stat, arg in ((SPREAD, 0), (QUORUM, 2)):
        assert raw.call(raw.args(good, stat, arg)) == INVALID and raw.intact()
    eng.set_active(B)
    # Q = 0 returns OK and writes nothing
    args = raw.args(good, QUORUM, 1)
    args[3] = 0
    assert raw.call(args) == 0 and raw.intact()
    # the context is usable afterwards, through the same scratch and outputs; the legal edge of every cap
    for stat, arg in ((QUORUM, 4), (QUORUM, 9), (SPREAD, 3)):
        assert raw.call(raw.args(good, stat, arg)) == 0
    want = eng.partners_spread_top(good, N, 3)
    for i in range(nq):
        assert bits(raw.outs[0][i].cpu().numpy()) == bits(want[i][0])
        assert bits(raw.outs[1][i].cpu().numpy()) == bits(want[i][1])
    assert raw.outs[2].cpu().tolist() == [N] * nq
    # the workspace is the partner scan's
    nbytes = ctypes.c_int64(-7)
    assert eng.lib.mmsbm_partners_workspace_bytes(eng.ctx, nq, N, ctypes.byref(nbytes)) == 0
    assert nbytes.value == raw.ws.numel() or 0 < nbytes.value <= raw.ws.numel()
    eng.close()


def test_the_ensemble_rule_of_the_partner_scan():
    """K = 30 with 12 active slots: 12 (4 ceil(30 / 4) + 2) = 408 > 384."""
    from trigenicinteractionpredictor_amd import _lib
    P, nq, N = 20, 2, 8
    th, pr = params(30, P, 12, 5)
    eng = make_engine(th, pr)
    raw = RawStat(eng, nq, N)
    for stat, arg in ((_lib.MMSBM_PARTNERS_STAT_QUORUM, 1), (_lib.MMSBM_PARTNERS_STAT_QUORUM, 12),
                      (_lib.MMSBM_PARTNERS_STAT_SPREAD, 0)):
        assert raw.call(raw.args([1, 7], stat, arg)) == _lib.MMSBM_ERR_UNSUPPORTED and raw.intact()
        assert b"LDS" in eng.lib.mmsbm_last_error()
    with pytest.raises(_lib.MMSBMError):
        eng.partners_quorum_top([1, 7], N, 1)
    eng.set_active(11)      # 11 x 34 = 374 fits
    assert raw.call(raw.args([1, 7], _lib.MMSBM_PARTNERS_STAT_QUORUM, 11)) == 0 and not raw.intact()
    eng.close()


def test_python_checks():
    th, pr = params(3, 20, 12, 5)
    eng = make_engine(th, pr)
    from trigenicinteractionpredictor_amd._lib import MMSBMError
    for m in (0, -1, 13):
        with pytest.raises(ValueError):
            eng.partners_quorum_top([1, 2], 8, m)
    for t in (-1, 6):
        with pytest.raises(ValueError):
            eng.partners_spread_top([1, 2], 8, t)
    for m in (5, 8):
        with pytest.raises(MMSBMError):
            eng.partners_quorum_top([1, 2], 8, m)
    with pytest.raises(MMSBMError):
        eng.partners_spread_top([1, 2], 8, 4)
    with pytest.raises(MMSBMError):
        eng.partners_quorum_top([1, 20], 8, 1)
    same_list(eng.partners_quorum_top([1], 8)[0], eng.partners_quorum_top([1], 8, 12)[0], "default")
    eng.close()


# ------------------------------------------------------------------ 8. the driver
def test_driver_writes_the_two_tables(tmp_path):
    from trigenicinteractionpredictor_amd import Model, _lib, scan
    from trigenicinteractionpredictor_amd.engine import EMEngine
    from trigenicinteractionpredictor_amd.restarts import stream_states
    g = os.path.join(GOLDEN, "tiny")
    train, test = os.path.join(g, "train.dat"), os.path.join(g, "test.dat")
    K, B, iters, seed, top = 3, 3, 5, 1, 6
    model = Model()
    model.get_traintest(train, test)

    def run(tag):
        files = {n: str(tmp_path / (n + tag + ".tsv")) for n in ("out", "quorum", "disputed")}
        argv = ["-t", train, "-e", test, "-k", str(K), "-n", str(B), "-i", str(iters), "--seed", str(seed), "-o",
                files["out"], "--gene", "7", "--top", str(top), "--partners-quorum", files["quorum"],
                "--partners-disputed", files["disputed"]]
        assert scan.main(argv, out=lambda *a: None) == 0
        return files

    files, again = run(""), run("-again")
    for n in files:
        assert open(files[n], "rb").read() == open(again[n], "rb").read(), n
    # the same fit
    random.seed(seed)
    eng = EMEngine(K, model.P, B=B, R=model.R, eps=model.eps)
    eng.set_links(_lib.SET_TRAIN, *model._link_arrays(0))
    for b, (_, theta, pr) in enumerate(stream_states(model, K, range(B))):
        eng.upload_slot(b, theta, pr)
    eng.iterate(iters)
    (query,) = scan.resolve_genes(model, ["7"])
    known = scan.partner_known(model, [query], ("train", "test"))
    for name, label, column, arg, lists in (("quorum", "votes", "quorum", B, eng.partners_quorum_top([query], top, None, known)),
                                            ("disputed", "trim", "spread", 0, eng.partners_spread_top([query], top, 0, known))):
        lines = open(files[name], encoding="utf-8").read().rstrip("\n").split("\n")
        assert lines[0] == "# samples\t%d" % B and lines[1] == "# partners %s\t%d" % (label, arg)
        assert lines[2].split("\t") == ["query", "rank", column, "ids", "names"]
        rows = [ln.split("\t") for ln in lines[3:]]
        (scores, ids), = lists
        assert len(rows) == len(scores) == top
        for rank, (r, v, row) in enumerate(zip(rows, scores, ids), 1):
            assert r[0] == model.id_gene[query] and int(r[1]) == rank and r[2] == repr(float(v))
            assert r[3] == "_".join(str(int(x)) for x in row) and query in row.tolist()
            assert r[4] == "_".join(sorted(model.id_gene[int(x)] for x in row))
    # the --gene table of the same run is what it is without the new tables
    plain = str(tmp_path / "plain.tsv")
    assert scan.main(["-t", train, "-e", test, "-k", str(K), "-n", str(B), "-i", str(iters), "--seed", str(seed), "-o",
                      plain, "--gene", "7", "--top", str(top)], out=lambda *a: None) == 0
    assert open(plain).read() == open(files["out"]).read()
    eng.close()
