"""The partner family on CONVERGED fits (tests/golden/converged/): partners_top with the ensemble,
with every slot of a batch and under a pair mask (partners_masked_kernel), and partners_quorum_top /
partners_spread_top (partners_stat_kernel), every gene of a set a query.

On a converged fit a query's best scores saturate at 1 - O(eps) and distinct candidates share their
bits, so the order of its list is not determined by the reference: the lists are compared by SET at
clear cuts (tests/partners_converged_ref.py; the preconditions are asserted on the reference alone
there and, for every case, in tests/test_converged_host.py).  The quorum's early exit stops a tile
once no element can reach the bound, and saturated, bit-equal values crowd at exactly that bound:
every quorum call is repeated with MMSBM_PARTNERS_STAT_EARLY=0 and must keep its bits.  Last,
without a tolerance, crowded or not: a statistic's list is numpy's order statistic and lexsort of
the slots' own words of EVERY candidate, which come from partners_top over chunks of at most 1024
candidates (a `known` table leaves each call one chunk)."""
import numpy as np
import pytest

import partners_converged_ref as pc
import partners_stat_ref as ps
import scan_ref
from scan_gpu import engine
from test_gpu_partners_stat import same_list

pytestmark = pytest.mark.gpu

EARLY = "MMSBM_PARTNERS_STAT_EARLY"
TOP_PARAMS = [(label, known) for label in pc.SETS for known in pc.KNOWN]
STAT_PARAMS = [(label, known) for label in pc.STAT_SETS for known in pc.KNOWN]
top_cases = pytest.mark.parametrize("label,known", TOP_PARAMS, ids=["%s-%s" % c for c in TOP_PARAMS])
stat_cases = pytest.mark.parametrize("label,known", STAT_PARAMS, ids=["%s-%s" % c for c in STAT_PARAMS])
masks = pytest.mark.parametrize("masked", [False, True], ids=["all", "masked"])


@pytest.fixture(autouse=True)
def plain_env(monkeypatch):
    monkeypatch.delenv(EARLY, raising=False)


def call(eng, stat, genes, n, known, mask):
    what, arg = stat
    if what == "quorum":
        return eng.partners_quorum_top(genes, n, arg, known, mask=mask)
    if what == "spread":
        return eng.partners_spread_top(genes, n, arg, known, mask=mask)
    return eng.partners_top(genes, n, known, sample=pc.sample_of(stat), mask=mask)


def at_clear_cuts(eng, label, known, masked, stat, also=None):
    """Every query at its two N, the queries of one N in one call, against the reference; also(got,
    genes, n, known table, indices): a further check of that call's lists."""
    c = pc.case(label, known, masked)
    plan = pc.plan(label, known, masked, stat)          # asserts the preconditions, on the reference alone
    assert sorted(i for idx in plan.by_n.values() for i in idx) == sorted(2 * list(range(c.P)))   # no query left out
    for n, idx in plan.by_n.items():
        genes = [c.genes[i] for i in idx]
        kn = pc.csr_take(c.known, idx)
        got = call(eng, stat, genes, n, kn, c.mask)
        assert len(got) == len(idx)
        for i, lst in zip(idx, got):
            pc.check_list(lst, c.refs[i], stat, n, c.P, c.genes[i])
        if also is not None:
            also(got, genes, n, kn, idx)


# --------------------------------------------------------------------- (a) the ensemble and every slot
@top_cases
def test_partners_top_of_the_ensemble_and_of_every_slot(label, known):
    c = pc.case(label, known, False)
    eng = engine(c.theta, c.pr)
    for stat in pc.lists_of(c.B):
        at_clear_cuts(eng, label, known, False, stat)
    if c.B > 1:     # slot 1 of the batch = an engine holding that sample alone
        solo = engine(c.theta[1:2], c.pr[1:2])
        for n in (pc.FULL, 64):
            for a, b in zip(eng.partners_top(c.genes, n, c.known, sample=1), solo.partners_top(c.genes, n, c.known, sample=0)):
                same_list(a, b, ("slot 1 alone", n))
        solo.close()
    eng.close()


# --------------------------------------------------------------------- (b) under a pair mask
@top_cases
def test_partners_top_under_a_pair_mask(label, known):
    """A masked call is, bit for bit, the unmasked call with the blocked candidates put into the
    query's known pairs; and it matches the reference over the candidates the mask leaves."""
    c = pc.case(label, known, True)
    whole = pc.case(label, known, False)
    for r, w in zip(c.refs, whole.refs):        # on the reference: every query keeps and loses candidates
        assert 0 < r.tkeys.size < w.tkeys.size
    eng = engine(c.theta, c.pr)
    for stat in pc.lists_of(c.B):
        def identity(got, genes, n, kn, idx, stat=stat):
            want = call(eng, stat, genes, n, pc.csr_take(c.merged, idx), None)
            for a, b in zip(got, want):
                same_list(a, b, ("mask = known", stat, n))
        at_clear_cuts(eng, label, known, True, stat, identity)
    eng.close()


# --------------------------------------------------------------------- (c) the statistics
@masks
@stat_cases
def test_partner_statistics_at_clear_cuts(monkeypatch, label, known, masked):
    c = pc.case(label, known, masked)
    calls = ps.stat_calls(c.B)
    assert calls == [("quorum", 1), ("quorum", 2), ("quorum", 3), ("spread", 0)]
    eng = engine(c.theta, c.pr)
    for stat in calls:
        def without_early_exit(got, genes, n, kn, idx, stat=stat):
            monkeypatch.setenv(EARLY, "0")
            again = call(eng, stat, genes, n, kn, c.mask)
            monkeypatch.delenv(EARLY)
            for a, b in zip(got, again):
                same_list(a, b, ("early exit", stat, n))
        at_clear_cuts(eng, label, known, masked, stat, without_early_exit if stat[0] == "quorum" else None)
    eng.close()


# --------------------------------------------------------------------- (d) exact, from the slots' own words
def slot_words(eng, c):
    """[slot][query] -> the slot's own words of EVERY eligible candidate in triple-key order: one
    partners_top call per chunk of at most 1024 candidates, the `known` table leaving each query that
    chunk alone; the chunks are disjoint and cover the candidates (words_from_chunks asserts it)."""
    _, rank = scan_ref.rank_tables(c.P)
    positions = [int(rank[g]) for g in c.genes]
    parts = max(len(pc.chunks(r)) for r in c.refs)
    assert parts >= 2 and max(r.tkeys.size for r in c.refs) > pc.FULL     # more candidates than a slot's list has rows
    out = []
    for s in range(c.B):
        by_part = [eng.partners_top(c.genes, pc.FULL, pc.chunk_known(c.P, positions, c.refs, part), sample=s, mask=c.mask)
                   for part in range(parts)]
        out.append([pc.words_from_chunks([by_part[part][i] for part in range(len(pc.chunks(r)))], r, c.P)
                    for i, r in enumerate(c.refs)])
    return out


def exact_lists(words, c, stat, n):
    """numpy's order statistic of the slots' words, lexsorted by (value descending, key ascending)."""
    return [ps.top_list(ps.stat(np.stack([words[s][i] for s in range(c.B)]), *stat), r.tkeys, c.P, n)
            for i, r in enumerate(c.refs)]


@masks
@stat_cases
def test_statistics_are_the_order_statistics_of_every_candidates_words(label, known, masked):
    c = pc.case(label, known, masked)
    eng = engine(c.theta, c.pr)
    words = slot_words(eng, c)
    for stat in ps.stat_calls(c.B):
        for n in (64, pc.FULL):
            got = call(eng, stat, c.genes, n, c.known, c.mask)
            for i, want in enumerate(exact_lists(words, c, stat, n)):
                same_list(got[i], want, (stat, n, i))
                if stat[0] == "spread":
                    assert not np.signbit(got[i][0]).any()
    eng.close()


# --------------------------------------------------------------------- (e) the bound at work
@masks
@pytest.mark.parametrize("label", pc.STAT_SETS)
def test_a_query_confined_to_one_workgroup_meets_its_own_bound(monkeypatch, label, masked):
    """With 60 queries in a call every query is spread over as many workgroups as it has items, no
    buffer ever fills and no bound is ever set: the early exit cannot fire.  Here the call repeats the
    60 genes until it has at least eight queries per compute unit, which leaves each query ONE
    workgroup: its buffer (512 entries for N <= 256) overflows under the query's candidates, is cut
    back to the best N, and the N-th best value becomes the bound the early exit and the selection
    compare with, while saturated, bit-equal values sit exactly on it.  Exact, as in (d): every copy
    of every query is numpy's list of the slots' own words, with the early exit and without it."""
    import torch
    c = pc.case(label, "fold", masked)
    eng = engine(c.theta, c.pr)
    words = slot_words(eng, c)
    units = torch.cuda.get_device_properties(eng.device).multi_processor_count
    reps = -(-8 * units // c.P) + 1
    genes = c.genes * reps
    idx = list(range(c.P)) * reps
    assert len(genes) >= 8 * units and len(genes) <= 65535
    known = pc.csr_take(c.known, idx)
    for stat in ps.stat_calls(c.B):
        for n in (8, 64, 256):
            assert all(r.tkeys.size > 512 >= 2 * n for r in c.refs)     # the buffer overflows
            want = exact_lists(words, c, stat, n)
            got = call(eng, stat, genes, n, known, c.mask)
            assert len(got) == len(genes)
            for i, lst in zip(idx, got):
                same_list(lst, want[i], (stat, n, i))
            if stat[0] == "quorum":
                monkeypatch.setenv(EARLY, "0")
                again = call(eng, stat, genes, n, known, c.mask)
                monkeypatch.delenv(EARLY)
                for a, b in zip(got, again):
                    same_list(a, b, ("early exit", stat, n))
    eng.close()
