"""Helper of tests/test_gpu_partners_converged.py, tests/test_gpu_partners_stat.py and their CPU
preconditions in tests/test_converged_host.py and tests/test_partners_stat_host.py (not a test): the
partner family's lists under the set-at-a-clear-cut rule of tests/converged_ref.py.

Per query the reference is partners_ref.ref_query of every slot; the ensemble is
scan_ref.prefix_mean in slot order, the quorum score and the spread are partners_stat_ref.stat.  A
list is compared by SET at a clear cut N (the reference's gap under its N-th value exceeds
census_ref.GAP: relative for a score and a quorum score, absolute for a spread), every value with
the reference value of its own key (scan_ref.RTOL relative; spread_ref.atol for a spread), the order
on the list's own bits, and every row holds the query.  Each query has two N: the smallest clear cut
in [8, 256] and the largest in [257, 1024]; a query without one fails the precondition, none is left
out.  numpy only: no GPU, no product code beyond the rank order, the fold's known pairs and the
shared pair mask."""
import collections
import functools

import numpy as np

import converged_ref as cr
import partners_masked_ref as pm
import partners_stat_ref as ps
import scan_ref
import spread_ref

FULL = 1024                     # mmsbm_partners_max_n()
STAT_SETS = ("A300", "A1000")   # three seeds as B = 3
SETS = STAT_SETS + ("C20",)     # and one K = 20 sample, for the calls that take one slot
KNOWN = ("none", "fold")
SMALL, LARGE = (8, 256), (257, FULL)
CROWDED = 57                    # of 60 queries, unmasked, for the ensemble and every statistic: see crowded_enough
TIGHT_REL, TIGHT_ABS = 1e-9, 4 * spread_ref.RTOL

Case = collections.namedtuple("Case", "P B theta pr genes known mask merged refs")
Query = collections.namedtuple("Query", "per tkeys pkeys total")     # eligible candidates, triple keys ascending


def csr_take(known, idx):
    """The (known_off, known_pairs) of the queries `idx` of a CSR table (None stays None)."""
    if known is None:
        return None
    off, pairs = known
    parts = [pairs[off[i]:off[i + 1]] for i in idx]
    out = np.zeros(len(idx) + 1, dtype=np.int64)
    out[1:] = np.cumsum([p.size for p in parts])
    return out, (np.concatenate(parts) if parts else np.zeros(0, np.int64)).astype(np.int64)


def query_of(thetas, prs, q, drop=None):
    """The reference of the query at rank position q over the candidates whose pair key is not in
    `drop` -> Query (per f64[B][n], triple keys ascending, their pair keys, all candidates)."""
    per, tk, pk = ps.ref_slots(thetas, prs, q)
    total = tk.size
    if drop is not None and len(drop):
        keep = ~np.isin(pk, drop)
        per, tk, pk = per[:, keep], tk[keep], pk[keep]
    at = np.argsort(tk)
    per, tk, pk = per[:, at], tk[at], pk[at]
    for a in (per, tk, pk):
        a.setflags(write=False)
    return Query(per, tk, pk, total)


@functools.lru_cache(maxsize=None)
def case(label, known, masked):
    """One parameter set with every gene as a query: the `known` table the calls take (none, or the
    fold's train and test pairs through scan.partner_known), the shared random pair mask (masked) and
    the table `merged` the masked call stands for, and every query's reference over its eligible
    candidates."""
    from trigenicinteractionpredictor_amd.scan import partner_known
    cks = [cr.load(n) for n in cr.SCAN_SETS[label]]
    P = cks[0].P
    th, pr = np.stack([c.theta for c in cks]), np.stack([c.pr for c in cks])
    genes = list(range(P))
    _, rank = scan_ref.rank_tables(P)
    kn = partner_known((P, cks[0].ids, cks[0].test_ids), genes) if known == "fold" else None
    mask = np.ascontiguousarray(cr.random_pair_mask_words(P)) if masked else None
    merged = pm.merged_known(mask, P, genes, kn) if masked else kn
    refs = []
    for i, g in enumerate(genes):
        drop = None if merged is None else merged[1][merged[0][i]:merged[0][i + 1]]
        refs.append(query_of(th, pr, int(rank[g]), drop))
    return Case(P, len(cks), th, pr, genes, kn, mask, merged, refs)


def lists_of(B):
    """What the partner scan ranks by at B slots: ("mean", None) the ensemble, ("slot", s)."""
    return ([("mean", None)] if B > 1 else []) + [("slot", s) for s in range(B)]


def sample_of(stat):
    return None if stat[0] == "mean" else stat[1]


def values(per, stat):
    """The ranking value of every candidate -> f64[n]."""
    what, arg = stat
    if what == "mean":
        return scan_ref.prefix_mean(per, per.shape[0])
    if what == "slot":
        return per[arg]
    return ps.stat(per, what, arg)


def clear(desc, what, lo, hi):
    return cr.clear_cuts_abs(desc, lo, hi) if what == "spread" else cr.clear_cuts(desc, lo, hi)


def two_cuts(v, what):
    """(the smallest clear cut in [8, 256], the largest in [257, 1024]) of one query's values; None
    where there is none."""
    desc = np.sort(v)[::-1]
    small, large = clear(desc, what, *SMALL), clear(desc, what, *LARGE)
    return (int(small[0]) if small.size else None, int(large[-1]) if large.size else None)


def tight(v, what, n=FULL):
    """The adjacent gaps inside the top n that an error within the tolerance could close."""
    s = np.sort(v)[::-1][:n]
    if what == "spread":
        return int(np.count_nonzero(s[:-1] - s[1:] <= TIGHT_ABS))
    return cr.tight_gaps(s, n, TIGHT_REL)


Plan = collections.namedtuple("Plan", "by_n crowded")


def plan_of(refs, stat):
    """The preconditions on the reference alone, and the calls: every query has both cuts ->
    Plan({N: [the indices of the queries with that cut]}, the number of queries with a tight gap
    inside their top 1024)."""
    by_n, crowded = {}, 0
    for i, r in enumerate(refs):
        v = values(r.per, stat)
        cuts = two_cuts(v, stat[0])
        assert None not in cuts, ("query %d has no clear cut" % i, stat, cuts)
        assert SMALL[0] <= cuts[0] <= SMALL[1] < cuts[1] <= min(LARGE[1], v.size - 1)
        for n in cuts:
            by_n.setdefault(n, []).append(i)
        crowded += tight(v, stat[0]) > 0
    return Plan(dict(sorted(by_n.items())), crowded)


@functools.lru_cache(maxsize=None)
def plan(label, known, masked, stat):
    """plan_of one case, with the crowding asserted: the order really is undetermined."""
    p = plan_of(case(label, known, masked).refs, stat)
    assert crowded_enough(p, label, masked, stat), (label, known, masked, stat, p.crowded)
    return p


def crowded_enough(p, label, masked, stat):
    """At least 57 of the 60 queries of a three-seed set have a tight gap inside their top 1024 for
    the ensemble and for every statistic of the unmasked call; one slot's list, a masked call's and
    the single K = 20 sample's crowd for fewer queries, but for some."""
    if label in STAT_SETS and not masked and stat[0] != "slot":
        return p.crowded >= CROWDED
    return p.crowded > 0


def check_list(got, r, stat, n, P, gene):
    """One query's (values, ids) against its reference under the four parts of the rule."""
    got_s, got_ids = got
    v = values(r.per, stat)
    if stat[0] == "spread":
        cr.check_set_cut_abs(got_s, got_ids, v, spread_ref.atol(r.per, stat[1]), r.tkeys, n, None, P)
        assert not np.signbit(got_s).any()
    else:
        cr.check_set_cut(got_s, got_ids, v, r.tkeys, n, None, P)
    assert (got_ids == gene).any(axis=1).all(), "a row without the query"


def chunks(r, limit=FULL):
    """The query's eligible candidates in pair-key order, split into the fewest near-equal chunks of
    at most `limit` -> [sorted pair keys]."""
    pk = np.sort(r.pkeys)
    parts = -(-pk.size // limit)
    return [c for c in np.array_split(pk, parts)] if parts else []


def all_pairs(P, q):
    """Every candidate pair key b P + c of the query at rank position q, ascending."""
    b, c = np.triu_indices(P, k=1)
    keep = (b != q) & (c != q)
    return b[keep].astype(np.int64) * P + c[keep]


def chunk_known(P, positions, refs, part, limit=FULL):
    """The `known` table that leaves each query only chunk `part` of its eligible candidates: every
    other pair of the query (the base table and the mask's pairs among them) -> CSR."""
    off, out = [0], []
    for q, r in zip(positions, refs):
        ch = chunks(r, limit)
        mine = ch[part] if part < len(ch) else np.zeros(0, np.int64)
        out.append(np.setdiff1d(all_pairs(P, q), mine))
        off.append(off[-1] + out[-1].size)
    return np.array(off, dtype=np.int64), np.concatenate(out).astype(np.int64)


def words_from_chunks(lists, r, P):
    """One slot's lists of one query, one per chunk -> its words of every eligible candidate in
    triple-key order; the chunks are disjoint and cover the reference's eligible candidates."""
    keys = np.concatenate([scan_ref.packed(ids, P) for _, ids in lists])
    words = np.concatenate([s for s, _ in lists])
    assert [s.size for s, _ in lists] == [c.size for c in chunks(r)], "a chunk's list is not complete"
    assert np.unique(keys).size == keys.size, "the chunks overlap"
    at = np.argsort(keys)
    np.testing.assert_array_equal(keys[at], r.tkeys, err_msg="the chunks do not cover the candidates")
    return words[at]


# ------------------------------------------------ long lists out of many candidates, random parameters
LONG_CASES = [(7, 100, 5, 9), (3, 300, 3, 11)]      # (K, P, B, seed): 4851 and 44 551 candidates per query
LONG_NS = (300, FULL)

Long = collections.namedtuple("Long", "theta pr positions genes refs")


@functools.lru_cache(maxsize=None)
def long_case(K, P, B, seed):
    """scan_ref.random_params with the queries partners_stat_ref.positions(P) and their reference."""
    th, pr = scan_ref.random_params(K, P, seed, B)
    for a in (th, pr):
        a.setflags(write=False)
    positions = ps.positions(P)
    return Long(th, pr, positions, ps.genes_at(P, positions), [query_of(th, pr, q) for q in positions])


def long_cuts(r, stat):
    """The N of one query and statistic, on the reference alone: for each of LONG_NS the nearest clear
    cut at or below it; 1024 itself must be one."""
    desc = np.sort(values(r.per, stat))[::-1]
    out = []
    for n in LONG_NS:
        cuts = clear(desc, stat[0], 1, n)
        assert cuts.size, ("no clear cut up to", n, stat)
        out.append(int(cuts[-1]))
    assert out[-1] == FULL and FULL // 8 < out[0] <= LONG_NS[0], (stat, out)
    return tuple(out)


# ------------------------------------------------ every candidate tied, in every slot
TIE_SHAPE = (4, 60, 3)              # K, P, B
TIE_LEVELS = (0.5, 0.25, 0.75)      # slot s scores every triple exactly TIE_LEVELS[s]
TIE_NS = (8, 64, 256)


@functools.lru_cache(maxsize=None)
def tie_case():
    """Parameters in powers of two, so that every product and sum of a score is exact in any order:
    every membership 1/4 and slot s's rating-1 probability TIE_LEVELS[s] everywhere.  Every candidate
    of every query then has the same word in a slot, each statistic is one value for all of them, and
    a list is decided by the triple keys alone: the N smallest.  -> Long, as long_case returns it."""
    K, P, B = TIE_SHAPE
    th = np.full((B, P, K), 1.0 / K)
    pr = np.empty((B, K, K, K, 2))
    for s, level in enumerate(TIE_LEVELS):
        pr[s, ..., 1], pr[s, ..., 0] = level, 1.0 - level
    for a in (th, pr):
        a.setflags(write=False)
    positions = ps.positions(P)
    refs = [query_of(th, pr, q) for q in positions]
    for r in refs:
        for s, level in enumerate(TIE_LEVELS):
            assert (r.per[s] == level).all()        # exactly, in the reference as well
    return Long(th, pr, positions, ps.genes_at(P, positions), refs)
