"""numpy reference of the partner scan's statistics (include/mmsbm.h mmsbm_partners_stat_topn), for
tests/test_partners_stat_host.py and tests/test_gpu_partners_stat.py: given every slot's score of a
query's candidates it forms the quorum score and the spread (tests/screen_stat_ref.py) and the
query's list by a lexsort over the triple keys.  The per-slot scores come either from
partners_ref.ref_query (the independent reference) or from the slots' own complete lists.
No GPU, no product code beyond the rank order."""
import numpy as np

import partners_ref
import scan_ref
import screen_stat_ref
import spread_ref
from scan_ref import keys_to_ids

MAX_DEPTH = 4       # mmsbm_partners_stat_max_depth()
legal_votes, legal_trims = screen_stat_ref.legal_votes, screen_stat_ref.legal_trims

REF_CASES = [(3, 37, 3, 11), (10, 50, 8, 6), (5, 33, 2, 3), (13, 40, 4, 7), (7, 100, 5, 9)]     # (K, P, B, seed)
REF_NS = (1, 5, 64)
QUORUM_GAP = 1e-9                       # relative: partners_ref.check_query's
SPREAD_GAP = spread_ref.SPREAD_GAP      # absolute


def positions(P):
    """Rank positions of the queries: the first tile, a tile edge from both sides, the middle, and
    the last, ragged tile."""
    return sorted({q for q in (0, 15, 16, 17, P // 2, P - 2, P - 1) if 0 <= q < P})


def genes_at(P, pos):
    order, _ = scan_ref.rank_tables(P)
    return [int(order[q]) for q in pos]


def stat_calls(ns):
    """Every legal (name, argument) within the caps."""
    return [("quorum", m) for m in legal_votes(ns)] + [("spread", t) for t in legal_trims(ns)]


def stat(per, what, arg):
    """per f64[ns][n] -> the statistic per candidate, f64[n]."""
    return screen_stat_ref.quorum(per, arg) if what == "quorum" else screen_stat_ref.spread(per, arg)


def ref_slots(thetas, prs, q):
    """The independent reference: (per f64[ns][n], triple keys, pair keys) of the query at rank
    position q, one partners_ref.ref_query per slot."""
    rows = [partners_ref.ref_query(th, pr, q) for th, pr in zip(thetas, prs)]
    return np.stack([r[0] for r in rows]), rows[0][1], rows[0][2]


def top_list(values, tkeys, P, n, keep=None, order_by=None):
    """(values, ids) of the query's list: value descending, triple key ascending, over the
    candidates `keep` (None: all), the first n.  order_by: the values that rank, when `values` are
    another quantity of the same candidates (a per-candidate tolerance)."""
    values, tkeys = np.asarray(values, dtype=np.float64), np.asarray(tkeys, dtype=np.int64)
    by = values if order_by is None else np.asarray(order_by, dtype=np.float64)
    if keep is not None:
        values, tkeys, by = values[keep], tkeys[keep], by[keep]
    pick = np.lexsort((tkeys, -by))[:n]
    return values[pick], keys_to_ids(tkeys[pick], P)


def gap_ok(values, what, n):
    """The precondition on the reference alone: the order inside the top n + 1 is determined
    (relative gap for the quorum score, absolute for the spread) -> (ok, the smallest gap)."""
    s = -np.sort(-np.asarray(values, dtype=np.float64))[:n + 1]
    if what == "quorum":
        gap = scan_ref.min_gap(s)
        return gap > QUORUM_GAP, gap
    gap = spread_ref.min_abs_gap(s)
    return gap > SPREAD_GAP, gap


def from_slot_lists(lists, P):
    """The slots' own complete lists [(scores, ids)] of one query (every eligible candidate listed)
    -> (per f64[ns][n] of the listed words, triple keys ascending)."""
    keys0 = None
    per = []
    for scores, ids in lists:
        keys = scan_ref.packed(ids, P)
        at = np.argsort(keys)
        if keys0 is None:
            keys0 = keys[at]
        assert keys[at].tolist() == keys0.tolist()      # every slot lists the same candidates
        per.append(np.asarray(scores, dtype=np.float64)[at])
    return np.stack(per), keys0
