"""numpy reference of the screen scan's statistics (include/mmsbm.h mmsbm_screen_stat_topn /
mmsbm_screen_stat_scores), for tests/test_screen_stat_host.py and tests/test_gpu_screen_stat.py: given
the slots' own rows it forms the quorum score by a descending sort and the spread by the difference,
and a query's list by a lexsort.  No GPU, no product code."""
import numpy as np

import screen_ref
from scan_ref import keys_to_ids

MAX_DEPTH = 4       # mmsbm_screen_stat_max_depth()


def sorted_desc(rows):
    """Per-slot rows [ns][P] -> [ns][P], every column sorted descending (a NaN column stays NaN)."""
    rows = np.asarray(rows, dtype=np.float64)
    return -np.sort(-rows, axis=0)


def quorum(rows, m):
    """q_m: the m-th largest of the slots' scores, per place -> f64[P]; each value is one slot's word."""
    rows = np.asarray(rows, dtype=np.float64)
    assert 1 <= m <= rows.shape[0]
    return sorted_desc(rows)[m - 1]


def spread(rows, t):
    """d_t = q_{1+t} - q_{ns-t}, per place -> f64[P]: one subtraction of two slot scores."""
    rows = np.asarray(rows, dtype=np.float64)
    ns = rows.shape[0]
    assert t >= 0 and ns - 2 * t >= 2
    s = sorted_desc(rows)
    return s[t] - s[ns - 1 - t]


def quorum_depth(m, ns):
    return min(m, ns - m + 1)


def legal_votes(ns, cap=MAX_DEPTH):
    """Every m in [1, ns] whose depth is within the cap."""
    return [m for m in range(1, ns + 1) if quorum_depth(m, ns) <= cap]


def legal_trims(ns, cap=MAX_DEPTH):
    """Every t >= 0 with ns - 2 t >= 2 and t + 1 within the cap."""
    return [t for t in range(cap) if ns - 2 * t >= 2]


def top_list(row, P, x, y, n):
    """A statistic's row in rank positions (NaN: not eligible) -> (scores, ids) of the query's list:
    value descending, screen_ref.row_keys ascending, over the non-NaN places, the first n."""
    row = np.asarray(row, dtype=np.float64)
    at = np.flatnonzero(~np.isnan(row))
    keys = screen_ref.row_keys(P, x, y)[at]
    pick = np.lexsort((keys, -row[at]))[:n]
    return row[at][pick], keys_to_ids(keys[pick], P)
