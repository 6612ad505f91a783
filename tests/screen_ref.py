"""numpy float64 reference of the screen scan (include/mmsbm.h mmsbm_screen_topn / mmsbm_screen_scores),
for tests/test_screen_host.py and tests/test_gpu_screen.py: for one query pair it forms the three
vectors v1, v2, v3 by einsum and scores every third position with the vector of its region.  No GPU,
no product code beyond the rank order."""
import numpy as np

from scan_ref import RTOL, keys_to_ids, min_gap, prefix_mean, rank_tables, top


def positions(P, pair):
    """A query pair of gene ids -> its rank positions x < y."""
    _, rank = rank_tables(P)
    a, b = int(rank[pair[0]]), int(rank[pair[1]])
    assert a != b
    return min(a, b), max(a, b)


def ref_row(theta, pr, x, y):
    """The score of {x, y, c} for every rank position c -> f64[P] (the entries at x and y are
    NaN).  theta [P][K], pr [K][K][K][R] in the reference nesting."""
    P = theta.shape[0]
    order, _ = rank_tables(P)
    Th = np.asarray(theta, dtype=np.float64)[order]
    p1 = np.asarray(pr, dtype=np.float64)[..., 1]
    v1 = np.einsum("ijk,j,k->i", p1, Th[x], Th[y])      # c < x
    v2 = np.einsum("ijk,i,k->j", p1, Th[x], Th[y])      # x < c < y
    v3 = np.einsum("ijk,i,j->k", p1, Th[x], Th[y])      # y < c
    c = np.arange(P)
    row = np.where(c < x, Th @ v1, np.where(c < y, Th @ v2, Th @ v3))
    row[[x, y]] = np.nan
    return row


def row_keys(P, x, y):
    """The packed key of {x, y, c} sorted, for every c -> int64[P] (meaningless at x and y)."""
    c = np.arange(P, dtype=np.int64)
    return np.where(c < x, (c * P + x) * P + y, np.where(c < y, (x * P + c) * P + y, (x * P + y) * P + c))


def ref_rows(thetas, prs, x, y, sample=None):
    """The row of one slot, or (sample None) the ensemble mean of thetas [B][P][K], prs, formed by
    scan_ref.prefix_mean."""
    if sample is not None:
        return ref_row(thetas[sample], prs[sample], x, y)
    per = [ref_row(thetas[b], prs[b], x, y) for b in range(len(thetas))]
    return prefix_mean(per, len(per))


def eligible(P, x, y, thirds=None, mask=None):
    """bool[P]: which positions c the query (x, y) may list: not x or y, not among `thirds`, and with
    a mask none of (x, y), (x, c), (y, c) blocked (read at the smaller position's row only)."""
    ok = np.ones(P, dtype=bool)
    ok[[x, y]] = False
    if thirds is not None and len(thirds):
        t = np.asarray(thirds, dtype=np.int64)
        ok[t[(t >= 0) & (t < P)]] = False
    if mask is not None:
        def bit(a, b):
            a, b = np.minimum(a, b), np.maximum(a, b)
            return ((mask[a, b >> 5] >> (b & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)
        c = np.arange(P)
        others = c[(c != x) & (c != y)]
        if bit(np.array([x]), np.array([y]))[0]:
            ok[:] = False
        ok[others] &= ~(bit(np.full(others.size, x), others) | bit(np.full(others.size, y), others))
    return ok


def want_list(row, P, x, y, n, ok=None):
    """(scores, ids, gap) of a query's reference list from its reference row: the best n among the
    eligible positions under (score descending, key ascending), and the smallest adjacent relative
    gap inside the best n + 1."""
    ok = eligible(P, x, y) if ok is None else ok
    ts, tk = top(row[ok], row_keys(P, x, y)[ok], n)
    return ts[:n], keys_to_ids(tk[:n], P), min_gap(ts)


def check_list(got, row, P, x, y, n, ok=None):
    """One query's (scores, ids) against the reference row: the precondition on the reference alone
    first, then the identical ordered id list and the scores within RTOL."""
    want_s, want_ids, gap = want_list(row, P, x, y, n, ok)
    assert gap > 1e-9, ((x, y), gap)
    got_s, got_ids = got
    assert got_ids.dtype == np.int32 and got_s.dtype == np.float64
    assert got_ids.shape == want_ids.shape, ((x, y), got_ids.shape, want_ids.shape)
    np.testing.assert_array_equal(got_ids, want_ids, err_msg="query %d %d" % (x, y))
    np.testing.assert_allclose(got_s, want_s, rtol=RTOL, atol=0)
    return gap


def check_row(got, row, ok):
    """A screen_scores row in RANK positions against the reference: NaN exactly at the ineligible
    places, elsewhere within RTOL."""
    np.testing.assert_array_equal(np.isnan(got), ~ok)
    np.testing.assert_allclose(got[ok], row[ok], rtol=RTOL, atol=0)
