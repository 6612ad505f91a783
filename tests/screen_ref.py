"""numpy float64 reference of the screen scan (include/mmsbm.h mmsbm_screen_topn / mmsbm_screen_scores),
for tests/test_screen_host.py, tests/test_gpu_screen.py and tests/test_gpu_screen_wide.py (whose designed
rows and shapes are at the end): for one query pair it forms the three
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


# ------------------------------------------------------------------ designed rows
# Random parameters do not determine an order at large N (a row of P scores in (0, 1) holds gaps
# below 1e-9 once N reaches the hundreds), so the tests of rows longer than the candidate buffer
# (tests/test_gpu_screen_wide.py) build their rows: K = 2, theta of the gene at rank position c is
# (t_c, 1 - t_c) with t on an evenly spaced grid, and p_1[i][j][k] = 0.15 + 0.1 [i = 0] + 0.2 [j = 0]
# + 0.3 [k = 0] + u, |u| <= 0.02.  A score is multilinear in (t_a, t_b, t_c), so within one region of
# a query it is affine in t_c, with a slope of 0.1, 0.2 or 0.3 (each within 0.04): the order of a
# region's scores is the order of its t, adjacent gaps are about 1 / P, and the three regions differ
# in slope and offset.  `order` lays the grid over c and so chooses the arrival order.
ORDERS = ("ascending", "descending", "shuffled", "sawtooth")
ROUND = 256     # positions one round of the select kernel's workgroup reads


# the shapes of tests/test_gpu_screen_wide.py, here so that tests/test_screen_host.py checks their
# preconditions without a GPU
WIDE_P = 1100                                   # arrival orders: every order at every N
WIDE_NS = (255, 256, 257, 512, 513, 1024)       # the tight fit N = 256 / cap = 512 and every growth step of cap
OVERFLOW_P, OVERFLOW_ORDERS = 2100, ("ascending", "shuffled")    # N = 1024, cap = 2048, B = 2
STRIDE_P = 262144 + 33                          # the score kernel's second c-tile per wave
LATE = [(1100, 8), (1100, 255), (1100, 256), (2100, 257), (2100, 512), (2600, 1024)]    # (P, N) of the order "late:N"
DESIGNED = [(WIDE_P, N, order, 1) for order in ORDERS for N in WIDE_NS] + \
    [(OVERFLOW_P, 1024, order, 2) for order in OVERFLOW_ORDERS] + \
    [(P, N, "late:%d" % N, 1) for P, N in LATE]                     # (P, N, order, B)
F_QUERY = (211, 402)                            # the independence test's query (rank positions)
G_CASE = (10, 600, 8, 5)                        # (K, P, B, seed) of the realistic width


def cap_of(n):
    """The select kernel's candidate buffer for lists of n: 512 entries, doubled until it holds 2 n."""
    cap = 512
    while cap < 2 * n:
        cap <<= 1
    return cap


def designed_places(P, order, seed=0):
    """place[c]: the index on the grid of t of rank position c, a permutation of 0..P-1.
    ascending / descending in c; shuffled; sawtooth: every ROUND consecutive positions rise from the
    bottom of the grid to its top; "late:N": see below."""
    c = np.arange(P, dtype=np.int64)
    if order == "ascending":
        return c
    if order == "descending":
        return P - 1 - c
    if order == "shuffled":
        return np.random.default_rng(seed).permutation(P).astype(np.int64)
    if order.startswith("late:"):
        # descending, but the N-th best third of the query (0, 1) comes last: it is judged against the
        # threshold of the keep-best before it, between that buffer's (N - 1)-th and N-th entries, and
        # nothing after it can push a wrongly kept N-th out of the list
        n = int(order[5:])
        assert 1 <= n < P - 2
        late = P - 2 - n        # positions 0 and 1 hold the two best places, the query's own
        return np.concatenate([np.arange(P - 1, late, -1), np.arange(late - 1, -1, -1), [late]]).astype(np.int64)
    assert order == "sawtooth", order
    rounds = (P + ROUND - 1) // ROUND
    return np.argsort(np.argsort((c % ROUND) * rounds + c // ROUND))


def designed_params(P, order, B=1, seed=0):
    """-> (theta [B][P][2] by gene id, pr [B][2][2][2][2], place).  Slot b has its own grid
    [0.1 + 0.05 b, 0.9 - 0.05 b] over the same places and its own u, so the ensemble mean is affine in
    the place within a region too."""
    tab, _ = rank_tables(P)
    place = designed_places(P, order, seed)
    i, j, k = np.meshgrid(np.arange(2), np.arange(2), np.arange(2), indexing="ij")
    th = np.empty((B, P, 2))
    pr = np.empty((B, 2, 2, 2, 2))
    for b in range(B):
        lo, hi = 0.1 + 0.05 * b, 0.9 - 0.05 * b
        t = lo + (hi - lo) * place / max(P - 1, 1)
        th[b, tab, 0] = t       # rank position c is gene tab[c]
        th[b, tab, 1] = 1.0 - t
        u = np.random.default_rng(1000 + 7 * seed + b).uniform(-0.02, 0.02, (2, 2, 2))
        pr[b, ..., 1] = 0.15 + 0.1 * (i == 0) + 0.2 * (j == 0) + 0.3 * (k == 0) + u
        pr[b, ..., 0] = 1.0 - pr[b, ..., 1]
    return th, pr, place


def regions(P, x, y):
    """The three index ranges of c around a query: c < x, x < c < y, y < c."""
    return [np.arange(0, x), np.arange(x + 1, y), np.arange(y + 1, P)]


def check_designed(row, place, P, x, y):
    """On the reference alone: within each region the row's order is the order of the places."""
    for c in regions(P, x, y):
        if c.size:
            np.testing.assert_array_equal(np.argsort(row[c], kind="stable"), np.argsort(place[c], kind="stable"))


def three_queries(P):
    """Rank positions with only the last region, only the first, and all three populated."""
    return [(0, 1), (P - 2, P - 1), (P // 3, 2 * P // 3 + 1)]


def check_row(got, row, ok):
    """A screen_scores row in RANK positions against the reference: NaN exactly at the ineligible
    places, elsewhere within RTOL."""
    np.testing.assert_array_equal(np.isnan(got), ~ok)
    np.testing.assert_allclose(got[ok], row[ok], rtol=RTOL, atol=0)
