"""numpy float64 reference of the partner scan (include/mmsbm.h mmsbm_partners_topn), for
tests/test_gpu_partners.py: for one query it forms the three P x P products Th' T^m Th'^T and picks
the region of every pair (b, c).  No GPU, no product code beyond the rank order."""
import numpy as np

from scan_ref import RTOL, keys_to_ids, min_gap, rank_tables, top


def ref_query(theta, pr, q):
    """Every candidate of the query at rank position q -> (scores, triple keys, pair keys), in pair
    order.  theta [P][K], pr [K][K][K][R] in the reference nesting."""
    P = theta.shape[0]
    order, _ = rank_tables(P)
    Th = np.asarray(theta, dtype=np.float64)[order]
    p1 = np.asarray(pr, dtype=np.float64)[..., 1]
    T1 = np.einsum("x,xyz->yz", Th[q], p1)      # q < b < c
    T2 = np.einsum("y,xyz->xz", Th[q], p1)      # b < q < c
    T3 = np.einsum("z,xyz->xy", Th[q], p1)      # b < c < q
    S1 = (Th @ T1) @ Th.T
    S2 = (Th @ T2) @ Th.T
    S3 = (Th @ T3) @ Th.T
    b, c = np.triu_indices(P, k=1)
    keep = (b != q) & (c != q)
    b, c = b[keep].astype(np.int64), c[keep].astype(np.int64)
    scores = np.where(b > q, S1[b, c], np.where(c > q, S2[b, c], S3[b, c]))
    tkeys = np.where(b > q, (q * P + b) * P + c, np.where(c > q, (b * P + q) * P + c, (b * P + c) * P + q))
    return scores, tkeys, b * P + c


def want_list(theta, pr, gene, n, known_pairs=None, scores=None):
    """(scores, ids, gap) of the gene's reference list: the best n outside known_pairs, and the
    smallest adjacent relative gap inside the best n + 1.  `scores` overrides the scorer's (an
    ensemble mean formed by the caller)."""
    P = theta.shape[0]
    _, rank = rank_tables(P)
    s, tk, pk = ref_query(theta, pr, int(rank[gene]))
    if scores is not None:
        s = scores
    if known_pairs is not None and len(known_pairs):
        keep = ~np.isin(pk, known_pairs)
        s, tk = s[keep], tk[keep]
    ts, tk = top(s, tk, n)
    return ts[:n], keys_to_ids(tk[:n], P), min_gap(ts)


def check_query(got, theta, pr, gene, n, known_pairs=None, scores=None):
    """One query's (scores, ids) against the reference: the precondition on the reference alone
    first, then the identical ordered id list and the scores within RTOL."""
    want_s, want_ids, gap = want_list(theta, pr, gene, n, known_pairs, scores)
    assert gap > 1e-9, (gene, gap)
    got_s, got_ids = got
    assert got_ids.dtype == np.int32 and got_s.dtype == np.float64
    assert got_ids.shape == want_ids.shape, (gene, got_ids.shape, want_ids.shape)
    np.testing.assert_array_equal(got_ids, want_ids, err_msg="gene %d" % gene)
    np.testing.assert_allclose(got_s, want_s, rtol=RTOL, atol=0)
    if known_pairs is not None and len(known_pairs):
        _, rank = rank_tables(theta.shape[0])
        pos = np.sort(rank[got_ids.astype(np.int64)], axis=1)
        q = int(rank[gene])
        P = theta.shape[0]
        others = np.array([[x for x in row if x != q] for row in pos.tolist()], dtype=np.int64).reshape(-1, 2)
        assert not np.isin(others[:, 0] * P + others[:, 1], known_pairs).any()
    return gap

