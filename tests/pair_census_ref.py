"""numpy reference of the pair census (include/mmsbm.h mmsbm_pair_census), for
tests/test_pair_census_host.py and tests/test_gpu_pair_census.py.  It builds on
scan_ref.ref_scores: every eligible score at or above a threshold is scattered to its three pairs
with np.add.at.  Counts are integers: every comparison is equality.  No GPU, no product code beyond
the rank order."""
import numpy as np

from scan_ref import rank_tables


def ref_pairs_rank(scores, keys, P, thresholds, known=None):
    """-> int32 [P][P][M] in rank positions, x < y filled: the eligible scores >= thresholds[m]
    (keys not in `known`) of the triples that contain positions x and y."""
    t = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    out = np.zeros((P, P, t.size), dtype=np.int32)
    scores, keys = np.asarray(scores), np.asarray(keys, dtype=np.int64)
    if known is not None and len(known):
        keep = ~np.isin(keys, known)
        scores, keys = scores[keep], keys[keep]
    a, b, c = keys // (P * P), (keys // P) % P, keys % P
    for m, thr in enumerate(t):
        hit = scores >= thr
        for x, y in ((a, b), (a, c), (b, c)):
            np.add.at(out[:, :, m], (x[hit], y[hit]), 1)
    return out


def to_gene_ids(rank_mat):
    """A rank-position matrix [P][P][...] filled for x < y -> the symmetric matrix in gene ids."""
    P = rank_mat.shape[0]
    _, rank = rank_tables(P) if P else (None, np.zeros(0, np.int64))
    sym = rank_mat + np.swapaxes(rank_mat, 0, 1)
    return sym[rank][:, rank]


def ref_pairs(scores, keys, P, thresholds, known=None):
    """-> (rank-position matrix, gene-id matrix), both int32 [P][P][M]."""
    r = ref_pairs_rank(scores, keys, P, thresholds, known)
    return r, to_gene_ids(r)


def ref_gene_counts(scores, keys, P, thresholds, known=None):
    """-> int64 [P][M] in gene ids: the eligible scores >= each threshold of the triples that
    contain each gene, counted directly (no pair matrix)."""
    t = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    scores, keys = np.asarray(scores), np.asarray(keys, dtype=np.int64)
    if known is not None and len(known):
        keep = ~np.isin(keys, known)
        scores, keys = scores[keep], keys[keep]
    order, _ = rank_tables(P)
    out = np.zeros((P, t.size), dtype=np.int64)
    for m, thr in enumerate(t):
        k = keys[scores >= thr]
        for pos in (k // (P * P), (k // P) % P, k % P):
            np.add.at(out[:, m], order[pos], 1)
    return out


def eligible_brute(P, known=None):
    """pair_eligible by a loop over every triple: int32 [P][P] in gene ids."""
    order, _ = rank_tables(P)
    known = set() if known is None else set(int(k) for k in known)
    out = np.zeros((P, P), dtype=np.int32)
    for a in range(P):
        for b in range(a + 1, P):
            for c in range(b + 1, P):
                if (a * P + b) * P + c in known:
                    continue
                for x, y in ((a, b), (a, c), (b, c)):
                    out[order[x], order[y]] += 1
                    out[order[y], order[x]] += 1
    return out


def top_pairs(rank_mat, n):
    """pairs_top's order from a rank-position count matrix [P][P]: -> (counts int64[n'], gene ids
    int32[n'][2] in key order) by count descending, then the key x P + y ascending."""
    P = rank_mat.shape[0]
    x, y = np.triu_indices(P, k=1)
    cnt = rank_mat[x, y].astype(np.int64)
    idx = np.lexsort((x * P + y, -cnt))[:n]
    order, _ = rank_tables(P)
    return cnt[idx], np.stack([order[x[idx]], order[y[idx]]], axis=1).astype(np.int32).reshape(-1, 2)
