"""numpy reference of the pair vote census (include/mmsbm.h mmsbm_pair_votes), for
tests/test_pair_votes_host.py and tests/test_gpu_pair_votes.py.  It joins votes_ref.ref_votes (per
eligible triple, the number of slots at or above the threshold) with pair_census_ref's scatter: per
vote level, every triple with at least that many votes goes to its three pairs with np.add.at.
Counts are integers: every comparison is equality.  The thresholds come from
votes_ref.clear_thresholds over the scores of ALL slots.  No GPU, no product code beyond the rank
order."""
import numpy as np

import pair_census_ref
import votes_ref


def ref_rank(per, keys, P, threshold, levels, ns=None, known=None):
    """-> int32 [P][P][M] in rank positions, x < y filled: the eligible triples (keys not in
    `known`) that contain positions x and y and that at least levels[m] of the first ns slots (None:
    all) score >= threshold.  The levels may come in any order."""
    votes, kept, _, _ = votes_ref.ref_votes(per, keys, threshold, ns, known)
    # votes as the scores and the levels as the thresholds: `votes >= level` is the scatter's test
    return pair_census_ref.ref_pairs_rank(votes.astype(np.float64), kept, P, np.asarray(levels, dtype=np.float64))


def ref_pairs(per, keys, P, threshold, levels, ns=None, known=None):
    """-> (rank-position matrix, gene-id matrix), both int32 [P][P][M]."""
    r = ref_rank(per, keys, P, threshold, levels, ns, known)
    return r, pair_census_ref.to_gene_ids(r)


def hist_tail(per, keys, threshold, levels, ns=None, known=None):
    """-> int64 [M]: the eligible triples with at least levels[m] votes, from the vote histogram."""
    hist = votes_ref.ref_votes(per, keys, threshold, ns, known)[3]
    return np.array([hist[int(v):].sum() for v in levels], dtype=np.int64)


def upper_sums(mat):
    """The sums over x < y of a [P][P][M] matrix -> int64 [M]."""
    P = mat.shape[0]
    return mat[np.triu(np.ones((P, P), dtype=bool), k=1)].sum(axis=0, dtype=np.int64)


def two_thresholds(per, n=257, high=0.999):
    """(near the median, near the `high` quantile) of the slots' concatenated scores, both from
    votes_ref.clear_thresholds: clear of every slot's scores by the project's gap.  At the first
    nearly every tile has hits and the level walk runs; at the second nearly every tile leaves at
    the first ballot."""
    t = votes_ref.clear_thresholds(per, n)
    return votes_ref.at_quantile(per, t, 0.5), votes_ref.at_quantile(per, t, high)
