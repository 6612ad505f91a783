"""numpy float64 reference of the vote scan (include/mmsbm.h mmsbm_scan_votes), for
tests/test_votes_host.py and tests/test_gpu_scan_votes.py: per slot the scores of
scan_ref.ref_scores, per triple the number of slots at or above the threshold, the histogram over
those votes, the hits and their ensemble scores (scan_ref.prefix_mean).  The thresholds come from
census_ref.gap_thresholds over the scores of ALL slots, so that no slot's score sits within the
project's 1e-7 gap of one.  No GPU, no product code beyond the rank order."""
import collections
import functools

import numpy as np

import census_ref
import scan_ref

Case = collections.namedtuple("Case", "theta pr per keys mean")


@functools.lru_cache(maxsize=None)
def case(K, P, seed, B):
    """scan_ref.random_params(K, P, seed, B) with its reference, read-only: theta [B][P][K], pr,
    per f64[B][C(P, 3)] (each slot's scores in key order), the packed keys and the ensemble mean of
    all B slots; computed once."""
    th, pr = scan_ref.random_params(K, P, seed, B)
    per, keys = [], None
    for b in range(B):
        s, keys = scan_ref.ref_scores(th[b], pr[b])
        per.append(s)
    per = np.stack(per) if per[0].size else np.zeros((B, 0))
    mean = scan_ref.prefix_mean(per, B)
    for a in (th, pr, per, keys, mean):
        a.setflags(write=False)
    return Case(th, pr, per, keys, mean)


def clear_thresholds(per, n=9):
    """Thresholds at midpoints of wide gaps of the slots' concatenated scores, ascending and unique
    (the first lies below every score, the last above every score), shown clear of every slot's
    scores by the project's gap."""
    flat = np.asarray(per).reshape(-1)
    t = np.unique(census_ref.gap_thresholds(flat, n))
    census_ref.assert_clear(flat, t)
    return t


def at_quantile(per, thresholds, q):
    """The clear threshold nearest the q-quantile of the concatenated scores."""
    target = np.quantile(np.asarray(per).reshape(-1), q)
    inner = thresholds[1:-1]
    return float(inner[np.argmin(np.abs(inner - target))])


def near_median(per, n=257):
    """The clear midpoint nearest the median of the concatenated scores."""
    return at_quantile(per, clear_thresholds(per, n), 0.5)


def ref_votes(per, keys, threshold, ns=None, known=None):
    """-> (votes int32 per eligible triple, those triples' keys, their ensemble scores, hist
    int64[ns + 1]) over the first ns slots (None: all), outside `known`."""
    per = np.asarray(per)
    ns = per.shape[0] if ns is None else ns
    votes = (per[:ns] >= threshold).sum(axis=0).astype(np.int32)
    mean = scan_ref.prefix_mean(per, ns)
    keep = np.ones(keys.size, dtype=bool) if known is None or not len(known) else ~np.isin(keys, known)
    votes, keys, mean = votes[keep], keys[keep], mean[keep]
    return votes, keys, mean, np.bincount(votes, minlength=ns + 1).astype(np.int64)


def ref_hits(votes, keys, mean, min_votes):
    """The rows with votes >= min_votes -> {key: (votes, ensemble score)}."""
    hit = votes >= min_votes
    return dict(zip(keys[hit].tolist(), zip(votes[hit].tolist(), mean[hit].tolist())))
