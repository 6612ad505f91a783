"""numpy float64 reference of the score census (include/mmsbm.h mmsbm_scan_census), for
tests/test_census_host.py and tests/test_gpu_census.py, over the scores of scan_ref.ref_scores: the
counts at or above each threshold, and the precondition that keeps a threshold away from every
score.  No GPU, no product code."""
import numpy as np

GAP = 1e-7   # a threshold must be further than this, relatively, from every reference score


def eligible(scores, keys, known=None):
    """The scores of the triples whose key is not in `known`, sorted ascending."""
    if known is not None and len(known):
        scores = scores[~np.isin(keys, known)]
    return np.sort(scores)


def ref_census(scores, keys, thresholds, known=None):
    """-> (counts int64[len(thresholds)] of eligible scores >= each threshold, total)."""
    s = eligible(scores, keys, known)
    t = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    return (s.size - np.searchsorted(s, t, side="left")).astype(np.int64), int(s.size)


def clear_of_scores(scores, thresholds):
    """bool per threshold: it is more than GAP relative from EVERY reference score (excluded ones
    too: the stricter test), so an error of RTOL in a score cannot move it across."""
    s = np.sort(np.asarray(scores, dtype=np.float64))
    t = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    if not s.size:
        return np.ones(t.size, dtype=bool)
    at = np.searchsorted(s, t)
    lo, hi = s[np.clip(at - 1, 0, s.size - 1)], s[np.clip(at, 0, s.size - 1)]
    return (np.abs(t - lo) > GAP * np.abs(lo)) & (np.abs(t - hi) > GAP * np.abs(hi))


def assert_clear(scores, thresholds):
    """The precondition of every threshold test, on the reference alone."""
    ok = clear_of_scores(scores, thresholds)
    assert ok.all(), np.asarray(thresholds)[~ok]


def gap_thresholds(scores, n, seed=0):
    """Up to n thresholds at midpoints of gaps of the sorted distinct scores that are wide enough
    for the precondition, spread over the whole range and including two ADJACENT gaps; plus one
    below the minimum, one above the maximum and one duplicate.  Unsorted on purpose."""
    s = np.unique(np.asarray(scores, dtype=np.float64))
    mid = (s[:-1] + s[1:]) / 2
    wide = np.flatnonzero((s[1:] - s[:-1]) > 4 * GAP * np.abs(s[1:]))
    pick = wide[np.linspace(0, wide.size - 1, min(n, wide.size)).astype(int)] if wide.size else wide
    both = np.flatnonzero(np.diff(wide) == 1)          # wide[i], wide[i] + 1: neighbours
    if both.size:
        j = both[both.size // 2]
        pick = np.concatenate([pick, wide[j:j + 2]])
    t = mid[np.unique(pick)]
    t = np.concatenate([t, [s[0] * (1 - 1e-3), s[-1] * (1 + 1e-3)], t[:1]])
    return np.random.default_rng(seed).permutation(t)
