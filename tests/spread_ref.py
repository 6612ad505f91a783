"""numpy float64 reference of the dispute scan (include/mmsbm.h mmsbm_scan_spread_topn), for
tests/test_spread_host.py, tests/test_gpu_scan_spread.py and tests/test_gpu_spread_converged.py: per
slot the scores of votes_ref.case(K, P, seed, B).per, per triple the spread d_t = the (1 + t)-th
largest minus the (1 + t)-th smallest of them, ranked by scan_ref.top.  The cases are the quorum
scan's (tests/quorum_ref.py); only the kernel matrix has a seed table of its own.

Tolerance and precondition, derived and not measured.  A slot score is within scan_ref.RTOL (1e-9)
relative of the reference, and order statistics are 1-Lipschitz in the sup norm, so the two scores a
spread subtracts (hi and lo) are each within RTOL relative and the spread within RTOL (hi + lo)
ABSOLUTE: `atol` gives that bound per triple, compared with rtol = 0.  Scores are <= 1, so a spread
moves by at most 2 RTOL and two neighbours of a list by at most 4 RTOL = 4e-9 against each other:
the order inside the reference's top n + 1 is determined when every adjacent absolute gap exceeds
that.  SPREAD_GAP = 1e-8 is asserted on the reference alone (tests/test_spread_host.py).
No GPU, no product code beyond the rank order."""
import numpy as np

import quorum_ref
import scan_ref

RTOL = scan_ref.RTOL
SPREAD_GAP = 1e-8                                   # absolute; > 4 RTOL, see above
TARGET_TRIM = 3                                     # mmsbm_scan_spread_max_trim(): every legal trim for ns <= 9

CASES = quorum_ref.CASES
EXACT_CASES = quorum_ref.EXACT_CASES
NS = quorum_ref.NS
MATRIX_P, MATRIX_N = quorum_ref.MATRIX_P, quorum_ref.MATRIX_N
reference_cases = quorum_ref.reference_cases
exclusions = quorum_ref.exclusions
matrix_cases = quorum_ref.matrix_cases
case = quorum_ref.case

# Seeds other than quorum_ref's, chosen on the reference alone: with quorum_ref.MATRIX_SEEDS the case
# (K, B) = (19, 12) leaves an adjacent gap of 2.1e-9 in the top 65 at t = 0.
MATRIX_SEEDS = {**quorum_ref.MATRIX_SEEDS, (19, 12): 919}


def matrix_case(K, B):
    return case(K, MATRIX_P, MATRIX_SEEDS.get((K, B), 700 + K), B)


def legal(ns):
    """Every trim t >= 0 with ns - 2 t >= 2."""
    return list(range((ns - 2) // 2 + 1)) if ns >= 2 else []


def trims(ns, cap=TARGET_TRIM):
    """The legal trims a kernel with the cap `cap` takes at ns slots."""
    return [t for t in legal(ns) if t <= cap]


def ends(per, t, ns=None):
    """(hi, lo) per triple: the (1 + t)-th largest and the (1 + t)-th smallest of the first ns slots'
    scores (None: all)."""
    per = np.asarray(per)
    ns = per.shape[0] if ns is None else ns
    assert t >= 0 and ns - 2 * t >= 2, (t, ns)
    srt = np.sort(per[:ns], axis=0)
    return srt[ns - 1 - t], srt[t]


def spread(per, t, ns=None):
    """d_t per triple: one subtraction of two slot scores."""
    hi, lo = ends(per, t, ns)
    return hi - lo


def atol(per, t, ns=None):
    """The absolute bound on a spread's error per triple: RTOL (hi + lo)."""
    hi, lo = ends(per, t, ns)
    return RTOL * (hi + lo)


def min_abs_gap(top_scores):
    """The smallest adjacent absolute gap of a descending list (inf when it has no two entries)."""
    if top_scores.size < 2:
        return np.inf
    return float((top_scores[:-1] - top_scores[1:]).min())


def assert_gaps(top_scores):
    """The precondition, on the reference alone: the order inside the top n + 1 is determined."""
    gap = min_abs_gap(top_scores)
    assert gap > SPREAD_GAP, gap


def ref_top(per, keys, t, n, known=None, ns=None):
    """The reference's best n + 1 (spreads, keys) under d_t, its gaps asserted."""
    s, k = scan_ref.top(spread(per, t, ns), keys, n, known)
    assert_gaps(s)
    return s, k
