"""numpy float64 reference of the quorum scan (include/mmsbm.h mmsbm_scan_quorum_topn), for
tests/test_quorum_host.py and tests/test_gpu_scan_quorum.py: per slot the scores of
votes_ref.case(K, P, seed, B).per, per triple the m-th largest of them, ranked by scan_ref.top.
Order statistics are 1-Lipschitz in the sup norm: a slot error of scan_ref.RTOL moves q_m by at most
RTOL, so the scan's tolerance and its gap precondition (scan_ref.assert_gaps) carry over unchanged.
No GPU, no product code beyond the rank order."""
import numpy as np

import scan_ref
import votes_ref

CASES = [(3, 37, 3, 11), (10, 50, 8, 5), (5, 33, 2, 3), (13, 40, 4, 7)]     # (K, P, B, seed): the vote scan's
OTHER_P = (20, 53)
EXACT_CASES = [(10, 53, 4, 21), (3, 211, 3, 11)]    # product against product; P = 211: the seeding pass
NS = (1, 5, 64)                                     # the N checked against the reference
TARGET_DEPTH = 4                                    # the depth the family aims at: every m for ns <= 8


MATRIX_P, MATRIX_N = 70, 64
MATRIX_K = (3, 7, 10, 13, 19, 22, 27, 30)           # KS = ceil(K / 4) = 1..8
MATRIX_SLOTS = 8                                    # the fewest slots with depth 4 in both directions


def matrix_slots(K, WB):
    """The ensemble the kernel matrix runs at row-block width WB: the largest of at most
    MATRIX_SLOTS slots with that width (scan_rule.width), else the smallest beyond."""
    import scan_rule
    fit = [ns for ns in range(2, MATRIX_SLOTS + 1) if scan_rule.width(K, ns) == WB]
    if fit:
        return fit[-1]
    ns = MATRIX_SLOTS + 1
    while scan_rule.width(K, ns) != WB:
        assert scan_rule.width(K, ns) > 0, (K, WB)
        ns += 1
    return ns


def matrix_cases():
    """(K, B, WB) of the kernel matrix, and its (K, P, B, seed) for votes_ref.case."""
    return [(K, matrix_slots(K, WB), WB) for K in MATRIX_K for WB in (4, 2, 1)]


# Seeds other than 700 + K, chosen on the reference alone: at these K the scores crowd, and the first
# seed left an adjacent gap of the top 65 below 2e-8 (tests/test_quorum_host.py asserts that bound).
MATRIX_SEEDS = {(10, 19): 910, (19, 12): 819, (27, 4): 827, (27, 8): 827, (30, 3): 830, (30, 7): 930, (30, 8): 930}
MATRIX_GAP = 2e-8


def matrix_case(K, B):
    return case(K, MATRIX_P, MATRIX_SEEDS.get((K, B), 700 + K), B)


def reference_cases():
    """Every (K, P, B, seed) the GPU tests hold against the reference."""
    return CASES + [(K, P, B, seed) for K, _, B, seed in CASES for P in OTHER_P]


def depth(m, ns):
    """The sorted-list depth of the m-th largest of ns: the shorter of the two lists."""
    assert 1 <= m <= ns
    return min(m, ns - m + 1)


def supported(ns, cap):
    """The min_votes a kernel of depth cap `cap` takes at ns slots."""
    return [m for m in range(1, ns + 1) if depth(m, ns) <= cap]


def quorum(per, m, ns=None):
    """q_m per triple: the m-th largest of the first ns slots' scores (None: all)."""
    per = np.asarray(per)
    ns = per.shape[0] if ns is None else ns
    return np.sort(per[:ns], axis=0)[ns - m]


def exclusions(keys, P):
    """No exclusion, every 9th key from the second on, every key with a = 3."""
    return [None, keys[1::9].copy(), keys[keys // (P * P) == 3].copy()]


def ref_top(per, keys, m, n, known=None, ns=None):
    """The reference's best n + 1 (scores, keys) under q_m, its gaps asserted."""
    s, k = scan_ref.top(quorum(per, m, ns), keys, n, known)
    scan_ref.assert_gaps(s)
    return s, k


def case(K, P, seed, B):
    return votes_ref.case(K, P, seed, B)
