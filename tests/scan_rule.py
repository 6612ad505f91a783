"""The row-block rule of the scan families (csrc/scan_host.h pick_wb) in Python, for
tests/test_scan_rule_host.py (which holds it against the C++) and tests/test_gpu_scan_matrix.py
(which takes from it the width each case is meant to hit).  No GPU, no product code."""

KIB = 1024
CENSUS_LIKE = (1, 64 * KIB)    # scan, census, pair census, threshold scan: one W row per row b
PARTNERS = (2, 96 * KIB)       # the partner scan: a U and an L row per row b
MAX_K = 32


def row_block_width(K, ns, rows_per_b, limit):
    """The widest row block WB in (4, 2, 1) whose W rows fit `limit` bytes of LDS: WB b-tiles of 16
    rows, rows_per_b W rows per row b, 4 ceil(K / 4) + 2 doubles per W row, ns samples.  0: the
    ensemble does not fit at WB = 1 and the call is refused (MMSBM_ERR_UNSUPPORTED)."""
    kp = (K + 3) // 4 * 4
    row_block = 8 * rows_per_b * ns * 16 * (kp + 2)
    for wb in (4, 2, 1):
        if row_block * wb <= limit:
            return wb
    return 0


def width(K, ns, family=CENSUS_LIKE):
    return row_block_width(K, ns, *family)


def last_supported(K, family=CENSUS_LIKE):
    """The largest ensemble the family takes at this K."""
    ns = 1
    while width(K, ns + 1, family):
        ns += 1
    return ns
