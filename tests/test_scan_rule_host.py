"""The row-block rule of the scan families (csrc/scan_host.h pick_wb) pinned on the CPU: a small
host program (tests/scan_host_check.cpp) prints what pick_wb returns for every K in 1..32 and every
ensemble size in 1..64, for the census-like families' constants and the partner scan's, and the
Python mirror (tests/scan_rule.py) must equal it on all 32 x 64 x 2 entries.  The GPU tests take the
width of every case from the mirror, so a retuned rule makes them fail loudly instead of testing
another layout.  The program includes HIP headers, so hipcc builds it; it makes no HIP call."""
import os
import subprocess

import pytest

import scan_rule

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)


def find_hipcc():
    """The compiler the package builds with (build.hipcc), or None."""
    from trigenicinteractionpredictor_amd import build
    try:
        return build.hipcc()
    except RuntimeError:
        return None


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    hipcc = find_hipcc()
    if hipcc is None:
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("scan_rule") / "scan_host_check")
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17",
                    "-I", os.path.join(REPO, "include"), "-o", exe, os.path.join(HERE, "scan_host_check.cpp")],
                   check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-500:] + res.stderr[-500:]
    rows = [tuple(int(v) for v in ln.split()) for ln in res.stdout.splitlines()]
    return {(r[0], r[1], r[2], r[3]): (r[4], r[5]) for r in rows}


def test_mirror_equals_pick_wb_everywhere(table):
    assert len(table) == 2 * 32 * 64
    for family in (scan_rule.CENSUS_LIKE, scan_rule.PARTNERS):
        rows_per_b, limit = family
        for K in range(1, 33):
            for ns in range(1, 65):
                wb, w_bytes = table[(rows_per_b, limit, K, ns)]
                assert scan_rule.row_block_width(K, ns, rows_per_b, limit) == wb, (family, K, ns, wb)
                assert wb in (0, 1, 2, 4)
                row_block = 8 * rows_per_b * ns * 16 * ((K + 3) // 4 * 4 + 2)
                if wb:
                    assert w_bytes == row_block * wb <= limit
                    assert wb == 4 or row_block * 2 * wb > limit        # the widest that fits
                else:
                    assert row_block > limit


def starts(K, family):
    """The smallest ns of each width 4, 2, 1 and of the refusal."""
    w = [scan_rule.width(K, ns, family) for ns in range(1, 65)]
    return tuple(1 + w.index(v) for v in (4, 2, 1, 0))


def test_documented_boundaries():
    """The rule in the words of include/mmsbm.h: refused when n_active (4 ceil(K / 4) + 2) exceeds
    512 (the scan, the censuses, the threshold scan) or 384 (the partner scan)."""
    assert scan_rule.CENSUS_LIKE == (1, 64 * 1024) and scan_rule.PARTNERS == (2, 96 * 1024)
    assert starts(10, scan_rule.CENSUS_LIKE) == (1, 10, 19, 37)
    assert starts(10, scan_rule.PARTNERS) == (1, 7, 14, 28)
    assert starts(30, scan_rule.CENSUS_LIKE) == (1, 4, 8, 16)
    assert starts(30, scan_rule.PARTNERS) == (1, 3, 6, 12)
    for K in range(1, 33):
        kp2 = (K + 3) // 4 * 4 + 2
        for ns in range(1, 65):
            assert (scan_rule.width(K, ns, scan_rule.CENSUS_LIKE) == 0) == (ns * kp2 > 512)
            assert (scan_rule.width(K, ns, scan_rule.PARTNERS) == 0) == (ns * kp2 > 384)
            assert scan_rule.width(K, 1, scan_rule.PARTNERS) == 4       # a single sample is never narrowed
    assert scan_rule.last_supported(10) == 36 and scan_rule.last_supported(32) == 15
    assert scan_rule.last_supported(10, scan_rule.PARTNERS) == 27
    assert scan_rule.last_supported(32, scan_rule.PARTNERS) == 11
