"""The plan of the three top-N scans (csrc/scan_topn.h make_plan, workspace_bytes) pinned on the CPU:
a small host program (tests/scan_topn_check.cpp, both mmsbm_detail_* functions stubbed, the number
of compute units settable) prints the plan of every shape and N of a table, and the layout restated
here, independently of the header, must equal it on every row: 256 bytes for the published bound,
then thT, T, the two candidate arrays and the two levels of lists, each part aligned to 256; a
candidate buffer of 512 entries doubled to >= 2 N; 4 / 2 / 1 workgroups per compute unit at
N <= 1024 / <= 2048 / above, no more than P P16 / 16 and at least 1; ceil(G / 32) lists on level 1.
The program includes HIP headers, so hipcc builds it; it makes no HIP call."""
import itertools
import os
import subprocess

import pytest

from test_scan_rule_host import find_hipcc

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)

KS, BS = (1, 10, 32), (1, 8)
PS = (0, 2, 3, 16, 17, 199, 200, 1500, 2000000)
NS = (1, 256, 257, 1024, 1025, 2048, 2049, 4096)
NCUS = (32, 64, 256)
WHATS = ("scan", "the quorum scan", "the dispute scan")
INVALID, UNSUPPORTED = -1, -4               # include/mmsbm.h


def align256(x):
    return (x + 255) // 256 * 256


def layout(K, B, P, N, ncu):
    """-> (cap, G, G2, total, [thT, T, cs, ck, ls0, lk0, ln0, ls1, lk1, ln1]) in bytes."""
    KP, P16 = (K + 3) // 4 * 4, max(16, (P + 15) // 16 * 16)
    cap = 512
    while cap < 2 * N:
        cap *= 2
    per_cu = 4 if N <= 1024 else 2 if N <= 2048 else 1
    G = max(1, min(per_cu * ncu, P * (P16 // 16)))
    G2 = -(-G // 32)
    parts = [8 * B * KP * P16, 8 * B * P * K * KP, 8 * G * cap, 8 * G * cap]
    for lists in (G, G2):
        parts += [8 * lists * N, 8 * lists * N, 4 * lists]
    offs, off = [], 256
    for size in parts:
        offs.append(off)
        off = align256(off + size)
    return cap, G, G2, off, offs


@pytest.fixture(scope="module")
def output(tmp_path_factory):
    hipcc = find_hipcc()
    if hipcc is None:
        pytest.skip("hipcc not available")
    exe = str(tmp_path_factory.mktemp("scan_topn") / "scan_topn_check")
    subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17",
                    "-I", os.path.join(REPO, "include"), "-o", exe, os.path.join(HERE, "scan_topn_check.cpp")],
                   check=True)
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-500:] + res.stderr[-500:]
    return [ln.split(None, 5) if ln.startswith("refuse") else ln.split() for ln in res.stdout.splitlines()]


def test_layout_equals_make_plan_on_every_row(output):
    plans = {tuple(int(v) for v in r[1:6]): [int(v) for v in r[6:]] for r in output if r[0] == "plan"}
    cases = list(itertools.product(KS, BS, PS, NS, NCUS))
    assert sorted(plans) == sorted(cases) and len(cases) == 3 * 2 * 9 * 8 * 3
    for case in cases:
        K, B, P, N, ncu = case
        cap, G, G2, total, offs = layout(*case)
        assert plans[case] == [cap, G, G2, total] + offs, case
        # what the kernels rely on, said directly
        assert cap >= max(512, 2 * N) and cap & (cap - 1) == 0 and (cap == 512 or cap < 4 * N)
        assert 1 <= G <= (4 if N <= 1024 else 2 if N <= 2048 else 1) * ncu and 1 <= G2 <= 32   # two levels suffice
        assert offs[0] == 256 and all(o % 256 == 0 for o in offs + [total])
        thT, T, cs, ck, ls0, lk0, ln0, ls1, lk1, ln1 = offs
        assert all(a < b for a, b in zip(offs, offs[1:] + [total]) if (a, P) != (T, 0))     # increasing
        assert T <= cs                                                         # P = 0: T is empty
        assert ck - cs >= 8 * G * cap and ls0 - ck >= 8 * G * cap                # a buffer per planned workgroup
        assert lk0 - ls0 >= 8 * G * N and ln0 - lk0 >= 8 * G * N and ls1 - ln0 >= 4 * G
        assert lk1 - ls1 >= 8 * G2 * N and ln1 - lk1 >= 8 * G2 * N and total - ln1 >= 4 * G2  # level 1: G2 lists of N


def test_refusals_keep_their_codes_whatever_the_family(output):
    rows = [r for r in output if r[0] == "refuse"]
    want = [(0, 1500, INVALID), (4097, 1500, UNSUPPORTED), (16, 2000001, UNSUPPORTED)]
    assert [(int(r[1]), int(r[2]), int(r[3]), int(r[4]), r[5]) for r in rows] == [
        (n, p, rc, 1, what) for what in WHATS for n, p, rc in want]
