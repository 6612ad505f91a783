"""Host side of the quorum scan: the gap precondition of every comparison the GPU tests make against
the numpy reference (tests/quorum_ref.py), the depth rule against the library's cap, and the scan
driver's --quorum options and table (trigenicinteractionpredictor_amd/scan.py).  No GPU."""
import io
import os

import numpy as np
import pytest

import quorum_ref
import scan_ref
from golden_util import GOLDEN
from test_votes_host import old_cfg

TRAIN = os.path.join(GOLDEN, "tiny", "train.dat")
TEST = os.path.join(GOLDEN, "tiny", "test.dat")


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("K,P,B,seed", quorum_ref.reference_cases() + quorum_ref.EXACT_CASES)
def test_the_reference_lists_are_determined(K, P, B, seed):
    """On the reference alone: for every m, N and exclusion the GPU tests name, every adjacent
    relative gap of the reference's top N + 1 exceeds the project's 1e-9 (by two orders: 1e-7)."""
    c = quorum_ref.case(K, P, seed, B)
    smallest = np.inf
    for known in quorum_ref.exclusions(c.keys, P):
        for m in range(1, B + 1):
            q = quorum_ref.quorum(c.per, m)
            for n in quorum_ref.NS:
                s, k = quorum_ref.ref_top(c.per, c.keys, m, n, known)       # asserts the gaps
                assert s.size == min(n + 1, c.keys.size - (0 if known is None else known.size))
                assert (np.diff(s) < 0).all() and np.unique(k).size == k.size
                assert known is None or not np.isin(k, known).any()
                at = np.searchsorted(c.keys, k)
                np.testing.assert_array_equal(q[at], s)
                smallest = min(smallest, scan_ref.min_gap(s))
    assert smallest >= 1e-7, smallest


def test_the_kernel_matrix_covers_every_instantiation_and_its_lists_are_determined():
    """The matrix of tests/test_gpu_scan_quorum.py: every width at every K, and at every K each depth
    up to the target in both directions (the largest kept: m <= ns - m + 1; the smallest kept:
    otherwise); the gap precondition of each of its lists."""
    import scan_rule
    cases = quorum_ref.matrix_cases()
    assert len(cases) == 24 and all(scan_rule.width(K, B) == WB for K, B, WB in cases)
    for K in quorum_ref.MATRIX_K:
        seen = set()
        for k, B, _ in cases:
            if k == K:
                seen |= {(quorum_ref.depth(m, B), m <= B - m + 1) for m in quorum_ref.supported(B, quorum_ref.TARGET_DEPTH)}
        assert seen >= {(d, up) for d in range(1, quorum_ref.TARGET_DEPTH + 1) for up in (True, False)}, (K, seen)
    for K, B, _ in cases:
        c = quorum_ref.matrix_case(K, B)
        for m in quorum_ref.supported(B, quorum_ref.TARGET_DEPTH):
            s, _ = quorum_ref.ref_top(c.per, c.keys, m, quorum_ref.MATRIX_N, c.keys[1::9])
            assert scan_ref.min_gap(s) >= quorum_ref.MATRIX_GAP, (K, B, m)


def test_reference_identities():
    K, P, B, seed = quorum_ref.CASES[3]
    c = quorum_ref.case(K, P, seed, B)
    np.testing.assert_array_equal(quorum_ref.quorum(c.per, B), c.per.min(axis=0))
    np.testing.assert_array_equal(quorum_ref.quorum(c.per, 1), c.per.max(axis=0))
    np.testing.assert_array_equal(quorum_ref.quorum(c.per, 1, ns=2), np.maximum(c.per[0], c.per[1]))
    for m in range(1, B + 1):
        q = quorum_ref.quorum(c.per, m)
        assert np.isin(q, c.per).all()                          # one of the slots' scores, bit for bit
        for t in np.quantile(c.per, [0.1, 0.5, 0.9]):           # votes(t) >= m exactly when q_m >= t
            np.testing.assert_array_equal((c.per >= t).sum(axis=0) >= m, q >= t)
    # the same list from the largest and from the smallest
    np.testing.assert_array_equal(quorum_ref.quorum(c.per, 2), -np.sort(-c.per, axis=0)[1])


# ------------------------------------------------------------------ the depth rule
def test_depth_rule_and_the_library_cap():
    from trigenicinteractionpredictor_amd import _lib, scan
    cap = int(_lib.load().mmsbm_scan_quorum_max_depth())
    assert 2 <= cap <= quorum_ref.TARGET_DEPTH
    assert scan.MAX_QUORUM_DEPTH == cap
    for ns in range(1, 20):
        depths = [quorum_ref.depth(m, ns) for m in range(1, ns + 1)]
        assert depths == [min(m, ns - m + 1) for m in range(1, ns + 1)] == depths[::-1]
        assert depths == [scan.quorum_depth(m, ns) for m in range(1, ns + 1)]
        assert depths[0] == depths[-1] == 1 and max(depths) == (ns + 1) // 2
        ok = quorum_ref.supported(ns, cap)
        assert set(ok) == {m for m in range(1, ns + 1) if m <= cap or m > ns - cap}
        if ns <= 2 * cap:
            assert ok == list(range(1, ns + 1))                  # every m
        assert {1, ns} <= set(ok)                                # min and max always
    assert quorum_ref.supported(3, 2) == [1, 2, 3]               # the majority of three at the lowest cap allowed


# ------------------------------------------------------------------ the driver's arguments
NEW_KEYS = ("quorum", "quorum_votes")


def test_driver_parses_the_quorum_flags():
    from trigenicinteractionpredictor_amd import scan
    cfg = scan.parse(["-t", TRAIN, "-e", TEST, "-k", "3", "-n", "8", "--quorum", "q.tsv", "--quorum-votes", "5"])
    assert [cfg[k] for k in NEW_KEYS] == ["q.tsv", 5]
    # the default: every restart
    cfg = scan.parse(["-t", TRAIN, "-n", "6", "--quorum", "q.tsv"])
    assert [cfg[k] for k in NEW_KEYS] == ["q.tsv", 6]
    assert scan.parse(["--quorum", "q.tsv"])["quorum_votes"] == 1          # -n defaults to 1
    # -n may follow --quorum-votes
    assert scan.parse(["--quorum-votes", "3", "-n", "3", "--quorum", "q.tsv"])["quorum_votes"] == 3
    # either option brings both keys, and none of the consensus keys
    cfg = scan.parse(["-n", "4", "--quorum-votes", "2"])
    assert [cfg[k] for k in NEW_KEYS] == [None, 2] and "min_votes" not in cfg and "consensus" not in cfg
    # --min-votes stays the consensus option
    cfg = scan.parse(["-n", "4", "--quorum", "q.tsv", "--min-votes", "2"])
    assert cfg["quorum_votes"] == 4 and cfg["min_votes"] == 2
    # beyond 2 * depth restarts: the lowest and the highest values of M
    D = scan.MAX_QUORUM_DEPTH
    for m in list(range(1, D + 1)) + list(range(2 * D + 3 - D, 2 * D + 3)):
        assert scan.parse(["-n", str(2 * D + 2), "--quorum", "q.tsv", "--quorum-votes", str(m)])["quorum_votes"] == m


BAD = [("--quorum-votes", v) for v in ("0", "-1", "5", "x", "1.5", "")]       # -n 4 below


@pytest.mark.parametrize("flag,value", BAD)
def test_bad_quorum_values_are_refused_with_exit_2(flag, value, monkeypatch):
    import sys
    from trigenicinteractionpredictor_amd import scan
    # the engine module (torch + the HIP library) must not be needed to refuse an argument
    monkeypatch.setitem(sys.modules, "trigenicinteractionpredictor_amd.engine", None)
    assert scan.main(["-t", TRAIN, "-n", "4", "--quorum", "q.tsv", flag, value]) == 2


def test_quorum_with_best_or_too_deep_is_refused(monkeypatch):
    import sys
    from trigenicinteractionpredictor_amd import cli, scan
    monkeypatch.setitem(sys.modules, "trigenicinteractionpredictor_amd.engine", None)
    D = scan.MAX_QUORUM_DEPTH
    deep = ["-n", str(2 * D + 1), "--quorum", "q.tsv", "--quorum-votes", str(D + 1)]    # the median of 2 D + 1
    for argv in (["--quorum", "q.tsv", "--best"], ["--best", "-n", "3", "--quorum", "q.tsv", "--quorum-votes", "2"],
                 deep):
        with pytest.raises(cli.ArgError):
            scan.parse(["-t", TRAIN] + argv)
        assert scan.main(["-t", TRAIN] + argv) == 2
    assert scan.parse(["-t", TRAIN, "--best"])["best"] is True         # --best alone is what it was


def test_parse_without_the_new_flags_is_unchanged():
    from trigenicinteractionpredictor_amd import scan
    old = old_cfg()
    assert scan.parse([]) == old
    cfg = scan.parse(["--quorum", "q.tsv"])
    assert cfg == dict(old, quorum="q.tsv", quorum_votes=1)
    argv = ["-t", TRAIN, "-e", TEST, "-k", "4", "-n", "3", "-i", "7", "--seed", "5", "--top", "77", "--exclude",
            "train", "-o", "o.tsv", "--census", "c.tsv", "--thresholds", "0.5,0.1", "--pairs", "p.tsv",
            "--pair-threshold", "0.3", "--gene-census", "g.tsv", "--heldout-ranks", "h.tsv"]
    want = dict(old, train=TRAIN, test=TEST, k=4, samples=3, iterations=7, seed=5, top=77, exclude=("train",),
                out="o.tsv", census="c.tsv", thresholds=[0.5, 0.1], pairs="p.tsv", pair_threshold=0.3,
                gene_census="g.tsv", heldout_ranks="h.tsv")
    assert scan.parse(argv) == want
    votes = {"consensus": "v.tsv", "consensus_threshold": 0.5, "min_votes": 3, "consensus_limit": 10000000}
    assert scan.parse(argv + ["--consensus", "v.tsv"]) == dict(want, **votes)  # --consensus brings its own four only
    assert scan.parse(argv + ["--quorum", "q.tsv"]) == dict(want, quorum="q.tsv", quorum_votes=3)
    for flag in ("--quorum", "--quorum-votes"):
        assert flag in scan.USAGE and flag in scan.__doc__


# ------------------------------------------------------------------ the table
def test_quorum_rows_and_writer():
    from trigenicinteractionpredictor_amd import scan
    id_gene = {0: "YAL001C", 1: "YBR002W", 2: "YCL003C", 10: "YDR010W"}
    scores = np.array([0.5, 0.25])
    ids = np.array([[0, 10, 2], [0, 1, 10]], dtype=np.int32)
    probs = np.array([[0.5, 0.75], [0.75, 0.25], [1.0, 0.5]])
    rows = scan.quorum_rows(id_gene, scores, ids, probs)
    assert rows == [[1, 0.5, 0.75, 0.5, 1.0, "0_10_2", ["YAL001C", "YCL003C", "YDR010W"]],
                    [2, 0.25, 0.5, 0.25, 0.75, "0_1_10", ["YAL001C", "YBR002W", "YDR010W"]]]
    out = io.StringIO()
    scan.write_quorum_tsv(3, 3, rows, out)
    assert out.getvalue() == ("# samples\t3\n"
                              "# quorum votes\t3\n"
                              "rank\tquorum\tmean\tmin\tmax\tids\tnames\n"
                              "1\t0.5\t0.75\t0.5\t1.0\t0_10_2\tYAL001C_YCL003C_YDR010W\n"
                              "2\t0.25\t0.5\t0.25\t0.75\t0_1_10\tYAL001C_YBR002W_YDR010W\n")
    assert scan.quorum_rows(id_gene, scores[:0], ids[:0], np.zeros((3, 0))) == []
    out = io.StringIO()
    scan.write_quorum_tsv(1, 1, [], out)
    assert out.getvalue() == "# samples\t1\n# quorum votes\t1\nrank\tquorum\tmean\tmin\tmax\tids\tnames\n"
