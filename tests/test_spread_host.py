"""Host side of the dispute scan: the gap precondition of every comparison the GPU tests make against
the numpy reference (tests/spread_ref.py), the reference's identities, the trim rule against the
library's cap, and the scan driver's --disputed options and table
(trigenicinteractionpredictor_amd/scan.py).  No GPU."""
import io
import os

import numpy as np
import pytest

import quorum_ref
import scan_ref
import spread_ref
from golden_util import GOLDEN
from test_votes_host import old_cfg

TRAIN = os.path.join(GOLDEN, "tiny", "train.dat")
TEST = os.path.join(GOLDEN, "tiny", "test.dat")


# ------------------------------------------------------------------ the reference
def test_the_gap_is_above_what_the_tolerance_can_move():
    assert spread_ref.SPREAD_GAP == 1e-8 > 4 * spread_ref.RTOL and spread_ref.RTOL == 1e-9


@pytest.mark.parametrize("K,P,B,seed", spread_ref.reference_cases())
def test_the_reference_lists_are_determined(K, P, B, seed):
    """On the reference alone: for every legal trim, N and exclusion the GPU tests name, every
    adjacent absolute gap of the reference's top N + 1 exceeds SPREAD_GAP."""
    c = spread_ref.case(K, P, seed, B)
    for known in spread_ref.exclusions(c.keys, P):
        for t in spread_ref.legal(B):
            d = spread_ref.spread(c.per, t)
            for n in spread_ref.NS:
                s, k = spread_ref.ref_top(c.per, c.keys, t, n, known)       # asserts the gaps
                assert s.size == min(n + 1, c.keys.size - (0 if known is None else known.size))
                assert (np.diff(s) < 0).all() and np.unique(k).size == k.size
                assert known is None or not np.isin(k, known).any()
                np.testing.assert_array_equal(d[np.searchsorted(c.keys, k)], s)
                assert spread_ref.min_abs_gap(s) > spread_ref.SPREAD_GAP


@pytest.mark.parametrize("K,P,B,seed", spread_ref.EXACT_CASES)
def test_the_exact_cases_have_no_zero_spread_and_no_duplicate_at_the_top(K, P, B, seed):
    c = spread_ref.case(K, P, seed, B)
    assert spread_ref.legal(B) == spread_ref.trims(B)
    for t in spread_ref.legal(B):
        d = spread_ref.spread(c.per, t)
        assert (d > 0).all()
        s, _ = scan_ref.top(d, c.keys, 4096)
        assert s.size == 4097 and np.unique(s).size == s.size


def test_the_kernel_matrix_covers_every_instantiation_and_its_lists_are_determined():
    """The matrix of tests/test_gpu_scan_spread.py: every width at every K, and at every K each depth
    1..4 (trim 0..3); the gap precondition of each of its lists."""
    import scan_rule
    cases = spread_ref.matrix_cases()
    assert len(cases) == 24 and all(scan_rule.width(K, B) == WB for K, B, WB in cases)
    assert {K for K, _, _ in cases} == set(quorum_ref.MATRIX_K)
    for K in quorum_ref.MATRIX_K:
        seen = set()
        for k, B, _ in cases:
            if k == K:
                seen |= set(spread_ref.trims(B))
        assert seen == set(range(spread_ref.TARGET_TRIM + 1)), (K, seen)
        assert max(B for k, B, _ in cases if k == K) >= 8               # D = 4 runs
    for K, B, _ in cases:
        c = spread_ref.matrix_case(K, B)
        for t in spread_ref.trims(B):
            spread_ref.ref_top(c.per, c.keys, t, spread_ref.MATRIX_N, c.keys[1::9])     # asserts the gaps
    # the seed table is the quorum matrix's but for the one case whose gap falls short there
    assert {k for k, v in spread_ref.MATRIX_SEEDS.items() if quorum_ref.MATRIX_SEEDS.get(k) != v} == {(19, 12)}
    c = quorum_ref.matrix_case(19, 12)
    s, _ = scan_ref.top(spread_ref.spread(c.per, 0), c.keys, spread_ref.MATRIX_N, c.keys[1::9])
    assert spread_ref.min_abs_gap(s) < spread_ref.SPREAD_GAP


def test_reference_identities():
    """Bit for bit: t = 0 is max - min, and d_t = q_{1+t} - q_{ns-t} of the quorum reference."""
    for K, P, B, seed in (spread_ref.CASES[1], spread_ref.CASES[3]):     # B = 8 and B = 4
        c = spread_ref.case(K, P, seed, B)
        np.testing.assert_array_equal(spread_ref.spread(c.per, 0), c.per.max(axis=0) - c.per.min(axis=0))
        for t in spread_ref.legal(B):
            d = spread_ref.spread(c.per, t)
            want = quorum_ref.quorum(c.per, 1 + t) - quorum_ref.quorum(c.per, B - t)
            assert scan_ref.bits(d) == scan_ref.bits(want)
            assert (d >= 0).all() and not np.signbit(d).any()
            hi, lo = spread_ref.ends(c.per, t)
            assert np.isin(hi, c.per).all() and np.isin(lo, c.per).all()    # slot scores, bit for bit
            if t:
                assert (d <= spread_ref.spread(c.per, t - 1)).all()         # a trim only narrows
            np.testing.assert_array_equal(spread_ref.atol(c.per, t), spread_ref.RTOL * (hi + lo))
        # a prefix of the slots
        np.testing.assert_array_equal(spread_ref.spread(c.per, 0, ns=2), np.abs(c.per[0] - c.per[1]))
        # the middle gap of an even ensemble
        srt = np.sort(c.per, axis=0)
        np.testing.assert_array_equal(spread_ref.spread(c.per, (B - 2) // 2), srt[B // 2] - srt[B // 2 - 1])


# ------------------------------------------------------------------ the trim rule
def test_trim_rule_and_the_library_cap():
    from trigenicinteractionpredictor_amd import _lib, scan
    cap = int(_lib.load().mmsbm_scan_spread_max_trim())
    assert cap == 3 == spread_ref.TARGET_TRIM == scan.MAX_SPREAD_TRIM
    assert cap + 1 == int(_lib.load().mmsbm_scan_quorum_max_depth())    # the quorum scan's depth at both ends
    assert spread_ref.legal(0) == spread_ref.legal(1) == scan.spread_trims(1) == scan.spread_trims(0) == []
    for ns in range(2, 24):
        legal = spread_ref.legal(ns)
        assert legal == [t for t in range(ns) if ns - 2 * t >= 2] and legal[0] == 0 and legal[-1] == (ns - 2) // 2
        assert scan.spread_trims(ns, None) == legal
        assert scan.spread_trims(ns) == spread_ref.trims(ns, cap) == [t for t in legal if t <= cap]
        if ns <= 9:
            assert spread_ref.trims(ns, cap) == legal                   # every legal trim
    assert spread_ref.trims(10, cap) == [0, 1, 2, 3] and spread_ref.legal(10) == [0, 1, 2, 3, 4]


# ------------------------------------------------------------------ the driver's arguments
NEW_KEYS = ("disputed", "disputed_trim")


def test_driver_parses_the_disputed_flags():
    from trigenicinteractionpredictor_amd import scan
    cfg = scan.parse(["-t", TRAIN, "-e", TEST, "-k", "3", "-n", "8", "--disputed", "d.tsv", "--disputed-trim", "2"])
    assert [cfg[k] for k in NEW_KEYS] == ["d.tsv", 2]
    # the default: the range
    cfg = scan.parse(["-t", TRAIN, "-n", "6", "--disputed", "d.tsv"])
    assert [cfg[k] for k in NEW_KEYS] == ["d.tsv", 0]
    # -n may follow --disputed-trim
    assert scan.parse(["--disputed-trim", "1", "-n", "4", "--disputed", "d.tsv"])["disputed_trim"] == 1
    # either option brings both keys, and none of the quorum or consensus keys
    cfg = scan.parse(["-n", "4", "--disputed-trim", "1"])
    assert [cfg[k] for k in NEW_KEYS] == [None, 1]
    assert not any(k in cfg for k in ("quorum", "quorum_votes", "min_votes", "consensus"))
    # every legal trim under the cap
    for n in range(2, 12):
        for t in scan.spread_trims(n):
            assert scan.parse(["-n", str(n), "--disputed", "d.tsv", "--disputed-trim", str(t)])["disputed_trim"] == t
    # the pair mask goes with --disputed, and still not with --quorum
    cfg = scan.parse(["-n", "3", "--disputed", "d.tsv", "--allow-genes", "g.txt", "--block-pairs", "b.txt"])
    assert cfg["allow_genes"] == "g.txt" and cfg["block_pairs"] == "b.txt" and cfg["disputed"] == "d.tsv"


BAD = [("--disputed-trim", v) for v in ("-1", "2", "3", "x", "1.5", "")]       # -n 4 below: trims 0 and 1


@pytest.mark.parametrize("flag,value", BAD)
def test_bad_disputed_values_are_refused_with_exit_2(flag, value, monkeypatch):
    import sys
    from trigenicinteractionpredictor_amd import scan
    # the engine module (torch + the HIP library) must not be needed to refuse an argument
    monkeypatch.setitem(sys.modules, "trigenicinteractionpredictor_amd.engine", None)
    assert scan.main(["-t", TRAIN, "-n", "4", "--disputed", "d.tsv", flag, value]) == 2


def test_disputed_with_best_one_restart_or_above_the_cap_is_refused(monkeypatch):
    import sys
    from trigenicinteractionpredictor_amd import cli, scan
    monkeypatch.setitem(sys.modules, "trigenicinteractionpredictor_amd.engine", None)
    T = scan.MAX_SPREAD_TRIM
    above = ["-n", str(2 * T + 4), "--disputed", "d.tsv", "--disputed-trim", str(T + 1)]    # legal, above the cap
    for argv in (["-n", "3", "--disputed", "d.tsv", "--best"], ["--best", "-n", "4", "--disputed", "d.tsv",
                                                                "--disputed-trim", "1"],
                 ["--disputed", "d.tsv"], ["-n", "1", "--disputed", "d.tsv"], ["--disputed-trim", "0"],
                 ["-n", "3", "--disputed", "d.tsv", "--disputed-trim", "1"], above,
                 ["-n", "3", "--quorum", "q.tsv", "--disputed", "d.tsv", "--allow-genes", "g.txt"]):
        with pytest.raises(cli.ArgError):
            scan.parse(["-t", TRAIN] + argv)
        assert scan.main(["-t", TRAIN] + argv) == 2
    assert scan.parse(["-t", TRAIN, "--best"])["best"] is True         # --best alone is what it was


def test_parse_without_the_new_flags_is_unchanged():
    from trigenicinteractionpredictor_amd import scan
    old = old_cfg()
    assert scan.parse([]) == old
    assert scan.parse(["-n", "2", "--disputed", "d.tsv"]) == dict(old, samples=2, disputed="d.tsv", disputed_trim=0)
    argv = ["-t", TRAIN, "-e", TEST, "-k", "4", "-n", "3", "-i", "7", "--seed", "5", "--top", "77", "--exclude",
            "train", "-o", "o.tsv", "--census", "c.tsv", "--thresholds", "0.5,0.1", "--pairs", "p.tsv",
            "--pair-threshold", "0.3", "--gene-census", "g.tsv", "--heldout-ranks", "h.tsv"]
    want = dict(old, train=TRAIN, test=TEST, k=4, samples=3, iterations=7, seed=5, top=77, exclude=("train",),
                out="o.tsv", census="c.tsv", thresholds=[0.5, 0.1], pairs="p.tsv", pair_threshold=0.3,
                gene_census="g.tsv", heldout_ranks="h.tsv")
    assert scan.parse(argv) == want
    assert scan.parse(argv + ["--quorum", "q.tsv"]) == dict(want, quorum="q.tsv", quorum_votes=3)
    assert scan.parse(argv + ["--disputed", "d.tsv"]) == dict(want, disputed="d.tsv", disputed_trim=0)
    for flag in ("--disputed", "--disputed-trim"):
        assert flag in scan.USAGE and flag in scan.__doc__


# ------------------------------------------------------------------ the table
def test_spread_rows_and_writer():
    from trigenicinteractionpredictor_amd import scan
    id_gene = {0: "YAL001C", 1: "YBR002W", 2: "YCL003C", 10: "YDR010W"}
    scores = np.array([0.5, 0.25])
    ids = np.array([[0, 10, 2], [0, 1, 10]], dtype=np.int32)
    probs = np.array([[0.5, 0.75], [0.75, 0.5], [1.0, 0.625]])
    rows = scan.spread_rows(id_gene, scores, ids, probs)
    assert rows == [[1, 0.5, 0.75, 0.5, 1.0, "0_10_2", ["YAL001C", "YCL003C", "YDR010W"]],
                    [2, 0.25, 0.625, 0.5, 0.75, "0_1_10", ["YAL001C", "YBR002W", "YDR010W"]]]
    out = io.StringIO()
    scan.write_disputed_tsv(3, 0, rows, out)
    assert out.getvalue() == ("# samples\t3\n"
                              "# disputed trim\t0\n"
                              "rank\tspread\tmean\tmin\tmax\tids\tnames\n"
                              "1\t0.5\t0.75\t0.5\t1.0\t0_10_2\tYAL001C_YCL003C_YDR010W\n"
                              "2\t0.25\t0.625\t0.5\t0.75\t0_1_10\tYAL001C_YBR002W_YDR010W\n")
    assert scan.spread_rows(id_gene, scores[:0], ids[:0], np.zeros((3, 0))) == []
    out = io.StringIO()
    scan.write_disputed_tsv(2, 0, [], out)
    assert out.getvalue() == "# samples\t2\n# disputed trim\t0\nrank\tspread\tmean\tmin\tmax\tids\tnames\n"
