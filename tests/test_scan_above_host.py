"""Host side of the threshold scan (trigenicinteractionpredictor_amd/scan.py: bracket_threshold, the
driver's --network options and its table).  No GPU."""
import io
import os

import numpy as np
import pytest

from golden_util import GOLDEN

TRAIN = os.path.join(GOLDEN, "tiny", "train.dat")
TEST = os.path.join(GOLDEN, "tiny", "test.dat")


class Census:
    """count_at over a fixed array of scores, as the census counts: scores >= each threshold."""

    def __init__(self, scores):
        self.s = np.sort(np.asarray(scores, dtype=np.float64))
        self.passes = 0
        self.most = 0

    def __call__(self, thresholds):
        t = np.asarray(thresholds, dtype=np.float64).reshape(-1)
        assert np.isfinite(t).all()
        self.passes += 1
        self.most = max(self.most, t.size)
        return (self.s.size - np.searchsorted(self.s, t, side="left")).astype(np.int64)

    def count(self, t):
        return int((self.s >= t).sum())

    def hi(self, max_n=4096):
        """The last score of scan_top(max_n)."""
        return float(self.s[-max_n])


def bracket(scores, n):
    from trigenicinteractionpredictor_amd.scan import MAX_CENSUS_M, bracket_threshold
    c = Census(scores)
    lo = bracket_threshold(n, c.hi(), c)
    assert c.passes <= 8 and c.most <= MAX_CENSUS_M
    assert c.count(lo) >= min(n, c.s.size)
    return lo, c


# ------------------------------------------------------------------ bracket_threshold
@pytest.mark.parametrize("n", [4097, 5000, 20000, 150000])
def test_bracket_on_well_separated_scores(n):
    """200,000 distinct scores; n just above the scan's cap and far above it."""
    scores = np.random.default_rng(1).random(200000) ** 3      # dense near 0, as probabilities are
    assert np.unique(scores).size == scores.size
    lo, c = bracket(scores, n)
    assert n <= c.count(lo) <= n + max(n // 8, 4096)


def test_bracket_with_equal_scores_straddling_rank_n():
    """3,000 distinct scores above a block of 50,000 equal ones, n inside the block: no threshold
    has a count in [n, n + slack], the search ends on adjacent doubles with the block just above lo."""
    rng = np.random.default_rng(2)
    tie = 0.3
    scores = np.concatenate([tie + 0.1 + 0.5 * rng.random(5000), np.full(50000, tie), tie * rng.random(100000)])
    n = 20000
    lo, c = bracket(scores, n)
    assert c.count(lo) == 55000 and lo <= tie
    assert np.nextafter(lo, np.inf) >= tie                     # nothing between lo and the block
    # the whole list of ties reaches rank n from hi itself: nothing above hi holds n rows
    c2 = Census(np.concatenate([np.full(30000, 0.5), 0.4 * rng.random(1000)]))
    from trigenicinteractionpredictor_amd.scan import bracket_threshold
    assert bracket_threshold(n, c2.hi(), c2) == 0.5 and c2.passes == 1


@pytest.mark.parametrize("extra", [0, 1, 5000])
def test_bracket_returns_everything_when_the_total_is_at_most_n(extra):
    scores = 0.01 + 0.9 * np.random.default_rng(3).random(6000)
    lo, c = bracket(scores, 6000 + extra)
    assert lo == 0.0 and c.count(lo) == 6000 and c.passes == 1


def test_bracket_just_above_the_cap():
    """n = 4097 on 9,880 scores (P = 40): a count within the slack is accepted at once."""
    scores = np.random.default_rng(4).random(9880)
    lo, c = bracket(scores, 4097)
    assert 4097 <= c.count(lo) <= 4097 + 4096


def test_limit_error_carries_the_count():
    from trigenicinteractionpredictor_amd.scan import LimitError
    e = LimitError(212408, 1000)
    assert isinstance(e, ValueError) and (e.count, e.limit) == (212408, 1000)
    assert "212408" in str(e) and "1000" in str(e)


# ------------------------------------------------------------------ the driver's arguments
def test_driver_parses_the_network_flags():
    from trigenicinteractionpredictor_amd import scan
    cfg = scan.parse(["-t", TRAIN, "-e", TEST, "-k", "3", "--network", "n.tsv", "--network-threshold", "0.25",
                      "--network-limit", "1234"])
    assert (cfg["network"], cfg["network_threshold"], cfg["network_limit"]) == ("n.tsv", 0.25, 1234)
    assert scan.parse(["--network-threshold", "1"])["network_threshold"] == 1.0
    # the defaults are in cfg with --network alone
    cfg = scan.parse(["-t", TRAIN, "--network", "n.tsv"])
    assert cfg["network"] == "n.tsv" and cfg["network_threshold"] == 0.5 and cfg["network_limit"] == 10000000
    # and with any of the three options the three keys are there
    cfg = scan.parse(["--network-limit", "5"])
    assert (cfg["network"], cfg["network_threshold"], cfg["network_limit"]) == (None, 0.5, 5)


@pytest.mark.parametrize("flag,value", [("--network-threshold", v) for v in ("0", "1.5", "-0.1", "nan", "inf", "x", "")]
                         + [("--network-limit", v) for v in ("0", "-3", "x", "1.5", "")])
def test_bad_network_values_are_refused_with_exit_2(flag, value, monkeypatch):
    import sys
    from trigenicinteractionpredictor_amd import scan
    # the engine module (torch + the HIP library) must not be needed to refuse an argument
    monkeypatch.setitem(sys.modules, "trigenicinteractionpredictor_amd.engine", None)
    assert scan.main(["-t", TRAIN, "--network", "n.tsv", flag, value]) == 2


def test_parse_without_the_new_flags_is_unchanged():
    """The cfg `parse` gave before the threshold scan, whole: an argv without the new flags gives
    exactly it (the three new keys come with the new flags only, as tests/test_pair_census_host.py
    demands of `parse([])`), and with them it differs by those keys alone."""
    from trigenicinteractionpredictor_amd import cli, scan
    new = {"network": "n.tsv", "network_threshold": 0.5, "network_limit": 10000000}
    old = dict(cli.DEFAULTS, samples=1, iterations=100, top=100, exclude=("train", "test"), best=False, out=None,
               seed=None, genes=[], all_genes=False, census=None, thresholds=None, heldout_ranks=None,
               pairs=None, pair_threshold=0.5, gene_census=None)
    assert scan.parse([]) == old
    cfg = scan.parse(["--network", "n.tsv"])
    assert {k: v for k, v in cfg.items() if k not in new} == old and {k: cfg[k] for k in new} == new
    argv = ["-t", TRAIN, "-e", TEST, "-k", "4", "-n", "3", "-i", "7", "--seed", "5", "--top", "77", "--exclude",
            "train", "--best", "-o", "o.tsv", "--census", "c.tsv", "--thresholds", "0.5,0.1", "--pairs", "p.tsv",
            "--pair-threshold", "0.3", "--gene-census", "g.tsv", "--heldout-ranks", "h.tsv"]
    want = dict(old, train=TRAIN, test=TEST, k=4, samples=3, iterations=7, seed=5, top=77, exclude=("train",),
                best=True, out="o.tsv", census="c.tsv", thresholds=[0.5, 0.1], pairs="p.tsv", pair_threshold=0.3,
                gene_census="g.tsv", heldout_ranks="h.tsv")
    assert scan.parse(argv) == want
    cfg = scan.parse(argv + ["--network", "n.tsv"])
    assert {k: v for k, v in cfg.items() if k not in new} == want and {k: cfg[k] for k in new} == new
    for flag in ("--network", "--network-threshold", "--network-limit"):
        assert flag in scan.USAGE and flag in scan.__doc__


# ------------------------------------------------------------------ the table
def test_network_rows_and_writer():
    from trigenicinteractionpredictor_amd import scan
    id_gene = {0: "YAL001C", 1: "YBR002W", 2: "YCL003C", 10: "YDR010W"}
    scores = np.array([0.75, 0.5, 0.5])
    ids = np.array([[0, 10, 2], [0, 1, 10], [1, 10, 2]], dtype=np.int32)
    rows = scan.network_rows(id_gene, scores, ids)
    assert rows == [[1, 0.75, "0_10_2", ["YAL001C", "YCL003C", "YDR010W"]],
                    [2, 0.5, "0_1_10", ["YAL001C", "YBR002W", "YDR010W"]],
                    [3, 0.5, "1_10_2", ["YBR002W", "YCL003C", "YDR010W"]]]
    out = io.StringIO()
    scan.write_tsv(rows, out)
    assert out.getvalue() == ("rank\tprobability\tids\tnames\n"
                              "1\t0.75\t0_10_2\tYAL001C_YCL003C_YDR010W\n"
                              "2\t0.5\t0_1_10\tYAL001C_YBR002W_YDR010W\n"
                              "3\t0.5\t1_10_2\tYBR002W_YCL003C_YDR010W\n")
    assert scan.network_rows(id_gene, np.zeros(0), np.zeros((0, 3), np.int32)) == []
