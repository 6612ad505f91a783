"""Host side of the vote scan: the numpy reference itself (tests/votes_ref.py), the scan driver's
--consensus options and its table (trigenicinteractionpredictor_amd/scan.py).  No GPU."""
import io
import os
from math import comb

import numpy as np
import pytest

import census_ref
import scan_ref
import votes_ref
from golden_util import GOLDEN

TRAIN = os.path.join(GOLDEN, "tiny", "train.dat")
TEST = os.path.join(GOLDEN, "tiny", "test.dat")
CASES = [(3, 37, 3, 11), (10, 50, 8, 5), (5, 33, 2, 3), (13, 40, 4, 7)]     # (K, P, B, seed)


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("K,P,B,seed", CASES)
def test_every_bucket_is_filled_near_the_median(K, P, B, seed):
    """On the reference alone: at the clear midpoint nearest the median of all slots' scores every
    vote count 0..B occurs, so the GPU tests at these cases exercise every counter."""
    c = votes_ref.case(K, P, seed, B)
    flat = c.per.reshape(-1)
    t = votes_ref.near_median(c.per)
    census_ref.assert_clear(flat, [t])
    assert abs((flat >= t).mean() - 0.5) < 0.05
    votes, keys, mean, hist = votes_ref.ref_votes(c.per, c.keys, t)
    assert hist.shape == (B + 1,) and hist.sum() == comb(P, 3)
    assert (hist > 0).all(), hist


def test_reference_identities():
    K, P, B, seed = CASES[0]
    c = votes_ref.case(K, P, seed, B)
    thresholds = votes_ref.clear_thresholds(c.per)
    assert thresholds.size >= 5
    known = c.keys[::7].copy()
    for t in thresholds:
        votes, keys, mean, hist = votes_ref.ref_votes(c.per, c.keys, t, known=known)
        assert keys.size == c.keys.size - known.size and not np.isin(keys, known).any()
        # the votes are the slots' censuses added up
        per_slot = [census_ref.ref_census(c.per[b], c.keys, [t], known)[0][0] for b in range(B)]
        assert (np.arange(B + 1) * hist).sum() == sum(per_slot)
        assert hist.sum() == keys.size
        for m in (1, 2, B):
            hits = votes_ref.ref_hits(votes, keys, mean, m)
            assert len(hits) == hist[m:].sum()
    # below every score: everything has every vote; above: none
    assert votes_ref.ref_votes(c.per, c.keys, thresholds[0])[3].tolist() == [0] * B + [comb(P, 3)]
    assert votes_ref.ref_votes(c.per, c.keys, thresholds[-1])[3].tolist() == [comb(P, 3)] + [0] * B
    # a prefix of the slots: ns + 1 buckets, the prefix's mean
    votes, keys, mean, hist = votes_ref.ref_votes(c.per, c.keys, thresholds[2], ns=2)
    assert hist.shape == (3,) and votes.max() <= 2
    np.testing.assert_array_equal(mean, (c.per[0] + c.per[1]) / 2)
    np.testing.assert_array_equal(c.mean, scan_ref.prefix_mean(c.per, B))


# ------------------------------------------------------------------ the driver's arguments
def old_cfg():
    from trigenicinteractionpredictor_amd import cli
    return dict(cli.DEFAULTS, samples=1, iterations=100, top=100, exclude=("train", "test"), best=False, out=None,
                seed=None, genes=[], all_genes=False, census=None, thresholds=None, heldout_ranks=None,
                pairs=None, pair_threshold=0.5, gene_census=None)


NEW_KEYS = ("consensus", "consensus_threshold", "min_votes", "consensus_limit")


def test_driver_parses_the_consensus_flags():
    from trigenicinteractionpredictor_amd import scan
    cfg = scan.parse(["-t", TRAIN, "-e", TEST, "-k", "3", "-n", "8", "--consensus", "c.tsv", "--consensus-threshold",
                      "0.25", "--min-votes", "5", "--consensus-limit", "1234"])
    assert [cfg[k] for k in NEW_KEYS] == ["c.tsv", 0.25, 5, 1234]
    assert scan.parse(["--consensus-threshold", "1"])["consensus_threshold"] == 1.0
    # the defaults: 0.5, every restart, ten million rows
    cfg = scan.parse(["-t", TRAIN, "-n", "6", "--consensus", "c.tsv"])
    assert [cfg[k] for k in NEW_KEYS] == ["c.tsv", 0.5, 6, 10000000]
    assert scan.parse(["--consensus", "c.tsv"])["min_votes"] == 1       # -n defaults to 1
    # -n may follow --min-votes
    assert scan.parse(["--min-votes", "3", "-n", "3", "--consensus", "c.tsv"])["min_votes"] == 3
    # any of the four options brings the four keys
    cfg = scan.parse(["--consensus-limit", "5"])
    assert [cfg[k] for k in NEW_KEYS] == [None, 0.5, 1, 5]


BAD = ([("--consensus-threshold", v) for v in ("0", "1.5", "-0.1", "nan", "inf", "x", "")]
       + [("--min-votes", v) for v in ("0", "-1", "5", "x", "1.5", "")]              # -n 4 below
       + [("--consensus-limit", v) for v in ("0", "-3", "x", "1.5", "")])


@pytest.mark.parametrize("flag,value", BAD)
def test_bad_consensus_values_are_refused_with_exit_2(flag, value, monkeypatch):
    import sys
    from trigenicinteractionpredictor_amd import scan
    # the engine module (torch + the HIP library) must not be needed to refuse an argument
    monkeypatch.setitem(sys.modules, "trigenicinteractionpredictor_amd.engine", None)
    assert scan.main(["-t", TRAIN, "-n", "4", "--consensus", "c.tsv", flag, value]) == 2


def test_consensus_with_best_is_refused(monkeypatch):
    import sys
    from trigenicinteractionpredictor_amd import cli, scan
    monkeypatch.setitem(sys.modules, "trigenicinteractionpredictor_amd.engine", None)
    for argv in (["--consensus", "c.tsv", "--best"], ["--best", "-n", "3", "--consensus", "c.tsv", "--min-votes", "2"]):
        with pytest.raises(cli.ArgError):
            scan.parse(["-t", TRAIN] + argv)
        assert scan.main(["-t", TRAIN] + argv) == 2
    assert scan.parse(["-t", TRAIN, "--best"])["best"] is True         # --best alone is what it was


def test_parse_without_the_new_flags_is_unchanged():
    from trigenicinteractionpredictor_amd import scan
    old = old_cfg()
    new = {"consensus": "c.tsv", "consensus_threshold": 0.5, "min_votes": 1, "consensus_limit": 10000000}
    assert scan.parse([]) == old
    cfg = scan.parse(["--consensus", "c.tsv"])
    assert {k: v for k, v in cfg.items() if k not in new} == old and {k: cfg[k] for k in new} == new
    argv = ["-t", TRAIN, "-e", TEST, "-k", "4", "-n", "3", "-i", "7", "--seed", "5", "--top", "77", "--exclude",
            "train", "-o", "o.tsv", "--census", "c.tsv", "--thresholds", "0.5,0.1", "--pairs", "p.tsv",
            "--pair-threshold", "0.3", "--gene-census", "g.tsv", "--heldout-ranks", "h.tsv"]
    want = dict(old, train=TRAIN, test=TEST, k=4, samples=3, iterations=7, seed=5, top=77, exclude=("train",),
                out="o.tsv", census="c.tsv", thresholds=[0.5, 0.1], pairs="p.tsv", pair_threshold=0.3,
                gene_census="g.tsv", heldout_ranks="h.tsv")
    assert scan.parse(argv) == want
    net = {"network": "n.tsv", "network_threshold": 0.5, "network_limit": 10000000}
    assert scan.parse(argv + ["--network", "n.tsv"]) == dict(want, **net)      # --network brings its own three only
    cfg = scan.parse(argv + ["--consensus", "v.tsv"])
    assert cfg == dict(want, **dict(new, consensus="v.tsv", min_votes=3))
    for flag in ("--consensus", "--consensus-threshold", "--min-votes", "--consensus-limit"):
        assert flag in scan.USAGE and flag in scan.__doc__


# ------------------------------------------------------------------ the table
def test_consensus_rows_and_writer():
    from trigenicinteractionpredictor_amd import scan
    id_gene = {0: "YAL001C", 1: "YBR002W", 2: "YCL003C", 10: "YDR010W"}
    votes = np.array([3, 3, 2], dtype=np.int32)
    scores = np.array([0.75, 0.5, 0.875])
    ids = np.array([[0, 10, 2], [0, 1, 10], [1, 10, 2]], dtype=np.int32)
    rows = scan.consensus_rows(id_gene, votes, scores, ids)
    assert rows == [[1, 3, 0.75, "0_10_2", ["YAL001C", "YCL003C", "YDR010W"]],
                    [2, 3, 0.5, "0_1_10", ["YAL001C", "YBR002W", "YDR010W"]],
                    [3, 2, 0.875, "1_10_2", ["YBR002W", "YCL003C", "YDR010W"]]]
    out = io.StringIO()
    scan.write_consensus_tsv(3, 0.25, [1, 0, 1, 2], rows, out)
    assert out.getvalue() == ("# samples\t3\n"
                              "# threshold\t0.25\n"
                              "# votes\t3\t2\n"
                              "# votes\t2\t1\n"
                              "# votes\t1\t0\n"
                              "# votes\t0\t1\n"
                              "rank\tvotes\tprobability\tids\tnames\n"
                              "1\t3\t0.75\t0_10_2\tYAL001C_YCL003C_YDR010W\n"
                              "2\t3\t0.5\t0_1_10\tYAL001C_YBR002W_YDR010W\n"
                              "3\t2\t0.875\t1_10_2\tYBR002W_YCL003C_YDR010W\n")
    assert scan.consensus_rows(id_gene, votes[:0], scores[:0], ids[:0]) == []
    out = io.StringIO()
    scan.write_consensus_tsv(1, 1.0, [4, 0], [], out)
    assert out.getvalue() == ("# samples\t1\n# threshold\t1.0\n# votes\t1\t0\n# votes\t0\t4\n"
                              "rank\tvotes\tprobability\tids\tnames\n")
