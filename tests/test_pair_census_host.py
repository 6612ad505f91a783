"""Host side of the pair census (trigenicinteractionpredictor_amd/scan.py: pair_eligible, the
threshold chunking at the pair census's cap, the pair key spelling, the driver's new options and TSV
writers) and the numpy reference of tests/pair_census_ref.py against itself.  No GPU."""
import io
import os

import numpy as np
import pytest

import census_ref
import pair_census_ref as ref
import scan_ref
from golden_util import GOLDEN

TRAIN = os.path.join(GOLDEN, "tiny", "train.dat")
TEST = os.path.join(GOLDEN, "tiny", "test.dat")


def all_keys(P):
    return np.array([(a * P + b) * P + c for a in range(P) for b in range(a + 1, P) for c in range(b + 1, P)],
                    dtype=np.int64)


# ------------------------------------------------------------------ pair_eligible
@pytest.mark.parametrize("P", [1, 2, 3, 7, 12])
def test_pair_eligible_against_a_brute_force_loop(P):
    """P = 12 has a rank order that is no identity (0, 1, 10, 11, 2, ...)."""
    from trigenicinteractionpredictor_amd.scan import pair_eligible
    keys = all_keys(P)
    got = pair_eligible(P, None)
    assert got.dtype == np.int32 and got.shape == (P, P)
    np.testing.assert_array_equal(got, ref.eligible_brute(P))
    np.testing.assert_array_equal(got, max(P - 2, 0) * (1 - np.eye(P, dtype=np.int32)))
    np.testing.assert_array_equal(pair_eligible(P, np.zeros(0, np.int64)), got)
    if P < 3:
        return
    known = keys[::3].copy()
    got = pair_eligible(P, known)
    np.testing.assert_array_equal(got, ref.eligible_brute(P, known))
    assert (got == got.T).all() and not np.diag(got).any() and got.min() >= 0 and got.max() <= P - 2
    assert got.sum() == 2 * 3 * (keys.size - known.size)           # three pairs per triple, both ways
    # keys of no triple are ignored, as the kernels ignore them
    junk = np.sort(np.concatenate([known, [(1 * P + 1) * P + 2, (2 * P + 1) * P + 0, P ** 3 + 7]]))
    np.testing.assert_array_equal(pair_eligible(P, junk), got)
    np.testing.assert_array_equal(pair_eligible(P, keys), np.zeros((P, P), np.int32))


def test_reference_pairs_sum_to_three_times_the_census():
    th, pr = scan_ref.random_params(3, 13, 5)
    scores, keys = scan_ref.ref_scores(th[0], pr[0])
    thresholds = np.sort(census_ref.gap_thresholds(scores, 6))
    known = keys[::4].copy()
    for kn in (None, known):
        rank_mat, gene_mat = ref.ref_pairs(scores, keys, 13, thresholds, kn)
        counts, _ = census_ref.ref_census(scores, keys, thresholds, kn)
        assert not np.tril(rank_mat.transpose(2, 0, 1)).any()       # x < y only
        np.testing.assert_array_equal(rank_mat.sum(axis=(0, 1)), 3 * counts)
        np.testing.assert_array_equal(gene_mat, gene_mat.transpose(1, 0, 2))
        np.testing.assert_array_equal(gene_mat.sum(axis=1) // 2, ref.ref_gene_counts(scores, keys, 13, thresholds, kn))
    # below every score: every eligible triple
    from trigenicinteractionpredictor_amd.scan import pair_eligible
    np.testing.assert_array_equal(ref.ref_pairs(scores, keys, 13, [scores.min() / 2], known)[1][:, :, 0],
                                  pair_eligible(13, known))


# ------------------------------------------------------------------ chunking at the new cap
@pytest.mark.parametrize("n", [0, 1, 8, 9, 17, 25])
def test_threshold_chunks_at_the_pair_census_cap(n):
    from trigenicinteractionpredictor_amd.scan import MAX_PAIR_CENSUS_M, census_chunks, census_unsort
    assert MAX_PAIR_CENSUS_M == 8
    t = np.random.default_rng(n).random(n)
    if n > 2:
        t[2] = t[0]                                                 # a duplicate
    chunks, perm = census_chunks(t, MAX_PAIR_CENSUS_M)
    assert len(chunks) == max(1, -(-n // 8)) and all(c.size <= 8 for c in chunks)
    assert sum(c.size for c in chunks) == n
    np.testing.assert_array_equal(np.concatenate(chunks), np.sort(t))
    # per-chunk answers, put back in the caller's order
    scores = np.random.default_rng(1).random(50)
    parts = [[int((scores >= v).sum()) for v in c] for c in chunks]
    np.testing.assert_array_equal(census_unsort(parts, perm), [int((scores >= v).sum()) for v in t])
    with pytest.raises(ValueError):
        census_chunks([0.5, float("nan")], MAX_PAIR_CENSUS_M)


# ------------------------------------------------------------------ key spelling and tie order
def test_pair_key_spelling_and_tie_order_of_a_hand_made_matrix():
    from trigenicinteractionpredictor_amd.scan import pair_key, pair_rows, rank_order
    assert pair_key(2, 10) == "10_2" and pair_key(10, 2) == "10_2"  # string order, as `links` spells keys
    assert pair_key(3, 7) == "3_7" and pair_key(0, 11) == "0_11" and pair_key(9, 10) == "10_9"
    P = 12
    order = rank_order(P)                                           # 0 1 10 11 2 3 ...
    assert order[:5].tolist() == [0, 1, 10, 11, 2]
    mat = np.zeros((P, P), dtype=np.int32)                          # rank positions, x < y
    mat[2, 4] = 5        # genes 10, 2
    mat[0, 3] = 5        # genes 0, 11: a tie, the smaller key x P + y first
    mat[0, 1] = 2        # genes 0, 1
    mat[4, 5] = 9        # genes 2, 3
    counts, ids = ref.top_pairs(mat, 5)
    assert counts.tolist() == [9, 5, 5, 2, 0]
    assert ids.tolist() == [[2, 3], [0, 11], [10, 2], [0, 1], [0, 10]]   # the first zero pair: key 0 P + 2
    names = {g: "G%02d" % (P - g) for g in range(P)}                # names sort against the ids
    rows = pair_rows(names, counts, [10, 9, 8, 7, 6], ids)
    assert rows[0] == [9, 10, "2_3", ["G09", "G10"]]
    assert rows[1] == [5, 9, "0_11", ["G01", "G12"]]
    assert rows[2] == [5, 8, "10_2", ["G02", "G10"]]
    assert all(isinstance(r[0], int) and isinstance(r[1], int) for r in rows)
    counts, ids = ref.top_pairs(mat, 1000)                          # n above C(P, 2)
    assert counts.size == P * (P - 1) // 2 and ids.shape == (P * (P - 1) // 2, 2)


# ------------------------------------------------------------------ the TSV writers
def test_pairs_tsv():
    from trigenicinteractionpredictor_amd.scan import write_pairs_tsv
    buf = io.StringIO()
    write_pairs_tsv([[9, 10, "2_3", ["A", "B"]], [5, 9, "10_2", ["C", "D"]]], buf)
    assert buf.getvalue() == "rank\tcount\teligible\tids\tnames\n1\t9\t10\t2_3\tA_B\n2\t5\t9\t10_2\tC_D\n"
    buf = io.StringIO()
    write_pairs_tsv([], buf)
    assert buf.getvalue() == "rank\tcount\teligible\tids\tnames\n"


def test_gene_census_tsv():
    from trigenicinteractionpredictor_amd.scan import write_gene_census_tsv
    buf = io.StringIO()
    write_gene_census_tsv([0.5, 0.001], ["YAL001", "YBR002"], np.array([[0, 12], [3, 40]], dtype=np.int64), buf)
    assert buf.getvalue() == "gene\tname\t0.5\t0.001\n0\tYAL001\t0\t12\n1\tYBR002\t3\t40\n"


# ------------------------------------------------------------------ the driver's arguments
def test_driver_parses_the_pair_flags():
    from trigenicinteractionpredictor_amd import scan
    cfg = scan.parse(["-t", TRAIN, "-e", TEST, "-k", "3", "--pairs", "p.tsv", "--pair-threshold", "0.25",
                      "--gene-census", "g.tsv", "--thresholds", "0.5,0.1"])
    assert (cfg["pairs"], cfg["pair_threshold"], cfg["gene_census"]) == ("p.tsv", 0.25, "g.tsv")
    assert cfg["thresholds"] == [0.5, 0.1]
    assert scan.parse(["--pair-threshold", "1"])["pair_threshold"] == 1.0
    cfg = scan.parse(["-t", TRAIN, "--pairs", "p.tsv"])
    assert cfg["pairs"] == "p.tsv" and cfg["pair_threshold"] == 0.5 and cfg["gene_census"] is None


@pytest.mark.parametrize("value", ["0", "1.5", "-0.1", "nan", "inf", "x", ""])
def test_pair_threshold_must_lie_in_0_1(value, monkeypatch):
    import sys
    from trigenicinteractionpredictor_amd import scan
    # the engine module (torch + the HIP library) must not be needed to refuse an argument
    monkeypatch.setitem(sys.modules, "trigenicinteractionpredictor_amd.engine", None)
    assert scan.main(["-t", TRAIN, "--pairs", "p.tsv", "--pair-threshold", value]) == 2


def test_parse_of_nothing_keeps_every_old_key_and_value():
    """The values `parse([])` had before the pair census, key by key; the new options are off."""
    from trigenicinteractionpredictor_amd import cli, scan
    cfg = scan.parse([])
    old = dict(cli.DEFAULTS, samples=1, iterations=100, top=100, exclude=("train", "test"), best=False, out=None,
               seed=None, genes=[], all_genes=False, census=None, thresholds=None, heldout_ranks=None)
    for key, value in old.items():
        assert cfg[key] == value, key
    assert set(cfg) - set(old) == {"pairs", "pair_threshold", "gene_census"}
    assert cfg["pairs"] is None and cfg["gene_census"] is None and cfg["pair_threshold"] == 0.5
    assert "--pairs" in scan.USAGE and "--pair-threshold" in scan.USAGE and "--gene-census" in scan.USAGE
    assert "--pairs" in scan.__doc__ and "--gene-census" in scan.__doc__
