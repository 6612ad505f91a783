"""Host side of the pair-masked scans (no GPU): scan.pair_mask against the per-bit packer of
tests/masked_ref.py, its three sources and errors, check_pair_mask, the reference's own expand,
bracket_threshold from hi = 1.0 as the masked scan_top_any uses it, and the driver's flags."""
import itertools
import os
import sys

import numpy as np
import pytest

import masked_ref
import scan_ref
from golden_util import GOLDEN

TRAIN = os.path.join(GOLDEN, "tiny", "train.dat")
TEST = os.path.join(GOLDEN, "tiny", "test.dat")
SIZES = [13, 31, 32, 33, 70]     # below, at and above a word; 70: three words, a halfword row end


# ------------------------------------------------------------------ pair_mask
@pytest.mark.parametrize("P", SIZES)
def test_pair_mask_shape_and_layout(P):
    from trigenicinteractionpredictor_amd import scan
    P16, MW = masked_ref.shape(P)
    assert scan.pair_mask_shape(P) == (P16, MW)
    assert P16 % 16 == 0 and P16 >= max(P, 16) and P16 - P < 16 or P < 16
    empty = scan.pair_mask(P)
    assert empty.dtype == np.uint32 and empty.shape == (P16, MW) and empty.flags.c_contiguous
    assert not empty.any()


@pytest.mark.parametrize("P", SIZES)
def test_pairs_against_the_naive_packer(P):
    """Pairs of gene ids, ids >= 10 among them (rank order differs from id order from P = 11 on),
    the last id and bits on both sides of every word and halfword boundary of the row."""
    from trigenicinteractionpredictor_amd import scan
    order, rank = scan_ref.rank_tables(P)
    assert P < 11 or (order != np.arange(P)).any()
    rng = np.random.default_rng(P)
    pairs = [(int(i), int(j)) for i, j in rng.integers(0, P, (4 * P, 2)) if i != j]
    # the genes AT the positions around every halfword boundary, paired with position 0's gene
    for y in (15, 16, 17, 31, 32, 33, 47, 48, 63, 64, 65, P - 1):
        if 0 < y < P:
            pairs.append((int(order[0]), int(order[y])))
            pairs.append((int(order[y]), int(order[y - 1])))
    pairs.append((P - 1, 10 if P > 11 else 0))
    got = scan.pair_mask(P, pairs=np.array(pairs))
    want = masked_ref.naive_from_ids(P, pairs)
    np.testing.assert_array_equal(got, want)
    # set on both sides, nothing on the diagonal, nothing at or past P
    for i, j in pairs[:10]:
        x, y = np.array([rank[i]]), np.array([rank[j]])
        assert masked_ref.bit(got, x, y)[0] == 1 and masked_ref.bit(got, y, x)[0] == 1
    d = np.arange(P)
    assert not masked_ref.bit(got, d, d).any()
    assert not got[P:].any()
    assert not any(masked_ref.bit(got, d, np.full(P, y)).any() for y in range(P, 32 * masked_ref.shape(P)[1]))


@pytest.mark.parametrize("P", SIZES)
def test_genes_and_matrix_against_the_naive_packer(P):
    from trigenicinteractionpredictor_amd import scan
    rng = np.random.default_rng(100 + P)
    genes = sorted(int(g) for g in rng.permutation(P)[:max(P // 3, 3)])
    np.testing.assert_array_equal(scan.pair_mask(P, genes=genes), masked_ref.naive_from_ids(P, genes=genes))
    matrix = np.triu(rng.random((P, P)) < 0.1, 1)       # one side only: either side blocks
    matrix[P - 1, 0] = True                             # and the lower side
    np.fill_diagonal(matrix, True)                      # the diagonal is ignored
    np.testing.assert_array_equal(scan.pair_mask(P, matrix=matrix), masked_ref.naive_from_ids(P, matrix=matrix))
    # every gene allowed blocks nothing; none allowed blocks every pair
    assert not scan.pair_mask(P, genes=range(P)).any()
    np.testing.assert_array_equal(scan.pair_mask(P, genes=[]), masked_ref.full_mask(P))


def test_the_three_sources_combine_by_or():
    from trigenicinteractionpredictor_amd import scan
    P = 33
    rng = np.random.default_rng(5)
    pairs = [(1, 12), (30, 2), (32, 31)]
    genes = [g for g in range(P) if g % 5]
    matrix = rng.random((P, P)) < 0.05
    each = [scan.pair_mask(P, pairs=pairs), scan.pair_mask(P, genes=genes), scan.pair_mask(P, matrix=matrix)]
    both = scan.pair_mask(P, pairs=pairs, genes=genes, matrix=matrix)
    np.testing.assert_array_equal(both, each[0] | each[1] | each[2])
    np.testing.assert_array_equal(both, masked_ref.naive_from_ids(P, pairs, genes, matrix))
    assert all((both != e).any() for e in each)         # each source adds something


@pytest.mark.parametrize("kw", [dict(pairs=[(0, 13)]), dict(pairs=[(-1, 2)]), dict(pairs=[(4, 4)]),
                                dict(genes=[0, 13]), dict(genes=[-1]), dict(matrix=np.zeros((12, 13), bool)),
                                dict(pairs=[(0.5, 2.0)])])
def test_pair_mask_value_errors(kw):
    from trigenicinteractionpredictor_amd import scan
    with pytest.raises(ValueError):
        scan.pair_mask(13, **kw)


def test_pair_mask_cap():
    from trigenicinteractionpredictor_amd import scan
    assert scan.MAX_MASK_P == 16384 and scan.pair_mask_shape(16384) == (16384, 512)
    with pytest.raises(ValueError):
        scan.pair_mask_shape(16385)


def test_check_pair_mask():
    from trigenicinteractionpredictor_amd import scan
    P = 33
    m = scan.pair_mask(P, pairs=[(1, 2)])
    assert scan.check_pair_mask(m, P) is m
    for bad in (m.astype(np.int32), m.astype(np.uint64), m[:-1], m[:, :1], np.asfortranarray(m), m.tolist(),
                np.zeros((64, 2), np.uint32)[::2], scan.pair_mask(70)):
        with pytest.raises(ValueError):
            scan.check_pair_mask(bad, P)


# ------------------------------------------------------------------ the reference itself
def test_expand_against_a_triple_loop():
    P = 13
    mask = masked_ref.random_mask(P, 0.15, seed=3)
    want = []
    for a, b, c in itertools.combinations(range(P), 3):
        hit = False
        for x, y in ((a, b), (a, c), (b, c)):
            hit |= bool((int(mask[x, y >> 5]) >> (y & 31)) & 1)
        if hit:
            want.append((a * P + b) * P + c)
    got = masked_ref.expand(mask, P)
    assert 0 < len(want) < 286
    np.testing.assert_array_equal(got, np.array(want, dtype=np.int64))
    assert masked_ref.expand(masked_ref.full_mask(P), P).size == 286
    assert masked_ref.expand(masked_ref.naive_mask(P, []), P).size == 0
    assert masked_ref.expand(masked_ref.single_pair_mask(P), P).size == P - 2


def test_the_shared_masks_block_what_the_issue_counted():
    """The figures the masks were chosen for, at P = 70 (54,740 triples): about a tenth of the pairs
    blocks between a fifth and a third of the triples, a third of the genes leaves C(24, 3)."""
    P = 70
    keys = masked_ref.all_keys(P)
    assert keys.size == 54740
    n = int(masked_ref.blocked(keys, masked_ref.random_mask(P), P).sum())
    assert 0.2 * keys.size < n < 0.35 * keys.size
    assert keys.size - int(masked_ref.blocked(keys, masked_ref.allowed_mask(P), P).sum()) == 24 * 23 * 22 // 6
    assert int(masked_ref.blocked(keys, masked_ref.block_mask(P), P).sum()) == 13568
    assert int(masked_ref.blocked(keys, masked_ref.full_mask(P), P).sum()) == keys.size
    last = masked_ref.blocked(keys, masked_ref.last_tile_mask(P), P)
    assert last.any() and (keys[last] % P >= 64).all()


# ------------------------------------------------------------------ bracket_threshold from 1.0
class Census:
    def __init__(self, scores):
        self.s = np.sort(np.asarray(scores, dtype=np.float64))
        self.passes = 0

    def __call__(self, thresholds):
        self.passes += 1
        t = np.asarray(thresholds, dtype=np.float64).reshape(-1)
        return (self.s.size - np.searchsorted(self.s, t, side="left")).astype(np.int64)


@pytest.mark.parametrize("n", [1, 64, 5000, 100000, 100001, 250000])
def test_bracket_from_one_on_a_fixed_score_array(n):
    """What the masked scan_top_any does: hi = 1.0, which no score reaches.  The cut holds at least
    min(n, total) rows and at most the slack above n; n above the total returns 0.0: everything."""
    from trigenicinteractionpredictor_amd.scan import bracket_threshold
    scores = np.random.default_rng(8).random(100000) ** 4 * 0.98
    c = Census(scores)
    lo = bracket_threshold(n, 1.0, c)
    count = int((scores >= lo).sum())
    assert count >= min(n, scores.size) and c.passes <= 8
    if n >= scores.size:
        assert lo == 0.0 and count == scores.size and c.passes == 1
    else:
        assert count <= n + max(n // 8, 4096)


# ------------------------------------------------------------------ the driver's flags
def test_driver_parses_the_mask_flags():
    from trigenicinteractionpredictor_amd import scan
    cfg = scan.parse(["-t", TRAIN, "--allow-genes", "a.txt", "--block-pairs", "b.txt", "--census", "c.tsv",
                      "--network", "n.tsv"])
    assert (cfg["allow_genes"], cfg["block_pairs"]) == ("a.txt", "b.txt")
    cfg = scan.parse(["--allow-genes", "a.txt"])
    assert (cfg["allow_genes"], cfg["block_pairs"]) == ("a.txt", None)
    cfg = scan.parse(["--block-pairs", "b.txt", "--heldout-ranks", "h.tsv", "-e", TEST])
    assert (cfg["allow_genes"], cfg["block_pairs"]) == (None, "b.txt")


@pytest.mark.parametrize("other", [["--gene", "3"], ["--all-genes"], ["--pairs", "p.tsv"], ["--gene-census", "g.tsv"],
                                   ["--consensus", "c.tsv", "-n", "2"], ["--quorum", "q.tsv", "-n", "2"]])
@pytest.mark.parametrize("flag", ["--allow-genes", "--block-pairs"])
def test_the_mask_flags_are_refused_with_the_unmasked_families(flag, other, monkeypatch, capsys):
    from trigenicinteractionpredictor_amd import scan
    monkeypatch.setitem(sys.modules, "trigenicinteractionpredictor_amd.engine", None)
    assert scan.main(["-t", TRAIN, flag, "f.txt", *other]) == 2
    assert scan.main(["-t", TRAIN, *other, flag, "f.txt"]) == 2        # in either order
    assert other[0] in capsys.readouterr().out


def test_a_bad_mask_file_is_refused_with_exit_2(tmp_path, monkeypatch):
    from trigenicinteractionpredictor_amd import scan
    monkeypatch.setitem(sys.modules, "trigenicinteractionpredictor_amd.engine", None)
    base = ["-t", TRAIN, "-e", TEST, "-k", "2"]
    assert scan.main(base + ["--allow-genes", str(tmp_path / "missing.txt")]) == 2
    bad = tmp_path / "bad.txt"
    bad.write_text("no_such_gene_name\n")
    assert scan.main(base + ["--allow-genes", str(bad)]) == 2
    bad.write_text("0 1 2\n")
    assert scan.main(base + ["--block-pairs", str(bad)]) == 2
    bad.write_text("3 3\n")
    assert scan.main(base + ["--block-pairs", str(bad)]) == 2
    bad.write_text("0 99999\n")
    assert scan.main(base + ["--block-pairs", str(bad)]) == 2


def test_driver_mask_from_files(tmp_path):
    """Names and ids, tabs and spaces, comments and blank lines -> the mask of those genes."""
    from trigenicinteractionpredictor_amd import Model, scan
    m = Model()
    m.get_traintest(TRAIN, TEST)
    allow = tmp_path / "allow.txt"
    genes = list(range(0, m.P, 2))
    allow.write_text("# the array\n" + "\n".join(m.id_gene[g] if g % 4 else str(g) for g in genes) + "\n\n")
    block = tmp_path / "block.txt"
    block.write_text("0\t2\n%s %s\n" % (m.id_gene[4], m.id_gene[10]))
    cfg = scan.parse(["-t", TRAIN, "--allow-genes", str(allow), "--block-pairs", str(block)])
    got = scan.driver_mask(m, cfg)
    np.testing.assert_array_equal(got, masked_ref.naive_from_ids(m.P, [(0, 2), (4, 10)], genes))
    np.testing.assert_array_equal(m.pair_mask(genes=[m.id_gene[g] for g in genes], pairs=[(0, "2"), (4, m.id_gene[10])]),
                                  got)
    assert scan.driver_mask(m, scan.parse(["-t", TRAIN])) is None


def test_parse_without_the_new_flags_is_unchanged():
    """cfg without --allow-genes / --block-pairs is what it was; with them it differs by their two
    keys alone."""
    from trigenicinteractionpredictor_amd import cli, scan
    old = dict(cli.DEFAULTS, samples=1, iterations=100, top=100, exclude=("train", "test"), best=False, out=None,
               seed=None, genes=[], all_genes=False, census=None, thresholds=None, heldout_ranks=None,
               pairs=None, pair_threshold=0.5, gene_census=None)
    assert scan.parse([]) == old
    argv = ["-t", TRAIN, "-e", TEST, "-k", "4", "-n", "3", "-i", "7", "--seed", "5", "--top", "77", "--exclude",
            "train", "--best", "-o", "o.tsv", "--census", "c.tsv", "--thresholds", "0.5,0.1", "--heldout-ranks",
            "h.tsv", "--network", "n.tsv"]
    want = scan.parse(argv)
    assert "allow_genes" not in want and "block_pairs" not in want
    cfg = scan.parse(argv + ["--allow-genes", "a.txt"])
    new = {"allow_genes": "a.txt", "block_pairs": None}
    assert {k: v for k, v in cfg.items() if k not in new} == want and {k: cfg[k] for k in new} == new
    for flag in ("--allow-genes", "--block-pairs"):
        assert flag in scan.USAGE and flag in scan.__doc__


def test_the_bindings_list_the_new_symbols():
    from trigenicinteractionpredictor_amd import _lib
    for name in ("mmsbm_pair_mask_shape", "mmsbm_scan_census_masked", "mmsbm_scan_above_masked"):
        assert name in _lib.SIGNATURES
    # the masked entries take the unmasked ones' arguments with the mask behind n_known
    for masked, plain in (("mmsbm_scan_census_masked", "mmsbm_scan_census"),
                          ("mmsbm_scan_above_masked", "mmsbm_scan_above")):
        res, args = _lib.SIGNATURES[masked]
        res0, args0 = _lib.SIGNATURES[plain]
        assert res == res0 and args[:4] == args0[:4] and args[5:] == args0[4:]
