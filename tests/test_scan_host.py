"""Host helpers of the genome-wide scan (trigenicinteractionpredictor_amd/scan.py): the rank
order of the reference's string-sorted keys, packed keys, the known-key table and the driver's
argument checks.  No GPU."""
import itertools
import os

import numpy as np
import pytest

from golden_util import GOLDEN

FOLDS = ("tiny", "small", "multi")


def _model(fold):
    from trigenicinteractionpredictor_amd import Model
    m = Model()
    m.get_traintest(os.path.join(GOLDEN, fold, "train.dat"), os.path.join(GOLDEN, fold, "test.dat"))
    return m


def test_rank_order_sorts_ids_as_decimal_strings():
    from trigenicinteractionpredictor_amd.scan import rank_of, rank_order
    assert rank_order(12).tolist() == [0, 1, 10, 11, 2, 3, 4, 5, 6, 7, 8, 9]
    assert rank_order(12).dtype == np.int32
    for P in (0, 1, 9, 10, 101, 1500):
        order = rank_order(P)
        assert [str(g) for g in order] == sorted(str(g) for g in range(P))
        assert rank_of(order)[order].tolist() == list(range(P))


def test_pack_keys_increase_along_lexicographic_rank_triples():
    from trigenicinteractionpredictor_amd.scan import pack_keys, rank_of, rank_order
    P = 13
    order = rank_order(P)
    triples = np.array(list(itertools.combinations(range(P), 3)))     # lexicographic a < b < c
    keys = pack_keys(order[triples], rank_of(order), P)
    assert keys.dtype == np.int64
    assert (np.diff(keys) > 0).all()
    np.testing.assert_array_equal(keys, (triples[:, 0] * P + triples[:, 1]) * P + triples[:, 2])
    # a row given in another order packs to the same key
    np.testing.assert_array_equal(pack_keys(order[triples][:, ::-1], rank_of(order), P), keys)
    # no overflow at a genome-sized P
    big = pack_keys(np.array([[1999997, 1999998, 1999999]]), np.arange(2000000), 2000000)
    assert int(big[0]) == (1999997 * 2000000 + 1999998) * 2000000 + 1999999


def _independent_keys(m, tables):
    """Packed keys from the key strings alone: split, drop repeated genes, rank by str sort."""
    P = m.P
    pos = {g: i for i, g in enumerate(sorted((str(g) for g in range(P))))}
    out, repeated = set(), 0
    for table in tables:
        for key in table.keys():
            parts = key.split("_")
            if len(set(parts)) < 3:
                repeated += 1
                continue
            a, b, c = sorted(pos[p] for p in parts)
            out.add((a * P + b) * P + c)
    return out, repeated


@pytest.mark.parametrize("fold", FOLDS)
def test_known_keys_match_the_key_strings(fold):
    from trigenicinteractionpredictor_amd.scan import known_keys
    m = _model(fold)
    want, _ = _independent_keys(m, (m.links, m.test_links))
    got = known_keys(m)
    assert got.dtype == np.int64
    assert (np.diff(got) > 0).all()                 # sorted, unique
    assert set(got.tolist()) == want
    want_train, _ = _independent_keys(m, (m.links,))
    assert set(known_keys(m, exclude=("train",)).tolist()) == want_train
    assert known_keys(m, exclude=()).size == 0
    assert known_keys(m, exclude="none").size == 0
    # the array form: (P, train ids, test ids)
    arrays = (m.P, m._link_arrays(0)[0], m._link_arrays(1)[0])
    np.testing.assert_array_equal(known_keys(arrays), got)
    # every key of the fold is already in rank order (slot 1, 2, 3 = ascending rank)
    from trigenicinteractionpredictor_amd.scan import rank_of, rank_order
    pos = rank_of(rank_order(m.P))[np.concatenate(arrays[1:])]
    assert (np.diff(pos, axis=1) >= 0).all()


def test_known_keys_drop_the_repeated_gene_keys_of_multi():
    from trigenicinteractionpredictor_amd.scan import known_keys
    m = _model("multi")
    want, repeated = _independent_keys(m, (m.links, m.test_links))
    assert repeated == 18
    n_keys = len(set(m.links.keys()) | set(m.test_links.keys()))
    assert known_keys(m).size == len(want) == n_keys - 18


@pytest.mark.parametrize("argv", [
    ["--top", "0"], ["--top", "-3"], ["--top", "x"], ["--top", "4097"],
    ["--exclude", "validation"], ["--exclude", "train,foo"],
    ["-k", "33"], ["-k", "0"], ["-n", "0"], ["-i", "0"], ["-t", "/no/such/file"], ["--nope"],
])
def test_driver_argument_errors_come_before_any_gpu_use(argv, monkeypatch, capsys):
    import sys
    from trigenicinteractionpredictor_amd import scan
    # the engine module (torch + the HIP library) must not be needed to refuse an argument
    monkeypatch.setitem(sys.modules, "trigenicinteractionpredictor_amd.engine", None)
    assert scan.main(argv) == 2


def test_driver_parses_its_flags():
    from trigenicinteractionpredictor_amd import scan
    train = os.path.join(GOLDEN, "tiny", "train.dat")
    cfg = scan.parse(["-t", train, "-k", "3", "-n", "2", "-i", "5", "--seed", "1", "--top", "10",
                      "--exclude", "train", "--best", "-o", "x.tsv"])
    assert (cfg["train"], cfg["k"], cfg["samples"], cfg["iterations"]) == (train, 3, 2, 5)
    assert (cfg["seed"], cfg["top"], cfg["exclude"], cfg["best"], cfg["out"]) == (1, 10, ("train",), True, "x.tsv")
    assert scan.parse(["--exclude", "none"])["exclude"] == ()
    assert scan.parse([])["exclude"] == ("train", "test")


# ------------------------------------------------------------------ the engine's argument checks
@pytest.mark.parametrize("known,want", [(None, []), ([], []), ([7], [7]), ([3, 5, 9], [3, 5, 9]),
                                        (np.array([1, 2, 8], dtype=np.int32)[::-1][::-1], [1, 2, 8])],
                         ids=["none", "empty", "one", "sorted", "int32-view"])
def test_check_known_keys_returns_contiguous_int64(known, want):
    from trigenicinteractionpredictor_amd.scan import check_known_keys
    got = check_known_keys(known)
    assert got.dtype == np.int64 and got.flags["C_CONTIGUOUS"] and got.tolist() == want


@pytest.mark.parametrize("known", [[3, 3], [1, 4, 4, 9], [5, 3], [1, 2, 9, 8]],
                         ids=["duplicate", "duplicate-inside", "descent", "descent-at-the-end"])
def test_check_known_keys_refuses_unsorted_or_repeated_keys(known):
    from trigenicinteractionpredictor_amd.scan import check_known_keys
    with pytest.raises(ValueError, match=r"^known keys must be sorted and unique \(scan\.known_keys\)$"):
        check_known_keys(np.array(known, dtype=np.int64))


OFFSETS = "known offsets must be 3 non-decreasing indices into the pair keys (scan.partner_known)"
SLICES = "each query's known pair keys must be sorted and unique (scan.partner_known)"


@pytest.mark.parametrize("off,pairs,message", [
    ([0, 2], [4, 5], OFFSETS),                  # offsets of another Q
    ([0, 1, 2, 4], [4, 5, 7, 9], OFFSETS),
    ([-1, 2, 4], [4, 5, 7, 9], OFFSETS),        # a negative first offset
    ([0, 3, 2], [4, 5, 7, 9], OFFSETS),         # a decreasing offset
    ([0, 2, 5], [4, 5, 7, 9], OFFSETS),         # a last offset beyond the pairs
    ([0, 2, 4], [5, 4, 7, 9], SLICES),          # a descent inside the first slice
    ([0, 2, 4], [4, 5, 9, 7], SLICES),          # ... inside the last
    ([0, 2, 4], [4, 5, 9, 9], SLICES),          # a repeated key
    ([1, 3, 4], [0, 9, 4, 7], SLICES)],         # ... inside a slice that starts past the first pair
    ids=["short-offsets", "long-offsets", "negative-offset", "decreasing-offset", "offset-beyond-pairs",
         "descent-first-slice", "descent-last-slice", "repeat", "descent-offset-start"])
def test_check_partner_known_refuses(off, pairs, message):
    from trigenicinteractionpredictor_amd.scan import check_partner_known
    with pytest.raises(ValueError) as e:
        check_partner_known((np.array(off), np.array(pairs)), 2)
    assert str(e.value) == message


def test_check_partner_known_accepts_a_descent_at_a_slice_boundary():
    from trigenicinteractionpredictor_amd.scan import check_partner_known, partner_known
    off, pairs = check_partner_known(([0, 2, 4], np.array([4, 9, 5, 7], dtype=np.int32)), 2)
    assert off.dtype == pairs.dtype == np.int64 and off.tolist() == [0, 2, 4] and pairs.tolist() == [4, 9, 5, 7]
    for known in (([0, 0, 0], []), ([0, 0, 2], [3, 1][::-1]), ([2, 3, 4], [9, 8, 5, 1])):   # empty slices; pairs
        off, pairs = check_partner_known(known, 2)                                          # outside every slice
        assert off.flags["C_CONTIGUOUS"] and pairs.flags["C_CONTIGUOUS"]
    m = _model("tiny")
    queries = [5, 0, 5, m.P - 1]
    off, pairs = partner_known(m, queries)              # what the helper builds passes its own check
    got = check_partner_known((off, pairs), len(queries))
    assert got[0].tolist() == off.tolist() and got[1].tolist() == pairs.tolist() and pairs.size > 0
