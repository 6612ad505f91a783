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
