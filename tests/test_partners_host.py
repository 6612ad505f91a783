"""Host helpers of the partner scan (trigenicinteractionpredictor_amd/scan.py): the per-query table
of measured partner pairs, gene resolution and the driver's --gene / --all-genes arguments.  No GPU."""
import os

import numpy as np
import pytest

from golden_util import GOLDEN


def _model(fold):
    from trigenicinteractionpredictor_amd import Model
    m = Model()
    m.get_traintest(os.path.join(GOLDEN, fold, "train.dat"), os.path.join(GOLDEN, fold, "test.dat"))
    return m


def _brute(m, tables):
    """{gene id: set of pair keys b P + c} from the key strings alone: split, drop the keys with a
    repeated gene, rank by str sort, and file the other two positions under each gene."""
    P = m.P
    pos = {g: i for i, g in enumerate(sorted(str(g) for g in range(P)))}
    out = {g: set() for g in range(P)}
    repeated = 0
    for table in tables:
        for key in table.keys():
            parts = key.split("_")
            if len(set(parts)) < 3:
                repeated += 1
                continue
            for me in parts:
                b, c = sorted(pos[p] for p in parts if p != me)
                out[int(me)].add(b * P + c)
    return out, repeated


def _slices(off, pairs):
    return [pairs[off[i]:off[i + 1]] for i in range(off.size - 1)]


@pytest.mark.parametrize("fold", ["edge", "tiny"])
def test_partner_known_matches_a_brute_force_set(fold):
    from trigenicinteractionpredictor_amd.scan import partner_known, rank_order
    m = _model(fold)
    if fold == "edge":
        assert m.P > 10 and rank_order(m.P).tolist() != list(range(m.P))    # rank order != id order
    want, _ = _brute(m, (m.links, m.test_links))
    queries = list(range(m.P))
    off, pairs = partner_known(m, queries)
    assert off.dtype == np.int64 and pairs.dtype == np.int64
    assert off.shape == (m.P + 1,) and off[0] == 0 and off[-1] == pairs.size
    for g, sl in zip(queries, _slices(off, pairs)):
        assert (np.diff(sl) > 0).all()                      # sorted, unique
        assert set(sl.tolist()) == want[g], g
    # every measured triple of distinct genes is filed under each of its three genes
    union = set(m.links.keys()) | set(m.test_links.keys())
    assert pairs.size == 3 * sum(1 for k in union if len(set(k.split("_"))) == 3)
    # queries in another order, repeated: every row is its gene's slice
    q2 = queries[::-1] + queries[:3]
    off2, pairs2 = partner_known(m, q2)
    for g, sl in zip(q2, _slices(off2, pairs2)):
        assert set(sl.tolist()) == want[g]
    # the array form: (P, train ids, test ids)
    arrays = (m.P, m._link_arrays(0)[0], m._link_arrays(1)[0])
    off3, pairs3 = partner_known(arrays, queries)
    np.testing.assert_array_equal(off3, off)
    np.testing.assert_array_equal(pairs3, pairs)


def test_partner_known_honours_exclude():
    from trigenicinteractionpredictor_amd.scan import partner_known
    m = _model("tiny")
    queries = list(range(m.P))
    for exclude, tables in ((("train",), (m.links,)), (("test",), (m.test_links,)),
                            ("train,test", (m.links, m.test_links))):
        want, _ = _brute(m, tables)
        off, pairs = partner_known(m, queries, exclude=exclude)
        for g, sl in zip(queries, _slices(off, pairs)):
            assert set(sl.tolist()) == want[g]
    for none in ((), "none"):
        off, pairs = partner_known(m, queries, exclude=none)
        assert off.tolist() == [0] * (m.P + 1) and pairs.size == 0


def test_partner_known_ignores_triples_with_a_repeated_gene():
    from trigenicinteractionpredictor_amd.scan import partner_known
    m = _model("multi")
    want, repeated = _brute(m, (m.links, m.test_links))
    assert repeated == 18
    off, pairs = partner_known(m, list(range(m.P)))
    for g, sl in enumerate(_slices(off, pairs)):
        assert set(sl.tolist()) == want[g]
    # a hand-made table: 1_1_2 is no candidate of gene 1 or 2; 0_1_2 is filed under all three
    off, pairs = partner_known((4, np.array([[1, 1, 2], [0, 1, 2]]), None), [0, 1, 2, 3])
    assert [s.tolist() for s in _slices(off, pairs)] == [[1 * 4 + 2], [0 * 4 + 2], [0 * 4 + 1], []]


def test_a_query_without_a_known_triple_and_bad_queries():
    from trigenicinteractionpredictor_amd.scan import partner_known
    ids = np.array([[0, 2, 5], [2, 3, 5]])
    off, pairs = partner_known((7, ids, None), [4, 2, 6])
    assert off.tolist() == [0, 0, 2, 2]
    assert pairs.tolist() == [0 * 7 + 5, 3 * 7 + 5]
    off, pairs = partner_known((7, ids, None), [])
    assert off.tolist() == [0] and pairs.size == 0
    for bad in ([7], [-1], [0, 99]):
        with pytest.raises(IndexError):
            partner_known((7, ids, None), bad)


def test_resolve_genes_takes_ids_and_names():
    from trigenicinteractionpredictor_amd.scan import resolve_genes
    m = _model("tiny")
    name = m.id_gene[3]
    assert resolve_genes(m, ["3", name, 0, str(m.P - 1)]) == [3, 3, 0, m.P - 1]
    with pytest.raises(KeyError):
        resolve_genes(m, ["no-such-gene"])
    for bad in (str(m.P), "-1"):
        with pytest.raises(IndexError):
            resolve_genes(m, [bad])


def test_driver_parses_gene_options():
    from trigenicinteractionpredictor_amd import scan
    cfg = scan.parse(["--gene", "YAL001", "--gene", "4,7", "--top", "10"])
    assert cfg["genes"] == ["YAL001", "4", "7"] and cfg["all_genes"] is False and cfg["top"] == 10
    cfg = scan.parse(["--all-genes"])
    assert cfg["all_genes"] is True and cfg["genes"] == []
    cfg = scan.parse([])
    assert cfg["genes"] == [] and cfg["all_genes"] is False
    assert scan.parse(["--gene", "1"])["genes"] == ["1"]
    assert scan.parse(["--gene", "1"])["genes"] == ["1"]       # no state carried between calls


@pytest.mark.parametrize("argv", [
    ["--gene", "1", "--all-genes"], ["--gene", ""], ["--gene", "1,,2"], ["--gene"],
    ["--gene", "1", "--top", "1025"], ["--all-genes", "--top", "4096"], ["--all-genes", "--top", "0"],
])
def test_driver_gene_argument_errors(argv, monkeypatch):
    import sys
    from trigenicinteractionpredictor_amd import scan
    monkeypatch.setitem(sys.modules, "trigenicinteractionpredictor_amd.engine", None)
    assert scan.main(argv) == 2


@pytest.mark.parametrize("gene", ["no-such-gene", "40", "-1", "3,bogus"])
def test_driver_refuses_a_bad_gene_before_any_gpu_use(gene, monkeypatch, capsys):
    import sys
    from trigenicinteractionpredictor_amd import scan
    # the engine module (torch + the HIP library) must not be needed to refuse a gene
    monkeypatch.setitem(sys.modules, "trigenicinteractionpredictor_amd.engine", None)
    g = os.path.join(GOLDEN, "tiny")
    rc = scan.main(["-t", os.path.join(g, "train.dat"), "-e", os.path.join(g, "test.dat"), "-k", "3",
                    "--gene", gene])
    assert rc == 2
    assert "--gene" in capsys.readouterr().out


def test_partner_table_format():
    import io
    from trigenicinteractionpredictor_amd import scan
    buf = io.StringIO()
    scan.write_tsv([["YAL001", 1, 0.5, "1_2_3", ["YAL001", "YAL002", "YAL003"]]], buf, partners=True)
    assert buf.getvalue() == "query\trank\tprobability\tids\tnames\nYAL001\t1\t0.5\t1_2_3\tYAL001_YAL002_YAL003\n"
    buf = io.StringIO()
    scan.write_tsv([[1, 0.5, "1_2_3", ["YAL001", "YAL002", "YAL003"]]], buf)
    assert buf.getvalue() == "rank\tprobability\tids\tnames\n1\t0.5\t1_2_3\tYAL001_YAL002_YAL003\n"
