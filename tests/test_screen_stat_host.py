"""Host side of the screen scan's statistics (no GPU): the header, the library and the ctypes
signatures agree; the numpy reference of tests/screen_stat_ref.py obeys the identities that define the
quorum score and the spread; the driver's --screen-quorum / --screen-disputed options."""
import os
import re
import sys

import numpy as np
import pytest

import screen_ref
import screen_stat_ref as ref
from golden_util import GOLDEN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(GOLDEN, "tiny", "train.dat")
TEST = os.path.join(GOLDEN, "tiny", "test.dat")
NEW = ("mmsbm_screen_stat_max_depth", "mmsbm_screen_stat_topn", "mmsbm_screen_stat_scores")


# ------------------------------------------------------------------ header, library, binding
def test_header_library_and_signatures_agree():
    from trigenicinteractionpredictor_amd import _lib, build
    text = open(os.path.join(REPO, "include", "mmsbm.h")).read()
    declared = dict(re.findall(r"^int (mmsbm_screen\w+)\s*\(([^;]*)\);", text, re.M))
    assert set(NEW) <= set(declared)
    for name in NEW:
        assert name in _lib.SIGNATURES
        args = [a for a in declared[name].split(",") if a.strip() != "void"]
        assert len(_lib.SIGNATURES[name][1]) == len(args), name
    assert re.search(r"^#define MMSBM_SCREEN_STAT_QUORUM 0$", text, re.M) and _lib.MMSBM_SCREEN_STAT_QUORUM == 0
    assert re.search(r"^#define MMSBM_SCREEN_STAT_SPREAD 1$", text, re.M) and _lib.MMSBM_SCREEN_STAT_SPREAD == 1
    # the stat entries are the plain entries with (stat, arg) in the sample's place
    top, rows = _lib.SIGNATURES["mmsbm_screen_stat_topn"][1], _lib.SIGNATURES["mmsbm_screen_stat_scores"][1]
    plain_top, plain_rows = _lib.SIGNATURES["mmsbm_screen_topn"][1], _lib.SIGNATURES["mmsbm_screen_scores"][1]
    assert top[:9] == plain_top[:9] and top[11:] == plain_top[10:] and len(top) == len(plain_top) + 1 == 18
    assert rows[:9] == plain_rows[:9] and rows[11:] == plain_rows[10:] and len(rows) == len(plain_rows) + 1 == 15
    build.build(verbose=False)
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.mmsbm_screen_stat_max_depth() == ref.MAX_DEPTH == 4
    assert lib.mmsbm_screen_stat_max_depth() == lib.mmsbm_scan_quorum_max_depth() == lib.mmsbm_scan_spread_max_trim() + 1


def test_the_engine_has_the_methods():
    from trigenicinteractionpredictor_amd.engine import EMEngine
    for name in ("screen_quorum_top", "screen_quorum_scores", "screen_spread_top", "screen_spread_scores"):
        assert callable(getattr(EMEngine, name)) and callable(getattr(EMEngine, name + "_async"))
    assert isinstance(EMEngine.screen_stat_max_depth, property)


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("ns,P,seed", [(1, 20, 0), (2, 33, 1), (3, 50, 2), (8, 64, 3), (9, 40, 4)])
def test_reference_identities(ns, P, seed):
    rng = np.random.default_rng(seed)
    rows = rng.random((ns, P))
    rows[:, rng.choice(P, 5, replace=False)] = rng.random(5)        # places where every slot agrees
    np.testing.assert_array_equal(ref.quorum(rows, 1), rows.max(axis=0))
    np.testing.assert_array_equal(ref.quorum(rows, ns), rows.min(axis=0))
    for m in range(1, ns + 1):
        q = ref.quorum(rows, m)
        assert (q[None] == rows).any(axis=0).all()                  # every value is one slot's word
        for T in (0.1, 0.5, 0.9, float(rows[0, 3]), float(q[7])):   # at least m votes exactly where q_m >= T
            np.testing.assert_array_equal(q >= T, (rows >= T).sum(axis=0) >= m)
    if ns >= 2:
        np.testing.assert_array_equal(ref.spread(rows, 0), rows.max(axis=0) - rows.min(axis=0))
        for t in range((ns - 2) // 2 + 1):
            d = ref.spread(rows, t)
            np.testing.assert_array_equal(d, ref.quorum(rows, 1 + t) - ref.quorum(rows, ns - t))
            assert (d >= 0).all() and not np.signbit(d).any()
        with pytest.raises(AssertionError):
            ref.spread(rows, (ns - 2) // 2 + 1)
    else:
        with pytest.raises(AssertionError):
            ref.spread(rows, 0)
    with pytest.raises(AssertionError):
        ref.quorum(rows, ns + 1)


def test_reference_legal_arguments():
    assert ref.legal_votes(1) == [1] and ref.legal_votes(8) == list(range(1, 9))
    assert ref.legal_votes(9) == [1, 2, 3, 4, 6, 7, 8, 9] and ref.legal_votes(12) == [1, 2, 3, 4, 9, 10, 11, 12]
    assert ref.legal_trims(1) == [] and ref.legal_trims(2) == [0] and ref.legal_trims(5) == [0, 1]
    assert ref.legal_trims(8) == [0, 1, 2, 3] and ref.legal_trims(12) == [0, 1, 2, 3]


def test_reference_list_is_value_descending_then_key():
    P, x, y = 30, 7, 19
    row = np.random.default_rng(5).random(P)
    row[[x, y, 3, 25]] = np.nan
    row[[4, 10, 22]] = 0.75             # a tie across the three regions: the smaller c first
    s, ids = ref.top_list(row, P, x, y, 40)
    assert s.size == P - 4 and (np.diff(s) <= 0).all() and ids.shape == (P - 4, 3)
    keys = screen_ref.row_keys(P, x, y)
    from scan_ref import packed
    got = packed(ids, P)
    at = np.flatnonzero(s == 0.75)
    assert got[at].tolist() == keys[[4, 10, 22]].tolist() == sorted(keys[[4, 10, 22]].tolist())
    s7, ids7 = ref.top_list(row, P, x, y, 7)
    assert s7.tolist() == s[:7].tolist() and ids7.tolist() == ids[:7].tolist()
    e = ref.top_list(np.full(P, np.nan), P, x, y, 5)
    assert e[0].size == 0 and e[1].shape == (0, 3)


# ------------------------------------------------------------------ the driver
def test_driver_parses_the_new_options():
    from trigenicinteractionpredictor_amd import scan
    cfg = scan.parse(["-t", TRAIN, "-n", "4", "--screen-quorum", "q.tsv", "--query-pairs", "p.txt"])
    assert (cfg["screen_quorum"], cfg["screen_votes"]) == ("q.tsv", 4)          # every restart
    assert (cfg["screen"], cfg["screen_top"], cfg["query_pairs"], cfg["screen_best"]) == (None, 20, "p.txt", None)
    assert "screen_disputed" not in cfg and "screen_trim" not in cfg
    cfg = scan.parse(["-t", TRAIN, "-n", "4", "--screen-disputed", "d.tsv", "--screen-best", "3"])
    assert (cfg["screen_disputed"], cfg["screen_trim"], cfg["screen_best"], cfg["screen"]) == ("d.tsv", 0, 3, None)
    assert "screen_quorum" not in cfg and "screen_votes" not in cfg
    # with --screen, and both at once
    cfg = scan.parse(["-t", TRAIN, "-n", "8", "--screen", "s.tsv", "--screen-top", "7", "--query-pairs", "p.txt",
                      "--screen-quorum", "q.tsv", "--screen-votes", "5", "--screen-disputed", "d.tsv", "--screen-trim",
                      "3", "--allow-genes", "a.txt", "--block-pairs", "b.txt", "--exclude", "train"])
    assert (cfg["screen"], cfg["screen_top"], cfg["screen_quorum"], cfg["screen_votes"], cfg["screen_disputed"],
            cfg["screen_trim"]) == ("s.tsv", 7, "q.tsv", 5, "d.tsv", 3)
    assert cfg["allow_genes"] == "a.txt" and cfg["block_pairs"] == "b.txt" and cfg["exclude"] == ("train",)
    # -n after the votes and the trim
    cfg = scan.parse(["-t", TRAIN, "--screen-quorum", "q.tsv", "--screen-votes", "3", "--screen-disputed", "d.tsv",
                      "--screen-trim", "1", "--query-pairs", "p.txt", "-n", "4"])
    assert (cfg["samples"], cfg["screen_votes"], cfg["screen_trim"]) == (4, 3, 1)
    # depth: 12 restarts take the four lowest and the four highest m, and trims up to 3
    for m in (1, 4, 9, 12):
        assert scan.parse(["-n", "12", "--screen-quorum", "q", "--screen-votes", str(m), "--query-pairs", "p"])
    for flag in ("--screen-quorum", "--screen-votes", "--screen-disputed", "--screen-trim"):
        assert flag in scan.USAGE and flag in scan.__doc__
    assert scan.MAX_SCREEN_STAT_DEPTH == ref.MAX_DEPTH


REFUSED = {
    "votes-0": ["-n", "4", "--screen-quorum", "q.tsv", "--screen-votes", "0", "--query-pairs", "p.txt"],
    "votes-above-n": ["-n", "4", "--screen-quorum", "q.tsv", "--screen-votes", "5", "--query-pairs", "p.txt"],
    "votes-above-n-late": ["--screen-quorum", "q.tsv", "--screen-votes", "3", "--query-pairs", "p.txt", "-n", "2"],
    "votes-text": ["-n", "4", "--screen-quorum", "q.tsv", "--screen-votes", "most", "--query-pairs", "p.txt"],
    "depth-5": ["-n", "12", "--screen-quorum", "q.tsv", "--screen-votes", "5", "--query-pairs", "p.txt"],
    "depth-5-from-below": ["-n", "12", "--screen-quorum", "q.tsv", "--screen-votes", "8", "--query-pairs", "p.txt"],
    "trim-negative": ["-n", "4", "--screen-disputed", "d.tsv", "--screen-trim", "-1", "--query-pairs", "p.txt"],
    "trim-leaves-one": ["-n", "4", "--screen-disputed", "d.tsv", "--screen-trim", "2", "--query-pairs", "p.txt"],
    "trim-leaves-one-odd": ["-n", "5", "--screen-disputed", "d.tsv", "--screen-trim", "2", "--query-pairs", "p.txt"],
    "trim-4": ["-n", "12", "--screen-disputed", "d.tsv", "--screen-trim", "4", "--query-pairs", "p.txt"],
    "trim-text": ["-n", "4", "--screen-disputed", "d.tsv", "--screen-trim", "some", "--query-pairs", "p.txt"],
    "disputed-one-restart": ["-n", "1", "--screen-disputed", "d.tsv", "--query-pairs", "p.txt"],
    "quorum-best": ["-n", "4", "--best", "--screen-quorum", "q.tsv", "--query-pairs", "p.txt"],
    "disputed-best": ["-n", "4", "--best", "--screen-disputed", "d.tsv", "--query-pairs", "p.txt"],
    "quorum-no-source": ["-n", "4", "--screen-quorum", "q.tsv"],
    "disputed-no-source": ["-n", "4", "--screen-disputed", "d.tsv"],
    "both-sources": ["-n", "4", "--screen-quorum", "q.tsv", "--query-pairs", "p.txt", "--screen-best", "3"],
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_the_driver_refuses_bad_options(name, monkeypatch):
    from trigenicinteractionpredictor_amd import cli, scan
    monkeypatch.setitem(sys.modules, "trigenicinteractionpredictor_amd.engine", None)    # refused before any GPU
    extra = REFUSED[name]
    with pytest.raises(cli.ArgError):
        scan.parse(["-t", TRAIN, "-e", TEST, "-k", "2", *extra])
    assert scan.main(["-t", TRAIN, "-e", TEST, "-k", "2", *extra]) == 2
    assert scan.main([*extra, "-t", TRAIN, "-e", TEST, "-k", "2"]) == 2


def test_a_bad_query_pairs_file_is_refused_for_the_new_tables_too(tmp_path, monkeypatch):
    from trigenicinteractionpredictor_amd import scan
    monkeypatch.setitem(sys.modules, "trigenicinteractionpredictor_amd.engine", None)
    base = ["-t", TRAIN, "-e", TEST, "-k", "2", "-n", "2", "--screen-quorum", str(tmp_path / "q.tsv"), "--query-pairs"]
    assert scan.main(base + [str(tmp_path / "missing.txt")]) == 2
    bad = tmp_path / "bad.txt"
    bad.write_text("3 3\n")
    assert scan.main(base + [str(bad)]) == 2
    assert not (tmp_path / "q.tsv").exists()


def test_screen_queries_serve_the_new_tables(tmp_path):
    from trigenicinteractionpredictor_amd import Model, scan
    m = Model()
    m.get_traintest(TRAIN, TEST)
    f = tmp_path / "q.txt"
    f.write_text("0\t2\n11 4\n")
    for flag in ("--screen-quorum", "--screen-disputed"):
        cfg = scan.parse(["-t", TRAIN, "-n", "2", flag, "x.tsv", "--query-pairs", str(f)])
        assert scan.screen_queries(m, cfg).tolist() == [[0, 2], [11, 4]]
        assert scan.screen_queries(m, scan.parse(["-t", TRAIN, "-n", "2", flag, "x.tsv", "--screen-best", "4"])) is None


def test_parse_without_the_new_options_is_unchanged():
    """cfg without a new option is what it was, with --screen too; with one it differs by that
    option's two keys (and, without --screen, by --screen's own four)."""
    from trigenicinteractionpredictor_amd import cli, scan
    old = dict(cli.DEFAULTS, samples=1, iterations=100, top=100, exclude=("train", "test"), best=False, out=None,
               seed=None, genes=[], all_genes=False, census=None, thresholds=None, heldout_ranks=None,
               pairs=None, pair_threshold=0.5, gene_census=None)
    assert scan.parse([]) == old
    argv = ["-t", TRAIN, "-e", TEST, "-k", "4", "-n", "3", "-i", "7", "--seed", "5", "--top", "77", "--exclude",
            "train", "-o", "o.tsv", "--census", "c.tsv", "--quorum", "qq.tsv", "--disputed", "dd.tsv", "--screen",
            "s.tsv", "--screen-best", "5"]
    want = scan.parse(argv)
    assert not [k for k in want if k in ("screen_quorum", "screen_votes", "screen_disputed", "screen_trim")]
    assert want["screen"] == "s.tsv" and want["quorum_votes"] == 3 and want["disputed_trim"] == 0
    cfg = scan.parse(argv + ["--screen-quorum", "q.tsv"])
    new = {"screen_quorum": "q.tsv", "screen_votes": 3}
    assert {k: v for k, v in cfg.items() if k not in new} == want and {k: cfg[k] for k in new} == new
    cfg = scan.parse(argv + ["--screen-disputed", "d.tsv", "--screen-trim", "0"])
    new = {"screen_disputed": "d.tsv", "screen_trim": 0}
    assert {k: v for k, v in cfg.items() if k not in new} == want and {k: cfg[k] for k in new} == new
    # without --screen: the query-pair keys come with the table
    plain = scan.parse(argv[:-4])
    cfg = scan.parse(argv[:-4] + ["--screen-quorum", "q.tsv", "--screen-best", "5"])
    new = {"screen_quorum": "q.tsv", "screen_votes": 3, "screen": None, "screen_top": 20, "query_pairs": None,
           "screen_best": 5}
    assert {k: v for k, v in cfg.items() if k not in new} == plain and {k: cfg[k] for k in new} == new


def test_screen_stat_rows_and_the_table():
    import io
    from trigenicinteractionpredictor_amd import scan

    class Eng:
        active = 2

        def predict(self, ids):
            assert ids.shape == (3, 3)
            return np.array([[0.5, 0.25, 0.75], [0.25, 0.75, 0.5], [np.nan] * 3])   # a third, inactive slot

    names = {0: "A", 1: "B", 2: "C", 10: "D"}
    lists = [(np.array([0.5, 0.25]), np.array([[0, 10, 2], [0, 1, 10]], dtype=np.int32)),
             (np.zeros(0), np.zeros((0, 3), np.int32)),
             (np.array([0.125]), np.array([[0, 1, 2]], dtype=np.int32))]
    rows = scan.screen_stat_rows(Eng(), names, [(10, 0), (1, 2), (2, 1)], lists)
    assert rows == [["A_D", 1, 0.5, 0.375, 0.25, 0.5, "0_10_2", ["A", "C", "D"]],
                    ["A_D", 2, 0.25, 0.5, 0.25, 0.75, "0_1_10", ["A", "B", "D"]],
                    ["B_C", 1, 0.125, 0.625, 0.5, 0.75, "0_1_2", ["A", "B", "C"]]]
    assert scan.screen_stat_rows(Eng(), names, [(1, 2)], lists[1:2]) == []
    for what, label in (("quorum", "votes"), ("spread", "trim")):
        f = io.StringIO()
        scan.write_screen_stat_tsv(2, 1, rows, f, what)
        lines = f.getvalue().split("\n")
        assert lines[:3] == ["# samples\t2", "# screen %s\t1" % label, "query\trank\t%s\tmean\tmin\tmax\tids\tnames" % what]
        assert lines[3] == "A_D\t1\t0.5\t0.375\t0.25\t0.5\t0_10_2\tA_C_D" and len(lines) == 7 and lines[6] == ""
