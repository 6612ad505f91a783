"""Host side of the partner scan's statistics (no GPU): the header, the library and the ctypes
signatures agree; the driver's --partners-quorum / --partners-disputed options; the ValueError paths
of EMEngine.partners_quorum_top / partners_spread_top that need no engine; and the gap preconditions
of tests/test_gpu_partners_stat.py's reference cases, asserted on the reference alone."""
import functools
import io
import os
import re
import sys

import numpy as np
import pytest

import partners_converged_ref as pc
import partners_stat_ref as ref
import scan_ref
from golden_util import GOLDEN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(GOLDEN, "tiny", "train.dat")
TEST = os.path.join(GOLDEN, "tiny", "test.dat")
NEW = ("mmsbm_partners_stat_max_depth", "mmsbm_partners_stat_topn")


# ------------------------------------------------------------------ header, library, binding
def test_header_library_and_signatures_agree():
    from trigenicinteractionpredictor_amd import _lib, build
    text = open(os.path.join(REPO, "include", "mmsbm.h")).read()
    declared = dict(re.findall(r"^int (mmsbm_partners\w+)\s*\(([^;]*)\);", text, re.M))
    assert set(NEW) <= set(declared)
    for name in NEW:
        assert name in _lib.SIGNATURES
        args = [a for a in declared[name].split(",") if a.strip() != "void"]
        assert len(_lib.SIGNATURES[name][1]) == len(args), name
    assert re.search(r"^#define MMSBM_PARTNERS_STAT_QUORUM 0$", text, re.M) and _lib.MMSBM_PARTNERS_STAT_QUORUM == 0
    assert re.search(r"^#define MMSBM_PARTNERS_STAT_SPREAD 1$", text, re.M) and _lib.MMSBM_PARTNERS_STAT_SPREAD == 1
    # the stat entry is the masked entry with (stat, arg) in the sample's place
    top, masked = _lib.SIGNATURES["mmsbm_partners_stat_topn"][1], _lib.SIGNATURES["mmsbm_partners_topn_masked"][1]
    assert top[:9] == masked[:9] and top[11:] == masked[10:] and len(top) == len(masked) + 1 == 18
    build.build(verbose=False)
    lib = _lib.load()
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.mmsbm_partners_stat_max_depth() == ref.MAX_DEPTH == 4
    assert lib.mmsbm_partners_stat_max_depth() == lib.mmsbm_screen_stat_max_depth() == lib.mmsbm_scan_quorum_max_depth()


def test_the_engine_has_the_methods():
    from trigenicinteractionpredictor_amd.engine import EMEngine
    for name in ("partners_quorum_top", "partners_spread_top"):
        assert callable(getattr(EMEngine, name)) and callable(getattr(EMEngine, name + "_async"))
    assert isinstance(EMEngine.partners_stat_max_depth, property)


@pytest.mark.parametrize("active", [1, 4, 12])
def test_out_of_range_arguments_raise_before_anything_is_uploaded(active):
    """The methods on an object that has no context, no device and no library: a ValueError comes
    before any of them is touched."""
    from trigenicinteractionpredictor_amd.engine import EMEngine
    fake = object.__new__(EMEngine)
    fake.active = active
    for m in (0, -1, active + 1):
        for f in (EMEngine.partners_quorum_top, EMEngine.partners_quorum_top_async):
            with pytest.raises(ValueError):
                f(fake, [0, 1], 8, m)
    bad_trims = (-1, max(0, (active - 2) // 2 + 1)) if active >= 2 else (0, 1, -1)
    for t in bad_trims:
        for f in (EMEngine.partners_spread_top, EMEngine.partners_spread_top_async):
            with pytest.raises(ValueError):
                f(fake, [0, 1], 8, t)
    # a legal argument passes the check and only then reaches for the engine
    with pytest.raises(AttributeError):
        EMEngine.partners_quorum_top(fake, [0, 1], 8, 1)
    with pytest.raises(AttributeError):
        EMEngine.partners_quorum_top(fake, [0, 1], 8)       # the default: every active slot


# ------------------------------------------------------------------ the driver
def test_driver_parses_the_new_options():
    from trigenicinteractionpredictor_amd import scan
    cfg = scan.parse(["-t", TRAIN, "-n", "4", "--gene", "7", "--partners-quorum", "q.tsv"])
    assert (cfg["partners_quorum"], cfg["partners_votes"], cfg["genes"]) == ("q.tsv", 4, ["7"])     # every restart
    assert "partners_disputed" not in cfg and "partners_trim" not in cfg
    cfg = scan.parse(["-t", TRAIN, "-n", "4", "--all-genes", "--partners-disputed", "d.tsv"])
    assert (cfg["partners_disputed"], cfg["partners_trim"], cfg["all_genes"]) == ("d.tsv", 0, True)
    assert "partners_quorum" not in cfg and "partners_votes" not in cfg
    cfg = scan.parse(["-t", TRAIN, "-n", "8", "--gene", "3,4", "--top", "1024", "--partners-quorum", "q.tsv",
                      "--partners-votes", "5", "--partners-disputed", "d.tsv", "--partners-trim", "3", "--exclude", "train"])
    assert (cfg["partners_quorum"], cfg["partners_votes"], cfg["partners_disputed"], cfg["partners_trim"],
            cfg["top"], cfg["exclude"]) == ("q.tsv", 5, "d.tsv", 3, 1024, ("train",))
    # -n after the votes and the trim
    cfg = scan.parse(["-t", TRAIN, "--gene", "1", "--partners-quorum", "q.tsv", "--partners-votes", "3",
                      "--partners-disputed", "d.tsv", "--partners-trim", "1", "-n", "4"])
    assert (cfg["samples"], cfg["partners_votes"], cfg["partners_trim"]) == (4, 3, 1)
    for m in (1, 4, 9, 12):     # depth: 12 restarts take the four lowest and the four highest m
        assert scan.parse(["-n", "12", "--gene", "1", "--partners-quorum", "q", "--partners-votes", str(m)])
    for flag in ("--partners-quorum", "--partners-votes", "--partners-disputed", "--partners-trim"):
        assert flag in scan.USAGE and flag in scan.__doc__
    assert scan.MAX_PARTNERS_STAT_DEPTH == ref.MAX_DEPTH


REFUSED = {
    "quorum-no-gene": ["-n", "4", "--partners-quorum", "q.tsv"],
    "disputed-no-gene": ["-n", "4", "--partners-disputed", "d.tsv"],
    "votes-0": ["-n", "4", "--gene", "7", "--partners-quorum", "q.tsv", "--partners-votes", "0"],
    "votes-above-n": ["-n", "4", "--gene", "7", "--partners-quorum", "q.tsv", "--partners-votes", "5"],
    "votes-above-n-late": ["--gene", "7", "--partners-quorum", "q.tsv", "--partners-votes", "3", "-n", "2"],
    "votes-text": ["-n", "4", "--gene", "7", "--partners-quorum", "q.tsv", "--partners-votes", "most"],
    "depth-5": ["-n", "12", "--gene", "7", "--partners-quorum", "q.tsv", "--partners-votes", "5"],
    "depth-5-from-below": ["-n", "12", "--gene", "7", "--partners-quorum", "q.tsv", "--partners-votes", "8"],
    "trim-negative": ["-n", "4", "--gene", "7", "--partners-disputed", "d.tsv", "--partners-trim", "-1"],
    "trim-leaves-one": ["-n", "4", "--gene", "7", "--partners-disputed", "d.tsv", "--partners-trim", "2"],
    "trim-leaves-one-odd": ["-n", "5", "--gene", "7", "--partners-disputed", "d.tsv", "--partners-trim", "2"],
    "trim-4": ["-n", "12", "--gene", "7", "--partners-disputed", "d.tsv", "--partners-trim", "4"],
    "trim-text": ["-n", "4", "--gene", "7", "--partners-disputed", "d.tsv", "--partners-trim", "some"],
    "disputed-one-restart": ["-n", "1", "--gene", "7", "--partners-disputed", "d.tsv"],
    "quorum-best": ["-n", "4", "--best", "--gene", "7", "--partners-quorum", "q.tsv"],
    "disputed-best": ["-n", "4", "--best", "--all-genes", "--partners-disputed", "d.tsv"],
    "top-above-the-cap": ["-n", "4", "--gene", "7", "--top", "1025", "--partners-quorum", "q.tsv"],
    "allow-genes": ["-n", "4", "--gene", "7", "--partners-quorum", "q.tsv", "--allow-genes", "a.txt"],
    "block-pairs": ["-n", "4", "--all-genes", "--partners-disputed", "d.tsv", "--block-pairs", "b.txt"],
    "unknown-gene": ["-n", "4", "--gene", "no-such-gene", "--partners-quorum", "q.tsv"],
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_the_driver_refuses_bad_options(name, monkeypatch, tmp_path):
    from trigenicinteractionpredictor_amd import cli, scan
    monkeypatch.setitem(sys.modules, "trigenicinteractionpredictor_amd.engine", None)    # refused before any GPU
    monkeypatch.chdir(tmp_path)
    extra = REFUSED[name]
    if name != "unknown-gene":      # that one is refused when the fold is read
        with pytest.raises(cli.ArgError):
            scan.parse(["-t", TRAIN, "-e", TEST, "-k", "2", *extra])
    assert scan.main(["-t", TRAIN, "-e", TEST, "-k", "2", *extra], out=lambda *a: None) == 2
    assert scan.main([*extra, "-t", TRAIN, "-e", TEST, "-k", "2"], out=lambda *a: None) == 2
    assert not os.listdir(tmp_path)         # nothing is written


def test_parse_without_the_new_options_is_unchanged():
    from trigenicinteractionpredictor_amd import cli, scan
    old = dict(cli.DEFAULTS, samples=1, iterations=100, top=100, exclude=("train", "test"), best=False, out=None,
               seed=None, genes=[], all_genes=False, census=None, thresholds=None, heldout_ranks=None,
               pairs=None, pair_threshold=0.5, gene_census=None)
    assert scan.parse([]) == old
    argv = ["-t", TRAIN, "-e", TEST, "-k", "4", "-n", "3", "-i", "7", "--seed", "5", "--top", "77", "--exclude",
            "train", "-o", "o.tsv", "--gene", "7"]
    want = scan.parse(argv)
    assert not [k for k in want if k.startswith("partners_")]
    cfg = scan.parse(argv + ["--partners-quorum", "q.tsv"])
    new = {"partners_quorum": "q.tsv", "partners_votes": 3}
    assert {k: v for k, v in cfg.items() if k not in new} == want and {k: cfg[k] for k in new} == new
    cfg = scan.parse(argv + ["--partners-disputed", "d.tsv", "--partners-trim", "0"])
    new = {"partners_disputed": "d.tsv", "partners_trim": 0}
    assert {k: v for k, v in cfg.items() if k not in new} == want and {k: cfg[k] for k in new} == new


def test_partner_rows_and_the_table():
    from trigenicinteractionpredictor_amd import scan
    names = {0: "A", 1: "B", 2: "C", 10: "D"}
    lists = [(np.array([0.5, 0.25]), np.array([[0, 10, 2], [0, 1, 10]], dtype=np.int32)),
             (np.zeros(0), np.zeros((0, 3), np.int32)),
             (np.array([0.125]), np.array([[0, 1, 2]], dtype=np.int32))]
    rows = scan.partner_rows(names, [10, 1, 2], lists)
    assert rows == [["D", 1, 0.5, "0_10_2", ["A", "C", "D"]], ["D", 2, 0.25, "0_1_10", ["A", "B", "D"]],
                    ["C", 1, 0.125, "0_1_2", ["A", "B", "C"]]]
    for what, label in (("quorum", "votes"), ("spread", "trim")):
        f = io.StringIO()
        scan.write_partners_stat_tsv(2, 1, rows, f, what)
        lines = f.getvalue().split("\n")
        assert lines[:3] == ["# samples\t2", "# partners %s\t1" % label, "query\trank\t%s\tids\tnames" % what]
        assert lines[3] == "D\t1\t0.5\t0_10_2\tA_C_D" and len(lines) == 7 and lines[6] == ""
    # below the comments the table is the --gene table with the statistic's name on the value column
    f, g = io.StringIO(), io.StringIO()
    scan.write_partners_stat_tsv(2, 1, rows, f, "quorum")
    scan.write_tsv(rows, g, partners=True)
    assert f.getvalue().split("\n")[3:] == g.getvalue().split("\n")[1:]


# ------------------------------------------------------------------ the reference
def test_reference_list_is_value_descending_then_key():
    P = 12
    rng = np.random.default_rng(3)
    th, pr = scan_ref.random_params(3, P, 1, 2)
    per, tk, pk = ref.ref_slots(th, pr, 5)
    assert per.shape == (2, (P - 1) * (P - 2) // 2) and np.unique(tk).size == tk.size
    v = ref.stat(per, "spread", 0)
    assert (v >= 0).all() and (v == per.max(axis=0) - per.min(axis=0)).all()
    v = rng.integers(0, 3, tk.size).astype(np.float64)          # many ties
    s, ids = ref.top_list(v, tk, P, 20)
    keys = scan_ref.packed(ids, P)
    assert (np.diff(s) <= 0).all() and all(keys[i] < keys[i + 1] for i in range(19) if s[i] == s[i + 1])
    keep = pk % 2 == 0
    s2, ids2 = ref.top_list(v, tk, P, 1000, keep)
    assert s2.size == int(keep.sum()) and set(scan_ref.packed(ids2, P).tolist()) == set(tk[keep].tolist())
    per2, keys2 = ref.from_slot_lists([ref.top_list(p, tk, P, 1024) for p in per], P)
    at = np.argsort(tk)
    assert keys2.tolist() == tk[at].tolist() and scan_ref.bits(per2) == scan_ref.bits(per[:, at])


def test_positions_cover_the_tiles():
    assert ref.positions(37) == [0, 15, 16, 17, 18, 35, 36]
    assert ref.positions(100) == [0, 15, 16, 17, 50, 98, 99]
    assert ref.positions(2) == [0, 1]


@functools.lru_cache(maxsize=None)
def case_slots(K, P, B, seed, q):
    th, pr = scan_ref.random_params(K, P, seed, B)
    return ref.ref_slots(th, pr, q)


@pytest.mark.parametrize("K,P,B,seed", ref.REF_CASES, ids=lambda v: str(v))
def test_reference_gaps(K, P, B, seed):
    """The precondition of the comparison with the independent reference, for every (case, query,
    argument, N) the GPU test runs: inside the reference's top N + 1 every adjacent relative gap of a
    quorum score exceeds 1e-9 and every adjacent absolute gap of a spread 1e-8 (spread_ref.SPREAD_GAP),
    so an error within the tolerance cannot reorder the list."""
    worst = {"quorum": np.inf, "spread": np.inf}
    for q in ref.positions(P):
        per, tk, _ = case_slots(K, P, B, seed, q)
        for what, arg in ref.stat_calls(B):
            v = ref.stat(per, what, arg)
            for n in ref.REF_NS:
                ok, gap = ref.gap_ok(v, what, n)
                assert ok, (q, what, arg, n, gap)
                worst[what] = min(worst[what], gap)
    assert worst["quorum"] > ref.QUORUM_GAP and worst["spread"] > ref.SPREAD_GAP


@pytest.mark.parametrize("K,P,B,seed", pc.LONG_CASES, ids=lambda v: str(v))
def test_long_lists_have_clear_cuts(K, P, B, seed):
    """The precondition of test_gpu_partners_stat.py's long lists, on the reference alone: for every
    query and every legal statistic N = 1024 is a clear cut (census_ref.GAP, relative for a quorum
    score, absolute for a spread), and so is 300 or a cut near below it; the candidates exceed what one
    workgroup's buffer and one slot's list hold."""
    c = pc.long_case(K, P, B, seed)
    assert len(c.refs) == 7 and all(r.tkeys.size == r.total == (P - 1) * (P - 2) // 2 > 4 * pc.FULL for r in c.refs)
    seen = set()
    for q, r in zip(c.positions, c.refs):
        for stat in ref.stat_calls(B):
            cuts = pc.long_cuts(r, stat)
            assert cuts[1] == pc.FULL
            seen.add(cuts)
        assert len(pc.chunks(r)) == -(-r.total // pc.FULL) == (5 if P == 100 else 44)
    print("K %d P %d B %d: N = %s" % (K, P, B, sorted(seen)))


def test_the_tie_case_ties_every_candidate():
    """test_gpu_partners_stat.py's total tie, on the reference alone: every statistic is one value for
    every candidate of a query, so its list is the N smallest triple keys; and a workgroup's buffer of
    512 entries cannot hold a query's candidates."""
    c = pc.tie_case()
    K, P, B = pc.TIE_SHAPE
    for r in c.refs:
        assert r.tkeys.size == 1711 > 512 >= 2 * max(pc.TIE_NS) and (np.diff(r.tkeys) > 0).all()
        for what, arg in ref.stat_calls(B):
            v = ref.stat(r.per, what, arg)
            assert np.unique(v).size == 1 and v[0] in (0.25, 0.5, 0.75)
            s, ids = ref.top_list(v, r.tkeys, P, 64)
            assert scan_ref.packed(ids, P).tolist() == r.tkeys[:64].tolist()
