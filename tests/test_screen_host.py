"""Host side of the screen scan (no GPU): the numpy reference of tests/screen_ref.py against the
all-triples scorer, scan.screen_known against a walk of the link tables, check_screen_known, and the
driver's --screen options."""
import os
import sys

import numpy as np
import pytest

import scan_ref
import screen_ref as ref
from golden_util import GOLDEN

TRAIN = os.path.join(GOLDEN, "tiny", "train.dat")
TEST = os.path.join(GOLDEN, "tiny", "test.dat")


# ------------------------------------------------------------------ the reference
@pytest.mark.parametrize("K,P,seed", [(3, 37, 11), (10, 50, 5), (2, 18, 4)])
def test_reference_rows_are_the_all_triples_scores(K, P, seed):
    th, pr = scan_ref.random_params(K, P, seed)
    scores, keys = scan_ref.ref_scores(th[0], pr[0])
    rng = np.random.default_rng(seed)
    queries = [(0, 1), (0, P - 1), (P - 2, P - 1), (15, 16), (7, 30 % P)] + \
        [tuple(sorted(rng.choice(P, 2, replace=False))) for _ in range(10)]
    for x, y in queries:
        x, y = int(min(x, y)), int(max(x, y))
        row, rk = ref.ref_row(th[0], pr[0], x, y), ref.row_keys(P, x, y)
        c = np.array([c for c in range(P) if c not in (x, y)])
        assert np.isnan(row[[x, y]]).all() and not np.isnan(row[c]).any()
        assert (np.diff(rk[c]) > 0).all()                    # the key rises with c across the regions
        at = np.searchsorted(keys, rk[c])
        np.testing.assert_array_equal(keys[at], rk[c])
        np.testing.assert_allclose(row[c], scores[at], rtol=1e-12, atol=0)


def test_reference_eligibility_with_a_mask():
    import masked_ref
    P = 40
    mask = masked_ref.naive_mask(P, [(3, 9), (9, 20), (5, 6)])
    assert not ref.eligible(P, 5, 6, mask=mask).any()                  # the query's own pair
    ok = ref.eligible(P, 3, 20, [7, 3, 50], mask)
    assert sorted(np.flatnonzero(~ok).tolist()) == [3, 7, 9, 20]       # x, a known third, (3, 9) and (9, 20), y


# ------------------------------------------------------------------ the designed rows of the wide tests
def test_designed_places_are_permutations_in_the_intended_order():
    for P in (600, ref.WIDE_P, ref.OVERFLOW_P):
        for order in ref.ORDERS:
            place = ref.designed_places(P, order)
            np.testing.assert_array_equal(np.sort(place), np.arange(P))
        assert (np.diff(ref.designed_places(P, "ascending")) == 1).all()
        assert (np.diff(ref.designed_places(P, "descending")) == -1).all()
        saw = ref.designed_places(P, "sawtooth")
        for r in range(0, P, ref.ROUND):                # every round rises from the bottom of the grid to its top
            part = saw[r:r + ref.ROUND]
            rounds = (P + ref.ROUND - 1) // ref.ROUND
            assert (np.diff(part) > 0).all() and part[0] < rounds
            assert part.size < ref.ROUND or part[-1] >= P - 2 * rounds
        assert not np.array_equal(ref.designed_places(P, "shuffled"), ref.designed_places(P, "shuffled", 1))


@pytest.mark.parametrize("P,order,B", sorted({(P, order, B) for P, _, order, B in ref.DESIGNED}))
def test_designed_rows_have_the_intended_order_and_clear_gaps(P, order, B):
    """Per region the reference row is in the order of the places, and inside the top N + 1 of every
    N the GPU tests ask, every adjacent relative gap exceeds 1e-9 (check_list's own assertion): for
    the slots and for the ensemble."""
    th, pr, place = ref.designed_params(P, order, B)
    assert th.shape == (B, P, 2) and np.allclose(th.sum(axis=2), 1) and (pr > 0).all() and np.allclose(pr.sum(axis=4), 1)
    Ns = [N for p, N, o, b in ref.DESIGNED if (p, o, b) == (P, order, B)]
    for sample in list(range(B)) + ([None] if B > 1 else []):
        for x, y in ref.three_queries(P):
            row = ref.ref_rows(th, pr, x, y, sample)
            ref.check_designed(row, place, P, x, y)
            for N in Ns:
                s, ids, gap = ref.want_list(row, P, x, y, N)
                assert s.size == min(N, P - 2) and gap > 1e-9, (sample, (x, y), N, gap)
    x, y = ref.three_queries(P)[2]                      # the regions differ: one vector for all three fails
    row = ref.ref_row(th[0], pr[0], x, y)
    t = th[0][scan_ref.rank_tables(P)[0], 0]
    fit = [np.polyfit(t[c], row[c], 1) for c in ref.regions(P, x, y)]
    assert all(abs(a[0] - b[0]) > 0.03 for a, b in zip(fit, fit[1:]))
    assert all(f[0] > 0.05 for f in fit)


@pytest.mark.parametrize("P,N", ref.LATE)
def test_a_late_row_holds_its_nth_best_last(P, N):
    """The order "late:N": for the query (0, 1) the last position is the N-th best of the row, every
    other eligible position descends, and it is read in a round past the buffer's first overflow."""
    th, pr, place = ref.designed_params(P, "late:%d" % N)
    np.testing.assert_array_equal(np.sort(place), np.arange(P))
    row = ref.ref_row(th[0], pr[0], 0, 1)
    assert (np.diff(row[2:P - 1]) < 0).all()
    assert int((row[2:] > row[P - 1]).sum()) == N - 1
    assert (P - 1) // ref.ROUND > ref.cap_of(N) // ref.ROUND


def test_the_stride_row_is_designed_too():
    P = ref.STRIDE_P
    th, pr, place = ref.designed_params(P, "shuffled")
    for x, y in [(0, 1), (262150, 262170)]:
        row = ref.ref_row(th[0], pr[0], x, y)
        ref.check_designed(row, place, P, x, y)
        assert ref.want_list(row, P, x, y, 8)[2] > 1e-9


def test_the_cap_rule_matches_the_documented_cap_of_n():
    """cap = 512, doubled until it holds 2 N; N is capped at mmsbm_screen_max_n() = 1024, so the
    buffer is at most 2048 entries and the shapes above overflow it or not as they say."""
    from trigenicinteractionpredictor_amd import _lib
    assert _lib.load().mmsbm_screen_max_n() == 1024 == max(ref.WIDE_NS)
    assert [ref.cap_of(n) for n in (1, 8, 100, 255, 256, 257, 512, 513, 1024)] == \
        [512, 512, 512, 512, 512, 1024, 1024, 2048, 2048]
    # the arrival-order rows overflow every buffer but the largest, which the rows of OVERFLOW_P overflow
    assert ref.cap_of(512) == 1024 < ref.WIDE_P - 2 < ref.cap_of(513) == ref.cap_of(1024) < ref.OVERFLOW_P - 2
    assert ref.STRIDE_P > 4096 * 4 * 16


def test_check_list_rejects_a_swap_and_a_replaced_entry():
    P, N = ref.WIDE_P, 256
    th, pr, _ = ref.designed_params(P, "shuffled")
    x, y = ref.three_queries(P)[2]
    row = ref.ref_row(th[0], pr[0], x, y)
    full_s, full_ids, _ = ref.want_list(row, P, x, y, N + 1)
    s, ids = full_s[:N].copy(), full_ids[:N].copy()
    ref.check_list((s, ids), row, P, x, y, N)
    for at in (0, 100, N - 2):                          # two adjacent entries swapped
        s2, ids2 = s.copy(), ids.copy()
        s2[[at, at + 1]], ids2[[at, at + 1]] = s[[at + 1, at]], ids[[at + 1, at]]
        with pytest.raises(AssertionError):
            ref.check_list((s2, ids2), row, P, x, y, N)
    for at in (0, 100, N - 1):                          # an entry replaced by the (N + 1)-th
        s2, ids2 = s.copy(), ids.copy()
        s2[at], ids2[at] = full_s[N], full_ids[N]
        with pytest.raises(AssertionError):
            ref.check_list((s2, ids2), row, P, x, y, N)
    with pytest.raises(AssertionError):                 # the N-th dropped: a list one short
        ref.check_list((s[:-1], ids[:-1]), row, P, x, y, N)


# ------------------------------------------------------------------ screen_known
def brute_known(m, pairs, exclude):
    _, rank = scan_ref.rank_tables(m.P)
    tables = [m.links if name == "train" else m.test_links for name in exclude]
    out = []
    for g1, g2 in pairs:
        thirds = set()
        for table in tables:
            for key in table:
                ids = [int(t) for t in key.split("_")]
                if len(set(ids)) == 3 and g1 in ids and g2 in ids:
                    (t,) = [g for g in ids if g not in (g1, g2)]
                    thirds.add(int(rank[t]))
        out.append(sorted(thirds))
    return out


@pytest.mark.parametrize("fold", ["tiny", "multi"])
@pytest.mark.parametrize("exclude", [("train", "test"), ("train",), ("test",), ()])
def test_screen_known_against_a_walk_of_the_link_tables(fold, exclude):
    from trigenicinteractionpredictor_amd import Model
    from trigenicinteractionpredictor_amd.scan import check_screen_known, screen_known
    train, test = os.path.join(GOLDEN, fold, "train.dat"), os.path.join(GOLDEN, fold, "test.dat")
    m = Model()
    m.get_traintest(train, test)
    rng = np.random.default_rng(1)
    measured = [[int(t) for t in key.split("_")] for key in list(m.links)[:40]]
    pairs = [(ids[0], ids[2]) for ids in measured if len(set(ids)) == 3] + [(ids[2], ids[1]) for ids in measured
                                                                            if len(set(ids)) == 3]
    pairs += [tuple(int(g) for g in rng.choice(m.P, 2, replace=False)) for _ in range(40)]
    off, thirds = screen_known(m, pairs, exclude)
    assert off.dtype == np.int64 and thirds.dtype == np.int32 and off.shape == (len(pairs) + 1,)
    want = brute_known(m, pairs, exclude)
    assert [thirds[off[i]:off[i + 1]].tolist() for i in range(len(pairs))] == want
    if exclude:
        assert thirds.size > 0
    check_screen_known((off, thirds), len(pairs))
    # a pair's slice does not depend on the order of its two genes or on the other pairs
    off2, thirds2 = screen_known(m, [(b, a) for a, b in pairs[::-1]], exclude)
    assert [thirds2[off2[i]:off2[i + 1]].tolist() for i in range(len(pairs))] == want[::-1]
    # the tables as arrays
    tabs = (m.P, m._link_arrays(0)[0], m._link_arrays(1)[0])
    off3, thirds3 = screen_known(tabs, pairs, exclude)
    assert off3.tolist() == off.tolist() and thirds3.tolist() == thirds.tolist()
    assert screen_known(m, [], exclude)[0].tolist() == [0]


def test_screen_known_refuses_bad_pairs():
    from trigenicinteractionpredictor_amd.scan import screen_known
    tabs = (10, np.zeros((0, 3), np.int64), None)
    with pytest.raises(IndexError):
        screen_known(tabs, [(0, 10)])
    with pytest.raises(IndexError):
        screen_known(tabs, [(-1, 3)])
    with pytest.raises(ValueError):
        screen_known(tabs, [(4, 4)])
    with pytest.raises(ValueError):
        screen_known(tabs, [(1, 2, 3)])


def test_check_screen_known():
    from trigenicinteractionpredictor_amd.scan import check_screen_known
    off = np.array([0, 2, 4], dtype=np.int64)
    o, t = check_screen_known((off, [4, 9, 5, 7]), 2)     # a position may fall from one slice to the next
    assert o.dtype == np.int64 and t.dtype == np.int32 and t.tolist() == [4, 9, 5, 7]
    with pytest.raises(ValueError):
        check_screen_known((off, [5, 4, 7, 9]), 2)        # an unsorted slice
    with pytest.raises(ValueError):
        check_screen_known((off, [4, 5, 9, 9]), 2)        # a repeated entry
    with pytest.raises(ValueError):
        check_screen_known((off[:2], [4, 5]), 2)          # offsets of another Q
    with pytest.raises(ValueError):
        check_screen_known(([0, 3, 2], [1, 2, 3]), 2)     # decreasing offsets
    with pytest.raises(ValueError):
        check_screen_known(([0, 2, 5], [1, 2, 3, 4]), 2)  # offsets beyond the thirds
    with pytest.raises(ValueError):
        check_screen_known(([-1, 2, 4], [1, 2, 3, 4]), 2)
    o, t = check_screen_known(([0, 0, 0], []), 2)
    assert o.tolist() == [0, 0, 0] and t.size == 0


# ------------------------------------------------------------------ the driver
def test_driver_parses_the_screen_options():
    from trigenicinteractionpredictor_amd import scan
    cfg = scan.parse(["-t", TRAIN, "--screen", "s.tsv", "--query-pairs", "q.txt"])
    assert (cfg["screen"], cfg["screen_top"], cfg["query_pairs"], cfg["screen_best"]) == ("s.tsv", 20, "q.txt", None)
    cfg = scan.parse(["-t", TRAIN, "--screen-best", "12", "--screen", "s.tsv", "--screen-top", "1024",
                      "--allow-genes", "a.txt", "--block-pairs", "b.txt"])
    assert (cfg["screen"], cfg["screen_top"], cfg["query_pairs"], cfg["screen_best"]) == ("s.tsv", 1024, None, 12)
    assert cfg["allow_genes"] == "a.txt"
    for flag in ("--screen", "--screen-top", "--query-pairs", "--screen-best"):
        assert flag in scan.USAGE and flag in scan.__doc__


@pytest.mark.parametrize("extra", [["--screen", "s.tsv"],
                                   ["--screen", "s.tsv", "--query-pairs", "q.txt", "--screen-best", "3"],
                                   ["--screen", "s.tsv", "--query-pairs", "q.txt", "--screen-top", "0"],
                                   ["--screen", "s.tsv", "--query-pairs", "q.txt", "--screen-top", "1025"],
                                   ["--screen", "s.tsv", "--screen-best", "0"],
                                   ["--screen", "s.tsv", "--query-pairs", "q.txt", "--screen-top", "many"]],
                         ids=["no-source", "both-sources", "top-0", "top-1025", "best-0", "top-text"])
def test_the_driver_refuses_bad_screen_options(extra, monkeypatch):
    from trigenicinteractionpredictor_amd import scan
    monkeypatch.setitem(sys.modules, "trigenicinteractionpredictor_amd.engine", None)
    assert scan.main(["-t", TRAIN, "-e", TEST, "-k", "2", *extra]) == 2
    assert scan.main([*extra, "-t", TRAIN, "-e", TEST, "-k", "2"]) == 2


def test_a_bad_query_pairs_file_is_refused_with_exit_2(tmp_path, monkeypatch):
    from trigenicinteractionpredictor_amd import scan
    monkeypatch.setitem(sys.modules, "trigenicinteractionpredictor_amd.engine", None)
    base = ["-t", TRAIN, "-e", TEST, "-k", "2", "--screen", str(tmp_path / "s.tsv"), "--query-pairs"]
    assert scan.main(base + [str(tmp_path / "missing.txt")]) == 2
    bad = tmp_path / "bad.txt"
    for text in ("no_such_gene_name 3\n", "0 1 2\n", "3 3\n", "0 99999\n", "7\n"):
        bad.write_text(text)
        assert scan.main(base + [str(bad)]) == 2, text
    assert not (tmp_path / "s.tsv").exists()


def test_screen_queries_from_a_file(tmp_path):
    from trigenicinteractionpredictor_amd import Model, scan
    m = Model()
    m.get_traintest(TRAIN, TEST)
    f = tmp_path / "q.txt"
    f.write_text("# the queries\n0\t2\n\n%s %s\n11 4\n" % (m.id_gene[4], m.id_gene[10]))
    cfg = scan.parse(["-t", TRAIN, "--screen", "s.tsv", "--query-pairs", str(f)])
    got = scan.screen_queries(m, cfg)
    assert got.dtype == np.int32 and got.tolist() == [[0, 2], [4, 10], [11, 4]]
    assert scan.screen_queries(m, scan.parse(["-t", TRAIN])) is None
    assert scan.screen_queries(m, scan.parse(["-t", TRAIN, "--screen", "s.tsv", "--screen-best", "4"])) is None


def test_screen_rows():
    from trigenicinteractionpredictor_amd import scan
    names = {0: "A", 1: "B", 2: "C", 10: "D"}
    lists = [(np.array([0.5, 0.25]), np.array([[0, 10, 2], [0, 1, 10]], dtype=np.int32)), (np.zeros(0), np.zeros((0, 3), np.int32))]
    rows = scan.screen_rows(names, [(10, 0), (1, 2)], lists)
    assert rows == [["A_D", 1, 0.5, "0_10_2", ["A", "C", "D"]], ["A_D", 2, 0.25, "0_1_10", ["A", "B", "D"]]]


def test_parse_without_the_screen_options_is_unchanged():
    """cfg without a screen option is what it was; with one it differs by the four keys alone."""
    from trigenicinteractionpredictor_amd import cli, scan
    old = dict(cli.DEFAULTS, samples=1, iterations=100, top=100, exclude=("train", "test"), best=False, out=None,
               seed=None, genes=[], all_genes=False, census=None, thresholds=None, heldout_ranks=None,
               pairs=None, pair_threshold=0.5, gene_census=None)
    assert scan.parse([]) == old
    argv = ["-t", TRAIN, "-e", TEST, "-k", "4", "-n", "3", "-i", "7", "--seed", "5", "--top", "77", "--exclude",
            "train", "--best", "-o", "o.tsv", "--census", "c.tsv", "--network", "n.tsv", "--allow-genes", "a.txt"]
    want = scan.parse(argv)
    new = {"screen": "s.tsv", "screen_top": 20, "query_pairs": None, "screen_best": 5}
    assert not set(new) & set(want)
    cfg = scan.parse(argv + ["--screen", "s.tsv", "--screen-best", "5"])
    assert {k: v for k, v in cfg.items() if k not in new} == want and {k: cfg[k] for k in new} == new


def test_the_bindings_list_the_new_symbols():
    from trigenicinteractionpredictor_amd import _lib, build
    for name in ("mmsbm_screen_max_n", "mmsbm_screen_workspace_bytes", "mmsbm_screen_topn", "mmsbm_screen_scores"):
        assert name in _lib.SIGNATURES
    top, rows = _lib.SIGNATURES["mmsbm_screen_topn"][1], _lib.SIGNATURES["mmsbm_screen_scores"][1]
    assert top[:10] == rows[:10] and len(top) == 17 and len(rows) == 14
    assert build.SRC_SCREEN in build.SRCS and build.SRC_SCREEN in build.DEPS
    assert os.path.exists(build.SRC_SCREEN)
