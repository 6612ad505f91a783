"""Host side of the score census (trigenicinteractionpredictor_amd/scan.py: the threshold helpers,
the binding's sort / chunk / unsort plan, the driver's new options and TSV writers) and the numpy
reference counter of tests/census_ref.py against the pinned C oracle.  No GPU."""
import io
import os

import numpy as np
import pytest

import census_ref as ref
import scan_ref
from golden_util import GOLDEN, load


# ------------------------------------------------------------------ the reference vs the oracle
def test_reference_counter_matches_the_c_oracle():
    """Sampled reference scores equal the oracle's do_prediction, and on a fixture small enough to
    push every triple through the oracle the counts are the oracle's own."""
    from oracle import c_oracle
    _, vec, _, _ = load("small", "K10_s1")
    theta, pr = vec["theta_5"], vec["pr_5"]
    scores, keys = scan_ref.ref_scores(theta, pr)
    P = theta.shape[0]
    assert scores.size == P * (P - 1) * (P - 2) // 6 and (np.diff(keys) > 0).all()
    pick = np.random.default_rng(0).choice(scores.size, 2000, replace=False)
    np.testing.assert_allclose(scores[pick], c_oracle.predict(scan_ref.keys_to_ids(keys[pick], P), theta, pr),
                               rtol=scan_ref.RTOL, atol=0)

    _, vec, _, _ = load("tiny", "K3_s1")
    theta, pr = vec["theta_5"], vec["pr_5"]
    scores, keys = scan_ref.ref_scores(theta, pr)
    P = theta.shape[0]
    full = c_oracle.predict(scan_ref.keys_to_ids(keys, P), theta, pr)
    np.testing.assert_allclose(scores, full, rtol=scan_ref.RTOL, atol=0)
    thresholds = ref.gap_thresholds(scores, 40)
    ref.assert_clear(scores, thresholds)
    known = keys[::3]
    for kn in (None, known):
        counts, total = ref.ref_census(scores, keys, thresholds, kn)
        keep = np.ones(keys.size, bool) if kn is None else ~np.isin(keys, kn)
        assert total == int(keep.sum())
        assert counts.tolist() == [int((full[keep] >= t).sum()) for t in thresholds]
    assert counts.max() == total and counts.min() == 0      # one below the minimum, one above the maximum


def test_reference_precondition_rejects_a_threshold_near_a_score():
    scores = np.array([0.1, 0.2, 0.4])
    assert ref.clear_of_scores(scores, [0.15, 0.3, 0.05, 0.5]).all()
    assert not ref.clear_of_scores(scores, [0.2 * (1 + 1e-8)]).any()
    assert not ref.clear_of_scores(scores, [0.4 * (1 - 1e-8)]).any()
    assert not ref.clear_of_scores(scores, [0.1]).any()


# ------------------------------------------------------------------ sort, chunk, unsort
def _fake_census(chunk, scores):
    s = np.sort(scores)
    return s.size - np.searchsorted(s, chunk, side="left")


@pytest.mark.parametrize("case", ["none", "one", "max", "max+1", "duplicates", "descending", "3max+5"])
def test_census_chunks_sort_split_and_unsort(case):
    from trigenicinteractionpredictor_amd.scan import MAX_CENSUS_M, census_chunks, census_unsort
    rng = np.random.default_rng(5)
    max_m = MAX_CENSUS_M
    assert max_m == 1024
    t = {"none": np.zeros(0), "one": np.array([0.25]), "max": rng.random(max_m), "max+1": rng.random(max_m + 1),
         "duplicates": np.array([0.5, 0.1, 0.5, 0.9, 0.1, 0.5]), "descending": np.linspace(0.9, 0.1, 50),
         "3max+5": rng.random(3 * max_m + 5)}[case]
    chunks, perm = census_chunks(t.tolist(), max_m)
    want_calls = {"none": 1, "one": 1, "max": 1, "max+1": 2, "duplicates": 1, "descending": 1, "3max+5": 4}[case]
    assert len(chunks) == want_calls                      # no threshold still makes the call for the total
    assert all(c.dtype == np.float64 and c.flags.c_contiguous and c.size <= max_m for c in chunks)
    flat = np.concatenate(chunks)
    assert flat.size == t.size and (np.diff(flat) >= 0).all()
    np.testing.assert_array_equal(flat, t[perm])
    assert sorted(perm.tolist()) == list(range(t.size))
    # counts of each chunk, put back: what one unsorted call would have returned
    scores = rng.random(1000)
    got = census_unsort([_fake_census(c, scores) for c in chunks], perm)
    assert got.dtype == np.int64
    np.testing.assert_array_equal(got, _fake_census(t, scores))


@pytest.mark.parametrize("bad", [[0.1, float("nan")], [float("inf")], [0.5, -float("inf")]])
def test_census_chunks_refuse_nan_and_infinity(bad):
    from trigenicinteractionpredictor_amd.scan import census_chunks
    with pytest.raises(ValueError):
        census_chunks(bad)


# ------------------------------------------------------------------ threshold helpers
def test_strict_thresholds_turn_at_or_above_into_strictly_above():
    from trigenicinteractionpredictor_amd.scan import strict_thresholds
    s = np.array([0.25, 0.25, 0.5, 1e-300, 1.0])
    t = strict_thresholds(s)
    assert t.dtype == np.float64 and (t > s).all()
    np.testing.assert_array_equal(t.view(np.int64), s.view(np.int64) + 1)     # the very next double
    pool = np.array([0.1, 0.25, 0.25, 0.5, 0.7])
    counts, _ = ref.ref_census(pool, np.arange(5), t[:3])
    assert counts.tolist() == [2, 2, 1]                   # strictly above 0.25, 0.25, 0.5
    assert strict_thresholds([]).size == 0


def test_log_thresholds():
    from trigenicinteractionpredictor_amd.scan import log_thresholds
    g = log_thresholds(1e-3, 0.5, 28)
    assert g.size == 28 and g[0] == 0.5 and g[-1] == 1e-3
    assert (np.diff(g) < 0).all()
    np.testing.assert_allclose(g[1:] / g[:-1], (1e-3 / 0.5) ** (1 / 27), rtol=1e-12)
    assert log_thresholds(0.2, 0.2, 1).tolist() == [0.2]
    for lo, hi, n in ((0.0, 0.5, 4), (0.5, 0.1, 4), (0.1, 0.5, 0), (0.1, float("inf"), 3)):
        with pytest.raises(ValueError):
            log_thresholds(lo, hi, n)


def test_default_thresholds_run_from_099_down_to_1e_3():
    from trigenicinteractionpredictor_amd.scan import DEFAULT_THRESHOLDS
    t = list(DEFAULT_THRESHOLDS)
    assert t[0] == 0.99 and t[-1] == 1e-3 and t == sorted(t, reverse=True) and len(set(t)) == len(t)


class _FakeEngine:
    """predict and census over a fixed pool of P = 6 genes whose scan scores sit one ulp ABOVE the
    predict probabilities: a listed triple compared with its own scan score would lose a place."""
    P, active = 6, 1

    def __init__(self):
        from trigenicinteractionpredictor_amd.scan import rank_order
        order = rank_order(self.P)
        self.ids = order[np.array([(a, b, c) for a in range(6) for b in range(a + 1, 6) for c in range(b + 1, 6)])]
        self.keys = np.array([(a * 6 + b) * 6 + c for a in range(6) for b in range(a + 1, 6) for c in range(b + 1, 6)])
        self.p = np.random.default_rng(1).permutation(np.linspace(0.05, 0.95, self.keys.size))
        self.p[3] = self.p[7]                               # one exact tie

    def predict(self, ids):
        table = {tuple(sorted(r)): v for r, v in zip(self.ids.tolist(), self.p)}
        return np.array([[table.get(tuple(sorted(r)), 0.5) for r in np.asarray(ids).tolist()]])

    def census(self, thresholds, known, sample):
        s = np.nextafter(self.p, np.inf)[~np.isin(self.keys, known)]
        return np.array([(s >= t).sum() for t in thresholds], dtype=np.int64), int(s.size)


def test_ranks_of_never_compares_a_triple_with_its_own_scan_score():
    from trigenicinteractionpredictor_amd.scan import ranks_of
    eng = _FakeEngine()
    known = np.sort(eng.keys[[2, 11]])
    listed = np.concatenate([np.arange(10), [11, 0]])       # one known triple, one listed twice
    ids = np.concatenate([eng.ids[listed][:, ::-1], [[1, 1, 2]]]).astype(np.int32)   # and a repeated gene
    p, ranks = ranks_of(eng, ids, known, sample=0)
    np.testing.assert_array_equal(p[:-1], eng.p[listed])
    el = ~np.isin(eng.keys, known)
    want = [1 + int((el & (eng.p > v) & (eng.keys != k)).sum()) for v, k in zip(eng.p[listed], eng.keys[listed])]
    assert not (eng.p == 0.5).any()
    want.append(1 + int((el & (eng.p > 0.5)).sum()))        # a repeated gene: no triple of the pool
    assert ranks.tolist() == want
    assert ranks[3] == ranks[7]                              # tied probabilities share a rank


# ------------------------------------------------------------------ the driver's arguments
TRAIN = os.path.join(GOLDEN, "tiny", "train.dat")
TEST = os.path.join(GOLDEN, "tiny", "test.dat")


@pytest.mark.parametrize("argv", [
    ["--census", "c.tsv", "--thresholds", "0.5,x"], ["--census", "c.tsv", "--thresholds", ""],
    ["--thresholds", "0.5,,0.1"], ["--thresholds", "0"], ["--thresholds", "1.5"], ["--thresholds", "-0.1"],
    ["--thresholds", "nan"], ["--thresholds", "inf"],
    ["-t", TRAIN, "--heldout-ranks", "h.tsv"],
])
def test_driver_census_argument_errors_come_before_any_gpu_use(argv, monkeypatch, capsys):
    import sys
    from trigenicinteractionpredictor_amd import scan
    # the engine module (torch + the HIP library) must not be needed to refuse an argument
    monkeypatch.setitem(sys.modules, "trigenicinteractionpredictor_amd.engine", None)
    assert scan.main(argv) == 2


def test_driver_parses_the_census_flags():
    from trigenicinteractionpredictor_amd import scan
    cfg = scan.parse(["-t", TRAIN, "-e", TEST, "-k", "3", "--census", "c.tsv", "--thresholds", "0.5, 1,1e-3",
                      "--heldout-ranks", "h.tsv"])
    assert (cfg["census"], cfg["heldout_ranks"], cfg["thresholds"]) == ("c.tsv", "h.tsv", [0.5, 1.0, 1e-3])
    cfg = scan.parse(["-t", TRAIN, "--test", TEST, "--heldout-ranks", "h.tsv"])
    assert cfg["heldout_ranks"] == "h.tsv" and cfg["test"] == TEST
    cfg = scan.parse(["-t", TRAIN, "--census", "c.tsv"])
    assert cfg["census"] == "c.tsv" and cfg["thresholds"] is None and cfg["heldout_ranks"] is None
    cfg = scan.parse(["-t", TRAIN])                       # the new options are off by default
    assert cfg["census"] is None and cfg["heldout_ranks"] is None and cfg["thresholds"] is None


# ------------------------------------------------------------------ the TSV writers
def test_census_tsv():
    from trigenicinteractionpredictor_amd.scan import write_census_tsv
    buf = io.StringIO()
    write_census_tsv([0.5, 0.1, 0.001], [0, 25, 100], 200, buf)
    lines = buf.getvalue().split("\n")
    assert lines[0] == "# total\t200"
    assert lines[1] == "threshold\tcount\tfraction"
    assert lines[2:5] == ["0.5\t0\t0.0", "0.1\t25\t0.125", "0.001\t100\t0.5"]
    assert lines[5:] == [""]
    buf = io.StringIO()
    write_census_tsv([0.5], [0], 0, buf)                  # nothing eligible: no division by zero
    assert buf.getvalue().split("\n")[2] == "0.5\t0\t0.0"


def test_heldout_rows_and_tsv():
    from trigenicinteractionpredictor_amd.scan import heldout_rows, write_heldout_tsv
    ids = np.array([[3, 4, 5], [0, 1, 2], [0, 10, 2], [1, 2, 3]], dtype=np.int32)
    link_counts = np.array([[1, 0], [0, 1], [0, 2], [1, 1]], dtype=np.int32)
    probs = np.array([0.25, 0.5, 0.5, 0.125])
    ranks = np.array([7, 2, 2, 40])
    rows = heldout_rows(ids, link_counts, probs, ranks)
    assert rows == [[2, 0.5, "0_10_2", 1], [2, 0.5, "0_1_2", 1], [7, 0.25, "3_4_5", 0], [40, 0.125, "1_2_3", 0]]
    buf = io.StringIO()
    write_heldout_tsv(rows, buf)
    assert buf.getvalue() == ("rank\tprobability\tids\treal\n2\t0.5\t0_10_2\t1\n2\t0.5\t0_1_2\t1\n"
                              "7\t0.25\t3_4_5\t0\n40\t0.125\t1_2_3\t0\n")
