"""The oracles above K = 10 against vectors written by the reference itself
(tests/golden/largek/, tests/golden/make_largek_golden.py).

Every GPU parity test above K = 10 compares with `oracle/mmsbm_oracle.c` or its Python twin, and
those were pinned to the reference only at K in {1, 2, 3, 10}.  Here they are held to it bit for
bit at K = 11..32: the seeded start, theta, p (a subset of cells first, so that a failure names a
cell, then the SHA-256 of all of p), q of the joint model, the log-likelihoods and the test-set
predictions.  The last tests show that the two checks of p can fail."""
import importlib.util
import os
import random

import numpy as np
import pytest

import golden_util as gu
from oracle import c_oracle
from oracle.joint_oracle import ALL, OracleJointModel
from oracle.mmsbm_oracle import OracleModel
from parity_util import close

CASES = gu.largek_cases()
JOINT_CASES = gu.largek_joint_cases()
LARGEST_OTHER_FIXTURE = 158347      # tests/golden/small/K10_s1.npz
# The Python oracles run at the reference's speed, about K^3 / 4000 s an iteration on these folds:
# five iterations up to K = 13, one up to K = 20, the rest is the C oracle's.
PY_ITERS = {13: 5, 20: 1}


def ids_of(cases):
    return ["%s/%s" % c for c in cases]


def generator():
    """tests/golden/make_largek_golden.py as a module (it is no package)."""
    path = os.path.join(gu.GOLDEN, "make_largek_golden.py")
    spec = importlib.util.spec_from_file_location("make_largek_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def check_p(pr, vec, it):
    """A cell before a hash; and the whole p where the file holds it."""
    pr = np.asarray(pr)
    np.testing.assert_array_equal(pr.reshape(-1)[vec["pr_idx"]], vec["pr_sub_%d" % it])
    if "pr_%d" % it in vec.files:
        np.testing.assert_array_equal(pr, vec["pr_%d" % it])
    np.testing.assert_array_equal(gu.pr_digest(pr), vec["pr_sha_%d" % it])


def start(meta, train, test):
    m = OracleModel()
    m.get_traintest(train, test)
    assert (m.P, len(m.links), len(m.test_links)) == (meta["P"], meta["n_links"], meta["n_test_links"])
    random.seed(meta["seed"])
    m.initialize_parameters(meta["K"])
    return m


def joint_start(meta, train, test):
    m = OracleJointModel()
    m.get_train_test(train, test)
    assert (m.P, len(m.links), len(m.test_links), len(m.dlinks), len(m.dtest_links)) == (
        meta["P"], meta["n_links"], meta["n_test_links"], meta["n_dlinks"], meta["n_dtest_links"])
    assert meta["interaction"] == "all"
    random.seed(meta["seed"])
    m.initialize_parameters(meta["K"], ALL)
    return m


# ------------------------------------------------------------------------------ C oracle
@pytest.mark.parametrize("fold,name", CASES, ids=ids_of(CASES))
def test_c_oracle_matches_reference_bitwise(fold, name):
    meta, vec, train, test = gu.largek_load(fold, name)
    m = start(meta, train, test)
    theta, pr = np.array(m.theta), np.array(m.pr)
    np.testing.assert_array_equal(theta, vec["theta_0"])     # the init stream at this K
    check_p(pr, vec, 0)
    ids, counts = c_oracle.links_to_arrays(m.links)
    tids, tcounts = c_oracle.links_to_arrays(m.test_links)
    done = 0
    for it in meta["iters"]:
        while done < it:
            theta, pr = c_oracle.make_iteration(ids, counts, theta, pr)
            done += 1
        np.testing.assert_array_equal(theta, vec["theta_%d" % it])
        check_p(pr, vec, it)
        assert c_oracle.loglik(ids, counts, theta, pr) == float(vec["L_%d" % it])
        assert c_oracle.loglik(tids, tcounts, theta, pr) == float(vec["LT_%d" % it])
    pred = c_oracle.predict(tids, theta, pr)
    assert sorted(pred.tolist(), reverse=True) == vec["pred"].tolist()


# ------------------------------------------------------------------------------ Python oracle
def _py_iters(meta):
    cap = next((n for top, n in sorted(PY_ITERS.items()) if meta["K"] <= top), -1)
    return [it for it in meta["iters"] if it <= cap]


PY_CASES = [c for c in CASES if _py_iters(gu.largek_load(*c)[0])]


@pytest.mark.parametrize("fold,name", PY_CASES, ids=ids_of(PY_CASES))
def test_python_oracle_matches_reference_bitwise(fold, name):
    meta, vec, train, test = gu.largek_load(fold, name)
    m = start(meta, train, test)
    done = 0
    for it in _py_iters(meta):
        while done < it:
            m.make_iteration()
            done += 1
        np.testing.assert_array_equal(np.array(m.theta), vec["theta_%d" % it])
        check_p(m.pr, vec, it)
        assert m.compute_likelihood("train") == float(vec["L_%d" % it])
        assert m.compute_likelihood("test") == float(vec["LT_%d" % it])
    if done == meta["iters"][-1]:   # the table is the last snapshot's
        m.calculate_test_set_results()
        np.testing.assert_array_equal(np.array([r[0] for r in m.results]), vec["pred"])
        assert [r[1] for r in m.results] == [str(k) for k in vec["pred_key"]]
        assert [r[2] for r in m.results] == vec["pred_real"].tolist()
        assert not np.isnan(vec["metrics"]).any()
        np.testing.assert_array_equal(np.array(m.calculate_metrics()), vec["metrics"])


def test_python_oracle_reaches_the_prediction_table_of_most_cases():
    """The cases whose last snapshot the Python oracle does not reach leave the table to the C
    oracle; at K = 11 and 13, on both folds, it is compared."""
    full = [c for c in PY_CASES if _py_iters(gu.largek_load(*c)[0])[-1] == gu.largek_load(*c)[0]["iters"][-1]]
    assert {c[0] for c in full} == {"tiny", "multi"} and {gu.largek_load(*c)[0]["K"] for c in full} == {11, 13}


# ------------------------------------------------------------------------------ joint model
@pytest.mark.parametrize("fold,name", JOINT_CASES, ids=ids_of(JOINT_CASES))
def test_joint_c_oracle_matches_reference_bitwise(fold, name):
    meta, vec, train, test = gu.largek_joint_load(fold, name)
    m = joint_start(meta, train, test)
    theta, pr, qr = np.array(m.theta), np.array(m.pr), np.array(m.qr)
    ids3, c3 = c_oracle.links_to_arrays(m.links)
    ids2, c2 = c_oracle.links_to_arrays(m.dlinks, arity=2)
    done = 0
    for it in meta["iters"]:
        while done < it:
            theta, pr, qr = c_oracle.joint_make_iteration(ids3, c3, ids2, c2, theta, pr, qr)
            done += 1
        np.testing.assert_array_equal(theta, vec["theta_%d" % it])
        check_p(pr, vec, it)
        np.testing.assert_array_equal(qr, vec["qr_%d" % it])
        assert c_oracle.joint_loglik(ids3, c3, ids2, c2, theta, pr, qr) == float(vec["L_%d" % it])
    pred = []
    for key in list(m.test_links) + list(m.dtest_links):
        ids = np.array([[int(s) for s in key.split("_")]], dtype=np.int32)
        pred.append(float((c_oracle.predict(ids, theta, pr) if ids.shape[1] == 3
                           else c_oracle.pair_predict(ids, theta, qr))[0]))
    assert sorted(pred, reverse=True) == vec["pred"].tolist()


PY_JOINT_CASES = [c for c in JOINT_CASES if gu.largek_joint_load(*c)[0]["K"] <= 20]


@pytest.mark.parametrize("fold,name", PY_JOINT_CASES, ids=ids_of(PY_JOINT_CASES))
def test_joint_python_oracle_matches_reference_bitwise(fold, name):
    meta, vec, train, test = gu.largek_joint_load(fold, name)
    m = joint_start(meta, train, test)
    done = 0
    for it in _py_iters(meta):
        while done < it:
            m.make_iteration()
            done += 1
        np.testing.assert_array_equal(np.array(m.theta), vec["theta_%d" % it])
        check_p(m.pr, vec, it)
        np.testing.assert_array_equal(np.array(m.qr), vec["qr_%d" % it])
        assert m.compute_likelihood() == float(vec["L_%d" % it])
    if done < meta["iters"][-1]:
        return
    m.calculate_test_set_results()
    assert [r[0] for r in m.results] == vec["pred"].tolist()
    assert [r[1] for r in m.results] == vec["pred_key"].tolist()
    assert [r[2] for r in m.results] == vec["pred_real"].tolist()
    np.testing.assert_array_equal(np.array(m.calculate_metrics()), vec["metrics"])


# ------------------------------------------------------------------------------ provenance, shape
def test_the_files_are_the_generators_case_table():
    gen = generator()       # importable without the reference
    want = sorted((fold, "K%d_s%d" % (K, seed)) for fold, cs in gen.CASES.items() for K, seed, _ in cs)
    assert sorted(CASES) == want and len(want) == 14
    want = sorted((fold, "K%d_s%d" % (K, seed)) for fold, cs in gen.JOINT_CASES.items() for K, seed, _ in cs)
    assert sorted(JOINT_CASES) == want and len(want) == 3
    on_disk = sorted(os.path.relpath(os.path.join(d, f), gu.LARGEK) for d, _, fs in os.walk(gu.LARGEK) for f in fs)
    stems = [os.path.join(fold, n) for fold, n in CASES] + [os.path.join("joint", fold, n) for fold, n in JOINT_CASES]
    assert on_disk == sorted(s + ext for s in stems for ext in (".json", ".npz"))
    for table, load, joint in ((gen.CASES, gu.largek_load, False), (gen.JOINT_CASES, gu.largek_joint_load, True)):
        for fold, cs in table.items():
            for K, seed, iters in cs:
                meta, vec, _, _ = load(fold, "K%d_s%d" % (K, seed))
                assert (meta["K"], meta["seed"], meta["iters"]) == (K, seed, iters)
                assert meta["fold"] == ("joint/" if joint else "") + fold
                keys = {"pr_idx", "pred", "pred_key", "pred_real", "metrics"}
                for it in iters:
                    keys |= {"%s_%d" % (q, it) for q in ("theta", "pr_sha", "pr_sub", "L", "qr" if joint else "LT")}
                if K <= gu.PR_FULL_MAX_K:
                    keys.add("pr_%d" % iters[-1])
                assert set(vec.files) == keys
                assert vec["theta_0"].shape == (meta["P"], K) and vec["pr_sha_0"].shape == (32,)
                assert vec["pr_sha_0"].dtype == np.uint8


def test_the_files_are_small():
    sizes = {os.path.join(d, f): os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(gu.LARGEK) for f in fs}
    assert max(sizes.values()) < LARGEST_OTHER_FIXTURE, sizes
    assert sum(sizes.values()) < 1_000_000, sum(sizes.values())


@pytest.mark.parametrize("K", [11, 12, 13, 16, 17, 20, 24, 25, 30, 32])
def test_pr_index_follows_its_rule(K):
    """Restated here without golden_util.pr_index: the cells are the multiples of one stride below
    K^3, the eight corners and the diagonal, nothing else; both ratings of each; at most 512."""
    files = [c for c in CASES if gu.largek_load(*c)[0]["K"] == K]
    joint = [c for c in JOINT_CASES if gu.largek_joint_load(*c)[0]["K"] == K]
    assert files
    idx = gu.largek_load(*files[0])[1]["pr_idx"]
    for other in [gu.largek_load(*c)[1] for c in files[1:]] + [gu.largek_joint_load(*c)[1] for c in joint]:
        np.testing.assert_array_equal(other["pr_idx"], idx)      # a rule of K alone
    np.testing.assert_array_equal(idx, gu.pr_index(K))
    assert idx.dtype == np.int64 and idx.size <= 512 and (np.diff(idx) > 0).all() and idx[-1] == 2 * K ** 3 - 1
    cells = idx[::2] // 2
    np.testing.assert_array_equal(idx[::2], 2 * cells)
    np.testing.assert_array_equal(idx[1::2], 2 * cells + 1)
    have = set(cells.tolist())
    corners = {(a * K + b) * K + c for a in (0, K - 1) for b in (0, K - 1) for c in (0, K - 1)}
    diagonal = {(i * K + i) * K + i for i in range(K)}
    assert len(corners) == 8 and corners <= have and diagonal <= have
    stride = min(have - corners - diagonal)                      # the walk's first step
    walk = set(range(0, K ** 3, stride))
    assert walk <= have and have == walk | corners | diagonal
    assert 64 <= len(walk) <= gu.PR_WALK_CELLS


# ------------------------------------------------------------------------------ the checks can fail
def test_one_flipped_bit_outside_the_subset_changes_the_digest():
    _, vec, _, _ = gu.largek_load("tiny", "K13_s1")
    pr = vec["pr_25"].copy()
    np.testing.assert_array_equal(gu.pr_digest(pr), vec["pr_sha_25"])
    flat = pr.reshape(-1)
    cell = next(i for i in range(flat.size) if i not in set(vec["pr_idx"].tolist()))
    flat.view(np.uint64)[cell] ^= 1
    assert flat[cell] != vec["pr_25"].reshape(-1)[cell]
    np.testing.assert_array_equal(flat[vec["pr_idx"]], vec["pr_sub_25"])     # the subset does not see it
    assert not np.array_equal(gu.pr_digest(pr), vec["pr_sha_25"])
    with pytest.raises(AssertionError):
        check_p(pr, vec, 25)


def test_the_gpu_comparison_rejects_1e_8_in_one_cell_of_the_subset():
    _, vec, _, _ = gu.largek_load("tiny", "K32_s1")
    sub = vec["pr_sub_5"].copy()
    close(sub, vec["pr_sub_5"])
    sub[sub.size // 2] *= 1 + 1e-8
    with pytest.raises(AssertionError):
        close(sub, vec["pr_sub_5"])
    sub = vec["pr_sub_5"] * (1 + 1e-11)                  # re-association noise passes
    close(sub, vec["pr_sub_5"])
