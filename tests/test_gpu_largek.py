"""GPU parity above K = 10 against vectors written by the reference itself
(tests/golden/largek/, tests/golden/make_largek_golden.py): K = 11 and 12 (the small-K families
with four gene stretches per unit), the large-K kernels at 13, 16 | 17 (two | up to four X groups
of gm_kernel), 20, 24 | 25 (BIG_K: merged rows, GM::Q4), 30 and 32 (MMSBM_MAX_K), and the joint
model at 13, 20 and 32.

The inputs are the committed 30- and 40-gene folds, the smallest that still reach every launch
of each family; larger plans stay with the oracle tests (tests/test_gpu_parity.py), and the oracle
is held to these same files bit for bit in tests/test_oracle_largek.py.  Tolerance as
tests/test_gpu_parity.py: rtol 1e-9, atol 1e-300.  A file holds p as a subset of cells and a
digest; the GPU's p is compared with the subset (and the whole p where the file has it), and the
whole p with the C oracle's run from the same start.

Every test prints the largest relative deviations it saw (`largek-dev ...`, pytest -s or -rP)."""
import functools
import random

import numpy as np
import pytest

import golden_util as gu
from parity_util import close, deviation, gm_valid_cs, isolated

pytestmark = pytest.mark.gpu

CASES = gu.largek_cases()
TINY = [c for c in CASES if c[0] == "tiny"]
JOINT_CASES = gu.largek_joint_cases()
BIG_K = 25
SWITCHES = ("MMSBM_SK", "MMSBM_SK_Y", "MMSBM_SK_FUSED", "MMSBM_UNITS", "MMSBM_GM_CS", "MMSBM_GM_Q4",
            "MMSBM_MERGE", "MMSBM_BALANCE", "MMSBM_SP_ROWS", "MMSBM_GCAP", "MMSBM_GRAPH", "MMSBM_SK_RHO")


def ids_of(cases):
    return ["%s/%s" % c for c in cases]


def k_of(case):
    return int(case[1][1:].split("_s")[0])


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


class Dev:
    """Largest relative deviations from the reference's values seen in one test."""

    def __init__(self, label):
        self.label, self.worst = label, {}

    def check(self, what, got, want):
        self.worst[what] = max(self.worst.get(what, 0.0), deviation(got, want))
        close(got, want, "%s: %s" % (self.label, what))

    def state(self, vec, it, theta, pr, L=None, LT=None):
        """theta, the stored cells of p (all of p where the file has it) and the likelihoods at
        snapshot `it`."""
        self.check("theta", theta, vec["theta_%d" % it])
        self.check("p", np.asarray(pr).reshape(-1)[vec["pr_idx"]], vec["pr_sub_%d" % it])
        if "pr_%d" % it in vec.files:
            self.check("p", pr, vec["pr_%d" % it])
        if L is not None:
            self.check("L", L, float(vec["L_%d" % it]))
        if LT is not None:
            self.check("L", LT, float(vec["LT_%d" % it]))

    def report(self):
        print("largek-dev %s %s" % (self.label, " ".join("%s=%.3e" % kv for kv in sorted(self.worst.items()))))


@functools.lru_cache(maxsize=None)
def start(fold, name):
    """The fold's tables and the seeded start (oracle/mmsbm_oracle.py, bit-equal to the file's
    theta_0 and digest of p: tests/test_oracle_largek.py), read-only."""
    from oracle.mmsbm_oracle import OracleModel
    from trigenicinteractionpredictor_amd.layout import links_to_arrays
    meta, vec, train, test = gu.largek_load(fold, name)
    m = OracleModel()
    m.get_traintest(train, test)
    random.seed(meta["seed"])
    m.initialize_parameters(meta["K"])
    theta, pr = np.array(m.theta), np.array(m.pr)
    np.testing.assert_array_equal(theta, vec["theta_0"])
    np.testing.assert_array_equal(gu.pr_digest(pr), vec["pr_sha_0"])
    tabs = (*links_to_arrays(m.links), *links_to_arrays(m.test_links))
    for a in (theta, pr) + tabs:
        a.setflags(write=False)
    return meta, vec, tabs, theta, pr


@functools.lru_cache(maxsize=None)
def oracle_states(fold, name):
    """The C oracle's (theta, p) at every snapshot, from the same start; computed once."""
    from oracle import c_oracle
    meta, _, (ids, counts, _, _), theta, pr = start(fold, name)
    out, done = {}, 0
    for it in meta["iters"]:
        while done < it:
            theta, pr = c_oracle.make_iteration(ids, counts, theta, pr)
            done += 1
        theta.setflags(write=False)
        pr.setflags(write=False)
        out[it] = (theta, pr)
    return out


def other_start(P, K, seed):
    rng = np.random.default_rng(seed)
    theta = rng.random((P, K))
    pr = rng.random((K, K, K, 2))
    return theta / theta.sum(1, keepdims=True), pr / pr.sum(3, keepdims=True)


def engine(K, P, tabs, B=1, **kw):
    from trigenicinteractionpredictor_amd import EMEngine
    eng = EMEngine(K, P, B=B, **kw)
    eng.set_links(0, tabs[0], tabs[1])
    eng.set_links(1, tabs[2], tabs[3])
    return eng


# ------------------------------------------------------------------------------ the drop-in Model
@pytest.mark.parametrize("fold,name", CASES, ids=ids_of(CASES))
def test_model_matches_reference_fixture(fold, name):
    from trigenicinteractionpredictor_amd import Model
    meta, vec, train, test = gu.largek_load(fold, name)
    K = meta["K"]
    m = Model()
    m.get_traintest(train, test)
    random.seed(meta["seed"])
    m.initialize_parameters(K)
    np.testing.assert_array_equal(np.array(m.theta), vec["theta_0"])            # host RNG: bit-exact
    np.testing.assert_array_equal(gu.pr_digest(np.array(m.pr)), vec["pr_sha_0"])
    dev, odev = Dev("model %s/%s K=%d" % (fold, name, K)), Dev("model-vs-oracle %s/%s K=%d" % (fold, name, K))
    states = oracle_states(fold, name)
    done = 0
    for it in meta["iters"]:
        if it > done:
            m.make_iterations(it - done)
            done = it
        theta, pr = np.array(m.theta), np.array(m.pr)
        dev.state(vec, it, theta, pr, m.compute_likelihood("train"), m.compute_likelihood("test"))
        odev.check("theta", theta, states[it][0])
        odev.check("p", pr, states[it][1])                                      # every cell of p
    info = m._engine.plan_info()
    assert info["small_k"] == (2 if K <= 12 else 0)
    if K <= 12:
        assert info["genes_per_wg_max"] == 4                                    # four stretches per unit
    else:
        assert info["gm_groups"] == max(gm_valid_cs(K))                         # one sample, a small plan
    m.calculate_test_set_results()
    dev.check("pred", np.array([r[0] for r in m.results]), vec["pred"])
    assert sorted(r[1] for r in m.results) == sorted(str(k) for k in vec["pred_key"])
    # the metrics follow the order of the predictions: asserted where no two are within the
    # re-association noise of each other (tests/test_gpu_parity.py)
    if not np.isnan(vec["metrics"]).any() and isolated(vec["pred"]):
        np.testing.assert_allclose(np.array(m.calculate_metrics()), vec["metrics"], rtol=1e-12)
    dev.report()
    odev.report()


# ------------------------------------------------------------------------------ families, plans
def switch_cases():
    out = []
    for case in CASES:
        K = k_of(case)
        if K <= 12:
            envs = [{"MMSBM_SK_Y": "1"}, {"MMSBM_SK_FUSED": "0"}, {"MMSBM_SK": "0"}, {"MMSBM_UNITS": "1,1"}]
        else:
            envs = [{"MMSBM_GM_CS": str(cs)} for cs in gm_valid_cs(K)] + [{"MMSBM_UNITS": "1,1"}]
            if K >= BIG_K:
                envs += [{"MMSBM_GM_Q4": "0"}, {"MMSBM_MERGE": "0"}, {"MMSBM_BALANCE": "0"}]
        out += [(case[0], case[1], env) for env in envs]
    return out


SWITCH_CASES = switch_cases()


@pytest.mark.parametrize("fold,name,env", SWITCH_CASES,
                         ids=["%s/%s-%s" % (f, n, ",".join("%s=%s" % kv for kv in e.items())) for f, n, e in SWITCH_CASES])
def test_family_and_plan_switches_match_reference_fixture(monkeypatch, fold, name, env):
    """Every kernel family and plan switch the K allows, one sample, at iteration 5."""
    meta, vec, tabs, theta, pr = start(fold, name)
    K, P = meta["K"], meta["P"]
    default = engine(K, P, tabs).plan_info()
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    eng = engine(K, P, tabs)
    info = eng.plan_info()
    switch = next(iter(env))
    print("largek-plan %s/%s %s default=%s forced=%s" % (fold, name, env, default, info))
    small = K <= 12 and switch != "MMSBM_SK"
    assert info["small_k"] == (0 if not small else 1 if switch == "MMSBM_SK_FUSED" else 3 if switch == "MMSBM_SK_Y" else 2)
    if small:
        assert info["genes_per_wg_max"] == 4
    if switch == "MMSBM_GM_CS":
        assert info["gm_groups"] == int(env[switch])
    elif switch == "MMSBM_GM_Q4":
        # without the four-group layout gm_kernel forms two X groups: at most two workgroups per part
        assert default["gm_groups"] == 4 and info["gm_groups"] == 2
    elif switch == "MMSBM_UNITS":
        # long units: never more of them than by default, and fewer in the fused small-K plan.
        # (At large K the cap on a workgroup's V-table genes cuts stream 0 of these 30- and
        # 40-gene folds before the unit target does, so at some K the plan equals the default
        # one: test_long_units_change_most_large_k_plans.)
        assert info["units"] <= default["units"]
        if small:
            assert info["unit_target"] == 1 and info["units"] < default["units"]
    elif switch in ("MMSBM_MERGE", "MMSBM_BALANCE"):
        # one partial row per unit stretch, not one per (workgroup, gene): merging needs the
        # balanced packing (csrc/plan.h), so either switch adds rows
        assert info["partial_rows"] > default["partial_rows"]
    eng.upload(theta[None], pr[None])
    eng.iterate(5)
    th, p = eng.download()
    dev = Dev("switch %s/%s K=%d %s" % (fold, name, K, env))
    dev.state(vec, 5, th[0], p[0], eng.loglik(0)[0], eng.loglik(1)[0])
    dev.report()
    eng.close()


def test_long_units_change_most_large_k_plans(monkeypatch):
    """MMSBM_UNITS=1,1 is no empty switch on these folds: it changes the plan of most large-K
    files, on either side of BIG_K."""
    changed = []
    for fold, name in [c for c in CASES if k_of(c) > 12]:
        meta, _, tabs, _, _ = start(fold, name)
        monkeypatch.delenv("MMSBM_UNITS", raising=False)
        default = engine(meta["K"], meta["P"], tabs).plan_info()
        monkeypatch.setenv("MMSBM_UNITS", "1,1")
        if engine(meta["K"], meta["P"], tabs).plan_info() != default:
            changed.append(meta["K"])
    assert len(changed) >= 6 and min(changed) < BIG_K <= max(changed), changed


# ------------------------------------------------------------------------------ inside a batch
@pytest.mark.parametrize("fold,name", TINY, ids=ids_of(TINY))
def test_slot_of_a_batch_matches_reference_fixture(fold, name):
    """B = 8 with the file's start in slot 3 and other starts around it: SK_Y up to K = 12, above
    it the batched large-K launch with the batch-dependent gm_kernel grid."""
    meta, vec, tabs, theta, pr = start(fold, name)
    K, P, B = meta["K"], meta["P"], 8
    thetas, prs = zip(*[(theta, pr) if b == 3 else other_start(P, K, 100 + b) for b in range(B)])
    eng = engine(K, P, tabs, B=B)
    info = eng.plan_info()
    assert info["small_k"] == (3 if K <= 12 else 0)
    if K > 12:
        assert info["gm_groups"] in gm_valid_cs(K)
    eng.upload(np.stack(thetas), np.stack(prs))
    eng.iterate(5)
    th, p = eng.download()
    dev = Dev("batch-slot-3 %s/%s K=%d gm_groups=%d" % (fold, name, K, info["gm_groups"]))
    dev.state(vec, 5, th[3], p[3], eng.loglik(0)[3], eng.loglik(1)[3])
    assert not np.array_equal(th[2], th[3])
    dev.report()
    eng.close()


# ------------------------------------------------------------------------------ link-sharded
SHARD = [c for c in TINY if c[1] in ("K13_s1", "K20_s1", "K30_s1")]


@pytest.mark.parametrize("fold,name", SHARD, ids=ids_of(SHARD))
def test_single_rank_link_sharded_matches_reference_fixture(fold, name):
    from trigenicinteractionpredictor_amd import EMEngine
    from trigenicinteractionpredictor_amd.linkshard import LinkShardedEM
    meta, vec, tabs, theta, pr = start(fold, name)
    K, P = meta["K"], meta["P"]
    em = LinkShardedEM(EMEngine(K, P), *tabs)
    em.upload(theta[None], pr[None])
    dev = Dev("linkshard-1 %s/%s K=%d" % (fold, name, K))
    for it, n in ((1, 1), (5, 4)):
        em.iterate(n)
        th, p = em.download()
        dev.state(vec, it, th[0], p[0], em.loglik(0)[0], em.loglik(1)[0])
    dev.report()
    em.engine.close()


@pytest.mark.parametrize("fold,name", SHARD, ids=ids_of(SHARD))
def test_two_link_blocks_with_summed_accumulators_match_reference_fixture(fold, name):
    """Two contexts, one block of the train links each and the degree of all of them; their
    accumulators summed as the all-reduce does (tests/test_gpu_linkshard.py)."""
    import torch
    from trigenicinteractionpredictor_amd import EMEngine
    from trigenicinteractionpredictor_amd.linkshard import shard_links, train_degree
    meta, vec, (ids, counts, tids, tcounts), theta, pr = start(fold, name)
    K, P, parts = meta["K"], meta["P"], 2
    deg = train_degree(ids, P)
    engs = []
    for r in range(parts):
        lo, hi = shard_links(ids.shape[0], parts, r)
        assert 0 < hi - lo < ids.shape[0]
        e = EMEngine(K, P)
        e.set_links(0, ids[lo:hi], counts[lo:hi], deg=deg)
        tlo, thi = shard_links(tids.shape[0], parts, r)
        e.set_links(1, tids[tlo:thi], tcounts[tlo:thi])
        e.upload(theta[None], pr[None])
        engs.append(e)
    bufs = [(torch.zeros((1, P, K), dtype=torch.float64, device=e.device),
             torch.zeros((1, 2, K ** 3), dtype=torch.float64, device=e.device)) for e in engs]
    dev = Dev("linkshard-2 %s/%s K=%d" % (fold, name, K))
    done = 0
    for it in (1, 5):
        while done < it:
            for e, (n, s) in zip(engs, bufs):
                e.accumulate(n, s)
            nsum, ssum = sum(b[0] for b in bufs), sum(b[1] for b in bufs)
            for e in engs:
                e.mstep(nsum, ssum)
            done += 1
        th, p = engs[0].download()
        dev.state(vec, it, th[0], p[0], sum(e.loglik(0)[0] for e in engs), sum(e.loglik(1)[0] for e in engs))
        t1, p1 = engs[1].download()
        np.testing.assert_array_equal(t1, th)
        np.testing.assert_array_equal(p1, p)
    dev.report()
    for e in engs:
        e.close()


# ------------------------------------------------------------------------------ joint model
@pytest.mark.parametrize("fold,name", JOINT_CASES, ids=ids_of(JOINT_CASES))
def test_joint_model_matches_reference_fixture(fold, name):
    from trigenicinteractionpredictor_amd.joint import DataType, Model
    meta, vec, train, test = gu.largek_joint_load(fold, name)
    K = meta["K"]
    m = Model()
    m.get_train_test(train, test)
    random.seed(meta["seed"])
    m.initialize_parameters(K, getattr(DataType, meta["interaction"]))
    np.testing.assert_array_equal(np.array(m.theta), vec["theta_0"])
    np.testing.assert_array_equal(gu.pr_digest(np.array(m.pr)), vec["pr_sha_0"])
    np.testing.assert_array_equal(np.array(m.qr), vec["qr_0"])
    dev = Dev("joint %s/%s K=%d" % (fold, name, K))
    done = 0
    for it in meta["iters"]:
        if it > done:
            m.make_iterations(it - done)
            done = it
        dev.state(vec, it, np.array(m.theta), np.array(m.pr), m.compute_likelihood())
        dev.check("q", np.array(m.qr), vec["qr_%d" % it])
    m.calculate_test_set_results()
    dev.check("pred", np.array([r[0] for r in m.results]), vec["pred"])
    assert sorted(r[1] for r in m.results) == sorted(vec["pred_key"].tolist())
    for arity in (3, 2):    # triplets predicted with p, pairs with q
        got = sorted(r[0] for r in m.results if len(r[1].split("_")) == arity)
        want = sorted(p for p, key in zip(vec["pred"].tolist(), vec["pred_key"].tolist()) if len(key.split("_")) == arity)
        # (a pair of the test file is in both test tables, so it has two rows)
        assert len(want) == (meta["n_test_links"] - meta["n_dtest_links"] if arity == 3 else 2 * meta["n_dtest_links"]) > 0
        dev.check("pred", np.array(got), np.array(want))
    dev.report()
