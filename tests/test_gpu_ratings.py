"""R = 2..8 rating classes, unobserved ratings and a non-default eps in every kernel family, on
the GPU (include/mmsbm.h and include/mmsbm_pairs.h accept 2 <= R <= 8; the drop-in Model keeps
the reference's R = 2, so everything here is at the EMEngine / JointEngine level).

Against the C oracle (oracle/mmsbm_oracle.c, general in R and tied to the direct longdouble
formulas by tests/test_ratings_host.py) the tolerance is the suite's: rtol 1e-9, atol 1e-300 on
theta, p, q, L and predictions.  "Bitwise" and "exactly 0" mean assert_array_equal.  The link
tables and the initial parameters come from tests/ratings_ref.py: every rating's lattice has its
own scale, so a slice read for the wrong rating fails the comparison.
"""
import functools

import numpy as np
import pytest

import ratings_ref as ref

pytestmark = pytest.mark.gpu

RTOL = 1e-9
ATOL = 1e-300
ENV = ("MMSBM_SK", "MMSBM_SK_Y", "MMSBM_SK_FUSED", "MMSBM_UNITS", "MMSBM_GM_CS", "MMSBM_GRAPH", "MMSBM_GCAP",
       "MMSBM_MERGE", "MMSBM_BALANCE", "MMSBM_SP_ROWS", "MMSBM_GM_Q4", "MMSBM_SK_RHO", "MMSBM_PAIR_PARTS")
WORST = {}      # label -> largest relative error against the oracle seen in this run


@pytest.fixture(autouse=True)
def plain_env(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


@pytest.fixture(scope="module", autouse=True)
def worst_errors():
    yield
    for label in sorted(WORST):
        print("max relative error vs oracle  %-14s %.3e" % (label, WORST[label]))


def close(label, got, want):
    err = ref.max_rel(got, want)
    WORST[label] = max(WORST.get(label, 0.0), err)
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL)


# ------------------------------------------------------------------------------ inputs, oracle
@functools.lru_cache(maxsize=None)
def table(P, E, R, seed, empty=()):
    ids, counts = ref.links(P, E, R, seed, empty=empty)
    for a in (ids, counts):
        a.setflags(write=False)
    return ids, counts


@functools.lru_cache(maxsize=None)
def start(P, K, R, seed):
    th, pr = ref.params(P, K, R, seed)
    for a in (th, pr):
        a.setflags(write=False)
    return th, pr


def sizes(K):
    """(P, E): smaller at large K, where the oracle's E K^3 R loop sets the test's time."""
    return (150, 2500) if K <= 12 else (100, 1200) if K < 25 else (60, 600)


def oracle_iterations(ids, counts, th, pr, n, eps=1e-10):
    from oracle import c_oracle
    for _ in range(n):
        th, pr = c_oracle.make_iteration(ids, counts, th, pr, eps)
    return th, pr


def engine(K, P, R, ids, counts, th, pr, B=1, eps=1e-10, family=None, test=None):
    """An EMEngine with the train (and test) links set and B samples uploaded; th / pr: one
    sample's arrays or a list of B."""
    from trigenicinteractionpredictor_amd import EMEngine
    eng = EMEngine(K, P, B=B, R=R, eps=eps, family=family)
    eng.set_links(0, ids, counts)
    if test is not None:
        eng.set_links(1, *test)
    if B == 1 and not isinstance(th, list):
        th, pr = [th], [pr]
    eng.upload(np.stack(th), np.stack(pr))
    return eng


def run_against_oracle(label, K, R, B=1, empty=(), eps=1e-10, family=None, small_k=None, seed=0, plan=None):
    """Two iterations, the train / test likelihood and 200 predictions of every sample against
    the oracle; after the first iteration the `empty` ratings' slices of p are exactly 0."""
    from oracle import c_oracle
    P, E = sizes(K)
    ids, counts = table(P, E, R, 100 * R + K + seed, empty)
    tids, tcounts = table(P, 120, R, 7 + R)                  # the test set observes every rating
    samples = [start(P, K, R, 1000 * s + 10 * K + R) for s in range(B)]
    eng = engine(K, P, R, ids, counts, [s[0] for s in samples], [s[1] for s in samples], B=B, eps=eps,
                 family=family, test=(tids, tcounts))
    info = eng.plan_info()
    for key, value in dict(plan or {}, **({} if small_k is None else {"small_k": small_k})).items():
        assert info[key] == value, (key, info[key], value)
    eng.iterate(1)
    th1, pr1 = eng.download()
    for r in empty:
        np.testing.assert_array_equal(pr1[..., r], 0.0)
    eng.iterate(1)
    th2, pr2 = eng.download()
    L, LT = eng.loglik(0), eng.loglik(1)
    pids = np.random.default_rng(K + R).integers(0, P, (200, 3)).astype(np.int32)
    pred = eng.predict(pids)
    for s in range(B):
        th_o, pr_o = oracle_iterations(ids, counts, *samples[s], 1, eps)
        close(label, th1[s], th_o)
        close(label, pr1[s], pr_o)
        th_o, pr_o = oracle_iterations(ids, counts, th_o, pr_o, 1, eps)
        close(label, th2[s], th_o)
        close(label, pr2[s], pr_o)
        for r in empty:
            np.testing.assert_array_equal(pr2[s][..., r], 0.0)
        assert np.isfinite(L[s]) and np.isfinite(LT[s])
        close(label, L[s], c_oracle.loglik(ids, counts, th_o, pr_o, eps))
        close(label, LT[s], c_oracle.loglik(tids, tcounts, th_o, pr_o, eps))
        close(label, pred[s], c_oracle.predict(pids, th_o, pr_o))
    eng.close()
    return th2, pr2, L


# ------------------------------------------------------------------ (a) every kernel family
# (label, K, environment, B, plan_info "small_k", ratings)
FAMILY_CASES = [
    ("sku-8", 3, {}, 1, 2, (3, 5, 8)), ("sku-8", 10, {}, 1, 2, (3, 5, 8)),
    ("sku-4", 12, {}, 1, 2, (3, 5, 8)),
    ("sky", 4, {"MMSBM_SK_Y": "1"}, 1, 3, (3, 8)), ("sky", 10, {"MMSBM_SK_Y": "1"}, 1, 3, (3, 8)),
    ("sky", 11, {"MMSBM_SK_Y": "1"}, 1, 3, (3, 8)), ("sky", 10, {}, 2, 3, (3,)),
    ("pass-a+b", 9, {"MMSBM_SK_FUSED": "0"}, 1, 1, (3, 8)),
    ("large-forced", 10, {"MMSBM_SK": "0"}, 1, 0, (3, 8)),
    ("large", 13, {}, 1, 0, (3, 8)), ("large", 16, {}, 1, 0, (3, 8)), ("large", 20, {}, 1, 0, (3, 8)),
    ("large-25", 30, {}, 1, 0, (3, 8)), ("large-25", 32, {}, 1, 0, (3, 8)),
]
FAMILY_PARAMS = [(label, K, env, B, sk, R) for label, K, env, B, sk, Rs in FAMILY_CASES for R in Rs]


@pytest.mark.parametrize("label,K,env,B,small_k,R", FAMILY_PARAMS,
                         ids=["%s-K%d-B%d-R%d" % (c[0], c[1], c[3], c[5]) for c in FAMILY_PARAMS])
def test_family_matches_oracle(monkeypatch, label, K, env, B, small_k, R):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    run_against_oracle(label, K, R, B=B, small_k=small_k)


@pytest.mark.parametrize("K", [10, 16])
def test_forced_unit_split_matches_oracle(monkeypatch, K):
    """MMSBM_UNITS=1,1: two units in all, every pivot run split at the unit's chunk cap."""
    monkeypatch.setenv("MMSBM_UNITS", "1,1")
    run_against_oracle("units-1,1", K, 3)


def test_gm_workgroups_per_part_keep_bits_at_three_ratings(monkeypatch):
    from parity_util import gm_valid_cs as _gm_valid_cs
    K, R = 20, 3
    valid = _gm_valid_cs(K)
    assert len(valid) >= 2, valid
    out = []
    for cs in valid:
        monkeypatch.setenv("MMSBM_GM_CS", str(cs))
        out.append(run_against_oracle("gm-cs", K, R, plan={"gm_groups": cs}))
    for th, pr, L in out[1:]:
        np.testing.assert_array_equal(th, out[0][0])
        np.testing.assert_array_equal(pr, out[0][1])
        np.testing.assert_array_equal(L, out[0][2])


def test_graph_replay_matches_direct_launches_bitwise_at_three_ratings(monkeypatch):
    """The section table of the small-K launch travels by value in the captured kernel node."""
    K, R, G = 10, 3, 3
    P, E = sizes(K)
    ids, counts = table(P, E, R, 100 * R + K)
    th, pr = start(P, K, R, 10 * K + R)
    out = {}
    for mode in ("0", str(G)):
        monkeypatch.setenv("MMSBM_GRAPH", mode)
        eng = engine(K, P, R, ids, counts, th, pr)
        eng.iterate(2 * G + 2)            # warm-up iteration, two graph launches, remainder
        out[mode] = eng.download() + (eng.loglik(0),)
        eng.close()
    for a, b in zip(out["0"], out[str(G)]):
        np.testing.assert_array_equal(a, b)
    th_o, pr_o = oracle_iterations(ids, counts, th, pr, 2 * G + 2)
    close("graph", out[str(G)][0][0], th_o)
    close("graph", out[str(G)][1][0], pr_o)


# ------------------------------------------------------------------ (b) empty rating classes
EMPTY_FAMILIES = [("sku-8", 10, "sku", 2), ("sky", 10, "sky", 3), ("large", 20, None, 0), ("large-25", 30, None, 0)]
EMPTY_CASES = [(3, (0,)), (3, (1,)), (3, (2,)), (2, (1,)), (8, (0, 1, 2, 3, 4, 5, 6))]


@pytest.mark.parametrize("R,empty", EMPTY_CASES,
                         ids=["R%d-empty%s" % (R, "".join(map(str, e))) for R, e in EMPTY_CASES])
@pytest.mark.parametrize("label,K,family,small_k", EMPTY_FAMILIES, ids=[c[0] for c in EMPTY_FAMILIES])
def test_unobserved_ratings_give_exact_zero_slices(label, K, family, small_k, R, empty):
    """A rating without observations: an empty (stream, rating) section per stream, no S partial
    rows; its slice of p is exactly 0 after one iteration and the run still matches the oracle
    (second iteration: d = eps for that rating, with a zero count)."""
    run_against_oracle(label + "-empty", K, R, empty=empty, family=family, small_k=small_k, seed=3)


# ------------------------------------------------------------------ (c) batch
@pytest.mark.parametrize("K,family", [(10, "sky"), (13, None)])
def test_batched_samples_at_three_ratings(K, family):
    R, B = 3, 3
    P, E = sizes(K)
    ids, counts = table(P, E, R, 100 * R + K)
    samples = [start(P, K, R, 1000 * s + 10 * K + R) for s in range(B)]
    thB, prB, LB = run_against_oracle("batch", K, R, B=B, family=family)
    for s in range(B):
        one = engine(K, P, R, ids, counts, *samples[s], family=family)
        one.iterate(2)
        th1, pr1 = one.download()
        np.testing.assert_array_equal(th1[0], thB[s])
        np.testing.assert_array_equal(pr1[0], prB[s])
        assert one.loglik(0)[0] == LB[s]
        one.close()
    # two active slots: slot 2 keeps its bits, slots 0 and 1 run as before
    eng = engine(K, P, R, ids, counts, [s[0] for s in samples], [s[1] for s in samples], B=B, family=family)
    before = eng.download()
    eng.set_active(2)
    eng.iterate(2)
    th, pr = eng.download()
    np.testing.assert_array_equal(th[2], before[0][2])
    np.testing.assert_array_equal(pr[2], before[1][2])
    np.testing.assert_array_equal(th[:2], thB[:2])
    np.testing.assert_array_equal(pr[:2], prB[:2])
    assert np.isnan(eng.loglik(0)[2])
    eng.close()


# ------------------------------------------------------------------ (d) link sharding
def sharded_iteration(K, R, eps=1e-10):
    """Two contexts, each with one block of the links and the global degree: their accumulators
    summed, then the M-step -> (theta', p') of context 0, the per-block (nth, S) and the inputs."""
    import torch
    from trigenicinteractionpredictor_amd import EMEngine
    from trigenicinteractionpredictor_amd.linkshard import shard_links, train_degree
    P, E = (100, 800)
    ids, counts = table(P, E, R, 300 + R + K)
    th, pr = start(P, K, R, 20 * K + R)
    deg = train_degree(ids, P)
    engs, bufs = [], []
    for r in range(2):
        lo, hi = shard_links(E, 2, r)
        e = EMEngine(K, P, R=R, eps=eps)
        e.set_links(0, ids[lo:hi], counts[lo:hi], deg=deg)
        e.upload(np.stack([th]), np.stack([pr]))
        n = torch.zeros((1, P, K), dtype=torch.float64, device=e.device)
        s = torch.zeros((1, R, K ** 3), dtype=torch.float64, device=e.device)
        e.accumulate(n, s)
        engs.append(e)
        bufs.append((n, s))
    nsum, ssum = bufs[0][0] + bufs[1][0], bufs[0][1] + bufs[1][1]
    out = []
    for e in engs:
        e.mstep(nsum, ssum)
        out.append(e.download())
        e.close()
    np.testing.assert_array_equal(out[0][0], out[1][0])
    np.testing.assert_array_equal(out[0][1], out[1][1])
    return out[0], [(n.cpu().numpy()[0], s.cpu().numpy()[0]) for n, s in bufs], (ids, counts, th, pr)


@pytest.mark.parametrize("K,R", [(10, 3), (16, 3), (4, 8)])
def test_link_blocks_at_more_ratings(K, R):
    from oracle import shard_oracle
    from trigenicinteractionpredictor_amd.linkshard import shard_links
    (th1, pr1), blocks, (ids, counts, th, pr) = sharded_iteration(K, R)
    th_o, pr_o = oracle_iterations(ids, counts, th, pr, 1)
    close("linkshard", th1[0], th_o)
    close("linkshard", pr1[0], pr_o)
    lo, hi = shard_links(ids.shape[0], 2, 1)
    n_o, s_o = shard_oracle.accumulate(ids[lo:hi], counts[lo:hi], th, pr)
    assert blocks[1][1].shape == (R, K ** 3)
    close("linkshard", blocks[1][0], n_o)
    close("linkshard", blocks[1][1], s_o)


# ------------------------------------------------------------------ (e) joint model
def joint_inputs(R, K, empty3=(), empty2=()):
    P, E3, E2 = 100, 600, 400
    ids3, counts3 = table(P - 6, E3, R, 500 + R + K, empty3)          # six pair-only genes
    ids2, counts2 = ref.pair_links(P, E2, R, 600 + R + K, empty=empty2)
    th, pr = start(P, K, R, 30 * K + R)
    _, qr = ref.params(P, K, R, 31 * K + R, pairs=True)
    return P, ids3, counts3, ids2, counts2, th, pr, qr


def joint_engine(K, P, R, tabs, th, pr, qr, eps=1e-10):
    from trigenicinteractionpredictor_amd import _lib
    from trigenicinteractionpredictor_amd.joint import JointEngine
    eng = JointEngine(K, P, B=1, R=R, eps=eps)
    eng.set_links(_lib.SET_TRAIN, *tabs)
    eng.upload(np.stack([th]), np.stack([pr]), np.stack([qr]))
    return eng


def run_joint_against_oracle(label, R, K, empty3=(), empty2=(), eps=1e-10):
    from oracle import c_oracle
    P, ids3, counts3, ids2, counts2, th, pr, qr = joint_inputs(R, K, empty3, empty2)
    eng = joint_engine(K, P, R, (ids3, counts3, ids2, counts2), th, pr, qr, eps)
    eng.iterate(1)
    _, p1, q1 = eng.download()
    for r in empty3:
        np.testing.assert_array_equal(p1[..., r], 0.0)
    for r in empty2:
        np.testing.assert_array_equal(q1[..., r], 0.0)
    eng.iterate(1)
    t, p, q = eng.download()
    th_o, pr_o, qr_o = th, pr, qr
    for _ in range(2):
        th_o, pr_o, qr_o = c_oracle.joint_make_iteration(ids3, counts3, ids2, counts2, th_o, pr_o, qr_o, eps)
    close(label, t[0], th_o)
    close(label, p[0], pr_o)
    close(label, q[0], qr_o)
    L = eng.loglik(0)[0]
    assert np.isfinite(L)
    close(label, L, c_oracle.joint_loglik(ids3, counts3, ids2, counts2, th_o, pr_o, qr_o, eps))
    rng = np.random.default_rng(R + K)
    pids3 = rng.integers(0, P, (100, 3)).astype(np.int32)
    pids2 = rng.integers(0, P, (100, 2)).astype(np.int32)
    close(label, eng.predict(pids3)[0], c_oracle.predict(pids3, th_o, pr_o))
    close(label, eng.predict(pids2)[0], c_oracle.pair_predict(pids2, th_o, qr_o))
    eng.close()


@pytest.mark.parametrize("R,K", [(3, 4), (3, 12), (3, 13), (8, 5), (8, 20)])
def test_joint_engine_matches_oracle_at_more_ratings(R, K):
    run_joint_against_oracle("joint", R, K)


@pytest.mark.parametrize("R,K,empty3,empty2", [(3, 12, (), (1,)), (3, 13, (2,), ()), (8, 5, (), (0, 3))],
                         ids=["pairs-empty1", "triplets-empty2", "pairs-empty03"])
def test_joint_engine_with_a_rating_unobserved_in_one_arity(R, K, empty3, empty2):
    run_joint_against_oracle("joint-empty", R, K, empty3, empty2)


def test_joint_fused_and_unfused_paths_agree_at_three_ratings():
    R, K = 3, 12
    P, ids3, counts3, ids2, counts2, th, pr, qr = joint_inputs(R, K)
    out = []
    for mode in ("iterate", "iterate_unfused"):
        eng = joint_engine(K, P, R, (ids3, counts3, ids2, counts2), th, pr, qr)
        getattr(eng, mode)(3)
        out.append(eng.download())
        eng.close()
    for a, b in zip(out[0], out[1]):
        np.testing.assert_allclose(a, b, rtol=1e-11, atol=1e-300)


def test_joint_pair_plan_splits_agree_at_three_ratings(monkeypatch):
    R, K = 3, 9
    P, ids3, counts3, ids2, counts2, th, pr, qr = joint_inputs(R, K)
    out = []
    for parts in (None, "16"):
        if parts:
            monkeypatch.setenv("MMSBM_PAIR_PARTS", parts)
        eng = joint_engine(K, P, R, (ids3, counts3, ids2, counts2), th, pr, qr)
        if parts:
            assert eng.plan_info(0)["pair_wg_parts_max"] <= 16 * 4
        eng.iterate(3)
        out.append(eng.download())
        eng.close()
    for a, b in zip(out[0], out[1]):
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-300)


# ------------------------------------------------------------------ (f) scan, partners, census
@functools.lru_cache(maxsize=None)
def scan_case(R, K, B):
    """B samples of random parameters at P = 40 and the reference scores of the rating-1 slice,
    of the mean over the samples, and of the same parameters with rating 0 / rating 2 in rating
    1's place (what a kernel reading the wrong slice would rank)."""
    import scan_ref
    P = 40
    th = np.stack([start(P, K, R, 50 * K + R + b)[0] for b in range(B)])
    pr = np.stack([start(P, K, R, 50 * K + R + b)[1] for b in range(B)])

    def mean_scores(prs):
        per = [scan_ref.ref_scores(th[b], prs[b]) for b in range(B)]
        total = per[0][0]
        for b in range(1, B):
            total = total + per[b][0]
        return total / B, per[0][1]
    scores, keys = mean_scores(pr)
    wrong = [mean_scores(np.roll(pr, shift, axis=-1))[0] for shift in (1, -1)]   # ratings 0 and 2
    return P, th, pr, scores, keys, wrong


SCAN_PARAMS = [(R, K, B) for R in (3, 8) for K in (4, 13) for B in (1, 2)]


@pytest.mark.parametrize("R,K,B", SCAN_PARAMS, ids=["R%d-K%d-B%d" % c for c in SCAN_PARAMS])
def test_scan_partners_and_census_read_the_rating_1_slice(R, K, B):
    import census_ref
    import partners_ref
    import scan_ref
    from test_gpu_scan import check
    from trigenicinteractionpredictor_amd import EMEngine
    N = 50
    P, th, pr, scores, keys, wrong = scan_case(R, K, B)
    want_keys = scan_ref.top(scores, keys, N)[1][:N]
    for other in wrong:     # on the reference alone: another rating's slice ranks another list
        assert not np.array_equal(scan_ref.top(other, keys, N)[1][:N], want_keys)
    eng = EMEngine(K, P, B=B, R=R)
    eng.upload(th, pr)
    # the genome-wide scan
    s, ids = eng.scan_top(N)
    check(s, ids, scores, keys, N, P)
    if B > 1:
        s1, ids1 = eng.scan_top(N, sample=1)
        check(s1, ids1, scan_ref.ref_scores(th[1], pr[1])[0], keys, N, P)
    # the partner scan of five genes
    _, rank = scan_ref.rank_tables(P)
    queries = [0, 7, 19, 20, P - 1]
    rows = eng.partners_top(queries, N)
    for g, row in zip(queries, rows):
        per = [partners_ref.ref_query(th[b], pr[b], int(rank[g]))[0] for b in range(B)]
        mean = per[0] if B == 1 else (per[0] + per[1]) / 2
        other = partners_ref.ref_query(th[0], np.roll(pr[0], 1, axis=-1), int(rank[g]))[0]
        assert not np.array_equal(np.argsort(-other)[:N], np.argsort(-per[0])[:N])
        partners_ref.check_query(row, th[0], pr[0], g, N, scores=mean)
    # the census
    thresholds = census_ref.gap_thresholds(scores, 40)
    census_ref.assert_clear(scores, thresholds)
    want, want_total = census_ref.ref_census(scores, keys, thresholds)
    for other in wrong:
        assert not np.array_equal(census_ref.ref_census(other, keys, thresholds)[0], want)
    got, got_total = eng.census(thresholds)
    np.testing.assert_array_equal(got, want)
    assert got_total == want_total
    eng.close()


# ------------------------------------------------------------------ (f2) the later scan families
@pytest.mark.parametrize("R,K,B", SCAN_PARAMS, ids=["R%d-K%d-B%d" % c for c in SCAN_PARAMS])
def test_the_later_scan_families_read_the_rating_1_slice(R, K, B):
    """The screen scan, the pair census, the threshold scan, the vote scan and the quorum scan at
    R = 3 and 8: each family's host entry hands its own prep launch the rating count, and the
    rating-1 slice of slot s lies at (s R + 1) K^3.  With B = 2 both slot 1 and the ensemble run:
    slot 0's offset is K^3 whatever R is.  Before each comparison, on the reference alone: ratings 0
    and 2 in rating 1's place give another answer."""
    import census_ref
    import pair_census_ref
    import quorum_ref
    import scan_ref
    import screen_ref
    import votes_ref
    from test_gpu_scan_above import assert_list_properties
    from test_gpu_screen import rank_rows, to_ids
    from trigenicinteractionpredictor_amd import EMEngine
    P, th, pr, mean, keys, wrong_mean = scan_case(R, K, B)
    rolled = [np.roll(pr, shift, axis=-1) for shift in (1, -1)]        # ratings 0 and 2 in rating 1's place
    per = np.stack([scan_ref.ref_scores(th[b], pr[b])[0] for b in range(B)])
    wrong_per = [np.stack([scan_ref.ref_scores(th[b], w[b])[0] for b in range(B)]) for w in rolled]
    eng = EMEngine(K, P, B=B, R=R)
    eng.upload(th, pr)
    pos = [(0, P - 1), (0, 1), (P - 2, P - 1), (15, 16), (3, 32), (14, 17), (7, 25), (20, 21)]
    pairs = to_ids(P, pos)
    N = 16
    for sample in (None, 1) if B == 2 else (None,):
        scored = slice(0, B) if sample is None else slice(sample, sample + 1)
        ns = scored.stop - scored.start
        scores = mean if sample is None else per[sample]
        wrong = wrong_mean if sample is None else [w[sample] for w in wrong_per]
        # the screen scan: rows and the top 16 of eight pairs
        rows = rank_rows(P, eng.screen_scores(pairs, sample=sample))
        lists = eng.screen_top(pairs, N, sample=sample)
        for i, (x, y) in enumerate(pos):
            want = screen_ref.ref_rows(th, pr, x, y, sample)
            for w in rolled:
                other = screen_ref.ref_rows(th, w, x, y, sample)
                assert not np.array_equal(screen_ref.want_list(other, P, x, y, N)[1], screen_ref.want_list(want, P, x, y, N)[1])
            screen_ref.check_row(rows[i], want, screen_ref.eligible(P, x, y))
            screen_ref.check_list(lists[i], want, P, x, y, N)
        # the pair census
        thresholds = census_ref.gap_thresholds(scores, 40)[:8]
        census_ref.assert_clear(scores, thresholds)
        want = pair_census_ref.ref_pairs(scores, keys, P, thresholds)[1]
        for other in wrong:
            assert not np.array_equal(pair_census_ref.ref_pairs(other, keys, P, thresholds)[1], want)
        np.testing.assert_array_equal(eng.pair_census(thresholds, sample=sample), want)
        # the threshold scan at a clear threshold near the 95 % quantile
        clear = np.sort(census_ref.gap_thresholds(scores, 40))[1:-1]
        t = float(clear[np.argmin(np.abs(clear - np.quantile(scores, 0.95)))])
        census_ref.assert_clear(scores, [t])
        hit = scores >= t
        assert 0 < hit.sum() < scores.size
        for other in wrong:
            assert not np.array_equal(other >= t, hit)
        s, ids = eng.scan_above(t, sample=sample)
        got = assert_list_properties(s, ids, P)
        np.testing.assert_array_equal(np.sort(got), keys[hit])
        np.testing.assert_allclose(s, scores[np.searchsorted(keys, got)], rtol=scan_ref.RTOL, atol=0)
        # the vote scan: a threshold clear of every scored slot's scores
        tv = votes_ref.at_quantile(per[scored], votes_ref.clear_thresholds(per[scored], 41), 0.8)
        census_ref.assert_clear(per[scored].reshape(-1), [tv])
        votes_r, keys_r, mean_r, hist_r = votes_ref.ref_votes(per[scored], keys, tv)
        for w in wrong_per:
            assert not np.array_equal(votes_ref.ref_votes(w[scored], keys, tv)[3], hist_r)
        np.testing.assert_array_equal(eng.vote_census(tv, sample=sample), hist_r)
        for m in sorted({1, ns}):
            v, s, ids = eng.consensus(tv, m, sample=sample)
            got = scan_ref.packed(ids, P)
            want_hits = votes_ref.ref_hits(votes_r, keys_r, mean_r, m)
            np.testing.assert_array_equal(np.sort(got), np.array(sorted(want_hits), dtype=np.int64))
            at = np.searchsorted(keys_r, got)
            np.testing.assert_array_equal(v, votes_r[at])
            np.testing.assert_allclose(s, mean_r[at], rtol=scan_ref.RTOL, atol=0)
        # the quorum scan at one supported m: the minimum over the scored slots
        m = ns
        assert m in quorum_ref.supported(ns, eng.quorum_max_depth)
        want_s, want_k = quorum_ref.ref_top(per[scored], keys, m, N)        # asserts the gaps
        for w in wrong_per:
            assert not np.array_equal(scan_ref.top(quorum_ref.quorum(w[scored], m), keys, N)[1][:N], want_k[:N])
        s, ids = eng.quorum_top(N, m, sample=sample)
        np.testing.assert_array_equal(ids, scan_ref.keys_to_ids(want_k[:N], P))
        np.testing.assert_allclose(s, want_s[:N], rtol=scan_ref.RTOL, atol=0)
    eng.close()


# ------------------------------------------------------------------ (f3) the newest families, the masked entries
NEWEST_N = 16
NEWEST_QUERIES = (0, 7, 19, 20, 39)     # gene ids: the five queries of (f) at P = 40


def newest_samples(B):
    """The ensemble, and slot 1 of two for the families that take `sample`."""
    return (None, 1) if B == 2 else (None,)


@functools.lru_cache(maxsize=None)
def newest_case(R, K, B):
    """The numpy side of (f3), computed once and shared with tests/test_ratings_host.py: every
    reference answer of the test below over scan_case(R, K, B), and, asserted here on the reference
    alone before anything is compared, that ratings 0 and 2 in rating 1's place give another answer.
    -> {"mask", "blocked", "merged", "partners_stat", (sample, masked): {family: reference}}."""
    import census_ref
    import converged_ref
    import pair_census_ref
    import pair_votes_ref
    import partners_masked_ref
    import partners_ref
    import partners_stat_ref
    import quorum_ref
    import scan_ref
    import spread_ref
    import votes_ref
    N = NEWEST_N
    P, th, pr, mean, keys, wrong_mean = scan_case(R, K, B)
    assert P == NEWEST_QUERIES[-1] + 1
    rolled = [np.roll(pr, shift, axis=-1) for shift in (1, -1)]        # ratings 0 and 2 in rating 1's place
    per = np.stack([scan_ref.ref_scores(th[b], pr[b])[0] for b in range(B)])
    wrong_per = [np.stack([scan_ref.ref_scores(th[b], w[b])[0] for b in range(B)]) for w in rolled]
    mask, blocked = converged_ref.random_pair_mask(P)       # scan.pair_mask of 10 % of the pairs, masked_ref.expand
    _, rank = scan_ref.rank_tables(P)
    queries = list(NEWEST_QUERIES)
    merged = partners_masked_ref.merged_known(mask, P, queries)
    out = {"mask": np.ascontiguousarray(mask), "blocked": blocked, "merged": merged, "queries": queries}

    def differ(a, b):
        assert not np.array_equal(a, b), "another rating's slice gives the same answer"

    # the partner statistics: the ensemble's only (the entry takes no sample)
    stats = {}
    calls = [("quorum", m) for m in sorted({1, B})] + ([("spread", 0)] if B >= 2 else [])
    for g in queries:
        q = int(rank[g])
        slots, tk, pk = partners_stat_ref.ref_slots(th, pr, q)
        others = [partners_stat_ref.ref_slots(th, w, q)[0] for w in rolled]
        for tab, keep in (("all", None), ("masked", ~np.isin(pk, partners_masked_ref.blocked_pairs(mask, P, q)))):
            for what, arg in calls:
                v = partners_stat_ref.stat(slots, what, arg)
                ok, gap = partners_stat_ref.gap_ok(v if keep is None else v[keep], what, N)
                assert ok, (g, what, arg, gap)
                want = partners_stat_ref.top_list(v, tk, P, N, keep)
                for o in others:
                    differ(partners_stat_ref.top_list(partners_stat_ref.stat(o, what, arg), tk, P, N, keep)[1], want[1])
                bound = partners_stat_ref.top_list(spread_ref.atol(slots, arg), tk, P, N, keep, order_by=v)[0] \
                    if what == "spread" else None
                stats[g, tab, what, arg] = want + (bound,)
    out["partners_stat"], out["stat_calls"] = stats, calls

    for sample in newest_samples(B):
        scored = slice(0, B) if sample is None else slice(sample, sample + 1)
        ns = scored.stop - scored.start
        scores = mean if sample is None else per[sample]
        wrong = wrong_mean if sample is None else [w[sample] for w in wrong_per]
        for tab, kn in (("all", None), ("masked", blocked)):
            e = out[sample, tab] = {"ns": ns}
            # the dispute scan: at least two scored slots
            if ns >= 2:
                want_s, want_k = spread_ref.ref_top(per[scored], keys, 0, N, kn)        # asserts the gaps
                for w in wrong_per:
                    differ(scan_ref.top(spread_ref.spread(w[scored], 0), keys, N, kn)[1][:N], want_k[:N])
                tol = spread_ref.atol(per[scored], 0)[np.searchsorted(keys, want_k[:N])]
                e["spread"] = (want_s[:N], want_k[:N], tol)
            # the pair vote census at a threshold clear of every scored slot's scores, the levels descending
            tv = votes_ref.at_quantile(per[scored], votes_ref.clear_thresholds(per[scored], 41), 0.8)
            census_ref.assert_clear(per[scored].reshape(-1), [tv])
            levels = list(range(ns, 0, -1))
            want = pair_votes_ref.ref_pairs(per[scored], keys, P, tv, levels, known=kn)[1]
            assert want.any()
            for w in wrong_per:
                differ(pair_votes_ref.ref_pairs(w[scored], keys, P, tv, levels, known=kn)[1], want)
            e["pair_votes"] = (tv, levels, want)
            if kn is None:
                continue        # (f) and (f2) hold the other unmasked entries
            # the masked entries that are also held against the reference
            top_s, top_k = scan_ref.top(scores, keys, N, kn)
            scan_ref.assert_gaps(top_s)
            for o in wrong:
                differ(scan_ref.top(o, keys, N, kn)[1][:N], top_k[:N])
            e["scan_top"] = (top_s[:N], top_k[:N])
            thresholds = census_ref.gap_thresholds(scores, 40)[:8]
            census_ref.assert_clear(scores, thresholds)
            counts = census_ref.ref_census(scores, keys, thresholds, kn)
            pairs = pair_census_ref.ref_pairs(scores, keys, P, thresholds, kn)[1]
            for o in wrong:
                differ(census_ref.ref_census(o, keys, thresholds, kn)[0], counts[0])
                differ(pair_census_ref.ref_pairs(o, keys, P, thresholds, kn)[1], pairs)
            e["census"] = (thresholds, counts[0], counts[1], pairs)
            clear = np.sort(census_ref.gap_thresholds(scores, 40))[1:-1]
            t = float(clear[np.argmin(np.abs(clear - np.quantile(scores, 0.95)))])
            census_ref.assert_clear(scores, [t])
            keep = ~np.isin(keys, kn)
            hit = (scores >= t) & keep
            assert 0 < hit.sum() < keep.sum()
            for o in wrong:
                differ((o >= t) & keep, hit)
            e["scan_above"] = (t, keys[hit])
            hist = votes_ref.ref_votes(per[scored], keys, tv, known=kn)[3]
            for w in wrong_per:
                differ(votes_ref.ref_votes(w[scored], keys, tv, known=kn)[3], hist)
            e["votes"] = (tv, hist)
            q_s, q_k = quorum_ref.ref_top(per[scored], keys, ns, N, kn)         # asserts the gaps
            for w in wrong_per:
                differ(scan_ref.top(quorum_ref.quorum(w[scored], ns), keys, N, kn)[1][:N], q_k[:N])
            e["quorum"] = (ns, q_s[:N], q_k[:N])
            # the partner scan of the five queries under the mask
            rows = []
            for i, g in enumerate(queries):
                q = int(rank[g])
                mine = [partners_ref.ref_query(th[b], pr[b], q)[0] for b in range(B)][scored]
                qmean = scan_ref.prefix_mean(np.stack(mine), ns)
                known_pairs = merged[1][merged[0][i]:merged[0][i + 1]]
                want_ids = partners_ref.want_list(th[0], pr[0], g, N, known_pairs, qmean)[1]
                for w in rolled:
                    other = [partners_ref.ref_query(th[b], w[b], q)[0] for b in range(B)][scored]
                    differ(partners_ref.want_list(th[0], pr[0], g, N, known_pairs,
                                                  scan_ref.prefix_mean(np.stack(other), ns))[1], want_ids)
                rows.append((known_pairs, qmean))
            e["partners"] = rows
    return out


@pytest.mark.parametrize("R,K,B", SCAN_PARAMS, ids=["R%d-K%d-B%d" % c for c in SCAN_PARAMS])
def test_the_newest_families_and_the_masked_entries_read_the_rating_1_slice(R, K, B):
    """The dispute scan, the pair vote census and the partner statistics, and every *_masked entry, at
    R = 3 and 8: scan_spread.hip and pair_votes.hip have host entries and prep launches of their own,
    and each masked entry hands its prep launch the rating count apart from the unmasked one.  The
    references and their preconditions (another rating's slice gives another answer) are newest_case's.
    A masked call equals the unmasked call with the key table the mask stands for (the blocked pairs
    of the query, for the partner scan): exactly for counts, in bits and ids for lists; and one call
    of every family is also held against the reference, so the identity cannot hold between two calls
    that are wrong alike."""
    import partners_ref
    import scan_ref
    from test_gpu_scan import check
    from test_gpu_scan_above import assert_list_properties
    from trigenicinteractionpredictor_amd import EMEngine
    N = NEWEST_N
    c = newest_case(R, K, B)
    P, th, pr = scan_case(R, K, B)[:3]
    keys = scan_case(R, K, B)[4]
    mask, blocked, merged, queries = c["mask"], c["blocked"], c["merged"], c["queries"]
    eng = EMEngine(K, P, B=B, R=R)
    eng.upload(th, pr)

    def same(x, y):
        if isinstance(x, (tuple, list)):
            assert len(x) == len(y)
            for u, v in zip(x, y):
                same(u, v)
        elif isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.shape == y.shape and scan_ref.bits(x) == scan_ref.bits(y)
        else:
            assert x == y

    # the partner statistics of the five queries, unmasked and masked
    for tab, kw, table in (("all", {}, None), ("masked", {"mask": mask}, merged)):
        for what, arg in c["stat_calls"]:
            f = eng.partners_quorum_top if what == "quorum" else eng.partners_spread_top
            got = f(queries, N, arg, **kw)
            if table is not None:
                same(got, f(queries, N, arg, table))
            for g, (s, ids) in zip(queries, got):
                want_s, want_ids, bound = c["partners_stat"][g, tab, what, arg]
                np.testing.assert_array_equal(ids, want_ids, err_msg=str((g, tab, what, arg)))
                if what == "quorum":
                    np.testing.assert_allclose(s, want_s, rtol=scan_ref.RTOL, atol=0)
                else:
                    assert (np.abs(s - want_s) <= bound).all() and not np.signbit(s).any()

    for sample in newest_samples(B):
        for tab, kw, table in (("all", {}, None), ("masked", {"mask": mask}, blocked)):
            e = c[sample, tab]
            # the dispute scan (the ensemble of two slots: it takes no sample)
            if "spread" in e:
                assert sample is None
                want_s, want_k, tol = e["spread"]
                s, ids = eng.spread_top(N, 0, **kw)
                np.testing.assert_array_equal(ids, scan_ref.keys_to_ids(want_k, P))
                assert (np.abs(s - want_s) <= tol).all() and not np.signbit(s).any()
                if table is not None:
                    same(eng.spread_top(N, 0, table), (s, ids))
            # the pair vote census
            tv, levels, want = e["pair_votes"]
            mat = eng.pair_vote_census(tv, levels, sample=sample, **kw)
            np.testing.assert_array_equal(mat, want)
            if table is None:
                continue
            same(eng.pair_vote_census(tv, levels, table, sample=sample), mat)
            # the other masked entries: the identity, and the reference
            want_s, want_k = e["scan_top"]
            got = eng.scan_top(N, sample=sample, mask=mask)
            check(got[0], got[1], c_scores(R, K, B, sample), keys, N, P, blocked)
            np.testing.assert_array_equal(got[1], scan_ref.keys_to_ids(want_k, P))
            same(eng.scan_top(N, blocked, sample=sample), got)
            thresholds, counts, total, pairs = e["census"]
            got = eng.census(thresholds, sample=sample, mask=mask)
            np.testing.assert_array_equal(got[0], counts)
            assert got[1] == total
            same(eng.census(thresholds, blocked, sample=sample), got)
            got = eng.pair_census(thresholds, sample=sample, mask=mask)
            np.testing.assert_array_equal(got, pairs)
            same(eng.pair_census(thresholds, blocked, sample=sample), got)
            t, hits = e["scan_above"]
            got = eng.scan_above(t, sample=sample, mask=mask)
            got_k = assert_list_properties(got[0], got[1], P)
            np.testing.assert_array_equal(np.sort(got_k), hits)
            np.testing.assert_allclose(got[0], c_scores(R, K, B, sample)[np.searchsorted(keys, got_k)], rtol=scan_ref.RTOL, atol=0)
            same(eng.scan_above(t, blocked, sample=sample), got)
            tv, hist = e["votes"]
            got = eng.vote_census(tv, sample=sample, mask=mask)
            np.testing.assert_array_equal(got, hist)
            same(eng.vote_census(tv, blocked, sample=sample), got)
            for m in sorted({1, e["ns"]}):
                same(eng.consensus(tv, m, blocked, sample=sample), eng.consensus(tv, m, sample=sample, mask=mask))
            m, want_s, want_k = e["quorum"]
            got = eng.quorum_top(N, m, sample=sample, mask=mask)
            np.testing.assert_array_equal(got[1], scan_ref.keys_to_ids(want_k, P))
            np.testing.assert_allclose(got[0], want_s, rtol=scan_ref.RTOL, atol=0)
            same(eng.quorum_top(N, m, blocked, sample=sample), got)
            rows = eng.partners_top(queries, N, sample=sample, mask=mask)
            same(eng.partners_top(queries, N, merged, sample=sample), rows)
            for g, row, (known_pairs, qmean) in zip(queries, rows, e["partners"]):
                partners_ref.check_query(row, th[0], pr[0], g, N, known_pairs, qmean)
    eng.close()


def c_scores(R, K, B, sample):
    """The reference scores the scans of (f3) rank: the ensemble's, or one slot's."""
    import scan_ref
    P, th, pr, mean, keys, _ = scan_case(R, K, B)
    return mean if sample is None else scan_ref.ref_scores(th[sample], pr[sample])[0]


# ------------------------------------------------------------------ (g) eps
EPS = [1e-3, 1e-30]


def test_oracle_sees_a_dropped_eps():
    """On the oracle alone: eps = 1e-3 moves theta by more than 1e-6 relative from the default's,
    so a kernel path that dropped its eps argument fails the comparisons below."""
    for K in (10, 20):
        P, E = sizes(K)
        ids, counts = table(P, E, 3, 300 + K + 0)
        th, pr = start(P, K, 3, 10 * K + 3)
        a = oracle_iterations(ids, counts, th, pr, 1, 1e-3)[0]
        b = oracle_iterations(ids, counts, th, pr, 1, 1e-10)[0]
        assert np.max(np.abs(a - b) / np.abs(b)) > 1e-6


@pytest.mark.parametrize("eps", EPS)
@pytest.mark.parametrize("label,K,family", [("sku-8", 10, "sku"), ("sky", 10, "sky"), ("large", 20, None)])
def test_eps_reaches_every_kernel(label, K, family, eps):
    run_against_oracle(label + "-eps", K, 3, eps=eps, family=family)


@pytest.mark.parametrize("eps", EPS)
def test_eps_reaches_the_joint_kernels(eps):
    from oracle import c_oracle
    P, ids3, counts3, ids2, counts2, th, pr, qr = joint_inputs(3, 5)
    a = c_oracle.joint_make_iteration(ids3, counts3, ids2, counts2, th, pr, qr, 1e-3)
    b = c_oracle.joint_make_iteration(ids3, counts3, ids2, counts2, th, pr, qr, 1e-10)
    assert np.max(np.abs(a[0] - b[0]) / np.abs(b[0])) > 1e-6
    assert np.max(np.abs(a[2] - b[2]) / np.abs(b[2])) > 1e-6
    run_joint_against_oracle("joint-eps", 3, 5, eps=eps)


@pytest.mark.parametrize("eps", EPS)
def test_eps_reaches_the_link_sharded_halves(eps):
    (th1, pr1), _, (ids, counts, th, pr) = sharded_iteration(10, 3, eps)
    a = oracle_iterations(ids, counts, th, pr, 1, 1e-3)
    b = oracle_iterations(ids, counts, th, pr, 1, 1e-10)
    assert np.max(np.abs(a[0] - b[0]) / np.abs(b[0])) > 1e-6
    th_o, pr_o = oracle_iterations(ids, counts, th, pr, 1, eps)
    close("linkshard-eps", th1[0], th_o)
    close("linkshard-eps", pr1[0], pr_o)


# ------------------------------------------------------------------ (h) refusals
@pytest.mark.parametrize("bad", [1, 9])
def test_rating_counts_outside_the_range_are_refused(bad):
    from oracle import c_oracle
    from trigenicinteractionpredictor_amd import EMEngine, _lib
    from trigenicinteractionpredictor_amd.joint import JointEngine
    K, R, P = 5, 3, 100
    with pytest.raises(_lib.MMSBMError) as e:
        EMEngine(K, P, R=bad)
    assert e.value.code == _lib.MMSBM_ERR_UNSUPPORTED
    # a context that refused a shape takes a valid one and iterates
    ids, counts = table(P, 800, R, 41)
    th, pr = start(P, K, R, 42)
    eng = EMEngine(K, P, R=R)
    assert eng.lib.mmsbm_set_shape(eng.ctx, K, bad, 1, P, 1e-10) == _lib.MMSBM_ERR_UNSUPPORTED
    _lib.check(eng.lib.mmsbm_set_shape(eng.ctx, K, R, 1, P, 1e-10))
    eng.set_links(0, ids, counts)
    eng.upload(np.stack([th]), np.stack([pr]))
    eng.iterate(1)
    th_o, pr_o = oracle_iterations(ids, counts, th, pr, 1)
    close("refusal", eng.download()[0][0], th_o)
    close("refusal", eng.download()[1][0], pr_o)
    eng.close()
    # the pair context
    P, ids3, counts3, ids2, counts2, th, pr, qr = joint_inputs(R, K)
    je = JointEngine(K, P, B=1, R=R)
    assert je.lib.mmsbm_pairs_set_shape(je.pctx, K, bad, 1, P, 1e-10) == _lib.MMSBM_ERR_UNSUPPORTED
    _lib.check(je.lib.mmsbm_pairs_set_shape(je.pctx, K, R, 1, P, 1e-10))
    je.set_links(_lib.SET_TRAIN, ids3, counts3, ids2, counts2)
    je.upload(np.stack([th]), np.stack([pr]), np.stack([qr]))
    je.iterate(1)
    want = c_oracle.joint_make_iteration(ids3, counts3, ids2, counts2, th, pr, qr)
    for got, w in zip(je.download(), want):
        close("refusal", got[0], w)
    je.close()
