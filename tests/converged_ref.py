"""Helper of tests/test_converged_host.py and tests/test_gpu_converged.py (not a test): the
converged checkpoints of tests/golden/converged/ (tests/golden/make_converged_golden.py) and the
set-at-a-clear-cut rule the scan families are held to on them.

On a converged fit the top scores saturate at 1 - O(eps): hundreds of adjacent gaps of the
reference's top 4096 lie at or below 1e-9 and distinct triples share their bits, so the ORDER of a
top-N list is not determined by the reference.  Its SET is, wherever the reference's gap between
the N-th and the (N + 1)-th score exceeds census_ref.GAP (1e-7, a hundred times the scores'
tolerance): `clear_cuts` finds those N and `check_set_cut` compares there.  numpy only: no GPU,
no product code beyond the rank order.
"""
import collections
import functools
import glob
import os

import numpy as np

import census_ref
import scan_ref

DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "converged")
RTOL = scan_ref.RTOL
TINY = float(np.finfo(np.float64).tiny)

A_SEEDS = (1, 2, 3)
A_ITERS = (80, 300, 1000)            # 80: make_converged_golden.SUBNORMAL_T
EM_A = ["A_s%d_T%d" % (s, t) for s in A_SEEDS for t in A_ITERS]
EM_B = ["B_s1_T300", "B_s1_T2000"]
EM_C = ["C13_s1_T300", "C20_s1_T300"]
RATINGS, JOINT = "D_s1_T300", "E_s1_T300"
ALL = EM_A + EM_B + EM_C + [RATINGS, JOINT]
# the parameter sets the scan families run on: the three A seeds as B = 3, or the single C sample
SCAN_SETS = {"A300": ["A_s%d_T300" % s for s in A_SEEDS], "A1000": ["A_s%d_T1000" % s for s in A_SEEDS],
             "C20": ["C20_s1_T300"]}


class Checkpoint(dict):
    __getattr__ = dict.__getitem__

    def state(self, prev=False):
        names = ("theta", "pr", "qr") if "qr" in self else ("theta", "pr")
        return tuple(self[n + "_prev" if prev else n] for n in names)

    def train(self):
        if "ids2" in self:
            return self.ids, self.counts, self.ids2, self.counts2
        return self.ids, self.counts

    def test(self):
        return self.test_ids, self.test_counts


def files():
    return sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(DIR, "*.npz")))


@functools.lru_cache(maxsize=None)
def load(name):
    """One checkpoint, read-only: arrays by name, the scalars of the meta data as Python values."""
    out = Checkpoint()
    with np.load(os.path.join(DIR, name + ".npz"), allow_pickle=False) as vec:
        for key in vec.files:
            a = vec[key]
            if a.ndim == 0:
                out[key] = a.item()
            else:
                a.setflags(write=False)
                out[key] = a
    out["name"] = name
    return out


def subnormals(a):
    a = np.asarray(a)
    return int(np.count_nonzero((a > 0) & (a < TINY)))


def step(ck, state, reverse=False, eps=1e-10):
    """One C-oracle iteration of the checkpoint's model from `state`; reverse: the link tables in
    reversed order (another summation order of the same sums)."""
    from oracle import c_oracle
    tabs = [np.ascontiguousarray(t[::-1]) if reverse else t for t in ck.train()]
    if len(tabs) == 4:
        return c_oracle.joint_make_iteration(*tabs, *state, eps)
    return c_oracle.make_iteration(*tabs, *state, eps)


def steps(ck, n, prev=False):
    """The oracle's states 1..n iterations after the stored one -> list of n state tuples."""
    return list(_steps(ck.name, n, prev))


@functools.lru_cache(maxsize=None)
def _steps(name, n, prev):
    ck, state, out = load(name), load(name).state(prev), []
    for _ in range(n):
        state = step(ck, state)
        for a in state:
            a.setflags(write=False)
        out.append(state)
    return tuple(out)


def generator():
    """tests/golden/make_converged_golden.py as a module (it is no package)."""
    import importlib.util
    path = os.path.join(os.path.dirname(DIR), "make_converged_golden.py")
    spec = importlib.util.spec_from_file_location("make_converged_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def deviation(got, want):
    """Largest relative deviation over the entries of `want` above 1e-290 in size (below, the
    suite's atol of 1e-300 is no longer negligible)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    big = np.abs(want) > 1e-290
    return float(np.max(np.abs(got[big] - want[big]) / np.abs(want[big]))) if big.any() else 0.0


Drift = collections.namedtuple("Drift", "ids counts start oracle L theta pr dL")
DRIFT_ITERS = 300


@functools.lru_cache(maxsize=None)
def drift():
    """Fit A, seed 1, from its seeded start for DRIFT_ITERS iterations twice on the CPU: the C
    oracle and pivot_model.iterate, two reference-grade orders of the same sums.  -> the link
    table, the start, the oracle's final state and likelihood, and the largest relative deviation
    of theta, p and L between the two runs (what a third order, the GPU's, is held against)."""
    import pivot_model
    from oracle import c_oracle
    tables, start, step_o = generator().setup("A_s1")
    ids, counts = tables["ids"], tables["counts"]
    o = p = start
    for _ in range(DRIFT_ITERS):
        o = step_o(o)
        p = pivot_model.iterate(ids, counts, *p)
    L_o = c_oracle.loglik(ids, counts, *o)
    L_p = pivot_model.loglik(ids, counts, *p)
    return Drift(ids, counts, start, o, L_o, deviation(p[0], o[0]), deviation(p[1], o[1]), abs(L_p - L_o) / abs(L_o))


# ------------------------------------------------------------------------------ scan references
Scores = collections.namedtuple("Scores", "P K theta pr per keys mean known")


@functools.lru_cache(maxsize=None)
def scan_set(label):
    """The parameter set SCAN_SETS[label] with its reference, read-only: theta [B][P][K], pr, per
    f64[B][C(P, 3)] (scan_ref.ref_scores of each slot), the packed keys, the ensemble mean
    (scan_ref.prefix_mean) and the three `known` tables the scan tests use: none, a random 5 % of
    the keys, and the fold's train and test keys."""
    from trigenicinteractionpredictor_amd.scan import known_keys
    cks = [load(n) for n in SCAN_SETS[label]]
    th, pr = np.stack([c.theta for c in cks]), np.stack([c.pr for c in cks])
    per, keys = [], None
    for c in cks:
        s, keys = scan_ref.ref_scores(c.theta, c.pr)
        per.append(s)
    per = np.stack(per)
    mean = scan_ref.prefix_mean(per, len(cks))
    P = cks[0].P
    rng = np.random.default_rng(5)
    known = {"none": None, "random": np.sort(rng.choice(keys, keys.size // 20, replace=False)),
             "fold": known_keys((P, cks[0].ids, cks[0].test_ids))}
    for a in (th, pr, per, keys, mean, known["random"], known["fold"]):
        a.setflags(write=False)
    return Scores(P, cks[0].K, th, pr, per, keys, mean, known)


KNOWN = ("none", "random", "fold")


def eligible_desc(scores, keys, known=None):
    """The eligible reference scores, descending."""
    return census_ref.eligible(scores, keys, known)[::-1]


def clear_cuts(scores, lo, hi):
    """The cut positions n in [lo, hi] of a DESCENDING score list at which a top-n set is
    determined: the relative gap between the n-th and the (n + 1)-th score exceeds census_ref.GAP
    (n = len(scores) is no cut: that list is everything)."""
    s = np.asarray(scores, dtype=np.float64)
    assert s.size < 2 or (s[:-1] >= s[1:]).all()
    lo, hi = max(int(lo), 1), min(int(hi), s.size - 1)
    if hi < lo:
        return np.zeros(0, dtype=np.int64)
    n = np.arange(lo, hi + 1)
    return n[(s[n - 1] - s[n]) > census_ref.GAP * np.abs(s[n - 1])]


def tight_gaps(scores, n, at=1e-9):
    """The adjacent relative gaps at or below `at` inside the first n of a descending list."""
    s = np.asarray(scores, dtype=np.float64)[:n]
    return int(np.count_nonzero((s[:-1] - s[1:]) <= at * np.abs(s[:-1])))


def mid_threshold(scores, n):
    """The threshold in the middle of the gap under the n-th of a descending list."""
    return float((scores[n - 1] + scores[n]) / 2)


def check_set_cut(got_scores, got_ids, ref_scores, ref_keys, n, known, P):
    """A top-n list of one of the scan families against the reference (all scores, all keys, in
    key order) at a clear cut n.  On the reference alone first: the gap under its n-th eligible
    score exceeds census_ref.GAP.  Then: the returned key set is the reference's top-n set; every
    score is within RTOL (atol 0) of the reference score of its own key; the list is sorted by its
    own bits, score descending, bit-equal scores by key ascending; keys unique; ids =
    keys_to_ids(keys); no key in `known`."""
    want_s, want_k = scan_ref.top(ref_scores, ref_keys, n, known)
    assert want_s.size == n + 1, (want_s.size, n)
    assert clear_cuts(want_s, n, n).size == 1, ("not a clear cut", n, want_s[n - 1], want_s[n])
    got_scores, got_ids = np.asarray(got_scores), np.asarray(got_ids)
    assert got_ids.dtype == np.int32 and got_scores.dtype == np.float64
    assert got_ids.shape == (n, 3) and got_scores.shape == (n,), (got_ids.shape, got_scores.shape, n)
    assert np.isfinite(got_scores).all()
    got_k = scan_ref.packed(got_ids, P)
    np.testing.assert_array_equal(got_ids, scan_ref.keys_to_ids(got_k, P))
    assert np.unique(got_k).size == n, "repeated keys"
    missing = np.setdiff1d(want_k[:n], got_k)
    extra = np.setdiff1d(got_k, want_k[:n])
    assert not missing.size and not extra.size, ("missing", missing[:5], "extra", extra[:5])
    at = np.searchsorted(ref_keys, got_k)
    np.testing.assert_array_equal(ref_keys[at], got_k)
    np.testing.assert_allclose(got_scores, ref_scores[at], rtol=RTOL, atol=0)
    down = got_scores[:-1] > got_scores[1:]
    tie = (got_scores[:-1] == got_scores[1:]) & (got_k[:-1] < got_k[1:])
    bad = np.flatnonzero(~(down | tie))
    assert not bad.size, ("not in the scan's order at", bad[:5], got_scores[bad[:5]], got_k[bad[:5]])
    if known is not None and len(known):
        assert not np.isin(got_k, known).any()
    return got_k


def clear_cuts_abs(desc, lo, hi):
    """clear_cuts for spreads: the cut positions n in [lo, hi] of a DESCENDING spread list at which
    the ABSOLUTE gap between the n-th and the (n + 1)-th spread exceeds census_ref.GAP."""
    s = np.asarray(desc, dtype=np.float64)
    assert (s[:-1] >= s[1:]).all()
    n = np.arange(max(int(lo), 1), min(int(hi), s.size - 1) + 1)
    return n[(s[n - 1] - s[n]) > census_ref.GAP]


def check_set_cut_abs(got_scores, got_ids, d, tol, ref_keys, n, known, P):
    """check_set_cut for spreads: on the reference alone, n is a clear cut (absolute gap); then the
    returned key set is the reference's top-n set, every spread is within its own key's absolute
    tolerance `tol` (spread_ref.atol) of the reference, and the list is sorted by its own bits under
    the scan's order."""
    want_s, want_k = scan_ref.top(d, ref_keys, n, known)
    assert want_s.size == n + 1 and clear_cuts_abs(want_s, n, n).size == 1, ("not a clear cut", n)
    assert got_ids.dtype == np.int32 and got_scores.dtype == np.float64
    assert got_ids.shape == (n, 3) and got_scores.shape == (n,)
    assert np.isfinite(got_scores).all() and (got_scores >= 0).all()
    got_k = scan_ref.packed(got_ids, P)
    np.testing.assert_array_equal(got_ids, scan_ref.keys_to_ids(got_k, P))
    assert np.unique(got_k).size == n, "repeated keys"
    missing, extra = np.setdiff1d(want_k[:n], got_k), np.setdiff1d(got_k, want_k[:n])
    assert not missing.size and not extra.size, ("missing", missing[:5], "extra", extra[:5])
    at = np.searchsorted(ref_keys, got_k)
    np.testing.assert_array_equal(ref_keys[at], got_k)
    assert (np.abs(got_scores - d[at]) <= tol[at]).all(), float(np.max(np.abs(got_scores - d[at]) - tol[at]))
    down = got_scores[:-1] > got_scores[1:]
    tie = (got_scores[:-1] == got_scores[1:]) & (got_k[:-1] < got_k[1:])
    bad = np.flatnonzero(~(down | tie))
    assert not bad.size, ("not in the scan's order at", bad[:5], got_scores[bad[:5]], got_k[bad[:5]])
    if known is not None and len(known):
        assert not np.isin(got_k, known).any()
    return got_k


def pick_cuts(desc):
    """The two N of the scan tests: the largest clear cut <= 4096 and the middle one of [64, 512]."""
    big = clear_cuts(desc, 513, 4096)
    small = clear_cuts(desc, 64, 512)
    assert big.size and small.size
    return int(big[-1]), int(small[small.size // 2])


@functools.lru_cache(maxsize=None)
def random_pair_mask_words(P):
    """10 % of the gene pairs, blocked through scan.pair_mask -> the mask alone (no key table: that
    one goes through all P^3 triples, too many at the screen scan's wide rows)."""
    from trigenicinteractionpredictor_amd.scan import pair_mask
    rng = np.random.default_rng(P)
    i, j = np.triu_indices(P, k=1)
    pick = rng.random(i.size) < 0.1
    return pair_mask(P, pairs=np.stack([i[pick], j[pick]], axis=1))


@functools.lru_cache(maxsize=None)
def random_pair_mask(P):
    """random_pair_mask_words(P) -> (mask, the key table it stands for)."""
    mask = random_pair_mask_words(P)
    import masked_ref
    keys = masked_ref.expand(mask, P)
    assert 0 < keys.size < P * (P - 1) * (P - 2) // 6
    return mask, keys
