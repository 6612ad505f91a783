"""Helper of tests/test_ratings_host.py and tests/test_gpu_ratings.py (not a test): link tables
with R rating classes, some of them never observed, and a direct numpy.longdouble restatement of
the model's formulas.

    T_e[a][b][g][r] = theta_i[a] theta_j[b] theta_k[g] p[a][b][g][r]      (link e = (i, j, k))
    d_e[r]          = eps + sum_abg T_e[a][b][g][r]
    c_e[r]          = n_e[r] / d_e[r]
    n theta_i[a]    = sum over the links holding i (once per slot) of sum_bgr c_e[r] T_e[a][b][g][r]
    n p[a][b][g][r] = sum_e c_e[r] T_e[a][b][g][r]
    theta'          = n theta / degree,      p' = n p / (eps + sum_r n p)
    L               = sum_e sum_r n_e[r] log d_e[r]
    P(r = 1)        = sum_abg T_e[a][b][g][1]                              (no eps)

and the same with two genes and q[a][b][r] for a pair link; the joint model adds both arities
into one n theta and one degree.  Written from these formulas alone: no oracle, no pivot_model,
no product code.
"""
import numpy as np

LD = np.longdouble
BLOCK = 128     # links per broadcast block (bounds the [E][K][K][K][R] temporary)


# ------------------------------------------------------------------------------ link tables
def _counts_row(rng, R, live, multi, both):
    c = [0] * R
    r = int(live[rng.integers(len(live))])
    c[r] = int(rng.integers(2, 5)) if rng.random() < multi else 1
    if rng.random() < both and len(live) > 1:
        others = [x for x in live if x != r]
        c[int(others[rng.integers(len(others))])] = 1
    return c


def _table(P, E, R, seed, arity, empty, multi, both, repeat):
    rng = np.random.default_rng(seed)
    live = [r for r in range(R) if r not in set(empty)]
    assert live and E * arity >= P
    seen, ids, counts = set(), [], []

    def add(t):
        t = tuple(sorted(t, key=str))      # the slots in the keys' string-sorted order
        if t in seen:
            return
        seen.add(t)
        ids.append(t)
        counts.append(_counts_row(rng, R, live, multi, both))

    perm = rng.permutation(P).tolist()     # coverage: every gene in at least one link
    perm += perm[:(-len(perm)) % arity]
    for q in range(0, len(perm), arity):
        add(perm[q:q + arity])
    while len(ids) < E:
        if rng.random() < repeat:
            t = rng.choice(P, arity - 1, replace=False).tolist()
            t.append(t[0])                 # a repeated gene
        else:
            t = rng.choice(P, arity, replace=False).tolist()
        add(t)
    ids, counts = np.array(ids, dtype=np.int32), np.array(counts, dtype=np.int32)
    assert ids.shape == (E, arity) and np.unique(ids).size == P
    assert not counts[:, list(empty)].any() and (counts[:, live].sum(axis=0) > 0).all()
    return ids, counts


def links(P, E, R, seed, empty=(), multi=0.05, both=0.03, repeat=0.01):
    """-> (ids int32[E][3], counts int32[E][R]); ratings in `empty` never receive a count, every
    other rating does, every gene of [0, P) has a link."""
    return _table(P, E, R, seed, 3, empty, multi, both, repeat)


def pair_links(P, E, R, seed, empty=(), multi=0.05, both=0.03):
    """The same for pair links -> (ids int32[E][2], counts int32[E][R])."""
    return _table(P, E, R, seed, 2, empty, multi, both, 0.0)


def params(P, K, R, seed, pairs=False):
    """Random row-normalised theta [P][K] and rating-normalised p [K][K][K][R] (q [K][K][R] with
    `pairs`); each rating's lattice has its own scale (1, 1/2, 1/3, ...), so a slice read for
    another rating shows."""
    rng = np.random.default_rng(seed)
    th = rng.random((P, K)) + 0.05
    th /= th.sum(axis=1, keepdims=True)
    shape = (K, K, R) if pairs else (K, K, K, R)
    lat = (rng.random(shape) + 0.05) / np.arange(1, R + 1)
    lat /= lat.sum(axis=-1, keepdims=True)
    return th, lat


# ------------------------------------------------------------------------------ direct formulas
def _terms(ids, theta, lat):
    """T [E][K]..[K][R] of a block of links of either arity, in longdouble."""
    th = np.asarray(theta, dtype=LD)
    A = ids.shape[1]
    T = np.asarray(lat, dtype=LD)[None]
    for s in range(A):
        shape = [ids.shape[0]] + [1] * (A + 1)
        shape[1 + s] = th.shape[1]
        T = T * th[ids[:, s]].reshape(shape)
    return T


def _blocks(ids):
    for lo in range(0, ids.shape[0], BLOCK):
        yield slice(lo, min(lo + BLOCK, ids.shape[0]))


def accumulate(ids, counts, theta, lat, eps=1e-10, nth=None):
    """-> (n theta [P][K], n lattice like `lat`) in longdouble; `nth` continues a running sum."""
    ids, counts = np.asarray(ids, dtype=np.int64), np.asarray(counts)
    A = ids.shape[1]
    nth = np.zeros(np.shape(theta), dtype=LD) if nth is None else nth
    nlat = np.zeros(np.shape(lat), dtype=LD)
    for b in _blocks(ids):
        T = _terms(ids[b], theta, lat)
        cell_axes = tuple(range(1, A + 1))
        d = LD(eps) + T.sum(axis=cell_axes)                       # [E][R]
        W = T * (counts[b].astype(LD) / d).reshape((-1,) + (1,) * A + (d.shape[1],))
        nlat += W.sum(axis=0)
        for s in range(A):
            other = tuple(x for x in range(1, A + 2) if x != 1 + s)
            np.add.at(nth, ids[b][:, s], W.sum(axis=other))
    return nth, nlat


def degree(P, *tables):
    deg = np.zeros(P, dtype=np.int64)
    for ids in tables:
        deg += np.bincount(np.asarray(ids, dtype=np.int64).ravel(), minlength=P)[:P]
    return deg


def _normalise(nlat, eps):
    return nlat / (LD(eps) + nlat.sum(axis=-1, keepdims=True))


def iteration(ids, counts, theta, pr, eps=1e-10):
    """One EM iteration -> (theta', p') in longdouble."""
    nth, npr = accumulate(ids, counts, theta, pr, eps)
    return nth / degree(nth.shape[0], ids)[:, None].astype(LD), _normalise(npr, eps)


def joint_iteration(ids3, counts3, ids2, counts2, theta, pr, qr, eps=1e-10):
    """One iteration of the joint model -> (theta', p', q') in longdouble."""
    nth, npr = accumulate(ids3, counts3, theta, pr, eps)
    nth, nqr = accumulate(ids2, counts2, theta, qr, eps, nth=nth)
    deg = degree(nth.shape[0], ids3, ids2)
    return nth / deg[:, None].astype(LD), _normalise(npr, eps), _normalise(nqr, eps)


def loglik(ids, counts, theta, lat, eps=1e-10):
    ids, counts = np.asarray(ids, dtype=np.int64), np.asarray(counts)
    total = LD(0)
    for b in _blocks(ids):
        T = _terms(ids[b], theta, lat)
        d = LD(eps) + T.sum(axis=tuple(range(1, ids.shape[1] + 1)))
        n = counts[b].astype(LD)
        total += np.where(n > 0, n * np.log(d), LD(0)).sum()      # an unobserved rating adds 0
    return total


def predict(ids, theta, lat):
    """P(r = 1) of each row of ids (either arity) in longdouble."""
    ids = np.asarray(ids, dtype=np.int64)
    out = np.zeros(ids.shape[0], dtype=LD)
    for b in _blocks(ids):
        T = _terms(ids[b], theta, lat)
        out[b] = T[..., 1].sum(axis=tuple(range(1, ids.shape[1] + 1)))
    return out


def f64(*arrays):
    """longdouble results rounded to float64 (what the oracles are compared with)."""
    out = tuple(np.asarray(a, dtype=np.float64) for a in arrays)
    return out if len(out) > 1 else out[0]


def max_rel(got, want):
    """Largest relative error over the elements where `want` is not 0."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nz = want != 0
    if not nz.any():
        return 0.0
    return float(np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz])))
