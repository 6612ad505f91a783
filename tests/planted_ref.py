"""A planted block model whose scan answers are closed-form, for tests/test_planted_host.py and
tests/test_gpu_scale.py: the reference of the scan families at sizes where numpy cannot score all
C(P, 3) triples.  numpy only: no GPU, no product code beyond the rank order.

The model.  The K groups split into Ke elite and Kc = K - Ke common groups.  All but E genes are
COMMON: their theta row is one-hot on a common group, the same in every slot.  E genes are ELITE: a
dense random row on the elite groups only, drawn per slot.  The genes are placed by rank POSITION
(theta[order[position]]); the elites sit where kernels go wrong (positions 0, 1, 15, 16, 17, both
sides of 64-row block edges, P - 2, P - 1, the ragged last tile) and otherwise at random.  The
rating-1 probabilities p[x][y][z] are drawn from [0.2, 0.9] where x, y, z are all elite, are exactly
MIXED = 1e-6 where elite and common indices mix, and are a per-slot permutation of Kc^3 distinct
values in [1e-3, 1e-2] where all three are common.

What follows.  The score phase (csrc/scan_score.h) forms T_a = sum_x th[x] p[x].., W = sum_y .. and
S = sum_z .. by fused multiply-adds from zero.  For a common gene every factor is 1.0 or 0.0, every
product is the other factor or zero and every sum adds zeros, so
  - an all-common triple at positions a < b < c scores p[g_a][g_b][g_c] bit for bit, in every slot
    (its CLASS value), and the ensemble mean is scan_ref.prefix_mean of the class values;
  - a triple with a common and an elite gene scores MIXED times a sum of theta products <= 1: at
    most MIXED (1 + 1e-12); any triple with a common gene scores at most 1e-2;
  - an all-elite triple scores at least 0.2 (1 - 1e-12).  There are C(E, 3) of them: numpy scores
    them outright (scan_ref.ref_scores on the gathered rows, the keys rewritten to the big P).
So counts are sums of class sizes, which prefix counts give in O(P K^2), plus what a brute-force list
of the elites adds, minus the known keys that would have counted."""
import collections
import functools
from math import comb

import numpy as np

import census_ref
import scan_ref

MIXED = 1e-6                 # p where elite and common indices mix
MIXED_TOP = MIXED * (1 + 1e-9)   # no mixed triple scores above this
BELOW_ALL = 1e-7             # a threshold below every score of the model
COMMON_LO, COMMON_HI = 1e-3, 1e-2
ELITE_LO, ELITE_HI = 0.2, 0.9
BETWEEN = 0.05               # a threshold between the common and the elite band

Planted = collections.namedtuple("Planted", "theta pr P K Ke Kc B E label elite_pos N cv per keys")
# label int64[P] by position: the common group's index in [0, Kc), Kc for an elite.  N int64
# [Kc + 1]^3 = class_counts(label).  cv f64[B][Kc][Kc][Kc]: the class values per slot.  per
# f64[B][C(E, 3)], keys int64[C(E, 3)] ascending: the elite triples' scores per slot.


def edge_positions(P):
    """Where kernels go wrong: tile and 64-row block edges, the ends, the ragged last tile."""
    last = 16 * ((P - 1) // 16)
    want = [0, 1, 15, 16, 17, 63, 64, 127, 128, P - 2, P - 1, last, last + (P - 1 - last) // 2,
            64 * ((P - 1) // 64) - 1, 64 * ((P - 1) // 64)]
    return np.unique([p for p in want if 0 <= p < P])


def group_sizes(n, Kc, small):
    """n common genes over Kc groups, deliberately unequal: two groups of about `small` (the second
    a quarter larger), the rest growing 2 : 3 : 4 : ..."""
    sizes = [min(small, n // Kc), min(small + small // 4, n // Kc)]
    w = np.arange(2, Kc) if Kc > 2 else np.zeros(0)
    rest = n - sum(sizes)
    big = [int(rest * x / w.sum()) for x in w]
    big[-1] += rest - sum(big)
    return np.array(sizes + big, dtype=np.int64)


def class_counts(label, G=None):
    """N[x][y][z] = the triples of positions a < b < c with label[a] = x, label[b] = y,
    label[c] = z, int64 and exact, in O(P G^2) from prefix counts."""
    label = np.asarray(label, dtype=np.int64)
    G = int(label.max()) + 1 if G is None else G
    onehot = np.zeros((label.size, G), dtype=np.int64)
    onehot[np.arange(label.size), label] = 1
    before = np.cumsum(onehot, axis=0) - onehot             # positions < b per label
    after = onehot.sum(axis=0) - before - onehot            # positions > b per label
    N = np.zeros((G, G, G), dtype=np.int64)
    for y in range(G):
        at = label == y
        N[:, y, :] = before[at].T @ after[at]
    return N


@functools.lru_cache(maxsize=None)
def build(P, K=10, Ke=4, E=96, B=1, seed=0, small=200, alpha=0.5, best=None, small_top=False):
    """The planted model, read-only; computed once.  best: a common class (x, y, z) in [0, Kc)^3
    that gets the largest class value in every slot (None: wherever the permutation puts it).
    small_top: the eight classes of the two small groups get the eight largest values in every slot,
    so a threshold under the eighth counts the small groups' triples alone."""
    rng = np.random.default_rng(seed)
    Kc = K - Ke
    order, _ = scan_ref.rank_tables(P)
    elite_pos = np.zeros(0, dtype=np.int64)
    if E:
        edges = edge_positions(P)[:E]
        free = np.setdiff1d(np.arange(P), edges)
        elite_pos = np.sort(np.concatenate([edges, rng.choice(free, E - edges.size, replace=False)]))
    label = np.full(P, Kc, dtype=np.int64)
    common = np.setdiff1d(np.arange(P), elite_pos)
    label[rng.permutation(common)] = np.repeat(np.arange(Kc), group_sizes(common.size, Kc, small))
    theta = np.zeros((B, P, K))
    theta[:, order[common], Ke + label[common]] = 1.0
    if E:
        dense = rng.dirichlet(np.full(Ke, alpha), size=(B, E))
        dense = np.maximum(dense, 1e-3)
        theta[:, order[elite_pos], :Ke] = dense / dense.sum(axis=2, keepdims=True)
    p1 = np.full((B, K, K, K), MIXED)
    p1[:, :Ke, :Ke, :Ke] = rng.uniform(ELITE_LO, ELITE_HI, (B, Ke, Ke, Ke))
    values = np.geomspace(COMMON_LO, COMMON_HI, Kc ** 3)
    cv = np.stack([rng.permutation(values).reshape(Kc, Kc, Kc) for _ in range(B)])
    if best is not None:
        for s in range(B):
            top = np.unravel_index(np.argmax(cv[s]), cv[s].shape)
            cv[s][top], cv[s][best] = cv[s][best], cv[s][top]
    if small_top:
        for s in range(B):
            flat = cv[s].reshape(-1)
            want = np.array([(x * Kc + y) * Kc + z for x in (0, 1) for y in (0, 1) for z in (0, 1)])
            want = rng.permutation(want)                # which of the eight gets which value: per slot
            for at in want:                             # swap the largest value not yet placed into it
                free = np.setdiff1d(np.arange(flat.size), want[:np.flatnonzero(want == at)[0]])
                top = free[np.argmax(flat[free])]
                flat[at], flat[top] = flat[top], flat[at]
    p1[:, Ke:, Ke:, Ke:] = cv
    pr = np.stack([1.0 - p1, p1], axis=4)
    per, keys = elite_scores(theta, pr, elite_pos, P)
    N = class_counts(label, Kc + 1)
    for a in (theta, pr, label, elite_pos, N, cv, per, keys):
        a.setflags(write=False)
    return Planted(theta, pr, P, K, Ke, Kc, B, E, label, elite_pos, N, cv, per, keys)


def elite_scores(theta, pr, elite_pos, P):
    """scan_ref.ref_scores of the elite rows per slot -> (per f64[B][C(E, 3)], keys of the big P)."""
    B, E = theta.shape[0], elite_pos.size
    if E < 3:
        return np.zeros((B, 0)), np.zeros(0, dtype=np.int64)
    order, _ = scan_ref.rank_tables(P)
    _, rank_e = scan_ref.rank_tables(E)
    per = []
    for s in range(B):
        rows = theta[s][order[elite_pos]]               # row i: the i-th elite position
        scores, k = scan_ref.ref_scores(rows[rank_e], pr[s])    # ref_scores reads theta[order_E]
        per.append(scores)
    a, b, c = elite_pos[k // (E * E)], elite_pos[(k // E) % E], elite_pos[k % E]
    keys = (a * P + b) * P + c
    assert (np.diff(keys) > 0).all()
    return np.stack(per), keys


def slots_of(model, sample=None, ns=None):
    """The scored slots of a call: that one slot, or the active prefix of ns (None: all B)."""
    return [int(sample)] if sample is not None else list(range(model.B if ns is None else ns))


def class_values(model, sample=None, ns=None):
    """The score of every common class under the call's mode, f64[Kc][Kc][Kc], bit for bit."""
    sl = slots_of(model, sample, ns)
    return scan_ref.prefix_mean(model.cv[sl], len(sl))


def elite_values(model, sample=None, ns=None):
    sl = slots_of(model, sample, ns)
    return scan_ref.prefix_mean(model.per[sl], len(sl))


def positions(keys, P):
    keys = np.asarray(keys, dtype=np.int64)
    return keys // (P * P), (keys // P) % P, keys % P


def classify(model, keys):
    """-> (kind int8 per key: 0 all common, 1 mixed, 2 all elite; the common class index tuple
    (valid where kind = 0); the index into model.keys (valid where kind = 2))."""
    a, b, c = positions(keys, model.P)
    la, lb, lc = model.label[a], model.label[b], model.label[c]
    n_elite = (la == model.Kc).astype(int) + (lb == model.Kc) + (lc == model.Kc)
    kind = np.where(n_elite == 0, 0, np.where(n_elite == 3, 2, 1)).astype(np.int8)
    at = np.searchsorted(model.keys, keys) if model.keys.size else np.zeros(len(keys), dtype=np.int64)
    at = np.minimum(at, max(model.keys.size - 1, 0))
    cls = (np.minimum(la, model.Kc - 1), np.minimum(lb, model.Kc - 1), np.minimum(lc, model.Kc - 1))
    if model.keys.size:
        assert (model.keys[at[kind == 2]] == np.asarray(keys)[kind == 2]).all()
    return kind, cls, at


def key_values(model, keys, cval, eval_):
    """Per key the reference value: the class value, the elite list's, MIXED for a mixed triple
    (an upper bound, and below every threshold above MIXED_TOP)."""
    kind, cls, at = classify(model, keys)
    out = np.full(len(keys), MIXED)
    out[kind == 0] = cval[cls[0][kind == 0], cls[1][kind == 0], cls[2][kind == 0]]
    if model.keys.size:
        out[kind == 2] = eval_[at[kind == 2]]
    return out


def n_mixed(model):
    N = model.N
    return comb(model.P, 3) - int(N[:model.Kc, :model.Kc, :model.Kc].sum()) - comb(model.E, 3)


def assert_thresholds(model, thresholds, cval, eval_):
    """The precondition: every threshold is further than census_ref.GAP relative from every class
    value and every elite score, and outside the mixed triples' sliver below MIXED_TOP."""
    t = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    census_ref.assert_clear(np.concatenate([cval.reshape(-1), eval_]), t)
    assert ((t > MIXED_TOP * (1 + 1e-3)) | (t < MIXED * 0.5)).all(), t


def census(model, thresholds, known=None, sample=None, ns=None):
    """-> (counts int64[M], total): the census's closed form."""
    cval, ev = class_values(model, sample, ns), elite_values(model, sample, ns)
    t = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    assert_thresholds(model, t, cval, ev)
    Nc = model.N[:model.Kc, :model.Kc, :model.Kc]
    es = np.sort(ev)
    counts = np.array([int(Nc[cval >= x].sum()) + int(es.size - np.searchsorted(es, x, side="left"))
                       + (n_mixed(model) if x < MIXED * 0.5 else 0) for x in t], dtype=np.int64)
    total = comb(model.P, 3)
    if known is not None and len(known):
        kv = key_values(model, known, cval, ev)
        counts -= (kv[None, :] >= t[:, None]).sum(axis=1)
        total -= len(known)
    return counts, total


def thresholds(model, sample=None, ns=None, n_common=3, n_elite=3, extra=(BELOW_ALL, BETWEEN)):
    """Midpoints of wide gaps in both bands, one between the bands and one below everything."""
    cval, ev = class_values(model, sample, ns), elite_values(model, sample, ns)
    out = list(extra)
    for values, n in ((cval.reshape(-1), n_common), (ev, n_elite)):
        s = np.unique(values)
        if s.size < 2 or not n:
            continue
        wide = np.flatnonzero((s[1:] - s[:-1]) > 1e-6 * s[1:])
        pick = wide[np.linspace(0, wide.size - 1, n + 2).astype(int)[1:-1]]
        out += ((s[pick] + s[pick + 1]) / 2).tolist()
    out = np.array(out)
    assert_thresholds(model, out, cval, ev)
    return out


def vote_thresholds(model):
    """Two common-band thresholds that every slot's values clear (the slots hold the same values,
    permuted): the median gap, where the histogram fills every bin, and the gap under the largest
    value, where all but at most ns classes stay at zero votes."""
    v = np.sort(model.cv[0].reshape(-1))
    return float((v[v.size // 2 - 1] + v[v.size // 2]) / 2), float((v[-2] + v[-1]) / 2)


def votes(model, threshold, ns=None, known=None):
    """-> hist int64[ns + 1]: the vote histogram's closed form over the first ns slots."""
    ns = model.B if ns is None else ns
    for s in range(ns):
        assert_thresholds(model, [threshold], model.cv[s], model.per[s])
    assert threshold > MIXED_TOP * (1 + 1e-3)           # a mixed triple never votes
    Nc = model.N[:model.Kc, :model.Kc, :model.Kc]
    cvotes = (model.cv[:ns] >= threshold).sum(axis=0)
    evotes = (model.per[:ns] >= threshold).sum(axis=0)
    hist = np.bincount(cvotes.reshape(-1), weights=Nc.reshape(-1), minlength=ns + 1).astype(np.int64)
    hist += np.bincount(evotes, minlength=ns + 1)
    hist[0] += n_mixed(model)
    if known is not None and len(known):
        hist -= np.bincount(key_votes(model, known, threshold, ns), minlength=ns + 1)
    return hist


def key_votes(model, keys, threshold, ns):
    out = np.zeros(len(keys), dtype=np.int64)
    for s in range(ns):
        out += key_values(model, keys, model.cv[s], model.per[s]) >= threshold
    return out


def pair_tables(model, hit_class, mixed_hit):
    """The pair matrix without the elite triples and the known keys, in factored form: -> (row
    int64[P][G], col int64[P][G]) with count[i][j] = row[i][label[j]] + col[j][label[i]] for
    positions i < j.  For such a pair the third gene adds class (g, g_i, g_j) before i,
    (g_i, g, g_j) between and (g_i, g_j, g) after j; prefix counts of the labels give each part in
    O(P G^2).  hit_class bool[Kc][Kc][Kc]: the common classes that count; mixed_hit: whether the
    mixed triples do; the all-elite class never does here."""
    P, Kc, G = model.P, model.Kc, model.Kc + 1
    H = np.full((G, G, G), bool(mixed_hit))
    H[:Kc, :Kc, :Kc] = hit_class
    H[Kc, Kc, Kc] = False                               # the elites come from their list
    H = H.astype(np.int64)
    label = model.label
    onehot = np.zeros((P, G), dtype=np.int64)
    onehot[np.arange(P), label] = 1
    cum = np.concatenate([np.zeros((1, G), np.int64), np.cumsum(onehot, axis=0)])   # cum[p]: positions < p
    before, upto, after = cum[:P], cum[1:], cum[P] - cum[1:]
    row, col = np.zeros((P, G), dtype=np.int64), np.zeros((P, G), dtype=np.int64)
    for y in range(G):
        at = label == y                                 # row[i][z] with g_i = y, col[j][y'] with g_j = y
        row[at] = before[at] @ H[:, y, :] - upto[at] @ H[y, :, :]
        col[at] = (before[at] @ H[:, :, y].T) + (after[at] @ H[:, y, :].T)
    return row, col


def pair_matrix(model, hit_class, elite_hit, mixed_hit, known=None, known_hit=None):
    """One column of a pair matrix in rank positions, int32 [P][P], x < y filled: per pair the
    triples that contain it and count.  pair_tables' part, then the elite triples of elite_hit
    bool[C(E, 3)] scattered to their three pairs and the known keys of known_hit taken out."""
    P = model.P
    row, col = pair_tables(model, hit_class, mixed_hit)
    out = np.triu(row[:, model.label] + col[:, model.label].T, k=1)
    if model.keys.size and elite_hit.any():
        a, b, c = positions(model.keys[elite_hit], P)
        for x, y in ((a, b), (a, c), (b, c)):
            np.add.at(out, (x, y), 1)
    if known is not None and len(known) and known_hit.any():
        a, b, c = positions(np.asarray(known)[known_hit], P)
        for x, y in ((a, b), (a, c), (b, c)):
            np.subtract.at(out, (x, y), 1)
    assert out.min() >= 0 and out.max() < 2 ** 31
    return out.astype(np.int32)


def pair_census(model, thresholds, known=None, sample=None, ns=None):
    """-> int32 [P][P][M] in rank positions, x < y filled: the pair census's closed form."""
    cval, ev = class_values(model, sample, ns), elite_values(model, sample, ns)
    t = np.asarray(thresholds, dtype=np.float64).reshape(-1)
    assert_thresholds(model, t, cval, ev)
    kv = key_values(model, known, cval, ev) if known is not None and len(known) else None
    cols = [pair_matrix(model, cval >= x, ev >= x, x < MIXED * 0.5, known, None if kv is None else kv >= x)
            for x in t]
    return np.stack(cols, axis=2) if cols else np.zeros((model.P, model.P, 0), np.int32)


def pair_votes(model, threshold, levels, ns=None, known=None):
    """-> int32 [P][P][M] in rank positions, x < y filled: the pair vote census's closed form."""
    ns = model.B if ns is None else ns
    for s in range(ns):
        assert_thresholds(model, [threshold], model.cv[s], model.per[s])
    assert threshold > MIXED_TOP * (1 + 1e-3)
    cvotes = (model.cv[:ns] >= threshold).sum(axis=0)
    evotes = (model.per[:ns] >= threshold).sum(axis=0)
    kvotes = key_votes(model, known, threshold, ns) if known is not None and len(known) else None
    cols = [pair_matrix(model, cvotes >= v, evotes >= v, False, known, None if kvotes is None else kvotes >= v)
            for v in levels]
    return np.stack(cols, axis=2) if cols else np.zeros((model.P, model.P, 0), np.int32)


def gene_counts(rank_mat):
    """Per gene id, the row sums of the symmetric matrix halved: int64 [P][M]."""
    P = rank_mat.shape[0]
    order, _ = scan_ref.rank_tables(P)
    m = rank_mat.astype(np.int64)
    by_pos = (m.sum(axis=1) + m.sum(axis=0)) // 2
    out = np.empty_like(by_pos)
    out[order] = by_pos
    return out


def first_keys(model, cls, n, known=None):
    """The first n packed keys, ascending, of the common class cls = (x, y, z) outside `known`, by
    lazy enumeration: the exact top n where every candidate ties."""
    P = model.P
    La, Lb, Lc = (np.flatnonzero(model.label == g) for g in cls)
    skip = set() if known is None else set(np.asarray(known).tolist())
    out = []
    for a in La:
        for b in Lb[np.searchsorted(Lb, a, side="right"):]:
            cs = Lc[np.searchsorted(Lc, b, side="right"):]
            keys = ((a * P + b) * P + cs).tolist()
            out += [k for k in keys if k not in skip] if skip else keys
            if len(out) >= n:
                return np.array(out[:n], dtype=np.int64)
    return np.array(out, dtype=np.int64)


def best_class(model, sample=None, ns=None):
    """The common class with the largest value under the call's mode and that value."""
    cval = class_values(model, sample, ns)
    cls = np.unravel_index(np.argmax(cval), cval.shape)
    return tuple(int(g) for g in cls), float(cval[cls])


ITEM_A = 5


def item_block(P):
    """The first row of the 64-row block of b that holds the work item's known keys."""
    return 64 * max(1, (P // 3) // 64)


def known_keys(model, n_item=100000, n_spread=200000, n_best=50, seed=1, stats=()):
    """Sorted unique known keys: n_item of them inside ONE work item's range (one a, one 64-row
    block of b), n_spread random triples over the whole triangle and the n_best best elite triples
    under each statistic of `stats` (arrays over model.keys)."""
    P = model.P
    rng = np.random.default_rng(seed)
    a, b0 = ITEM_A, item_block(P)
    bs = np.arange(b0, min(b0 + 64, P - 1))
    pool = np.concatenate([(a * P + b) * P + np.arange(b + 1, P) for b in bs])
    parts = [rng.choice(pool, min(n_item, pool.size), replace=False)]
    pos = np.sort(np.stack([rng.integers(0, P, n_spread) for _ in range(3)], axis=1), axis=1)
    pos = pos[(pos[:, 0] < pos[:, 1]) & (pos[:, 1] < pos[:, 2])]
    parts.append((pos[:, 0] * P + pos[:, 1]) * P + pos[:, 2])
    for stat in stats:
        parts.append(model.keys[np.argsort(-stat, kind="stable")[:n_best]])
    return np.unique(np.concatenate(parts))


def confined_mask(P, universe, blocked=()):
    """The pair mask (scan.pair_mask's layout: uint32 [P16][MW] in rank positions, bit y & 31 of
    mask[x][y >> 5] set = the pair of positions (x, y) is BLOCKED) that blocks every pair but those
    inside `universe` (positions), and the `blocked` pairs of positions too.  Packed one row
    pattern at a time with np.packbits: no [P][P] array of 64-bit words is ever made.  The diagonal,
    rows >= P and bits >= P stay zero."""
    P16 = max(16, (P + 15) // 16 * 16)                  # masked_ref.shape
    MW = (P16 + 31) // 32
    universe = np.asarray(universe, dtype=np.int64)
    bits = np.zeros(32 * MW, dtype=np.uint8)
    bits[:P] = 1
    every = np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)
    bits[universe] = 0
    outside = np.packbits(bits, bitorder="little").view("<u4").astype(np.uint32)
    out = np.zeros((P16, MW), dtype=np.uint32)
    out[:P] = every
    out[universe] = outside
    at = np.arange(P)
    out[at, at >> 5] &= ~(np.uint32(1) << (at & 31).astype(np.uint32))
    for i, j in blocked:
        out[i, j >> 5] |= np.uint32(1 << (j & 31))
        out[j, i >> 5] |= np.uint32(1 << (i & 31))
    return out


# ------------------------------------------------------------------ top-N lists
def stat(model, what="mean", arg=None, sample=None, ns=None):
    """The elite triples' statistic under a call's mode, over model.keys: the ensemble "mean", the
    "quorum" score q_m (arg = m: the m-th largest of the slots' scores) or the "spread" d_t
    (arg = t: the (1 + t)-th largest minus the (1 + t)-th smallest)."""
    sl = slots_of(model, sample, ns)
    per = model.per[sl]
    if what == "mean":
        return scan_ref.prefix_mean(per, len(sl))
    srt = np.sort(per, axis=0)
    if what == "quorum":
        return srt[len(sl) - arg]
    assert what == "spread" and len(sl) - 2 * arg >= 2
    return srt[len(sl) - 1 - arg] - srt[arg]


# The gap a list of spreads needs, absolute, as tests/spread_ref.py derives it: a slot score is
# within scan_ref.RTOL relative of the reference and below 1, so a spread moves by at most 2 RTOL and
# two neighbours by at most 4 RTOL = 4e-9 against each other.  spread_ref rounds that up to 1e-8 for
# its lists of 65; among 4097 entries some 4e-5 apart on average almost no seed leaves 1e-8
# everywhere, so the bound here stays just above what the derivation needs.
SPREAD_GAP = 5e-9


def top_reference(model, n, what="mean", arg=None, known=None, sample=None, ns=None):
    """The best n (values, keys) of the model under the scan's total order, from the elite list
    alone.  Preconditions, on the reference: there are n + 1 eligible elites, the order inside the
    best n + 1 is determined (scan_ref.assert_gaps; a spread: both that and SPREAD_GAP absolute) and the
    (n + 1)-th value is above COMMON_HI, which bounds the mean, every q_m and every spread of a
    triple with a common gene: nothing but elites can enter the list."""
    s, k = scan_ref.top(stat(model, what, arg, sample, ns), model.keys, n, known)
    assert s.size == n + 1, s.size
    scan_ref.assert_gaps(s)
    if what == "spread":
        assert float((s[:-1] - s[1:]).min()) > SPREAD_GAP, float((s[:-1] - s[1:]).min())
    assert s[n] > COMMON_HI * (1 + 1e-6), s[n]
    return s[:n], k[:n]


# ------------------------------------------------------------------ the cases the GPU tests run
# Seeds chosen on the reference alone (tests/test_planted_host.py asserts what they were chosen for):
# with E = 96 the top 4097 of C(96, 3) = 142,880 elite values lie about 4e-5 apart on average, and
# most seeds leave one adjacent pair closer than the gap the order needs.
SCALE_SLOTS, SCALE_ACTIVE, SCALE_E = 8, 5, 96
SCALE_SEEDS = {("mean", 3001): 8, ("quorum", 3001): 8, ("spread", 3001): 79, ("mean", 6007): 7}
SCALE_SAMPLE = 2    # the single slot the lists are also run on
SMALL_P = 90        # every case once against brute force


def scale_model(what="mean", P=3001):
    if P == SMALL_P:
        return build(P, B=SCALE_SLOTS, E=16, seed=3, small=6)
    return build(P, B=SCALE_SLOTS, E=SCALE_E, seed=SCALE_SEEDS[(what, P)])


def scale_case(model, which, what="mean", arg=None):
    """One list case -> (known keys or None, the call's sample or None, the reference's mode):
    "all"; "known": the scale's known keys, the 50 best under the statistic among them; "sample":
    the single slot SCALE_SAMPLE."""
    if which == "sample":
        return None, SCALE_SAMPLE, dict(sample=SCALE_SAMPLE)
    known = scale_known(model, [stat(model, what, arg, ns=SCALE_ACTIVE)]) if which == "known" else None
    return known, None, dict(ns=SCALE_ACTIVE)


def scale_known(model, stats=()):
    """The known keys of the scale cases: 300,000 at P = 3001 (fewer where the triangle is small)."""
    if model.P == SMALL_P:
        return known_keys(model, 2000, 20000, 5, stats=stats)
    return known_keys(model, stats=stats)


# ------------------------------------------------------------------ closed form, held to brute force
# What the GPU tests ask for.  At P <= SMALL_P every answer is also formed from the scores of all
# C(P, 3) triples by the suite's older references and must equal the closed form, so a failure at
# scale can be told apart from a wrong closed form.
_BRUTE = {}


def brute(model):
    """(per f64[B][C(P, 3)], keys) of scan_ref.ref_scores on the full theta; computed once."""
    assert model.P <= SMALL_P
    if id(model) not in _BRUTE:
        per = [scan_ref.ref_scores(model.theta[s], model.pr[s]) for s in range(model.B)]
        _BRUTE[id(model)] = (model, np.stack([p[0] for p in per]), per[0][1])
    return _BRUTE[id(model)][1:]


def brute_stat(model, what="mean", arg=None, sample=None, ns=None):
    per, keys = brute(model)
    return stat(model._replace(per=per), what, arg, sample, ns), keys


def ref_census(model, thresholds, known=None, sample=None, ns=None):
    counts, total = census(model, thresholds, known, sample, ns)
    if model.P <= SMALL_P:
        scores, keys = brute_stat(model, "mean", None, sample, ns)
        want, want_total = census_ref.ref_census(scores, keys, thresholds, known)
        assert (counts == want).all() and total == want_total
    return counts, total


def ref_votes(model, threshold, ns=None, known=None):
    import votes_ref
    hist = votes(model, threshold, ns, known)
    if model.P <= SMALL_P:
        per, keys = brute(model)
        assert (hist == votes_ref.ref_votes(per, keys, threshold, model.B if ns is None else ns, known)[3]).all()
    return hist


def ref_pair_census(model, thresholds, known=None, sample=None, ns=None):
    import pair_census_ref
    mat = pair_census(model, thresholds, known, sample, ns)
    if model.P <= SMALL_P:
        scores, keys = brute_stat(model, "mean", None, sample, ns)
        assert (mat == pair_census_ref.ref_pairs_rank(scores, keys, model.P, thresholds, known)).all()
    return mat


def ref_pair_votes(model, threshold, levels, ns=None, known=None):
    import pair_votes_ref
    mat = pair_votes(model, threshold, levels, ns, known)
    if model.P <= SMALL_P:
        per, keys = brute(model)
        assert (mat == pair_votes_ref.ref_rank(per, keys, model.P, threshold, levels, ns, known)).all()
    return mat


def ref_top(model, n, what="mean", arg=None, known=None, sample=None, ns=None):
    s, k = top_reference(model, n, what, arg, known, sample, ns)
    if model.P <= SMALL_P:
        values, keys = brute_stat(model, what, arg, sample, ns)
        ws, wk = scan_ref.top(values, keys, n, known)
        assert (k == wk[:n]).all() and np.abs(s - ws[:n]).max() <= 2e-9
    return s, k


# ------------------------------------------------------------------ the partner scan
def partner_elite_list(model, q, n, what="mean", arg=None, sample=None, ns=None):
    """The best n (values, triple keys) of the ELITE query at position q, from the elite list: its
    partner pairs inside the elites are C(E - 1, 2) triples above ELITE_LO, every other pair gives a
    mixed triple.  The preconditions are top_reference's."""
    a, b, c = positions(model.keys, model.P)
    has = (a == q) | (b == q) | (c == q)
    assert model.label[q] == model.Kc and has.sum() == comb(model.E - 1, 2)
    s, k = scan_ref.top(stat(model, what, arg, sample, ns)[has], model.keys[has], n)
    assert s.size == n + 1, s.size
    scan_ref.assert_gaps(s)
    if what == "spread":
        assert float((s[:-1] - s[1:]).min()) > SPREAD_GAP
    assert s[n] > COMMON_HI * (1 + 1e-6)
    return s[:n], k[:n]


def partner_common_list(model, q, n, sample=None, ns=None):
    """The best n (value, triple keys ascending) of the COMMON query at position q where the whole
    list ties: the candidates of its best class, in the partner scan's order for equal scores (the
    packed triple key ascending), by lazy enumeration.  Asserted: the class holds more than n
    candidates and the next value of the query lies clearly below."""
    P, Kc, label = model.P, model.Kc, model.label
    g = int(label[q])
    assert g < Kc
    cval = class_values(model, sample, ns)
    L = [np.flatnonzero(label == y) for y in range(Kc)]
    options = []
    for y in range(Kc):
        for z in range(Kc):
            lo_y, hi_y, hi_z = L[y][L[y] < q], L[y][L[y] > q], L[z][L[z] > q]
            for region, cls, some in ((0, (g, y, z), hi_y.size and hi_z.size and hi_z[-1] > hi_y[0]),
                                      (1, (y, g, z), lo_y.size and hi_z.size),
                                      (2, (y, z, g), lo_y.size and ((L[z] < q) & (L[z] > lo_y[0])).any())):
                if some:
                    options.append((float(cval[cls]), region, y, z))
    options.sort(reverse=True)
    (value, region, y, z), runner_up = options[0], options[1][0]
    assert runner_up < value * (1 - 1e-6)
    keys = []
    if region == 0:
        for b in L[y][L[y] > q]:
            keys += ((q * P + b) * P + L[z][L[z] > b]).tolist()
            if len(keys) > n:
                break
    else:
        for a in L[y][L[y] < q]:
            if region == 1:
                keys += ((a * P + q) * P + L[z][L[z] > q]).tolist()
            else:
                keys += ((a * P + L[z][(L[z] > a) & (L[z] < q)]) * P + q).tolist()
            if len(keys) > n:
                break
    assert len(keys) > n, len(keys)
    return value, np.array(keys[:n], dtype=np.int64)


def partner_plan(P, Q, ncu, fan=32):
    """(workgroups per query, merge levels) as csrc/partners.hip plans them: the device's worth of
    8 workgroups per compute unit over the Q queries, no more than a query has items at the
    narrowest row block, at most fan^2; a merge level per factor of `fan`."""
    P16 = max(16, (P + 15) // 16 * 16)
    items_max = ((P + 15) // 16) * (P16 // 16)
    gpq = max(1, min((8 * max(ncu, 1) + max(Q, 1) - 1) // max(Q, 1), items_max, fan * fan))
    return gpq, 0 if gpq == 1 else 1 if gpq <= fan else 2


# ------------------------------------------------------------------ confined masks at full width
CONFINED_UNIVERSE = 200
CONFINED_CASES = [(10, 203, 2), (10, 4099, 2), (10, 16384, 2), (32, 16384, 8)]   # (K, P, B); 203: the small tests' size


def blocked_keys(keys, mask, P):
    """bool per packed key: one of its three pairs is set in `mask` (read at x < y only)."""
    a, b, c = positions(keys, P)

    def bit(x, y):
        return (mask[x, y >> 5] >> (y & 31).astype(np.uint32)) & np.uint32(1)
    return (bit(a, b) | bit(a, c) | bit(b, c)).astype(bool)


# Seeds chosen on the reference alone: the lists of 64 (scan, quorum, spread, partners) leave every
# adjacent gap above the bound their references assert.
CONFINED_SEEDS = {(10, 203, 2): 0, (10, 4099, 2): 0, (10, 16384, 2): 0, (32, 16384, 8): 1}


@functools.lru_cache(maxsize=None)
def confined_case(K, P, B, seed=None):
    """-> (theta, pr, universe positions, mask, per f64[B][n], keys int64[n]): the eligible triples
    of the confined scan and each slot's reference scores; computed once."""
    seed = CONFINED_SEEDS[(K, P, B)] if seed is None else seed
    rng = np.random.default_rng(K + P + B + 100 * seed)
    th, pr = scan_ref.random_params(K, P, 1000 + K + P + 100 * seed, B)
    edge = 1 << (int(P - 1).bit_length() - 1)          # the largest 2^k below P: a word edge high in the row
    fixed = [0, 31, 32, 63, 64, edge - 1, edge, edge // 2 - 1, edge // 2, P - 2, P - 1]
    fixed = np.unique([p for p in fixed if 0 <= p < P])
    free = np.setdiff1d(np.arange(P), fixed)
    U = np.sort(np.concatenate([fixed, rng.choice(free, min(CONFINED_UNIVERSE, P) - fixed.size, replace=False)]))
    blocked = [(0, P - 1), (edge - 1, edge), (31, 32), (int(U[20]), int(U[150])), (int(U[77]), int(U[78]))]
    mask = confined_mask(P, U, blocked)
    per, keys = elite_scores(th, pr, U, P)
    keep = ~blocked_keys(keys, mask, P)
    assert comb(U.size, 3) - 5 * (U.size - 2) <= keep.sum() < comb(U.size, 3)
    per, keys = np.ascontiguousarray(per[:, keep]), keys[keep]
    for a in (th, pr, U, mask, per, keys):
        a.setflags(write=False)
    return th, pr, U, mask, per, keys


def any_length(mean, keys, max_n):
    """A list length above the scan's cap at which the reference's cut is determined: the first n
    from max_n + 900 on whose n-th and (n + 1)-th scores lie more than 2 census_ref.GAP relative apart."""
    ws, _ = scan_ref.top(mean, keys, max_n + 1500)
    gap = (ws[:-1] - ws[1:]) / ws[1:]
    n = max_n + 900 + int(np.flatnonzero(gap[max_n + 899:] > 2 * census_ref.GAP)[0])
    assert max_n < n <= max_n + 1500
    return n


def small_keys(keys, U, P):
    """Packed keys of the big P -> the packed keys of the universe's own positions 0..|U|-1."""
    a, b, c = positions(keys, P)
    n = U.size
    return (np.searchsorted(U, a) * n + np.searchsorted(U, b)) * n + np.searchsorted(U, c)
