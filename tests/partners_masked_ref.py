"""numpy reference of the pair mask in the partner scan (include/mmsbm.h mmsbm_partners_topn_masked),
for tests/test_gpu_partners_masked.py and tests/test_masked_topn_host.py: per query, the pair keys
b P + c a mask blocks, and those keys merged into the CSR key table mmsbm_partners_topn takes, which
is what a masked call stands for.  numpy only: no GPU, no product code beyond the rank order."""
import numpy as np

import masked_ref
from scan_ref import rank_tables


def pair_bit(mask, x, y):
    """The bit of the unordered pair {x, y} of rank positions (arrays, x != y), read at (min, max)."""
    lo, hi = np.minimum(x, y), np.maximum(x, y)
    return masked_ref.bit(mask, lo, hi).astype(bool)


def blocked_pairs(mask, P, q):
    """The sorted pair keys b P + c (b < c, both != q) of the query at rank position q with any of
    {q, b}, {q, c}, (b, c) blocked."""
    b, c = np.triu_indices(P, k=1)
    keep = (b != q) & (c != q)
    b, c = b[keep].astype(np.int64), c[keep].astype(np.int64)
    qq = np.full(b.size, q, dtype=np.int64)
    out = pair_bit(mask, qq, b) | pair_bit(mask, qq, c) | masked_ref.bit(mask, b, c).astype(bool)
    return b[out] * P + c[out]


def query_positions(P, queries):
    _, rank = rank_tables(P)
    return [int(rank[int(g)]) for g in queries]


def merged_known(mask, P, queries, known=None):
    """(known_off, known_pairs) for the gene ids `queries`: each query's slice of `known` (the same
    CSR pair, or None) united with the keys the mask blocks for it: sorted and unique, as
    scan.partner_known gives them."""
    off = np.zeros(len(queries) + 1, dtype=np.int64)
    parts = []
    for i, q in enumerate(query_positions(P, queries)):
        keys = blocked_pairs(mask, P, q)
        if known is not None:
            keys = np.union1d(keys, known[1][known[0][i]:known[0][i + 1]])
        parts.append(keys.astype(np.int64))
        off[i + 1] = off[i] + keys.size
    return off, (np.concatenate(parts) if parts else np.zeros(0, np.int64)).astype(np.int64)


def query_all_mask(P, q):
    """Every pair that contains rank position q blocked, nothing else."""
    return masked_ref.naive_mask(P, [(q, x) for x in range(P) if x != q])


def only_with_query_mask(P, q, every=3):
    """Every `every`-th pair that contains rank position q (from the first other position on)."""
    others = [x for x in range(P) if x != q]
    return masked_ref.naive_mask(P, [(q, x) for x in others[::every]])


def only_without_query_mask(P, q, fraction=0.15, seed=3):
    """A random choice of pairs none of which contains rank position q."""
    rng = np.random.default_rng(seed)
    sel = np.triu(rng.random((P, P)) < fraction, 1)
    sel[q, :] = False
    sel[:, q] = False
    return masked_ref.position_mask(P, sel)
