"""numpy reference of the pair mask (include/mmsbm.h mmsbm_scan_census_masked, scan.pair_mask), for
tests/test_masked_host.py and tests/test_gpu_scan_masked.py: which reference keys a mask blocks, the
key table a mask stands for, a per-bit packer to hold scan.pair_mask against and the masks the GPU
tests share.  numpy only: no GPU, no product code beyond the rank order."""
import numpy as np

import scan_ref


def shape(P):
    """(P16, MW): P rounded up to 16 (at least 16), and the 32-bit words of a row of P16 bits."""
    P16 = max(16, (P + 15) // 16 * 16)
    return P16, (P16 + 31) // 32


def bit(mask, x, y):
    """The bit of the pair of rank positions (x, y), arrays allowed."""
    return (mask[x, y >> 5] >> (y & 31).astype(np.uint32)) & np.uint32(1)


def blocked(keys, mask, P):
    """bool per packed key: one of (a, b), (a, c), (b, c) is set in `mask` (read at x < y only)."""
    k = np.asarray(keys, dtype=np.int64)
    a, b, c = k // (P * P), (k // P) % P, k % P
    return (bit(mask, a, b) | bit(mask, a, c) | bit(mask, b, c)).astype(bool)


def all_keys(P):
    """The packed keys of all C(P, 3) triples a < b < c, ascending."""
    a, b, c = np.meshgrid(np.arange(P), np.arange(P), np.arange(P), indexing="ij")
    keep = (a < b) & (b < c)
    return ((a[keep].astype(np.int64) * P + b[keep]) * P + c[keep])


def expand(mask, P):
    """The key table a mask stands for: the sorted packed keys of every triple that contains a
    blocked pair."""
    keys = all_keys(P)
    return keys[blocked(keys, mask, P)]


def naive_mask(P, position_pairs):
    """The mask with exactly these pairs of RANK positions set, on both sides, one bit at a time."""
    P16, MW = shape(P)
    mask = np.zeros((P16, MW), dtype=np.uint32)
    for x, y in position_pairs:
        x, y = int(x), int(y)
        assert 0 <= x < P and 0 <= y < P and x != y
        mask[x, y >> 5] |= np.uint32(1 << (y & 31))
        mask[y, x >> 5] |= np.uint32(1 << (x & 31))
    return mask


def naive_from_ids(P, pairs=(), genes=None, matrix=None):
    """scan.pair_mask's contract in loops over gene ids: the pairs, every pair touching a gene
    outside `genes`, every pair with a matrix entry on either side."""
    _, rank = scan_ref.rank_tables(P)
    out = set()
    for i, j in pairs:
        out.add((int(rank[i]), int(rank[j])))
    if genes is not None:
        allowed = set(int(g) for g in genes)
        for i in range(P):
            for j in range(P):
                if i != j and (i not in allowed or j not in allowed):
                    out.add((int(rank[i]), int(rank[j])))
    if matrix is not None:
        for i in range(P):
            for j in range(P):
                if i != j and (matrix[i][j] or matrix[j][i]):
                    out.add((int(rank[i]), int(rank[j])))
    return naive_mask(P, out)


# ------------------------------------------------------------------ the masks the GPU tests share
def position_mask(P, sel):
    """The mask of a bool [P][P] in rank positions (either side blocks), through the naive packer's
    layout but vectorised: tests' masks are made here, never by the code under test."""
    P16, MW = shape(P)
    sel = np.asarray(sel, dtype=bool)
    sel = sel | sel.T
    np.fill_diagonal(sel, False)
    full = np.zeros((P16, MW * 32), dtype=bool)
    full[:P, :P] = sel
    weights = (np.uint64(1) << np.arange(32, dtype=np.uint64))
    return (full.reshape(P16, MW, 32).astype(np.uint64) * weights).sum(axis=2).astype(np.uint32)


def random_mask(P, fraction=0.1, seed=11):
    rng = np.random.default_rng(seed)
    return position_mask(P, np.triu(rng.random((P, P)) < fraction, 1))


def allowed_mask(P, every=3, seed=11):
    """A third of the rank positions allowed (a seeded choice): every other pair blocked."""
    rng = np.random.default_rng(seed)
    allowed = np.zeros(P, dtype=bool)
    allowed[rng.permutation(P)[:(P + every - 1) // every]] = True
    return position_mask(P, ~(allowed[:, None] & allowed[None, :]))


def block_mask(P, rows=(0, 16), cols=(32, 48)):
    """Every pair (x in rows) x (y in cols) blocked: whole 16 x 16 tiles of (a, c) and (b, c) bits."""
    sel = np.zeros((P, P), dtype=bool)
    sel[rows[0]:min(rows[1], P), cols[0]:min(cols[1], P)] = True
    return position_mask(P, sel)


def single_pair_mask(P):
    return naive_mask(P, [(P // 3, 2 * P // 3)])


def last_tile_mask(P):
    """Only pairs whose second position lies in the last, partial tile of columns."""
    c0 = (P - 1) // 16 * 16
    sel = np.zeros((P, P), dtype=bool)
    sel[::3, c0:] = True
    sel[c0:, c0:] = True
    return position_mask(P, sel)


def tiles_mask(P):
    """Every pair of one whole b-tile (positions 16..31 against everything) and of one whole c-tile
    (every position of the tiles below it against the last full tile of columns; none when that is
    tile 0)."""
    sel = np.zeros((P, P), dtype=bool)
    if P > 16:
        sel[16:min(32, P), :] = True
    c0 = (P // 16 - 1) * 16
    if c0 > 0:
        sel[:c0, c0:c0 + 16] = True
    return position_mask(P, sel)


def full_mask(P):
    return position_mask(P, np.ones((P, P), dtype=bool))
