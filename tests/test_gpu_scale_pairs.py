"""The pair families (pair_census, pair_vote_census, pairs_top, gene_census, gene_vote_census) at
genome scale against the closed forms of tests/planted_ref.py: whole matrices at P = 3001 and, at
P = 8200, an output of 2.15e9 bytes, whose offsets pass 2^31.  The matrices are compared on the
device: the closed form is uploaded (at P = 8200 in its factored form, two [P][G] tables, and
expanded there by two gathers) and must equal the product's matrix entry for entry.  Each case also
runs at P = 90, where planted_ref's ref_* functions form the same answer from all C(P, 3) scores."""
import numpy as np
import pytest

import pair_census_ref
import pair_votes_ref
import planted_ref as pl
import scan_gpu
import scan_ref
from scan_gpu import known_of, planted_engine

pytestmark = pytest.mark.gpu

ACTIVE = pl.SCALE_ACTIVE

LEVELS = [1, 2, 3, 4, 5, 1, 3, 5]       # M = 8, unsorted and with duplicates


def to_gene_ids(eng, rank_mat):
    """A rank-position matrix filled for x < y (numpy, or already on the device) -> the symmetric
    matrix in gene ids on the device."""
    import torch
    _, rank = scan_ref.rank_tables(eng.P)
    d = rank_mat if isinstance(rank_mat, torch.Tensor) else torch.from_numpy(rank_mat).to(eng.device)
    d = d + d.transpose(0, 1)
    r = torch.from_numpy(rank).to(eng.device)
    return d[r][:, r]


def upper_sums(mat):
    """Device [P][P][M], symmetric -> the sums over g1 < g2, int64[M] on the host."""
    import torch
    return (mat.sum(dim=(0, 1), dtype=torch.int64) // 2).cpu().numpy()


@pytest.mark.parametrize("with_known", [False, True], ids=["all", "known"])
@pytest.mark.parametrize("P", [pl.SMALL_P, 3001])
def test_pair_census_whole_matrix(P, with_known):
    import torch
    m = pl.scale_model("mean", P)
    known = known_of(m, with_known)
    eng = planted_engine(m)
    t = pl.thresholds(m, ns=ACTIVE)                 # M = 8: below everything, between and in both bands
    assert t.size == 8
    want = pl.ref_pair_census(m, t, known, ns=ACTIVE)
    counts, _ = pl.census(m, t, known, ns=ACTIVE)
    np.testing.assert_array_equal(pair_votes_ref.upper_sums(want), 3 * counts)
    got = eng.pair_census_async(t, known)
    assert got.dtype == torch.int32 and tuple(got.shape) == (P, P, 8)
    assert torch.equal(got, to_gene_ids(eng, want))
    np.testing.assert_array_equal(upper_sums(got), 3 * eng.census(t, known)[0])
    np.testing.assert_array_equal(eng.gene_census(t, known), pl.gene_counts(want))
    # the best pairs at an elite-band threshold and in the common band; column 0 is every pair's
    # eligible triples (the threshold below everything)
    for col in (5, 3):
        cnt, eligible, ids = eng.pairs_top(100, t[col], known)
        want_cnt, want_ids = pair_census_ref.top_pairs(want[:, :, col], 100)
        np.testing.assert_array_equal(cnt, want_cnt)
        np.testing.assert_array_equal(ids, want_ids)
        _, rank = scan_ref.rank_tables(P)
        pos = np.sort(rank[ids.astype(np.int64)], axis=1)
        np.testing.assert_array_equal(eligible, want[pos[:, 0], pos[:, 1], 0])
    eng.close()


@pytest.mark.parametrize("with_known", [False, True], ids=["all", "known"])
@pytest.mark.parametrize("P", [pl.SMALL_P, 3001])
def test_pair_vote_census_whole_matrix(P, with_known):
    import torch
    m = pl.scale_model("mean", P)
    known = known_of(m, with_known)
    eng = planted_engine(m)
    elite = float(pl.thresholds(m, ns=ACTIVE, n_common=0, n_elite=1, extra=())[0])
    for s in range(ACTIVE):
        pl.assert_thresholds(m, [elite], m.cv[s], m.per[s])
    for thr in (pl.vote_thresholds(m)[0], elite):   # the common band's median gap; the elite band
        want = pl.ref_pair_votes(m, thr, LEVELS, ACTIVE, known)
        hist = pl.votes(m, thr, ACTIVE, known)
        tail = np.array([hist[v:].sum() for v in LEVELS])
        np.testing.assert_array_equal(pair_votes_ref.upper_sums(want), 3 * tail)
        got = eng.pair_vote_census_async(thr, LEVELS, known)
        assert got.dtype == torch.int32 and tuple(got.shape) == (P, P, len(LEVELS))
        assert torch.equal(got, to_gene_ids(eng, want))
        np.testing.assert_array_equal(eng.gene_vote_census(thr, LEVELS, known), pl.gene_counts(want))
    eng.close()


# ------------------------------------------------------------------ an output past 2^31 bytes
WIDE_P, WIDE_E = 8200, 96


WIDE_SLOTS = 3


def wide_model(P):
    if P == pl.SMALL_P:
        return pl.build(P, B=WIDE_SLOTS, E=16, seed=4, small=6, small_top=True)
    return pl.build(P, B=WIDE_SLOTS, E=WIDE_E, seed=4, small_top=True)


def wide_thresholds(m):
    """Ascending: one in the common band, under which only the eight classes of the two small
    groups count, and seven in the elite band."""
    v = np.sort(m.cv[0].reshape(-1))
    common = float((v[-9] + v[-8]) / 2)
    t = np.concatenate([[common], pl.thresholds(m, sample=0, n_common=0, n_elite=7, extra=())])
    pl.assert_thresholds(m, t, m.cv[0], m.per[0])
    hit = m.cv[0] >= common
    assert hit.sum() == 8 and hit[:2, :2, :2].all()
    return t, hit


def wide_closed_form(eng, m, columns):
    """The closed-form matrix on the device, int32 [P][P][M] in rank positions, x < y filled.
    columns: per column (the common classes that count, bool[Kc][Kc][Kc] or None; the elite
    triples that count, bool[C(E, 3)]).  pair_tables' two [P][G] tables are expanded by two gathers
    (count[i][j] = row[i][label[j]] + col[j][label[i]]) and the elite triples scattered on top."""
    import torch
    P, dev = m.P, eng.device
    label = torch.from_numpy(m.label).to(dev)
    out = torch.zeros((P, P, len(columns)), dtype=torch.int32, device=dev)
    for i, (hit, elite) in enumerate(columns):
        if hit is not None and hit.any():
            row, col = pl.pair_tables(m, hit, False)
            row = torch.from_numpy(row).to(dev).to(torch.int32)
            col = torch.from_numpy(col).to(dev).to(torch.int32)
            out[:, :, i] = torch.triu(row[:, label] + col[:, label].T, diagonal=1)
        a, b, c = (torch.from_numpy(p).to(dev) for p in pl.positions(m.keys[elite], P))
        one = torch.ones(int(elite.sum()), dtype=torch.int32, device=dev)
        for x_, y_ in ((a, b), (a, c), (b, c)):
            out[:, :, i].index_put_((x_, y_), one, accumulate=True)
    return out


@pytest.mark.parametrize("P", [pl.SMALL_P, WIDE_P])
def test_pair_census_output_past_two_gib(P):
    """P = 8200 is no multiple of 16 and [P][P][8] int32 is 2,151,680,000 bytes.  The matrix is
    written into a buffer with sentinel words behind it: every entry equals the closed form and
    nothing behind the last row is touched."""
    import torch
    m = wide_model(P)
    eng = scan_gpu.engine(m.theta[:1], m.pr[:1])
    t, hit = wide_thresholds(m)
    counts, _ = pl.ref_census(m, t, None, sample=0)
    assert counts[0] < 10 ** 9 and (np.diff(t) > 0).all()
    if P == WIDE_P:
        assert P % 16 and P * P * t.size * 4 > 2 ** 31 and counts[0] > 10 ** 7
    want = wide_closed_form(eng, m, [(hit if i == 0 else None, m.per[0] >= x) for i, x in enumerate(t)])
    if P == pl.SMALL_P:
        assert (want.cpu().numpy() == pl.ref_pair_census(m, t, None, sample=0)).all()
    assert (want.sum(dim=(0, 1), dtype=torch.int64).cpu().numpy() == 3 * counts).all()
    # the C call on a buffer of the matrix and 4096 sentinel words
    raw = scan_gpu.Raw(eng, "pair_census", int(t.size))
    words = P * P * t.size
    buf = raw.full((words + 4096,), torch.int32)
    thr_d = raw.upload(t)
    rc = raw.call((thr_d.data_ptr(), int(t.size)), [buf], 0)
    assert rc == 0
    assert bool((buf[words:] == scan_gpu.SENTINEL).all())
    got = buf[:words].view(P, P, t.size)
    assert torch.equal(got, want)
    del buf, got
    # the binding's matrix in gene ids
    got = eng.pair_census_async(t)
    assert torch.equal(got, to_gene_ids(eng, want))
    np.testing.assert_array_equal(upper_sums(got), 3 * counts)
    eng.close()


WIDE_LEVELS = [1, 2, 3, 1, 2, 3, 1, 3]      # M = 8: the kernel takes them sorted, the binding puts them back


@pytest.mark.parametrize("P", [pl.SMALL_P, WIDE_P])
def test_pair_vote_census_output_past_two_gib(P):
    """The pair vote census holds its own copy of the matrix arithmetic.  Three slots; the threshold
    lies under the fourth largest class value, and which four of the small groups' eight classes hold
    the four largest differs from slot to slot, so the levels give different columns.  Every elite
    triple has all three votes."""
    import torch
    m = wide_model(P)
    eng = scan_gpu.engine(m.theta, m.pr)
    v = np.sort(m.cv[0].reshape(-1))
    thr = float((v[-5] + v[-4]) / 2)
    for s in range(m.B):
        pl.assert_thresholds(m, [thr], m.cv[s], m.per[s])
    cvotes = (m.cv >= thr).sum(axis=0)
    evotes = (m.per >= thr).sum(axis=0)
    assert (cvotes[:2, :2, :2] > 0).sum() == (cvotes > 0).sum() and np.unique(cvotes).size >= 3
    assert (evotes == m.B).all()
    hist = pl.ref_votes(m, thr, m.B)
    assert hist[1:].sum() < 10 ** 9
    if P == WIDE_P:
        assert P * P * len(WIDE_LEVELS) * 4 > 2 ** 31
    want = wide_closed_form(eng, m, [(cvotes >= lv, evotes >= lv) for lv in WIDE_LEVELS])
    if P == pl.SMALL_P:
        assert (want.cpu().numpy() == pl.ref_pair_votes(m, thr, WIDE_LEVELS, m.B)).all()
    tail = np.array([hist[lv:].sum() for lv in WIDE_LEVELS])
    assert (want.sum(dim=(0, 1), dtype=torch.int64).cpu().numpy() == 3 * tail).all()
    assert want[:, :, 0].sum().item() > want[:, :, 2].sum().item()        # the levels differ
    got = eng.pair_vote_census_async(thr, WIDE_LEVELS)
    assert got.dtype == torch.int32 and tuple(got.shape) == (P, P, len(WIDE_LEVELS))
    assert torch.equal(got, to_gene_ids(eng, want))
    np.testing.assert_array_equal(upper_sums(got), 3 * tail)
    eng.close()
