"""Every pair-masked entry at full mask width: P = 4099 and P = 16384 (MW = 512 words a row), with a
mask that confines the scan to a universe of 200 genes, "an array of a few hundred strains inside a
genome".  Theta and p are dense random (scan_ref.random_params): real scores.  The reference is the
brute-force scan of the universe's gathered rows (scan_ref.ref_scores through
planted_ref.elite_scores, the keys mapped back to the big P) without the triples of the five pairs
blocked inside the universe; the older references (census_ref, votes_ref, quorum_ref, spread_ref,
pair_census_ref, pair_votes_ref) then run on those scores.  The universe holds positions 0, 31, 32,
63, 64, P - 1 and both sides of the word edges at 2^k high in the row, so the `w0 + 1 < MW` skip,
the bit offsets of the c-tiles and the partner scan's column read are used at the last words."""
from math import comb

import numpy as np
import pytest

import census_ref
import pair_census_ref
import pair_votes_ref
import planted_ref as pl
import quorum_ref
import scan_ref
import spread_ref
import votes_ref
from scan_gpu import engine
from scan_ref import packed

pytestmark = pytest.mark.gpu

CASES = pl.CONFINED_CASES
confined = pl.confined_case


def sub_matrix(got, U, P):
    """A device pair matrix in gene ids -> (its [U][U][M] part in rank positions, upper triangle, on
    the host; the sums over all pairs, int64[M])."""
    import torch
    order, _ = scan_ref.rank_tables(P)
    ids = torch.from_numpy(order[U].astype(np.int64)).to(got.device)
    sub = got[ids][:, ids].cpu().numpy()
    sub = np.triu(np.moveaxis(sub, 2, 0), k=1)
    return np.moveaxis(sub, 0, 2), (got.sum(dim=(0, 1), dtype=torch.int64) // 2).cpu().numpy()


@pytest.mark.parametrize("K,P,B", CASES)
def test_counts_and_lists(K, P, B):
    th, pr, U, mask, per, keys = confined(K, P, B)
    mean = scan_ref.prefix_mean(per, B)
    eng = engine(th, pr)
    # census and threshold scan
    t = census_ref.gap_thresholds(mean, 5)
    census_ref.assert_clear(mean, t)
    want, total = census_ref.ref_census(mean, keys, t)
    counts, eligible = eng.census(t, mask=mask)
    np.testing.assert_array_equal(counts, want)
    assert eligible == total == keys.size
    mid = float(np.sort(t)[t.size // 2])
    s, ids = eng.scan_above(mid, mask=mask)
    got = packed(ids, P)
    np.testing.assert_array_equal(np.sort(got), keys[mean >= mid])
    np.testing.assert_allclose(s, mean[np.searchsorted(keys, got)], rtol=scan_ref.RTOL, atol=0)
    # the lists
    n = 64
    ws, wk = scan_ref.top(mean, keys, n)
    scan_ref.assert_gaps(ws)
    s, ids = eng.scan_top(n, mask=mask)
    np.testing.assert_array_equal(ids, scan_ref.keys_to_ids(wk[:n], P))
    np.testing.assert_allclose(s, ws[:n], rtol=scan_ref.RTOL, atol=0)
    n_any = pl.any_length(mean, keys, int(eng.lib.mmsbm_scan_max_n()))
    ws, wk = scan_ref.top(mean, keys, n_any)
    s, ids = eng.scan_top_any(n_any, mask=mask)
    got = packed(ids, P)
    assert s.size == n_any and (np.diff(s) <= 0).all()
    np.testing.assert_array_equal(np.sort(got), np.sort(wk[:n_any]))
    np.testing.assert_allclose(s, mean[np.searchsorted(keys, got)], rtol=scan_ref.RTOL, atol=0)
    for m in sorted({1, (B + 1) // 2, B}):
        ws, wk = quorum_ref.ref_top(per, keys, m, n)
        s, ids = eng.quorum_top(n, m, mask=mask)
        np.testing.assert_array_equal(ids, scan_ref.keys_to_ids(wk[:n], P))
        np.testing.assert_allclose(s, ws[:n], rtol=scan_ref.RTOL, atol=0)
    ws, wk = spread_ref.ref_top(per, keys, 0, n)
    s, ids = eng.spread_top(n, 0, mask=mask)
    np.testing.assert_array_equal(ids, scan_ref.keys_to_ids(wk[:n], P))
    np.testing.assert_allclose(s, ws[:n], rtol=0, atol=2 * scan_ref.RTOL)
    # the votes
    thr = votes_ref.at_quantile(per, votes_ref.clear_thresholds(per, 33), 0.9)
    votes, vkeys, vmean, hist = votes_ref.ref_votes(per, keys, thr)
    np.testing.assert_array_equal(eng.vote_census(thr, mask=mask), hist)
    v, s, ids = eng.consensus(thr, 2, mask=mask)         # two votes: the most that some triple gets in every case
    want_hits = votes_ref.ref_hits(votes, vkeys, vmean, 2)
    got = packed(ids, P)
    assert sorted(got.tolist()) == sorted(want_hits) and len(want_hits) > 0
    assert v.tolist() == [want_hits[k][0] for k in got.tolist()]
    np.testing.assert_allclose(s, [want_hits[k][1] for k in got.tolist()], rtol=scan_ref.RTOL, atol=0)
    eng.close()


@pytest.mark.parametrize("K,P,B", CASES)
def test_pair_matrices_and_partners(K, P, B):
    th, pr, U, mask, per, keys = confined(K, P, B)
    mean = scan_ref.prefix_mean(per, B)
    eng = engine(th, pr)
    order, _ = scan_ref.rank_tables(P)
    wide = P > 5000                                     # M = 1 there: the matrix is a gigabyte a column
    t = np.sort(census_ref.gap_thresholds(mean, 5))
    census_ref.assert_clear(mean, t)
    t = t[t.size // 2:t.size // 2 + 1] if wide else t[1:4]
    sk = pl.small_keys(keys, U, P)
    want = pair_census_ref.ref_pairs_rank(mean, sk, U.size, t)
    sub, sums = sub_matrix(eng.pair_census_async(t, mask=mask), U, P)
    np.testing.assert_array_equal(sub, want)
    np.testing.assert_array_equal(sums, pair_votes_ref.upper_sums(want))    # nothing outside the universe
    np.testing.assert_array_equal(sums, 3 * census_ref.ref_census(mean, keys, t)[0])
    thr = votes_ref.at_quantile(per, votes_ref.clear_thresholds(per, 33), 0.9)
    levels = [2] if wide else sorted({1, 2, B})
    want = pair_votes_ref.ref_rank(per, sk, U.size, thr, levels)
    sub, sums = sub_matrix(eng.pair_vote_census_async(thr, levels, mask=mask), U, P)
    np.testing.assert_array_equal(sub, want)
    np.testing.assert_array_equal(sums, pair_votes_ref.upper_sums(want))
    # the partner scan: the universe's genes at the lowest, a middle and the highest position read
    # mask row q and column q over the whole width
    n = 64
    pos = [int(U[0]), int(U[U.size // 2]), int(U[-1])]
    assert pos[0] == 0 and pos[-1] == P - 1
    a, b, c = pl.positions(keys, P)
    rows = eng.partners_top([int(order[q]) for q in pos], n, mask=mask)
    for q, (s, ids) in zip(pos, rows):
        has = (a == q) | (b == q) | (c == q)
        ws, wk = scan_ref.top(mean[has], keys[has], n)
        scan_ref.assert_gaps(ws)
        np.testing.assert_array_equal(ids, scan_ref.keys_to_ids(wk[:n], P))
        np.testing.assert_allclose(s, ws[:n], rtol=scan_ref.RTOL, atol=0)
    eng.close()


def test_masked_total_and_its_complement():
    """P = 4099.  The masked call's eligible triples are the reference's list, and the unmasked call
    with exactly those keys known counts everything else: the two totals add up to C(P, 3).  (The
    small tests' identity, masked == unmasked with every blocked triple known, needs a key table of
    1.1e10 keys here.)"""
    K, P, B = CASES[1]
    th, pr, U, mask, per, keys = confined(K, P, B)
    eng = engine(th, pr)
    _, masked_total = eng.census([], mask=mask)
    _, rest = eng.census([], keys)
    assert masked_total == keys.size and masked_total + rest == comb(P, 3)
    eng.close()
