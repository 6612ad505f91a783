"""The screen scan at rows longer than the select kernel's candidate buffer (csrc/screen.hip
screen_select_kernel: cap = max(512, the power of two >= 2 N) entries, so P - 2 > cap): the
reservation that does not fit, the keep-best inside the row loop, the threshold it raises and the
pruning compare against it; the pair mask beyond three words a row, long known slices, N up to the
documented 1024 and the score kernel's stride over c-tiles.  tests/test_gpu_screen.py keeps P <= 80,
where none of that runs.

Against tests/screen_ref.py in float64, as there: every test first asserts, on the reference alone,
that the order it demands is determined (check_list: every adjacent relative gap inside the
reference's top N + 1 exceeds 1e-9), and skips no query.  Random parameters do not determine an order
at N in the hundreds, so the exact lists at N > 100 are demanded of designed rows
(screen_ref.designed_params: scores affine in a grid value within each region, adjacent gaps about
1 / P); random parameters are held to exact lists at N <= 100 and to the set at a clear cut
(converged_ref.check_set_cut) above.  tests/test_screen_host.py runs the reference-only halves.

The pruning compare can only lose an entry that would end as the N-th of the list (anything better is
above every threshold a correct or off-by-one keep-best raises), and only when nothing read later
displaces it: the rows of order "late:N" are built so, and are the ones a threshold one entry too
high fails.  Keys rise with the position read, so a candidate that ties the threshold's score always
has the larger key: how the compare treats the key on a tie cannot change a list of this kernel.
"""
import numpy as np
import pytest

import converged_ref
import scan_ref
import screen_ref as ref
from scan_gpu import engine
from scan_ref import bits
from test_gpu_screen import csr, edge_positions, named_thirds, rank_rows, same_rows, to_ids

pytestmark = pytest.mark.gpu

RTOL = scan_ref.RTOL
WORST = {"rows": 0.0}       # the largest relative error of a row entry against the reference in this run


@pytest.fixture(scope="module", autouse=True)
def worst_error():
    yield
    print("max relative error of a screen row vs the reference  %.3e" % WORST["rows"])


def check_row(got, want, ok):
    if ok.any():
        WORST["rows"] = max(WORST["rows"], float(np.max(np.abs(got[ok] - want[ok]) / np.abs(want[ok]))))
    ref.check_row(got, want, ok)


def lists_of(eng, pairs, N, **kw):
    """screen_top through the device outputs: the count and the NaN / -1 tail checked on the way."""
    import torch
    sd, idd, cd = eng.screen_top_async(pairs, N, **kw)
    torch.cuda.synchronize()
    sd, idd, cd = sd.cpu().numpy(), idd.cpu().numpy(), cd.cpu().numpy()
    assert cd.dtype == np.int64 and sd.shape == (len(pairs), N) and idd.shape == (len(pairs), N, 3)
    out = []
    for i in range(len(pairs)):
        n = int(cd[i])
        assert 0 <= n <= N
        assert np.isnan(sd[i, n:]).all() and not np.isnan(sd[i, :n]).any() and (idd[i, n:] == -1).all()
        out.append((sd[i, :n].copy(), idd[i, :n].copy()))
    return out


def check_query(lst, row_by_id, want, P, pair, N, ok=None):
    """One query's list: count = min(N, eligible), the reference's ordered ids, the row's own words."""
    x, y = ref.positions(P, pair)
    ok = ref.eligible(P, x, y) if ok is None else ok
    assert lst[0].size == min(N, int(ok.sum())), ((x, y), lst[0].size, N, int(ok.sum()))
    ref.check_list(lst, want, P, x, y, N, ok)
    assert bits(named_thirds(P, pair, *lst, row_by_id)) == bits(lst[0])


# ------------------------------------------------------------------ a. row counts around the buffer
def buffer_positions(P):
    """test_regions_and_small_gene_counts' edges, pairs on both sides of 255 / 256 (a round of the
    select kernel) and 511 / 512 (its buffer), and random pairs: 33 queries."""
    cand = edge_positions(P) + [(255, 256), (254, 257), (256, 257), (100, 255), (100, 256), (255, 511), (256, 512),
                                (511, 512), (510, 513), (512, P - 1), (0, 511), (0, 512), (511, P - 1)]
    out = []
    for x, y in cand:
        if 0 <= x < y < P and (x, y) not in out:
            out.append((x, y))
    rng = np.random.default_rng(P)
    while len(out) < 33:
        x, y = sorted(int(v) for v in rng.choice(P, 2, replace=False))
        if (x, y) not in out:
            out.append((x, y))
    return out


BUFFER_SEEDS = {513: 1, 514: 1, 515: 1, 600: 1}


@pytest.mark.parametrize("P", sorted(BUFFER_SEEDS))
def test_row_counts_around_the_buffer(P):
    """P - 2 candidates = cap - 1, cap, cap + 1 and well past it (cap = 512 for N <= 256)."""
    K, B = 3, 2
    th, pr = scan_ref.random_params(K, P, BUFFER_SEEDS[P], B)
    pos = buffer_positions(P)
    assert len(pos) == 33 and max(ref.cap_of(N) for N in (1, 8, 100)) == 512
    pairs = to_ids(P, pos)
    eng = engine(th, pr)
    for sample in (0, None):
        want = [ref.ref_rows(th, pr, x, y, sample) for x, y in pos]
        rows = eng.screen_scores(pairs, sample=sample)
        assert rows.shape == (33, P) and rows.dtype == np.float64
        by_rank = rank_rows(P, rows)
        for i, (x, y) in enumerate(pos):
            check_row(by_rank[i], want[i], ref.eligible(P, x, y))
        for N in (1, 8, 100):
            lists = lists_of(eng, pairs, N, sample=sample)
            for i in range(33):
                check_query(lists[i], rows[i], want[i], P, pairs[i], N)
    eng.close()


# ------------------------------------------------------------------ b. arrival orders
@pytest.mark.parametrize("order", ref.ORDERS)
def test_arrival_orders_on_designed_rows(order):
    """ascending: every round passes the threshold and overflows; descending: nothing passes after
    the first keep-best; shuffled; a sawtooth of one round.  N: the tight fit 256 (a buffer of 512
    that holds 256 takes one whole round, exactly), its neighbours and every growth step of cap."""
    P = ref.WIDE_P
    th, pr, place = ref.designed_params(P, order)
    pos = ref.three_queries(P)
    pairs = to_ids(P, pos)
    want = [ref.ref_row(th[0], pr[0], x, y) for x, y in pos]
    for (x, y), row in zip(pos, want):
        ref.check_designed(row, place, P, x, y)
    eng = engine(th, pr)
    rows = eng.screen_scores(pairs, sample=0)
    for i, (x, y) in enumerate(pos):
        check_row(rank_rows(P, rows)[i], want[i], ref.eligible(P, x, y))
    for N in ref.WIDE_NS:
        assert (P - 2 > ref.cap_of(N)) == (N <= 512)    # cap = 2048 (N > 512) holds the whole row: c. overflows that one
        lists = lists_of(eng, pairs, N, sample=0)
        for i in range(len(pos)):
            check_query(lists[i], rows[i], want[i], P, pairs[i], N)
    eng.close()


@pytest.mark.parametrize("P,N", ref.LATE, ids=["P%d-N%d" % c for c in ref.LATE])
def test_the_nth_best_arrives_after_the_last_keep_best(P, N):
    """A descending row whose N-th best third of the query (0, 1) sits at the last position: the
    keep-best before it holds the best N of the rest, the late one lies between that buffer's
    (N - 1)-th and N-th entries, and it must pass the pruning compare.  A threshold one entry too
    high (the (N - 1)-th) loses it and nothing later can hide that."""
    order = "late:%d" % N
    th, pr, place = ref.designed_params(P, order)
    pos = ref.three_queries(P)
    assert pos[0] == (0, 1) and (P - 1) // ref.ROUND > ref.cap_of(N) // ref.ROUND     # a round past the first overflow
    pairs = to_ids(P, pos)
    want = [ref.ref_row(th[0], pr[0], x, y) for x, y in pos]
    for (x, y), row in zip(pos, want):
        ref.check_designed(row, place, P, x, y)
    assert int((want[0][2:] > want[0][P - 1]).sum()) == N - 1      # on the reference: the last position is the N-th best
    eng = engine(th, pr)
    rows = eng.screen_scores(pairs, sample=0)
    lists = lists_of(eng, pairs, N, sample=0)
    eng.close()
    for i, (x, y) in enumerate(pos):
        check_row(rank_rows(P, rows)[i], want[i], ref.eligible(P, x, y))
        check_query(lists[i], rows[i], want[i], P, pairs[i], N)
    order_tab, _ = scan_ref.rank_tables(P)
    assert lists[0][1][N - 1].tolist() == [int(order_tab[0]), int(order_tab[1]), int(order_tab[P - 1])]


# ------------------------------------------------------------------ c. N = 1024 overflowing
@pytest.mark.parametrize("order", ref.OVERFLOW_ORDERS)
def test_the_largest_list_overflows_its_buffer(order):
    P, N, B = ref.OVERFLOW_P, 1024, 2
    assert P - 2 > ref.cap_of(N) == 2048
    th, pr, place = ref.designed_params(P, order, B)
    pos = ref.three_queries(P)
    pairs = to_ids(P, pos)
    eng = engine(th, pr)
    for sample in (1, None):
        want = [ref.ref_rows(th, pr, x, y, sample) for x, y in pos]
        for (x, y), row in zip(pos, want):      # the ensemble of designed slots keeps the order and (check_list) its gaps
            ref.check_designed(row, place, P, x, y)
        rows = eng.screen_scores(pairs, sample=sample)
        lists = lists_of(eng, pairs, N, sample=sample)
        for i, (x, y) in enumerate(pos):
            check_row(rank_rows(P, rows)[i], want[i], ref.eligible(P, x, y))
            check_query(lists[i], rows[i], want[i], P, pairs[i], N)
    eng.close()


# ------------------------------------------------------------------ d. ties through the threshold
def test_bit_equal_scores_through_the_threshold():
    """K = 1: every score is bit-equal, so after a keep-best a candidate is judged by its key
    against thr_k alone.  The list is the N smallest keys in key order."""
    P = 600
    th, pr = scan_ref.random_params(1, P, 3, 2)
    pos = ref.three_queries(P)
    pairs = to_ids(P, pos)
    eng = engine(th, pr)
    for sample in (0, None):
        for N in (8, 256, 598):
            assert P - 2 > ref.cap_of(N) or N == 598
            for (x, y), (s, ids) in zip(pos, lists_of(eng, pairs, N, sample=sample)):
                assert s.size == N and np.unique(s.view(np.int64)).size == 1
                c = np.array([c for c in range(P) if c not in (x, y)])
                keys = ref.row_keys(P, x, y)[c]
                assert (np.diff(keys) > 0).all()
                np.testing.assert_array_equal(ids, scan_ref.keys_to_ids(keys[:N], P))
    eng.close()


@pytest.mark.parametrize("which", [0, 1, 2])
def test_twins_on_both_sides_of_a_keep_best(which):
    """K = 4, N = 8, P = 1100: the genes at positions 300 and 900 take the theta row of the best gene
    of their region.  The first keep-best of a row of 1100 runs in the third round (positions 512 to
    767), so one twin is kept by it and the other is judged against the threshold it raised: the
    three are bit-equal, adjacent in the list and in key order."""
    K, P, N = 4, 1100, 8
    a, b = 300, 900
    x, y = [(0, 1), (P - 2, P - 1), (10, 1000)][which]       # both twins in the last, the first, the middle region
    th, pr = scan_ref.random_params(K, P, 8)
    order, _ = scan_ref.rank_tables(P)
    region = [r for r in ref.regions(P, x, y) if a in r and b in r]
    assert len(region) == 1
    row = ref.ref_row(th[0], pr[0], x, y)
    best = int(region[0][np.argmax(row[region[0]])])
    assert best not in (a, b)
    th[0, order[a]] = th[0, order[b]] = th[0, order[best]]
    want = ref.ref_row(th[0], pr[0], x, y)
    tied = sorted((a, b, best))
    top_s, top_k = scan_ref.top(want[ref.eligible(P, x, y)], ref.row_keys(P, x, y)[ref.eligible(P, x, y)], N)
    assert np.isin(ref.row_keys(P, x, y)[tied], top_k[:N]).all()         # on the reference: all three are listed
    pairs = to_ids(P, [(x, y)])
    eng = engine(th, pr)
    ((s, ids),) = lists_of(eng, pairs, N)
    rows = rank_rows(P, eng.screen_scores(pairs))[0]
    eng.close()
    assert s.size == N
    got = scan_ref.packed(ids, P)
    at = [int(np.flatnonzero(got == k)[0]) for k in ref.row_keys(P, x, y)[tied]]
    assert at[1] == at[0] + 1 and at[2] == at[0] + 2, at
    assert rows[tied[0]].tobytes() == rows[tied[1]].tobytes() == rows[tied[2]].tobytes()
    assert s[at[0]].tobytes() == s[at[1]].tobytes() == s[at[2]].tobytes() == rows[tied[0]].tobytes()
    # the list is the reference's set (a clear cut under the N-th), each score within RTOL of its own key's
    assert top_s[N - 1] - top_s[N] > 1e-7 * top_s[N - 1]
    np.testing.assert_array_equal(np.sort(got), np.sort(top_k[:N]))
    np.testing.assert_allclose(s[np.argsort(got)], top_s[:N][np.argsort(top_k[:N])], rtol=RTOL, atol=0)
    assert (np.diff(s) <= 0).all()


# ------------------------------------------------------------------ e. exclusion and mask at width
E_K, E_P, E_B, E_N, E_SEED = 3, 600, 2, 16, 2


def wide_slices(P, pos, N, seed):
    """One known slice per query, cycling through 0, 1, 300 and P - 2 - n thirds for n = N - 1, N,
    N + 1 (none of them x or y, so n third genes stay eligible): sorted rank positions."""
    rng = np.random.default_rng(seed)
    sizes = [0, 1, 300, P - 2 - (N - 1), P - 2 - N, P - 2 - (N + 1)]
    out = []
    for i, (x, y) in enumerate(pos):
        others = np.array([c for c in range(P) if c not in (x, y)])
        out.append(np.sort(rng.choice(others, sizes[i % len(sizes)], replace=False)))
    return out, [P - 2 - sizes[i % len(sizes)] for i in range(len(pos))]


def random_positions(P, n, seed):
    rng = np.random.default_rng(seed)
    return [tuple(sorted(int(v) for v in rng.choice(P, 2, replace=False))) for _ in range(n)]


def test_known_slices_at_width():
    """Eligible counts on both sides of N, on rows that overflow the buffer (slices of 0, 1) and rows
    that no longer do (slices of 300 and more); third_known searches slices of hundreds of entries."""
    K, P, B, N = E_K, E_P, E_B, E_N
    th, pr = scan_ref.random_params(K, P, E_SEED, B)
    pos = random_positions(P, 30, 12) + ref.three_queries(P)
    pairs = to_ids(P, pos)
    base, left = wide_slices(P, pos, N, 13)
    assert {N - 1, N, N + 1, P - 2, P - 3, P - 302} <= set(left)
    eng = engine(th, pr)
    for sample in (0, None):
        rows = eng.screen_scores(pairs, csr(base), sample=sample)
        lists = lists_of(eng, pairs, N, known=csr(base), sample=sample)
        for i, (x, y) in enumerate(pos):
            ok = ref.eligible(P, x, y, base[i])
            assert int(ok.sum()) == left[i]
            want = ref.ref_rows(th, pr, x, y, sample)
            check_row(rank_rows(P, rows)[i], want, ok)
            check_query(lists[i], rows[i], want, P, pairs[i], N, ok)
    eng.close()


def wide_masks(P):
    from trigenicinteractionpredictor_amd.scan import pair_mask
    genes = np.sort(np.random.default_rng(6).choice(P, 200, replace=False))
    return {"random": (converged_ref.random_pair_mask_words(P), None), "allow": (pair_mask(P, genes=genes), genes)}


@pytest.mark.parametrize("which", ["random", "allow"])
def test_a_mask_at_width_is_the_blocked_thirds_added_to_known(which):
    """Mask rows of 19 words (P = 600): mask = blocked thirds merged into known, bit for bit, and
    eligibility as screen_ref.eligible has it."""
    K, P, B, N = E_K, E_P, E_B, E_N
    th, pr = scan_ref.random_params(K, P, E_SEED, B)
    mask, genes = wide_masks(P)[which]
    assert mask.shape == (608, 19)
    _, rank = scan_ref.rank_tables(P)
    rng = np.random.default_rng(14)
    pool = np.arange(P) if genes is None else np.sort(rank[genes])         # rank positions to draw most queries from
    pos = [tuple(sorted(int(v) for v in rng.choice(pool, 2, replace=False))) for _ in range(24)]
    pos += random_positions(P, 8, 15)
    bx, by = np.nonzero(np.triu(np.unpackbits(mask.view(np.uint8), axis=1, bitorder="little")[:P, :P], 1))
    assert bx.size
    own = len(pos)
    pos.append((int(bx[bx.size // 2]), int(by[bx.size // 2])))             # a query whose own pair is blocked
    pairs = to_ids(P, pos)
    base, _ = wide_slices(P, pos, N, 16)
    oks = [ref.eligible(P, x, y, mask=mask) for x, y in pos]
    assert not oks[own].any() and sum(int(ok.sum()) > N for ok in oks) >= 16
    merged = csr([np.union1d(b, np.flatnonzero(~ok)) for b, ok in zip(base, oks)])
    eng = engine(th, pr)
    for sample in (0, None):
        for n in (N, P):
            got = lists_of(eng, pairs, n, known=csr(base), sample=sample, mask=mask)
            want = lists_of(eng, pairs, n, known=merged, sample=sample)
            assert all(same_rows(g, w) for g, w in zip(got, want))
        rows = eng.screen_scores(pairs, csr(base), sample=sample, mask=mask)
        assert bits(rows) == bits(eng.screen_scores(pairs, merged, sample=sample))
        assert got[own][0].size == 0 and got[own][1].shape == (0, 3) and np.isnan(rows[own]).all()
        lists = lists_of(eng, pairs, N, known=csr(base), sample=sample, mask=mask)
        for i, (x, y) in enumerate(pos):
            ok = ref.eligible(P, x, y, base[i], mask)
            ref_row = ref.ref_rows(th, pr, x, y, sample)
            check_row(rank_rows(P, rows)[i], ref_row, ok)
            check_query(lists[i], rows[i], ref_row, P, pairs[i], N, ok)
    eng.close()


# ------------------------------------------------------------------ f. independence at width
def test_a_wide_query_does_not_depend_on_the_call(monkeypatch):
    """P = 600: the lists' rows sit in a workspace of leading dimension 608, the rows output has 600."""
    K, P, B, N = E_K, E_P, E_B, 64
    th, pr = scan_ref.random_params(K, P, E_SEED, B)
    rng = np.random.default_rng(2)
    others = np.array([rng.choice(P, 2, replace=False) for _ in range(40)], dtype=np.int32)
    q = to_ids(P, [ref.F_QUERY])
    x, y = ref.positions(P, q[0])
    assert (x, y) == ref.F_QUERY and P - 2 > ref.cap_of(N)
    eng = engine(th, pr)
    th0, p0 = bits(eng.theta.cpu().numpy()), bits(eng.pr.cpu().numpy())
    for sample in (0, None):
        (solo,) = eng.screen_top(q, N, sample=sample)
        solo_row = eng.screen_scores(q, sample=sample)[0]
        want = ref.ref_rows(th, pr, x, y, sample)
        check_row(rank_rows(P, solo_row[None])[0], want, ref.eligible(P, x, y))
        check_query(solo, solo_row, want, P, q[0], N)
        calls = [(np.concatenate([others[:at], q, others[at:]]), at) for at in (0, 17, 40)]
        calls.append((np.concatenate([q[:, ::-1], others]), 0))
        for chunk in (None, 1, 16, 17):
            if chunk is None:
                monkeypatch.delenv("MMSBM_SCREEN_CHUNK", raising=False)
            else:
                monkeypatch.setenv("MMSBM_SCREEN_CHUNK", str(chunk))    # read at every call
            for pairs, at in calls:
                lists = eng.screen_top(pairs, N, sample=sample)
                rows = eng.screen_scores(pairs, sample=sample)
                assert same_rows(lists[at], solo), (sample, chunk, at)
                assert bits(rows[at]) == bits(solo_row), (sample, chunk, at)
        monkeypatch.delenv("MMSBM_SCREEN_CHUNK", raising=False)
    assert bits(eng.theta.cpu().numpy()) == th0 and bits(eng.pr.cpu().numpy()) == p0
    eng.close()


# ------------------------------------------------------------------ g. realistic width
def test_realistic_width():
    """K = 10, P = 600, B = 8: rows within RTOL, lists exact at N = 8, and by set at each query's
    middle clear cut in [64, 512] (the order of hundreds of random scores is not the reference's to
    determine)."""
    K, P, B, seed = ref.G_CASE
    th, pr = scan_ref.random_params(K, P, seed, B)
    pos = random_positions(P, 32, 7)
    pairs = to_ids(P, pos)
    eng = engine(th, pr)
    for sample in (0, None):
        rows = eng.screen_scores(pairs, sample=sample)
        by_rank = rank_rows(P, rows)
        want = [ref.ref_rows(th, pr, x, y, sample) for x, y in pos]
        cuts = []
        for i, (x, y) in enumerate(pos):
            ok = ref.eligible(P, x, y)
            check_row(by_rank[i], want[i], ok)
            clear = converged_ref.clear_cuts(np.sort(want[i][ok])[::-1], 64, 512)
            assert clear.size, (sample, (x, y))         # no query is skipped
            cuts.append(int(clear[clear.size // 2]))
        lists = lists_of(eng, pairs, 8, sample=sample)
        for i in range(32):
            check_query(lists[i], rows[i], want[i], P, pairs[i], 8)
        for n in sorted(set(cuts)):
            idx = [i for i, c in enumerate(cuts) if c == n]
            for i, (s, ids) in zip(idx, lists_of(eng, pairs[idx], n, sample=sample)):
                ok = ref.eligible(P, *pos[i])
                converged_ref.check_set_cut(s, ids, want[i][ok], ref.row_keys(P, *pos[i])[ok], n, None, P)
    eng.close()


# ------------------------------------------------------------------ h. the c-tile stride
def test_the_score_kernel_strides_over_c_tiles():
    """The score kernel's grid holds at most 4096 workgroups of four c-tiles of 16 positions along c:
    past 4096 * 4 * 16 = 262,144 positions a wave takes a second tile.  A designed row of 262,177,
    a query at its start and one with both genes past 262,144."""
    P, N = ref.STRIDE_P, 8
    assert (P + 15) // 16 > 4096 * 4
    th, pr, place = ref.designed_params(P, "shuffled")
    pos = [(0, 1), (262150, 262170)]
    pairs = to_ids(P, pos)
    eng = engine(th, pr)
    rows = eng.screen_scores(pairs, sample=0)
    lists = lists_of(eng, pairs, N, sample=0)
    eng.close()
    by_rank = rank_rows(P, rows)
    for i, (x, y) in enumerate(pos):
        want = ref.ref_row(th[0], pr[0], x, y)
        ref.check_designed(want, place, P, x, y)
        check_row(by_rank[i], want, ref.eligible(P, x, y))
        check_query(lists[i], rows[i], want, P, pairs[i], N)
