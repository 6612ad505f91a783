"""Host side of the pair mask in the genome-wide top-N scan and the partner scan (no GPU): the two
masked entries in the header and the binding, tests/partners_masked_ref.py against a triple loop,
the driver's refusal of --gene with the mask flags, the routing of EMEngine.scan_top_any on a fake
engine, and the Python-side checks of the mask's shape and dtype."""
import itertools
import os
import re

import numpy as np
import pytest

import masked_ref
import partners_masked_ref as pm
import scan_ref
from golden_util import GOLDEN

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRAIN = os.path.join(GOLDEN, "tiny", "train.dat")
MASKS = {"random": masked_ref.random_mask, "allowed": masked_ref.allowed_mask, "single": masked_ref.single_pair_mask,
         "last_tile": masked_ref.last_tile_mask, "full": masked_ref.full_mask,
         "zero": lambda P: masked_ref.naive_mask(P, [])}


# ------------------------------------------------------------------ the header and the binding
@pytest.mark.parametrize("entry,behind", [("mmsbm_scan_topn_masked", "int64_t n_known"),
                                          ("mmsbm_partners_topn_masked", "const int64_t *known_pairs")])
def test_the_binding_and_the_header_name_the_two_entries(entry, behind):
    from trigenicinteractionpredictor_amd import _lib
    header = open(os.path.join(REPO, "include", "mmsbm.h")).read()
    assert entry in _lib.SIGNATURES
    res, args = _lib.SIGNATURES[entry]
    res0, args0 = _lib.SIGNATURES[entry.replace("_masked", "")]

    def params_of(name):
        m = re.search(r"^int %s\(([^;]*)\);" % name, header, re.M)
        assert m, name + " is not declared"
        return [" ".join(p.split()) for p in m.group(1).replace("\n", " ").split(",")]

    params, params0 = params_of(entry), params_of(entry.replace("_masked", ""))
    at = params0.index(behind) + 1
    # the unmasked call with one pointer behind n_known / known_pairs, in the header and in the binding
    assert params == params0[:at] + ["const uint32_t *mask"] + params0[at:]
    assert res is res0 and list(args) == list(args0[:at]) + [args0[0]] + list(args0[at:])
    assert len(params) == len(args)


def test_the_masked_calls_share_the_unmasked_workspaces():
    header = open(os.path.join(REPO, "include", "mmsbm.h")).read()
    assert not re.search(r"mmsbm_(scan_topn|partners_topn|partners)_masked_workspace_bytes", header)


# ------------------------------------------------------------------ the support module
def loop_blocked_pairs(mask, P, q):
    """One triple at a time: the pair keys b P + c of the candidates of q that hold a blocked pair,
    each pair read at (min, max) only."""
    def blocked(x, y):
        x, y = min(x, y), max(x, y)
        return bool((int(mask[x, y >> 5]) >> (y & 31)) & 1)

    out = []
    for b, c in itertools.combinations(range(P), 2):
        if q in (b, c):
            continue
        if blocked(q, b) or blocked(q, c) or blocked(b, c):
            out.append(b * P + c)
    return np.array(out, dtype=np.int64)


@pytest.mark.parametrize("name", sorted(MASKS))
@pytest.mark.parametrize("P", [3, 12, 33])
def test_blocked_pairs_against_a_triple_loop(P, name):
    mask = np.ascontiguousarray(MASKS[name](P))
    # only x < y is read: the lower triangle, the diagonal, the rows and the bits beyond P change nothing
    noisy = masked_ref.position_mask(P, np.zeros((P, P), dtype=bool))
    for x in range(P):
        for y in range(x + 1, P):
            noisy[x, y >> 5] |= mask[x, y >> 5] & np.uint32(1 << (y & 31))
    noisy[P:, :] = np.uint32(0xFFFFFFFF)
    for x in range(P):
        noisy[x, x >> 5] |= np.uint32(1 << (x & 31))
    every = masked_ref.all_keys(P)
    for q in range(P):
        got = pm.blocked_pairs(mask, P, q)
        want = loop_blocked_pairs(mask, P, q)
        assert got.dtype == np.int64
        np.testing.assert_array_equal(got, want)
        assert (np.diff(got) > 0).all()                          # sorted and unique, as known_pairs must be
        np.testing.assert_array_equal(pm.blocked_pairs(noisy, P, q), want)
        # the same triples the genome-wide rule blocks among those that contain q
        a, b, c = every // (P * P), (every // P) % P, every % P
        has_q = (a == q) | (b == q) | (c == q)
        gone = every[has_q & masked_ref.blocked(every, mask, P)]
        x, y = [], []
        for k in gone.tolist():
            rest = [v for v in (k // (P * P), (k // P) % P, k % P) if v != q]
            x.append(rest[0]), y.append(rest[1])
        np.testing.assert_array_equal(np.sort(np.array(x, dtype=np.int64) * P + np.array(y, dtype=np.int64)), want)
    if name == "full":
        assert all(pm.blocked_pairs(mask, P, q).size == (P - 1) * (P - 2) // 2 for q in range(P))
    if name == "zero":
        assert all(pm.blocked_pairs(mask, P, q).size == 0 for q in range(P))


def test_merged_known_and_the_query_masks():
    P = 33
    order, rank = scan_ref.rank_tables(P)
    mask = np.ascontiguousarray(masked_ref.random_mask(P))
    queries = [4, 0, 4, 32]
    known = (np.array([0, 2, 2, 3, 5], dtype=np.int64), np.array([1 * P + 2, 5 * P + 9, 3 * P + 7, 0 * P + 1, 2 * P + 3]))
    off, pairs = pm.merged_known(mask, P, queries, known)
    assert off.dtype == np.int64 and pairs.dtype == np.int64 and off.size == 5 and off[-1] == pairs.size
    for i, g in enumerate(queries):
        sl = pairs[off[i]:off[i + 1]]
        want = np.union1d(loop_blocked_pairs(mask, P, int(rank[g])), known[1][known[0][i]:known[0][i + 1]])
        np.testing.assert_array_equal(sl, want)
    off0, pairs0 = pm.merged_known(mask, P, queries)
    assert [pairs0[off0[i]:off0[i + 1]].tolist() for i in range(4)] == \
        [loop_blocked_pairs(mask, P, int(rank[g])).tolist() for g in queries]
    q = 7
    others = (P - 1) * (P - 2) // 2
    assert pm.blocked_pairs(pm.query_all_mask(P, q), P, q).size == others
    assert pm.blocked_pairs(pm.query_all_mask(P, q), P, 8).size == P - 2        # the pairs that hold q
    part = pm.blocked_pairs(pm.only_with_query_mask(P, q), P, q)
    assert 0 < part.size < others
    without = pm.only_without_query_mask(P, q)
    assert without.any() and not masked_ref.bit(without, np.full(P, q), np.arange(P)).any()
    assert not masked_ref.bit(without, np.arange(P), np.full(P, q)).any()


# ------------------------------------------------------------------ the driver
@pytest.mark.parametrize("flag", [["--allow-genes", "f.txt"], ["--block-pairs", "f.txt"]])
@pytest.mark.parametrize("other", [["--gene", "3"], ["--all-genes"]])
def test_the_driver_still_refuses_gene_tables_under_the_mask_flags(other, flag, capsys):
    from trigenicinteractionpredictor_amd import cli, scan
    with pytest.raises(cli.ArgError):
        scan.parse(["-t", TRAIN, *flag, *other])
    text = capsys.readouterr().out
    assert other[0] in text
    assert "takes no" not in text           # the kernel takes a mask by now: the driver does not apply it
    cfg = scan.parse(["-t", TRAIN, *flag])   # the main table goes with them
    assert cfg[flag[0][2:].replace("-", "_")] == "f.txt"


# ------------------------------------------------------------------ scan_top_any's routing
class FakeEngine:
    """EMEngine.scan_top_any on an engine whose three calls answer from a list of scores (key =
    index) and record what they were asked."""

    def __init__(self, scores, cap=4):
        from trigenicinteractionpredictor_amd.engine import EMEngine
        self.scores = np.sort(np.asarray(scores, dtype=np.float64))[::-1]
        self.calls = []
        self.lib = type("Lib", (), {"mmsbm_scan_max_n": staticmethod(lambda: cap)})()
        self.scan_top_any = EMEngine.scan_top_any.__get__(self)

    def _ids(self, n):
        return np.arange(n, dtype=np.int32)[:, None].repeat(3, axis=1)

    def scan_top(self, n, known=None, sample=None, stream=None, mask=None):
        self.calls.append(("scan_top", n, mask))
        m = min(n, self.scores.size)
        return self.scores[:m].copy(), self._ids(m)

    def census(self, thresholds, known=None, sample=None, stream=None, mask=None):
        self.calls.append(("census", len(thresholds), mask))
        return np.array([(self.scores >= t).sum() for t in thresholds], dtype=np.int64), self.scores.size

    def scan_above(self, threshold, known=None, sample=None, stream=None, limit=1 << 26, mask=None):
        self.calls.append(("scan_above", threshold, mask))
        m = int((self.scores >= threshold).sum())
        return self.scores[:m].copy(), self._ids(m)


@pytest.mark.parametrize("mask", [None, "a mask"])
def test_scan_top_any_routes_through_the_masked_scan_top(mask):
    scores = np.linspace(0.05, 0.95, 19)
    kw = {} if mask is None else {"mask": mask}
    # n <= cap: one scan_top with the mask, no census, no threshold scan
    eng = FakeEngine(scores)
    s, ids = eng.scan_top_any(3, **kw)
    assert eng.calls == [("scan_top", 3, mask)] and s.tolist() == eng.scores[:3].tolist()
    eng = FakeEngine(scores)
    eng.scan_top_any(4, **kw)
    assert eng.calls == [("scan_top", 4, mask)]
    # above the cap: scan_top(max), then the bracket from its last score and one threshold scan, all masked
    eng = FakeEngine(scores)
    s, ids = eng.scan_top_any(7, **kw)
    assert eng.calls[0] == ("scan_top", 4, mask)
    assert [c[0] for c in eng.calls[1:]] == ["census"] * (len(eng.calls) - 2) + ["scan_above"]
    assert len(eng.calls) >= 3 and all(c[2] == mask for c in eng.calls)
    assert eng.calls[-1][1] <= eng.scores[6] and s.tolist() == eng.scores[:7].tolist() and ids.shape == (7, 3)
    # fewer eligible than the cap: the masked scan_top(max) is all there is
    eng = FakeEngine(scores[:3])
    s, ids = eng.scan_top_any(7, **kw)
    assert eng.calls == [("scan_top", 4, mask)] and s.size == 3
    with pytest.raises(ValueError):
        eng.scan_top_any(0, **kw)


# ------------------------------------------------------------------ shape and dtype checks
def test_the_python_side_checks_the_mask():
    from trigenicinteractionpredictor_amd import scan
    P = 33
    mask = np.ascontiguousarray(masked_ref.random_mask(P))
    assert scan.check_pair_mask(mask, P) is mask
    for bad in (mask.astype(np.int64), mask.astype(np.int32), mask[:-1], mask[:, :-1], mask.T, mask.tolist(),
                np.asfortranarray(mask) if mask.shape[1] > 1 else mask.tolist()):
        with pytest.raises(ValueError):
            scan.check_pair_mask(bad, P)
    # the engine's entry points take the keyword and hand it to the one check (EMEngine._scan_call)
    import inspect
    from trigenicinteractionpredictor_amd import Model
    from trigenicinteractionpredictor_amd import joint
    from trigenicinteractionpredictor_amd.engine import EMEngine
    for fn in (EMEngine.scan_top, EMEngine.scan_top_async, EMEngine.partners_top, EMEngine.partners_top_async,
               EMEngine.scan_top_any, Model.predict_novel, Model.predict_partners, Model.predict_third):
        p = inspect.signature(fn).parameters
        assert "mask" in p and p["mask"].default is None, fn
    p = inspect.signature(joint.Model.predict_trigenic_partners).parameters
    assert list(p)[1:] == ["gene", "n", "threshold", "exclude"]
    assert p["threshold"].default == 0.5 and tuple(p["exclude"].default) == ("train", "test")
