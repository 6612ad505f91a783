#!/usr/bin/env python3
"""Pair-masked census and threshold scan timings (include/mmsbm.h mmsbm_scan_census_masked,
mmsbm_scan_above_masked), one GPU.

    python tools/scan_masked_bench.py [--reps 10] [--warmup 2] [--out profiles/scan_masked_bench.json]
    python tools/scan_masked_bench.py --families [--out profiles/scan_masked_families_bench.json]

Prints (and with --out writes) one JSON record stamped with mmsbm_build_id():
  * for K = 10 at B = 1 and B = 8 and K = 30 at B = 3, all at P = 1500 without a key table, at one
    threshold near the 1 % quantile of the scores, the median device time (HIP events around the
    whole call, after a warm-up, the calls of one case taking turns inside every repetition) of the
    bare C calls on resident tensors of
      - mmsbm_scan_census / mmsbm_scan_above: the yardstick, the unmasked kernels of the same build;
      - the masked calls with (i) an all-zero mask, (ii) 10 % of the pairs blocked at random,
        (iii) 300 allowed genes of the 1500;
    with each masked call's ratio over its yardstick, the yardstick's own min-max spread between
    repetitions (the margin for "no cost"), what (i) costs beyond it, and whether (iii) runs faster
    than (i) by more than that spread (four fifths of its work items are skipped before their W
    rows are formed);
  * per case the masked top-N route end to end on the host clock: EMEngine.scan_top_any(1000,
    mask=) under mask (ii) (masked censuses bracket the cut, the masked threshold scan lists above
    it) next to the unmasked EMEngine.scan_top(1000).
--families times, in the same way, on the same shapes and under the same three masks, the masked
pair census (mmsbm_pair_census_masked: M = 1 at that threshold, and M = 8 over the thresholds that
10 % down to 0.1 % of the scores reach), the masked vote scan (mmsbm_scan_votes_masked at that
threshold: histogram-only, and listing every triple with a vote) and the masked quorum scan
(mmsbm_scan_quorum_topn_masked: N = 1000 at m = ns and, where it differs, at the majority
m = ns / 2 + 1), each next to the unmasked call of the same build in the same run.
Parameters are random normalised theta / p from a seeded generator.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from scan_bench import params  # noqa: E402
from scan_votes_bench import host_ms, taking_turns_ms  # noqa: E402

MASKED = {"census": "mmsbm_scan_census_masked", "scan_above": "mmsbm_scan_above_masked"}
PLAIN = {"census": "mmsbm_scan_census", "scan_above": "mmsbm_scan_above"}


def masks(P, seed):
    """{label: uint32 mask}: all zero, 10 % of the pairs at random, 300 allowed genes."""
    from trigenicinteractionpredictor_amd.scan import pair_mask
    rng = np.random.default_rng(seed)
    x, y = np.triu_indices(P, 1)
    pick = rng.random(x.size) < 0.1
    return {"zero": pair_mask(P), "random_10pct": pair_mask(P, pairs=np.stack([x[pick], y[pick]], axis=1)),
            "allowed_300": pair_mask(P, genes=rng.permutation(P)[:300])}


def quantile_threshold(eng, P, fraction, sample, seed):
    """The score that about `fraction` of the triples reach: a quantile over 200,000 random triples."""
    from trigenicinteractionpredictor_amd.scan import rank_order
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.integers(0, P, (220000, 3)), axis=1)
    pos = pos[(pos[:, 0] < pos[:, 1]) & (pos[:, 1] < pos[:, 2])][:200000]
    p = eng.predict(rank_order(P)[pos].astype(np.int32))
    p = p[sample] if sample is not None else p[:eng.active].mean(axis=0)
    return float(np.quantile(p, 1.0 - fraction))


def shape_record(K, P, B, reps, warmup):
    import torch
    from trigenicinteractionpredictor_amd.engine import EMEngine
    eng = EMEngine(K, P, B=B)
    eng.upload(*params(K, P, B, 1))
    sample = 0 if B == 1 else None
    t = quantile_threshold(eng, P, 0.01, sample, 4)
    rec = {"K": K, "P": P, "B": B, "threshold": t, "triples": P * (P - 1) * (P - 2) // 6}
    host = masks(P, 7)
    dev = {label: torch.from_numpy(m.view(np.int32)).to(eng.device) for label, m in host.items()}
    head = (eng.ctx, eng.scan_order.data_ptr(), None, 0)
    tail = (eng.theta.data_ptr(), eng.pr.data_ptr(), -1 if sample is None else sample)
    thr_d = torch.tensor([t], dtype=torch.float64, device=eng.device)
    rows = {label: int(eng.census([t], None, sample, mask=m)[0][0]) for label, m in host.items()}
    rows["unmasked"] = int(eng.census([t], None, sample)[0][0])
    assert rows["zero"] == rows["unmasked"]
    rec["rows_at_threshold"] = rows
    rec["eligible"] = {label: int(eng.census([], None, sample, mask=m)[1]) for label, m in host.items()}
    keep = []

    def bind(family, label):
        ws = eng.scan_workspace(family, *((1,) if family == "census" else ()))
        n = max(rows[label or "unmasked"], 1)
        if family == "census":
            outs = [torch.empty(2, dtype=torch.int64, device=eng.device)]
            mid = (thr_d.data_ptr(), 1)
        else:
            outs = [torch.empty(n, dtype=torch.float64, device=eng.device),
                    torch.empty(n, dtype=torch.int64, device=eng.device),
                    torch.empty(1, dtype=torch.int64, device=eng.device)]
            mid = (t, n)
        keep.append(outs)
        entry = getattr(eng.lib, (MASKED if label else PLAIN)[family])
        args = (*head, *((dev[label].data_ptr(),) if label else ()), *tail, *mid, ws.data_ptr(), ws.numel(),
                *[o.data_ptr() for o in outs])

        def call():
            assert entry(*args, eng._stream()) == 0
        return call

    for family in ("census", "scan_above"):
        calls = {"unmasked": bind(family, None)}
        for label in host:
            calls["masked_" + label] = bind(family, label)
        c = taking_turns_ms(calls, reps, warmup)
        base = c["unmasked"]
        spread = base["max_ms"] - base["min_ms"]
        for label in host:
            c["masked_" + label]["over_unmasked_median"] = c["masked_" + label]["median_ms"] / base["median_ms"]
        c["unmasked_spread_ms"] = spread
        c["zero_mask_minus_unmasked_ms"] = c["masked_zero"]["median_ms"] - base["median_ms"]
        c["zero_mask_within_unmasked_spread"] = bool(c["zero_mask_minus_unmasked_ms"] <= spread)
        c["allowed_300_below_zero_mask_ms"] = c["masked_zero"]["median_ms"] - c["masked_allowed_300"]["median_ms"]
        c["item_skip_works"] = bool(c["allowed_300_below_zero_mask_ms"] > spread)
        rec[family] = c
    top_ms, (s0, _) = host_ms(lambda: eng.scan_top(1000, None, sample), max(3, reps // 3))
    any_ms, (s1, _) = host_ms(lambda: eng.scan_top_any(1000, None, sample, mask=host["random_10pct"]),
                              max(3, reps // 3))
    rec["top_1000_host_clock"] = {"scan_top_unmasked_ms": top_ms, "scan_top_any_masked_random_10pct_ms": any_ms,
                                  "rows": [int(s0.size), int(s1.size)]}
    eng.close()
    return rec


def ratios(c, host):
    """The derived figures of one case {label: times}, as shape_record reports them."""
    base = c["unmasked"]
    spread = base["max_ms"] - base["min_ms"]
    for label in host:
        c["masked_" + label]["over_unmasked_median"] = c["masked_" + label]["median_ms"] / base["median_ms"]
    c["unmasked_spread_ms"] = spread
    c["unmasked_spread_over_median"] = spread / base["median_ms"]
    c["zero_mask_minus_unmasked_ms"] = c["masked_zero"]["median_ms"] - base["median_ms"]
    c["zero_mask_within_unmasked_spread"] = bool(c["zero_mask_minus_unmasked_ms"] <= spread)
    c["allowed_300_below_unmasked_ms"] = base["median_ms"] - c["masked_allowed_300"]["median_ms"]
    c["allowed_300_below_unmasked_by_more_than_spread"] = bool(c["allowed_300_below_unmasked_ms"] > spread)
    return c


FAMILY_ENTRIES = {"pair_census": ("mmsbm_pair_census", "mmsbm_pair_census_masked"),
                  "scan_votes": ("mmsbm_scan_votes", "mmsbm_scan_votes_masked"),
                  "scan_quorum": ("mmsbm_scan_quorum_topn", "mmsbm_scan_quorum_topn_masked")}


def families_record(K, P, B, reps, warmup):
    """The pair census, the vote scan and the quorum scan of one shape: unmasked and under the three masks."""
    import torch
    from trigenicinteractionpredictor_amd.engine import EMEngine
    eng = EMEngine(K, P, B=B)
    eng.upload(*params(K, P, B, 1))
    sample = 0 if B == 1 else None
    ns = 1 if B == 1 else B
    t = quantile_threshold(eng, P, 0.01, sample, 4)
    t8 = sorted(quantile_threshold(eng, P, f, sample, 4) for f in (0.1, 0.05, 0.03, 0.02, 0.01, 0.005, 0.002, 0.001))
    rec = {"K": K, "P": P, "B": B, "threshold": t, "thresholds_M8": t8, "triples": P * (P - 1) * (P - 2) // 6}
    host = masks(P, 7)
    dev = {label: torch.from_numpy(m.view(np.int32)).to(eng.device) for label, m in host.items()}
    head = (eng.ctx, eng.scan_order.data_ptr(), None, 0)
    tail = (eng.theta.data_ptr(), eng.pr.data_ptr(), -1 if sample is None else sample)
    hists = {label: eng.vote_census(t, None, sample, mask=m) for label, m in host.items()}
    hists["unmasked"] = eng.vote_census(t, None, sample)
    assert (hists["zero"] == hists["unmasked"]).all()
    rec["eligible"] = {label: int(h.sum()) for label, h in hists.items()}
    rec["rows_with_a_vote"] = {label: int(h[1:].sum()) for label, h in hists.items()}
    thr1 = torch.tensor([t], dtype=torch.float64, device=eng.device)
    thr8 = torch.tensor(t8, dtype=torch.float64, device=eng.device)
    keep = [thr1, thr8]

    def empty(shape, dtype):
        keep.append(torch.empty(shape, dtype=dtype, device=eng.device))
        return keep[-1]

    def bind(family, size_args, mid, outs, label):
        ws = eng.scan_workspace(family, *size_args)
        entry = getattr(eng.lib, FAMILY_ENTRIES[family][1 if label else 0])
        args = (*head, *((dev[label].data_ptr(),) if label else ()), *tail, *mid, ws.data_ptr(), ws.numel(),
                *[None if o is None else o.data_ptr() for o in outs])

        def call():
            assert entry(*args, eng._stream()) == 0
        return call

    def case(family, size_args, mid, outs):
        calls = {"unmasked": bind(family, size_args, mid, outs, None)}
        for label in host:
            calls["masked_" + label] = bind(family, size_args, mid, outs, label)
        return ratios(taking_turns_ms(calls, reps, warmup), host)

    rec["pair_census_M1"] = case("pair_census", (1,), (thr1.data_ptr(), 1), [empty((P, P, 1), torch.int32)])
    rec["pair_census_M8"] = case("pair_census", (8,), (thr8.data_ptr(), 8), [empty((P, P, 8), torch.int32)])
    hist_d, found = empty(ns + 1, torch.int64), empty(1, torch.int64)
    rec["votes_histogram_only"] = case("scan_votes", (), (t, ns, 0), [hist_d, None, None, None, found])
    n = max(rec["rows_with_a_vote"]["unmasked"], 1)
    rows = [empty(n, torch.float64), empty(n, torch.int64), empty(n, torch.int32)]
    rec["votes_list_min_votes_1"] = case("scan_votes", (), (t, 1, n), [hist_d, *rows, found])
    N = 1000
    qouts = [empty(N, torch.float64), empty((N, 3), torch.int32), found]
    for m in sorted({ns, ns // 2 + 1}, reverse=True):
        rec["quorum_top_1000_m%d" % m] = dict(case("scan_quorum", (N,), (m, N), qouts), min_votes=m,
                                              depth=min(m, ns - m + 1) if ns > 1 else 0)
    eng.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--families", action="store_true",
                    help="the masked pair census, vote scan and quorum scan instead of the census and threshold scan")
    a = ap.parse_args()

    import torch
    from trigenicinteractionpredictor_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("scan_masked_bench needs the GPU")
    torch.cuda.set_device(0)
    record = families_record if a.families else shape_record
    shapes = [record(K, 1500, B, a.reps, a.warmup) for K, B in ((10, 1), (10, 8), (30, 3))]
    metric = ("pair-masked pair census, vote scan and quorum scan" if a.families
              else "pair-masked census and threshold scan") + ", median ms per call"
    rec = {"metric": metric, "build_id": _lib.build_id(),
           "device": torch.cuda.get_device_name(0), "dtype": "f64",
           "timing": "HIP events around one whole bare C call on resident tensors; the calls of one case take "
                     "turns inside every repetition; medians over reps after a warm-up",
           "shapes": shapes}
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
