#!/usr/bin/env python3
"""Vote scan timings (EMEngine.vote_census / consensus, include/mmsbm.h mmsbm_scan_votes), one GPU.

    python tools/scan_votes_bench.py [--reps 10] [--warmup 2] [--out profiles/scan_votes_bench.json]

Prints (and with --out writes) one JSON record stamped with mmsbm_build_id():
  * for the K = 10, B = 8 and the K = 30, B = 3 ensembles at P = 1500, each with a known-key table of
    100,000 random triples, at the thresholds where about 1 % and about 0.01 % of the triples have
    any vote, the median device time (HIP events around the whole call, after a warm-up, the calls
    of one case taking turns inside every repetition) of the bare C calls on resident tensors of
      - mmsbm_scan_census with that one threshold on the ensemble: the yardstick, existing code
        doing the same MFMA work;
      - mmsbm_scan_votes as the histogram-only call (capacity 0);
      - mmsbm_scan_votes listing at min_votes = ns and at min_votes = 1, capacity = the count (at
        least 1: the listing kernel, also when no triple is unanimous);
    with the ratios over the census and the census's own spread between repetitions;
  * per case the only route to the unanimous list without the vote scan, host clock: one
    EMEngine.scan_above per slot and the intersection of their keys on the host, against one
    EMEngine.consensus (both end to end, sorted, on the host).
Parameters are random normalised theta / p from a seeded generator.
"""
from __future__ import annotations

import argparse
import functools
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from scan_bench import params, random_known, resident  # noqa: E402


def taking_turns_ms(calls, reps, warmup):
    """{label: call} -> {label: median / min / max ms}: every repetition times each call once, in
    turn, so that a drift of the device's clocks falls on all of them alike."""
    import torch
    for _ in range(warmup):
        for call in calls.values():
            call()
    torch.cuda.synchronize()
    out = {label: [] for label in calls}
    for _ in range(reps):
        for label, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            out[label].append(e0.elapsed_time(e1))
    return {label: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "reps": reps}
            for label, v in out.items()}


def any_vote_thresholds(eng, P, fractions, seed):
    """The thresholds that about each of `fractions` of the triples reach in at least one slot: the
    quantiles of the per-triple maximum over the slots of the scores of 200,000 random triples."""
    from trigenicinteractionpredictor_amd.scan import rank_order
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.integers(0, P, (220000, 3)), axis=1)
    pos = pos[(pos[:, 0] < pos[:, 1]) & (pos[:, 1] < pos[:, 2])][:200000]
    best = eng.predict(rank_order(P)[pos].astype(np.int32)).max(axis=0)
    return [float(np.quantile(best, 1.0 - f)) for f in fractions]


def host_ms(call, reps):
    import torch
    out = []
    for i in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        result = call()
        out.append(time.perf_counter() - t0)
    return statistics.median(out[1:]) * 1e3, result


def shape_record(K, P, B, n_known, fractions, reps, warmup):
    import torch
    from trigenicinteractionpredictor_amd.engine import EMEngine
    from trigenicinteractionpredictor_amd.scan import pack_keys, rank_of, rank_order
    eng = EMEngine(K, P, B=B)
    eng.upload(*params(K, P, B, 1))
    known = random_known(P, n_known, 2)
    rank = rank_of(rank_order(P))
    rec = {"K": K, "P": P, "B": B, "known_keys": int(known.size), "triples": P * (P - 1) * (P - 2) // 6}
    bind = resident(eng, known, None)
    for f, t in zip(fractions, any_vote_thresholds(eng, P, fractions, 4)):
        hist = eng.vote_census(t, known)
        total = int(hist.sum())
        rows = {"all": int(hist[B]), "any": int(hist[1:].sum())}
        dev = lambda n, dt: torch.empty(max(n, 1), dtype=dt, device=eng.device)   # noqa: E731
        thr_d = torch.tensor([t], dtype=torch.float64, device=eng.device)
        counts = torch.empty(2, dtype=torch.int64, device=eng.device)
        hist_d, found = dev(B + 1, torch.int64), dev(1, torch.int64)
        calls = {"census": bind("census", (1,), (thr_d, 1), (counts,))}
        for label, m, n in (("votes_histogram_only", B, 0), ("votes_list_min_votes_ns", B, rows["all"]),
                            ("votes_list_min_votes_1", 1, rows["any"])):
            # a listing call has capacity >= 1 (capacity 0 is the histogram-only kernel), also when
            # nothing is unanimous
            calls[label] = bind("scan_votes", (), (t, m, max(n, 1) if label != "votes_histogram_only" else 0),
                                (hist_d, dev(n, torch.float64), dev(n, torch.int64), dev(n, torch.int32), found))
        c = taking_turns_ms(calls, reps, warmup)
        base = c["census"]
        spread = base["max_ms"] - base["min_ms"]
        for label in list(calls)[1:]:
            c[label]["over_census_median"] = c[label]["median_ms"] / base["median_ms"]
        c["census_spread_ms"] = spread
        c["histogram_only_minus_census_ms"] = c["votes_histogram_only"]["median_ms"] - base["median_ms"]
        c["histogram_only_within_census_spread"] = bool(c["histogram_only_minus_census_ms"] <= spread)
        c["histogram_is_the_bindings"] = bool((hist_d.cpu().numpy() == hist).all())

        def by_slot():      # today's only route to the unanimous list
            lists = [pack_keys(eng.scan_above(t, known, sample=s)[1], rank, P) for s in range(B)]
            return functools.reduce(np.intersect1d, lists)

        slot_ms, keys = host_ms(by_slot, max(3, reps // 3))
        cons_ms, (_, _, ids) = host_ms(lambda: eng.consensus(t, None, known), max(3, reps // 3))
        c["unanimous_list_host_clock"] = {
            "scan_above_per_slot_and_intersection_ms": slot_ms, "consensus_ms": cons_ms,
            "ratio": slot_ms / cons_ms, "same_keys": bool(np.array_equal(np.sort(pack_keys(ids, rank, P)), keys))}
        rec["any_vote_%g" % f] = {"threshold": t, "eligible": total, "any_vote_fraction": rows["any"] / total,
                                  "rows_min_votes_ns": rows["all"], "rows_min_votes_1": rows["any"],
                                  "hist": [int(h) for h in hist], "c_calls_on_resident_tensors": c}
    eng.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--known", type=int, default=100000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from trigenicinteractionpredictor_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("scan_votes_bench needs the GPU")
    torch.cuda.set_device(0)
    shapes = [shape_record(K, 1500, B, a.known, (0.01, 0.0001), a.reps, a.warmup) for K, B in ((10, 8), (30, 3))]
    rec = {"metric": "vote scan, median ms per call", "build_id": _lib.build_id(),
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
