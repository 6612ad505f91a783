#!/usr/bin/env python3
"""Dispute scan timings (EMEngine.spread_top, include/mmsbm.h mmsbm_scan_spread_topn), one GPU.

    python tools/scan_spread_bench.py [--reps 10] [--warmup 2] [--out profiles/scan_spread_bench.json]

Prints (and with --out writes) one JSON record stamped with mmsbm_build_id():
  * for the K = 10, B = 8 and the K = 30, B = 3 ensembles at P = 1500, each with a known-key table of
    100,000 random triples, at N = 1000, the median device time (HIP events around the whole call,
    after a warm-up, the calls of one case taking turns inside every repetition) of the bare C calls
    on resident tensors of
      - mmsbm_scan_quorum_topn with the early exit off (MMSBM_SCAN_QUORUM_EARLY=0) at the majority
        min_votes = ns / 2 + 1: the yardstick, existing code that runs the same MFMA chains over
        every slot and keeps a sorted list of similar depth;
      - mmsbm_scan_spread_topn at trim 0 and at the largest legal trim;
    with the ratios over the yardstick and the yardstick's own spread between repetitions;
  * per case today's route to the same list, host clock: one EMEngine.scan_above(lo, sample=s) per
    slot, lo below every score, sorted[ns - 1 - t] - sorted[t] per key and the sort on the host,
    against one EMEngine.spread_top (end to end, on the host); at a smaller P (--join-p, default
    300), since the route holds C(P, 3) rows per slot.
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

from scan_bench import params, random_known, resident  # noqa: E402
from scan_quorum_bench import with_early  # noqa: E402
from scan_votes_bench import host_ms, taking_turns_ms  # noqa: E402


def shape_record(K, P, B, N, n_known, reps, warmup):
    import torch
    from trigenicinteractionpredictor_amd.engine import EMEngine
    eng = EMEngine(K, P, B=B)
    eng.upload(*params(K, P, B, 1))
    known = random_known(P, n_known, 2)
    rec = {"K": K, "P": P, "B": B, "N": N, "known_keys": int(known.size), "triples": P * (P - 1) * (P - 2) // 6}
    bind = resident(eng, known, None)
    outs = lambda: (torch.empty(N, dtype=torch.float64, device=eng.device),                  # noqa: E731
                    torch.empty((N, 3), dtype=torch.int32, device=eng.device),
                    torch.empty(1, dtype=torch.int64, device=eng.device))
    majority = B // 2 + 1
    trims = sorted({0, eng.spread_trims()[-1]})
    calls = {"quorum_early_off_majority": with_early(bind("scan_quorum", (N,), (majority, N), outs()), "0")}
    for t in trims:
        calls["spread_trim_%d" % t] = bind("scan_spread", (N,), (t, N), outs())
    c = taking_turns_ms(calls, reps, warmup)
    base = c["quorum_early_off_majority"]
    for label in list(calls)[1:]:
        c[label]["over_yardstick_median"] = c[label]["median_ms"] / base["median_ms"]
    c["yardstick_spread_ms"] = base["max_ms"] - base["min_ms"]
    c["yardstick_spread_over_median"] = (base["max_ms"] - base["min_ms"]) / base["median_ms"]
    rec["majority"], rec["yardstick_depth"] = majority, eng.quorum_depth(majority)
    rec["trims"], rec["spread_depths"] = trims, [t + 1 for t in trims]
    rec["c_calls_on_resident_tensors"] = c
    eng.close()
    return rec


def join_record(K, P, B, N, reps):
    """Today's route against spread_top, host clock, at trim 0 and at the largest legal trim."""
    from trigenicinteractionpredictor_amd.engine import EMEngine
    from trigenicinteractionpredictor_amd.scan import pack_keys, rank_of, rank_order
    eng = EMEngine(K, P, B=B)
    eng.upload(*params(K, P, B, 1))
    known = random_known(P, 1000, 2)
    rank = rank_of(rank_order(P))
    rec = {"K": K, "P": P, "B": B, "N": N, "known_keys": int(known.size)}
    for t in sorted({0, eng.spread_trims()[-1]}):
        def by_slot():
            per, keys = [], None
            for s in range(B):
                sc, ids = eng.scan_above(1e-300, known, sample=s)
                k = pack_keys(ids, rank, P)
                at = np.argsort(k)
                keys = k[at]
                per.append(sc[at])
            srt = np.sort(np.stack(per), axis=0)
            d = srt[B - 1 - t] - srt[t]
            order = np.lexsort((keys, -d))[:N]
            return d[order], keys[order]

        slot_ms, (d, keys) = host_ms(by_slot, reps)
        top_ms, (s, ids) = host_ms(lambda: eng.spread_top(N, t, known), reps)
        rec["trim_%d" % t] = {
            "scan_above_per_slot_and_join_ms": slot_ms, "spread_top_ms": top_ms, "ratio": slot_ms / top_ms,
            "same_list": bool(s.tobytes() == d.tobytes() and np.array_equal(pack_keys(ids, rank, P), keys))}
    eng.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--known", type=int, default=100000)
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--p", type=int, default=1500)
    ap.add_argument("--join-p", type=int, default=300)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from trigenicinteractionpredictor_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("scan_spread_bench needs the GPU")
    torch.cuda.set_device(0)
    cases = ((10, 8), (30, 3))
    shapes = [shape_record(K, a.p, B, a.n, a.known, a.reps, a.warmup) for K, B in cases]
    joins = [join_record(K, a.join_p, B, a.n, 3) for K, B in cases]
    rec = {"metric": "dispute scan, median ms per call", "build_id": _lib.build_id(),
           "device": torch.cuda.get_device_name(0), "dtype": "f64",
           "timing": "HIP events around one whole bare C call on resident tensors; the calls of one case take "
                     "turns inside every repetition; medians over reps after a warm-up",
           "yardstick": "mmsbm_scan_quorum_topn, MMSBM_SCAN_QUORUM_EARLY=0, min_votes = ns / 2 + 1",
           "shapes": shapes, "todays_route_host_clock": joins}
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
