#!/usr/bin/env python3
"""Partner statistics timings (EMEngine.partners_quorum_top / partners_spread_top, include/mmsbm.h
mmsbm_partners_stat_topn), one GPU.

    python tools/partners_stat_bench.py [--reps 10] [--warmup 2] [--out profiles/partners_stat_bench.json]

Prints (and with --out writes) one JSON record stamped with mmsbm_build_id().  At P = 1500, K = 10,
N = 100, the B = 8 ensemble and Q = 1, 64 and 1500 query genes (Q = 1500: every gene), the device time
of one call's launches (HIP events around the _async form, medians over reps after a warm-up):
  * partners_quorum_top at m = 1, 5 and 8, with the early exit and with MMSBM_PARTNERS_STAT_EARLY=0;
  * partners_spread_top at t = 0 and 3;
  * partners_top over the ensemble mean on the same engine: the yardstick, the kernel that does the
    same MFMA work with a slot-order sum in place of the sorted lists;
  * each stat call's ratio to the yardstick, the three calls of a comparison alternating in one loop;
  * same_lists: whether the quorum lists with and without the early exit are identical (they must be).
Parameters are random normalised theta / p from a seeded generator.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

EARLY = "MMSBM_PARTNERS_STAT_EARLY"     # read by the library at every call


def params(K, P, B, seed):
    rng = np.random.default_rng(seed)
    th = rng.random((B, P, K))
    th /= th.sum(axis=2, keepdims=True)
    pr = rng.random((B, K, K, K, 2))
    pr /= pr.sum(axis=4, keepdims=True)
    return th, pr


def set_early(on):
    if on:
        os.environ.pop(EARLY, None)
    else:
        os.environ[EARLY] = "0"


def device_ms(calls, reps, warmup):
    """{name: [ms]} of the named calls, alternating inside every repetition."""
    import torch
    for _ in range(warmup):
        for call in calls.values():
            call()
    torch.cuda.synchronize()
    out = {name: [] for name in calls}
    for _ in range(reps):
        for name, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            out[name].append(e0.elapsed_time(e1))
    return out


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def identical(mine, theirs):
    return all(a[1].shape == b[1].shape and bool((a[1] == b[1]).all()) and a[0].tobytes() == b[0].tobytes()
               for a, b in zip(mine, theirs))


def shape_record(K, P, B, Q, N, votes, trims, reps, warmup):
    from trigenicinteractionpredictor_amd.engine import EMEngine
    eng = EMEngine(K, P, B=B)
    eng.upload(*params(K, P, B, 1))
    rng = np.random.default_rng(4)
    genes = np.arange(P, dtype=np.int32) if Q >= P else rng.choice(P, Q, replace=False).astype(np.int32)
    pairs = (P - 1) * (P - 2) // 2
    rec = {"K": K, "P": P, "B": B, "Q": int(genes.size), "N": N, "scores": int(genes.size) * pairs,
           "score_flop": 2.0 * K * int(genes.size) * pairs * B}

    def quorum(m, early):
        def call():
            set_early(early)
            out = eng.partners_quorum_top_async(genes, N, m)
            set_early(True)
            return out
        return call

    calls = {"mean_top": lambda: eng.partners_top_async(genes, N)}
    for m in votes:
        calls["quorum_m%d" % m] = quorum(m, True)
        calls["quorum_m%d_no_exit" % m] = quorum(m, False)
    for t in trims:
        calls["spread_t%d" % t] = (lambda t: lambda: eng.partners_spread_top_async(genes, N, t))(t)
    ms = device_ms(calls, reps, warmup)
    for name, v in ms.items():
        rec[name + "_device"] = spread(v)
    base = rec["mean_top_device"]["median_ms"]
    for name in ms:
        if name != "mean_top":
            rec[name + "_ratio_over_mean_top"] = rec[name + "_device"]["median_ms"] / base
    same = True
    for m in votes:
        set_early(True)
        on = eng.partners_quorum_top(genes, N, m)
        set_early(False)
        off = eng.partners_quorum_top(genes, N, m)
        set_early(True)
        same = same and identical(on, off)
    rec["same_lists"] = same
    eng.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--top", type=int, default=100)
    ap.add_argument("--genes", type=int, default=1500)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--queries", default="1,64,1500")
    ap.add_argument("--votes", default="1,5,8")
    ap.add_argument("--trims", default="0,3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from trigenicinteractionpredictor_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("partners_stat_bench needs the GPU")
    torch.cuda.set_device(0)
    ints = lambda text: [int(x) for x in text.split(",")]
    rec = {"metric": "partner statistics against the ensemble-mean partner scan, median device ms per call",
           "build_id": _lib.build_id(), "device": torch.cuda.get_device_name(0), "dtype": "f64",
           "timing": "HIP events around one call's launches; the calls of a shape alternate inside every repetition; "
                     "medians over reps after a warm-up",
           "shapes": [shape_record(a.k, a.genes, a.samples, Q, a.top, ints(a.votes), ints(a.trims), a.reps, a.warmup)
                      for Q in ints(a.queries)]}
    text = json.dumps(rec, indent=1)
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
