#!/usr/bin/env python3
"""Screen statistics timings (EMEngine.screen_quorum_top / screen_spread_top, include/mmsbm.h
mmsbm_screen_stat_topn), one GPU.

    python tools/screen_stat_bench.py [--reps 10] [--host-reps 3] [--warmup 2] [--out profiles/screen_stat_bench.json]

Prints (and with --out writes) one JSON record stamped with mmsbm_build_id().  At the shapes of
tools/screen_bench.py (P = 1500, K = 10, N = 100, the B = 8 ensemble, Q = 64 and Q = 1024 random
query pairs):
  * screen_quorum_top at m = 5 and screen_spread_top at t = 0: the host wall clock of one call, ending
    with the Q lists on the host, and the device time of its launches (HIP events around the _async
    form);
  * screen_top over the ensemble mean, the same two clocks: the yardstick, the call whose MFMA chains
    a stat call repeats;
  * the route the stat calls replace: B calls of screen_scores(sample=s), each ending with f64[Q][P]
    on the host, numpy's partition (quorum) or max - min (spread) over the slots, and per query a host
    lexsort under the scan's order (value descending, packed key ascending), ending with the same
    lists on the host.  The keys are formed before the clock starts;
  * same_lists: whether the two routes return identical ordered id lists and score words (they
    must: a stat value is a slot's own word, or one subtraction of two);
  * the ratios of the wall clocks.
Parameters are random normalised theta / p from a seeded generator.
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def params(K, P, B, seed):
    rng = np.random.default_rng(seed)
    th = rng.random((B, P, K))
    th /= th.sum(axis=2, keepdims=True)
    pr = rng.random((B, K, K, K, 2))
    pr /= pr.sum(axis=4, keepdims=True)
    return th, pr


def query_keys(P, pairs):
    """-> (order, keys int64[Q][P]): per query pair the packed key of {x, y, c} sorted, for every
    rank position c (meaningless at x and y, which the rows mark NaN)."""
    from trigenicinteractionpredictor_amd.scan import rank_of, rank_order
    order = rank_order(P)
    rank = rank_of(order)
    c = np.arange(P, dtype=np.int64)
    keys = np.empty((len(pairs), P), dtype=np.int64)
    for i, (g1, g2) in enumerate(pairs):
        x, y = sorted((int(rank[g1]), int(rank[g2])))
        keys[i] = np.where(c < x, (c * P + x) * P + y, np.where(c < y, (x * P + c) * P + y, (x * P + y) * P + c))
    return order, keys


def host_route(eng, pairs, order, keys, N, B, stat, arg):
    """Today's route to a stat list: every slot's rows to the host, the statistic and the sort there."""
    P = eng.P
    rows = np.stack([eng.screen_scores(pairs, sample=s) for s in range(B)])[:, :, order]   # [B][Q][rank position]
    if stat == "quorum":
        value = np.partition(rows, B - arg, axis=0)[B - arg]        # the arg-th largest of B
    else:
        s = np.sort(rows, axis=0)
        value = s[B - 1 - arg] - s[arg]
    lists = []
    for i in range(len(pairs)):
        at = np.flatnonzero(~np.isnan(value[i]))
        k = keys[i, at]
        top = np.lexsort((k, -value[i, at]))[:N]
        kk = k[top]
        ids = np.stack([order[kk // (P * P)], order[(kk // P) % P], order[kk % P]], axis=1).astype(np.int32)
        lists.append((value[i, at][top], ids))
    return lists


def device_ms(call, reps, warmup):
    import torch
    for _ in range(warmup):
        call()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def wall_ms(call, reps, warmup):
    import torch
    out, last = [], None
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last = call()
        t1 = time.perf_counter()
        if i >= warmup:
            out.append((t1 - t0) * 1e3)
    return out, last


def spread(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms)}


def identical(mine, theirs):
    return all(a[1].shape == b[1].shape and bool((a[1] == b[1]).all()) and a[0].tobytes() == b[0].tobytes()
               for a, b in zip(mine, theirs))


def shape_record(K, P, B, Q, N, votes, trim, reps, host_reps, warmup):
    from trigenicinteractionpredictor_amd.engine import EMEngine
    eng = EMEngine(K, P, B=B)
    eng.upload(*params(K, P, B, 1))
    rng = np.random.default_rng(4)
    pairs = np.array([rng.choice(P, 2, replace=False) for _ in range(Q)], dtype=np.int32)
    order, keys = query_keys(P, pairs.tolist())
    rec = {"K": K, "P": P, "B": B, "Q": Q, "N": N, "scores": Q * (P - 2), "score_flop": 2.0 * K * Q * (P - 2) * B,
           "votes": votes, "trim": trim}
    wall, _ = wall_ms(lambda: eng.screen_top(pairs, N), reps, warmup)
    rec["mean_top_wall"] = spread(wall)
    rec["mean_top_device"] = spread(device_ms(lambda: eng.screen_top_async(pairs, N), reps, warmup))
    stats = (("quorum", votes, eng.screen_quorum_top, eng.screen_quorum_top_async),
             ("spread", trim, eng.screen_spread_top, eng.screen_spread_top_async))
    mine = {}
    for name, arg, top, top_async in stats:     # every device route before the host routes churn the heap
        wall, mine[name] = wall_ms(lambda: top(pairs, N, arg), reps, warmup)
        rec[name + "_top_wall"] = spread(wall)
        rec[name + "_top_device"] = spread(device_ms(lambda: top_async(pairs, N, arg), reps, warmup))
    for name, arg, _, _ in stats:
        host, theirs = wall_ms(lambda: host_route(eng, pairs, order, keys, N, B, name, arg), host_reps, 1)
        rec[name + "_host_route_wall"] = spread(host)
        rec[name + "_same_lists"] = identical(mine[name], theirs)
        rec[name + "_ratio_host_route_over_stat_top"] = \
            rec[name + "_host_route_wall"]["median_ms"] / rec[name + "_top_wall"]["median_ms"]
        rec[name + "_device_ratio_stat_over_mean"] = \
            rec[name + "_top_device"]["median_ms"] / rec["mean_top_device"]["median_ms"]
    eng.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--top", type=int, default=100)
    ap.add_argument("--genes", type=int, default=1500)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--votes", type=int, default=5)
    ap.add_argument("--trim", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from trigenicinteractionpredictor_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("screen_stat_bench needs the GPU")
    torch.cuda.set_device(0)
    rec = {"metric": "screen statistics against the ensemble-mean screen scan and the per-slot host route, "
                     "median ms per call",
           "build_id": _lib.build_id(), "device": torch.cuda.get_device_name(0), "dtype": "f64",
           "timing": "host wall clock around calls that end with the lists on the host (device: HIP events around "
                     "one call's launches); medians over reps after a warm-up",
           "shapes": [shape_record(a.k, a.genes, a.samples, Q, a.top, a.votes, a.trim, a.reps, a.host_reps, a.warmup)
                      for Q in (64, 1024)]}
    text = json.dumps(rec, indent=1)
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
