#!/usr/bin/env python3
"""Screen scan timings (EMEngine.screen_top, include/mmsbm.h mmsbm_screen_topn), one GPU.

    python tools/screen_bench.py [--reps 10] [--listed-reps 3] [--warmup 2] [--out profiles/screen_bench.json]

Prints (and with --out writes) one JSON record stamped with mmsbm_build_id().  At the fold0 shape
(P = 1500, K = 10), for B = 1 and the B = 8 ensemble and for Q = 64 and Q = 1024 random query pairs
with N = 100:
  * screen_top: the host wall clock of one call, ending with the Q lists on the host, and the device
    time of its launches (HIP events around screen_top_async);
  * the path it replaces, what Model.predict_third does per pair: the pair's P - 2 listed triples
    through EMEngine.predict, the slots' mean added in slot order, and a host sort under the scan's
    order (score descending, packed key ascending), query after query, ending with the same lists
    on the host.  The id rows are enumerated before the clock starts;
  * same_lists: whether the two paths return the same ordered id lists (they may differ where two
    scores lie within rounding distance: the two paths sum in different orders);
  * the ratio of the two wall clocks.
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


def listed_rows(P, pairs):
    """Per query pair, the P - 2 id rows in key order and their packed keys."""
    from trigenicinteractionpredictor_amd.scan import pack_keys, rank_of, rank_order
    order = rank_order(P)
    rank = rank_of(order)
    out = []
    for g1, g2 in pairs:
        third = np.array([g for g in range(P) if g != g1 and g != g2], dtype=np.int64)
        pos = np.sort(np.stack([np.full(third.size, rank[g1]), np.full(third.size, rank[g2]), rank[third]], axis=1),
                      axis=1)
        ids = order[pos].astype(np.int32)
        out.append((ids, pack_keys(ids, rank, P)))
    return out


def listed_path(eng, rows, N, B):
    lists = []
    for ids, keys in rows:
        probs = eng.predict(ids)
        p = probs[0]
        for b in range(1, B):
            p = p + probs[b]
        if B > 1:
            p = p / B
        top = np.lexsort((keys, -p))[:N]
        lists.append((p[top], ids[top]))
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


def shape_record(K, P, B, Q, N, reps, listed_reps, warmup):
    from trigenicinteractionpredictor_amd.engine import EMEngine
    eng = EMEngine(K, P, B=B)
    eng.upload(*params(K, P, B, 1))
    sample = None if B > 1 else 0
    rng = np.random.default_rng(4)
    pairs = np.array([rng.choice(P, 2, replace=False) for _ in range(Q)], dtype=np.int32)
    rows = listed_rows(P, pairs.tolist())
    kernel, mine = wall_ms(lambda: eng.screen_top(pairs, N, None, sample), reps, warmup)
    device = device_ms(lambda: eng.screen_top_async(pairs, N, None, sample), reps, warmup)
    listed, theirs = wall_ms(lambda: listed_path(eng, rows, N, B), listed_reps, 1)
    eng.close()
    same = all(a[1].shape == b[1].shape and bool((a[1] == b[1]).all()) for a, b in zip(mine, theirs))
    worst = max(float(np.max(np.abs(a[0] - b[0]) / np.abs(b[0]))) for a, b in zip(mine, theirs))
    rec = {"K": K, "P": P, "B": B, "Q": Q, "N": N, "scores": Q * (P - 2), "score_flop": 2.0 * K * Q * (P - 2) * B,
           "screen_top_wall": spread(kernel), "screen_top_device": spread(device), "listed_wall": spread(listed),
           "same_lists": same, "max_relative_score_difference": worst}
    rec["ratio_listed_over_screen_top"] = rec["listed_wall"]["median_ms"] / rec["screen_top_wall"]["median_ms"]
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--listed-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--top", type=int, default=100)
    ap.add_argument("--genes", type=int, default=1500)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from trigenicinteractionpredictor_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("screen_bench needs the GPU")
    torch.cuda.set_device(0)
    rec = {"metric": "screen scan against the listed-triplet path, median ms per call", "build_id": _lib.build_id(),
           "device": torch.cuda.get_device_name(0), "dtype": "f64",
           "timing": "host wall clock around calls that end with the lists on the host (device: HIP events around "
                     "one call's launches); medians over reps after a warm-up",
           "shapes": [shape_record(a.k, a.genes, B, Q, a.top, a.reps, a.listed_reps, a.warmup)
                      for B in (1, 8) for Q in (64, 1024)]}
    text = json.dumps(rec, indent=1)
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
