#!/usr/bin/env python3
"""Pair vote census timings (EMEngine.pair_vote_census, include/mmsbm.h mmsbm_pair_votes), one GPU.

    python tools/pair_votes_bench.py [--reps 10] [--warmup 2] [--out profiles/pair_votes_bench.json]

Prints (and with --out writes) one JSON record stamped with mmsbm_build_id(): at P = 1500, K = 10,
the B = 8 ensemble, all 8 vote levels and a known-key table of 100,000 random triples, at one
threshold near the median of the slots' scores and one near their 0.999 quantile (quantiles of the
slots' own scores of 200,000 random triples),
  (a) EMEngine.pair_vote_census_async: the median device time (HIP events around the whole call,
      after a warm-up) and the median host time to the synchronised result;
  (b) the only route to the same matrix without the call: EMEngine.consensus_async(threshold, 1),
      then a device scatter of its rows to their three pairs per level (index_add_), host time to the
      synchronised result, and whether the matrix equals (a)'s; where consensus' `limit` refuses the
      list, "refused at N rows";
  (c) for context, EMEngine.vote_census_async and the ensemble EMEngine.pair_census_async at the same
      threshold, device time, and their sum against (a).
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
sys.path.insert(0, os.path.join(REPO, "tools"))

from census_bench import device_ms  # noqa: E402
from scan_bench import params, random_known  # noqa: E402


def slot_quantiles(eng, P, qs, seed):
    """The quantiles qs of every slot's own scores of 200,000 random triples."""
    from trigenicinteractionpredictor_amd.scan import rank_order
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.integers(0, P, (220000, 3)), axis=1)
    pos = pos[(pos[:, 0] < pos[:, 1]) & (pos[:, 1] < pos[:, 2])][:200000]
    probs = eng.predict(rank_order(P)[pos].astype(np.int32))[:eng.active]
    return [float(q) for q in np.quantile(probs.reshape(-1), qs)]


def host_ms(call, reps, warmup):
    """Median host time of call() to its synchronised end; -> (record, the last result)."""
    import torch
    out, last = [], None
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        last = call()
        torch.cuda.synchronize()
        if i >= warmup:
            out.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out), "reps": reps}, last


def listed_route(eng, t, known, levels):
    """consensus_async(t, 1), then its rows scattered to their three pairs per level: the matrix of
    pair_vote_census_async(t, levels, known)."""
    import torch
    P = eng.P
    votes, _, ids = eng.consensus_async(t, 1, known)
    ids = ids.to(torch.int64)
    mat = torch.zeros((len(levels), P * P), dtype=torch.int32, device=eng.device)
    for m, level in enumerate(levels):
        rows = ids[votes >= level]
        one = torch.ones(rows.shape[0], dtype=torch.int32, device=eng.device)
        for x, y in ((0, 1), (0, 2), (1, 2)):
            mat[m].index_add_(0, rows[:, x] * P + rows[:, y], one)
            mat[m].index_add_(0, rows[:, y] * P + rows[:, x], one)
    return mat.view(len(levels), P, P).permute(1, 2, 0).contiguous()


def threshold_record(eng, label, t, known, levels, reps, warmup):
    import torch
    from trigenicinteractionpredictor_amd.scan import LimitError
    rec = {"label": label, "threshold": t}
    hist = eng.vote_census(t, known)
    rec["vote_histogram"] = [int(c) for c in hist]
    rec["rows_with_a_vote"] = int(hist[1:].sum())
    call = lambda: eng.pair_vote_census_async(t, levels, known)        # noqa: E731
    rec["a_pair_vote_census"] = device_ms(call, reps, warmup)
    rec["a_pair_vote_census_host"], mat = host_ms(call, reps, warmup)
    upper = torch.triu(torch.ones((eng.P, eng.P), dtype=torch.bool, device=eng.device), 1)
    sums = mat[upper].sum(dim=0, dtype=torch.int64).cpu().tolist()
    rec["pair_sums_are_3x_histogram_tail"] = sums == [3 * int(hist[v:].sum()) for v in levels]
    try:
        r = max(3, reps // 3)
        rec["b_consensus_then_scatter_host"], listed = host_ms(lambda: listed_route(eng, t, known, levels), r, 1)
        rec["b_equals_a"] = bool(torch.equal(listed, mat))
        rec["b_over_a"] = rec["b_consensus_then_scatter_host"]["median_ms"] / rec["a_pair_vote_census_host"]["median_ms"]
    except LimitError as e:
        rec["b_consensus_then_scatter_host"] = "refused at %d rows (limit %d)" % (e.count, e.limit)
    thr = np.array([t])
    rec["c_vote_census"] = device_ms(lambda: eng.vote_census_async(t, known), reps, warmup)
    rec["c_pair_census_ensemble"] = device_ms(lambda: eng.pair_census_async(thr, known), reps, warmup)
    both = rec["c_vote_census"]["median_ms"] + rec["c_pair_census_ensemble"]["median_ms"]
    rec["a_over_sum_of_c"] = rec["a_pair_vote_census"]["median_ms"] / both
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
    from trigenicinteractionpredictor_amd.engine import EMEngine
    if not torch.cuda.is_available():
        raise SystemExit("pair_votes_bench needs the GPU")
    torch.cuda.set_device(0)
    K, P, B = 10, 1500, 8
    eng = EMEngine(K, P, B=B)
    eng.upload(*params(K, P, B, 1))
    known = random_known(P, a.known, 2)
    levels = list(range(1, B + 1))
    mid, high = slot_quantiles(eng, P, (0.5, 0.999), 4)
    rec = {"metric": "pair vote census, median ms per call", "build_id": _lib.build_id(),
           "device": torch.cuda.get_device_name(0), "dtype": "f64",
           "timing": "device: HIP events around one whole call (the upload of the known keys, the memset of the "
                     "matrix and the mapping to gene ids included); host: perf_counter to the synchronised result; "
                     "medians over reps after a warm-up",
           "K": K, "P": P, "B": B, "levels": levels, "known_keys": int(known.size),
           "triples": P * (P - 1) * (P - 2) // 6,
           "thresholds": [threshold_record(eng, "median", mid, known, levels, a.reps, a.warmup),
                          threshold_record(eng, "quantile_0.999", high, known, levels, a.reps, a.warmup)]}
    eng.close()
    text = json.dumps(rec, indent=1)
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
