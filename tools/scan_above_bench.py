#!/usr/bin/env python3
"""Threshold scan timings (EMEngine.scan_above, include/mmsbm.h mmsbm_scan_above), one GPU.

    python tools/scan_above_bench.py [--reps 10] [--warmup 2] [--out profiles/scan_above_bench.json]

Prints (and with --out writes) one JSON record stamped with mmsbm_build_id():
  * for K = 10 with B = 1, the K = 10, B = 8 ensemble and K = 30 with B = 1, each with a known-key
    table of 100,000 random triples, at P = 1500 for a threshold above every score, one where about
    0.1 % and one where about 1 % of the triples hit, and at P = 600 for a threshold below every score
    (every triple a row: 3.6 10^7 rows; at P = 1500 it would be 9 GB), the median device time (HIP
    events around the whole call, after a warm-up) of
      - EMEngine.scan_above_async: the census that sizes the list, the kernel, the two sorts and
        the mapping to gene ids;
      - EMEngine.census_async at the same threshold, in the same run: the yardstick;
      - the bare C calls of both on resident tensors (no upload, no sort), the list's with
        capacity = its count, and the stored bytes (16 per row) over that time;
  * at P = 300, K = 10 the listed path to the same list (EMEngine.predict over all C(300, 3) rows
    plus a numpy filter and sort) against one scan_above, host clock.
Parameters are random normalised theta / p from a seeded generator.
"""
from __future__ import annotations

import argparse
import itertools
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from census_bench import device_ms, quantile_thresholds  # noqa: E402
from scan_bench import params, random_known, resident  # noqa: E402


def resident_calls(eng, known, sample, threshold, rows):
    """The bare C calls (census, threshold scan with capacity = rows) at one threshold."""
    import torch
    thr_d = torch.tensor([threshold], dtype=torch.float64, device=eng.device)
    out = torch.empty(2, dtype=torch.int64, device=eng.device)
    scores = torch.empty(max(rows, 1), dtype=torch.float64, device=eng.device)
    keys = torch.empty(max(rows, 1), dtype=torch.int64, device=eng.device)
    found = torch.zeros(1, dtype=torch.int64, device=eng.device)
    bind = resident(eng, known, sample)
    return (bind("census", (1,), (thr_d, 1), (out,)),
            bind("scan_above", (), (threshold, rows), (scores, keys, found)), found)


def shape_record(K, P, B, n_known, cases, reps, warmup):
    """cases: (label, threshold, or the index of the quantile of 1000 to take it from)."""
    from trigenicinteractionpredictor_amd.engine import EMEngine
    eng = EMEngine(K, P, B=B)
    eng.upload(*params(K, P, B, 1))
    known = random_known(P, n_known, 2)
    sample = None if B > 1 else 0
    rec = {"K": K, "P": P, "B": B, "known_keys": int(known.size), "triples": P * (P - 1) * (P - 2) // 6}
    q = quantile_thresholds(eng, P, sample, 1000, 4)         # q[i]: about (999.5 - i) / 10 % score above it
    for label, t in cases:
        t = float(q[t]) if isinstance(t, int) else t
        counts, total = eng.census([t], known, sample)
        rows = int(counts[0])
        r = device_ms(lambda: eng.scan_above_async(t, known, sample), reps, warmup)
        s, ids = eng.scan_above(t, known, sample)
        r.update(threshold=t, rows=rows, hit_fraction=rows / total, list_length_is_census_count=bool(s.size == rows))
        r["census_same_threshold"] = device_ms(lambda: eng.census_async([t], known, sample), reps, warmup)
        census_c, above_c, found = resident_calls(eng, known, sample, t, rows)
        c = {"census": device_ms(census_c, reps, warmup), "scan_above": device_ms(above_c, reps, warmup)}
        c["scan_above_count_is_census_count"] = bool(int(found.cpu()[0]) == rows)
        c["scan_above_over_census_median"] = c["scan_above"]["median_ms"] / c["census"]["median_ms"]
        c["scan_above_median_within_census_max"] = bool(c["scan_above"]["median_ms"] <= c["census"]["max_ms"])
        c["stored_bytes"] = 16 * rows
        c["stored_gb_per_s"] = 16 * rows / (c["scan_above"]["median_ms"] * 1e-3) / 1e9
        r["c_call_on_resident_tensors"] = c
        rec[label] = r
    eng.close()
    return rec


def listed_comparison(K, P, reps, warmup):
    """The way to this list without the threshold scan: predict every row, filter and sort on the host."""
    import torch
    from trigenicinteractionpredictor_amd.engine import EMEngine
    from trigenicinteractionpredictor_amd.scan import rank_order
    eng = EMEngine(K, P, B=1)
    eng.upload(*params(K, P, 1, 3))
    pos = np.array(list(itertools.combinations(range(P), 3)), dtype=np.int64)
    ids = rank_order(P)[pos].astype(np.int32)
    keys = (pos[:, 0] * P + pos[:, 1]) * P + pos[:, 2]
    t = float(np.sort(eng.scan_top(1000, None, 0)[0])[0]) * (1 - 1e-6)     # about 1000 hits
    listed, above = [], []
    diff = 0
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p = eng.predict(ids)[0]
        hit = np.flatnonzero(p >= t)
        hit = hit[np.lexsort((keys[hit], -p[hit]))]
        want = ids[hit]
        t1 = time.perf_counter()
        _, got = eng.scan_above(t, None, 0)
        t2 = time.perf_counter()
        if i >= warmup:
            listed.append(t1 - t0)
            above.append(t2 - t1)
        # the predict kernel sums in another order: a score at the threshold may move across it
        diff = max(diff, len(set(map(tuple, got.tolist())) ^ set(map(tuple, want.tolist()))))
    eng.close()
    lm, am = statistics.median(listed) * 1e3, statistics.median(above) * 1e3
    return {"K": K, "P": P, "triples": int(ids.shape[0]), "threshold": t, "rows": int(got.shape[0]),
            "listed_total_ms": lm, "scan_above_ms": am, "ratio_listed_over_scan_above": lm / am,
            "rows_differing": diff, "reps": reps}


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
        raise SystemExit("scan_above_bench needs the GPU")
    torch.cuda.set_device(0)
    sparse = (("above_all", 2.0), ("hits_0.1pct", 998), ("hits_1pct", 989))
    dense = (("below_all", 1e-300),)
    shapes = []
    for K, B in ((10, 1), (10, 8), (30, 1)):
        shapes.append(shape_record(K, 1500, B, a.known, sparse, a.reps, a.warmup))
        shapes.append(shape_record(K, 600, B, a.known, dense, a.reps, a.warmup))
    rec = {"metric": "threshold scan, median ms per call", "build_id": _lib.build_id(),
           "device": torch.cuda.get_device_name(0), "dtype": "f64",
           "timing": "HIP events around one whole call; scan_above_async holds the census that sizes the list, "
                     "the upload of the known keys, the kernel, two stable sorts and the mapping to gene ids; "
                     "medians over reps after a warm-up",
           "shapes": shapes,
           "listed_vs_scan_above": listed_comparison(10, 300, max(3, a.reps // 3), 1)}
    text = json.dumps(rec, indent=1)
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
