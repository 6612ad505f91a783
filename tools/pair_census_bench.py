#!/usr/bin/env python3
"""Pair census timings (EMEngine.pair_census, include/mmsbm.h mmsbm_pair_census), one GPU.

    python tools/pair_census_bench.py [--reps 10] [--warmup 2] [--out profiles/pair_census_bench.json]

Prints (and with --out writes) one JSON record stamped with mmsbm_build_id():
  * at P = 1500, K = 10 for B = 1 and the B = 8 ensemble, and at K = 30, B = 1, each with a
    known-key table of 100,000 random triples, the median device time (HIP events around the whole
    call, after a warm-up) of
      - EMEngine.census_async with one threshold above every score: the yardstick of the same run;
      - EMEngine.pair_census_async with that threshold (the census's work per tile and nothing more),
        with one threshold each where about 0.1 % and about 1 % of the triples hit (the hit fractions
        are the census's own counts over its total), and with one threshold below every score (every
        eligible triple makes its three adds; the atomic adds and bytes of that call are computed on
        the host from the tile layout, known keys ignored);
      - the bare C calls of both on resident tensors (no upload, no memset of the matrix by torch,
        no mapping to gene ids) for the threshold above every score;
  * at P = 300, K = 10 the listed path to the same matrix (EMEngine.predict over all C(300, 3) rows
    plus a numpy scatter) against one pair census, host clock.
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


def dense_adds(P):
    """Atomic adds of a call whose every triple hits, at one threshold, no known keys, one wave per
    b-tile (WB = 4): (b, c) one per triple; (a, c) one per 16-row b-tile that holds a b between a
    and c; (a, b) one per row a < b < P - 1."""
    a, c = np.triu_indices(P, k=2)
    ac = int(((c - 1) // 16 - (a + 1) // 16 + 1).sum())
    return {"bc": P * (P - 1) * (P - 2) // 6, "ac": ac, "ab": (P - 1) * (P - 2) // 2}


def resident_calls(eng, known, sample):
    """The bare C calls (census, pair census) at one threshold above every score."""
    import torch
    thr_d = torch.tensor([2.0], dtype=torch.float64, device=eng.device)
    out = torch.empty(2, dtype=torch.int64, device=eng.device)
    mat = torch.empty((eng.P, eng.P, 1), dtype=torch.int32, device=eng.device)
    bind = resident(eng, known, sample)
    return bind("census", (1,), (thr_d, 1), (out,)), bind("pair_census", (1,), (thr_d, 1), (mat,))


def shape_record(K, P, B, n_known, reps, warmup):
    from trigenicinteractionpredictor_amd.engine import EMEngine
    eng = EMEngine(K, P, B=B)
    eng.upload(*params(K, P, B, 1))
    known = random_known(P, n_known, 2)
    sample = None if B > 1 else 0
    rec = {"K": K, "P": P, "B": B, "known_keys": int(known.size), "triples": P * (P - 1) * (P - 2) // 6}
    q = quantile_thresholds(eng, P, sample, 1000, 4)         # q[i]: about (999.5 - i) / 10 % score above it
    cases = (("above_all", 2.0), ("hits_0.1pct", float(q[998])), ("hits_1pct", float(q[989])), ("below_all", 1e-300))
    above = np.array([2.0])
    rec["census_above_all"] = device_ms(lambda: eng.census_async(above, known, sample), reps, warmup)
    base = rec["census_above_all"]
    for label, t in cases:
        thr = np.array([t])
        r = device_ms(lambda: eng.pair_census_async(thr, known, sample), reps, warmup)
        counts, total = eng.census(thr, known, sample)
        mat = eng.pair_census(thr, known, sample)
        r["threshold"] = t
        r["hit_fraction"] = int(counts[0]) / total
        r["sum_is_3x_census"] = bool(int(mat.sum(dtype=np.int64)) == 6 * int(counts[0]))   # both triangles
        r["ratio_over_census_above_all"] = r["median_ms"] / base["median_ms"]
        r["census_same_threshold"] = device_ms(lambda: eng.census_async(thr, known, sample), reps, warmup)
        rec[label] = r
    adds = dense_adds(P)
    rec["below_all"]["atomic_adds"] = adds
    rec["below_all"]["atomic_bytes"] = 4 * sum(adds.values())
    rec["below_all"]["atomic_gb_per_s"] = 4 * sum(adds.values()) / (rec["below_all"]["median_ms"] * 1e-3) / 1e9
    census_c, pair_c = resident_calls(eng, known, sample)
    rec["c_call_on_resident_tensors"] = {"census_above_all": device_ms(census_c, reps, warmup),
                                         "pair_census_above_all": device_ms(pair_c, reps, warmup)}
    eng.close()
    return rec


def listed_comparison(K, P, reps, warmup):
    """The way to this matrix without the pair census: predict every row, scatter on the host."""
    import torch
    from trigenicinteractionpredictor_amd.engine import EMEngine
    from trigenicinteractionpredictor_amd.scan import rank_of, rank_order
    eng = EMEngine(K, P, B=1)
    eng.upload(*params(K, P, 1, 3))
    pos = np.array(list(itertools.combinations(range(P), 3)), dtype=np.int64)
    ids = rank_order(P)[pos].astype(np.int32)
    rank = rank_of(rank_order(P))
    t = float(np.sort(eng.scan_top(1000, None, 0)[0])[0]) * (1 - 1e-6)     # about 1000 hits
    listed, pair = [], []
    diff = 0
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hit = pos[eng.predict(ids)[0] >= t]
        want = np.zeros((P, P), dtype=np.int32)
        for x, y in ((0, 1), (0, 2), (1, 2)):
            np.add.at(want, (hit[:, x], hit[:, y]), 1)
        want = (want + want.T)[rank][:, rank]
        t1 = time.perf_counter()
        got = eng.pair_census([t], None, 0)[:, :, 0]
        t2 = time.perf_counter()
        if i >= warmup:
            listed.append(t1 - t0)
            pair.append(t2 - t1)
        # the predict kernel sums in another order: a score at the threshold may move across it
        diff = max(diff, int(np.abs(got - want).sum()))
    eng.close()
    lm, pm = statistics.median(listed) * 1e3, statistics.median(pair) * 1e3
    return {"K": K, "P": P, "triples": int(ids.shape[0]), "threshold": t, "listed_total_ms": lm,
            "pair_census_ms": pm, "ratio_listed_over_pair_census": lm / pm, "entries_differing": diff, "reps": reps}


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
        raise SystemExit("pair_census_bench needs the GPU")
    torch.cuda.set_device(0)
    rec = {"metric": "pair census, median ms per call", "build_id": _lib.build_id(),
           "device": torch.cuda.get_device_name(0), "dtype": "f64",
           "timing": "HIP events around one whole call (uploads of the known keys and thresholds, the memset "
                     "of the matrix and the mapping to gene ids included); medians over reps after a warm-up",
           "shapes": [shape_record(10, 1500, 1, a.known, a.reps, a.warmup),
                      shape_record(10, 1500, 8, a.known, a.reps, a.warmup),
                      shape_record(30, 1500, 1, a.known, a.reps, a.warmup)],
           "listed_vs_pair_census": listed_comparison(10, 300, max(3, a.reps // 3), 1)}
    text = json.dumps(rec, indent=1)
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
