#!/usr/bin/env python3
"""Score census timings (EMEngine.census, include/mmsbm.h mmsbm_scan_census), one GPU.

    python tools/census_bench.py [--reps 10] [--warmup 2] [--out profiles/census_bench.json]

Prints (and with --out writes) one JSON record stamped with mmsbm_build_id():
  * at P = 1500, K = 10 for B = 1 and the B = 8 ensemble, and at K = 30, B = 1, each with a
    known-key table of 100,000 random triples, the median device time (HIP events around the call's
    launches, after a warm-up) of a census with
      - one threshold above every score (the pure score phase plus the per-tile ballot),
      - the 1000 scores of a scan_top(1000) list,
      - 1024 thresholds at quantiles of the score distribution (every score is binned),
    next to the scan's score-only time of the same run (MMSBM_SCAN_SELECT=0); for the first case
    also the same pair without a known-key table and the bare C call on resident tensors;
  * Model.heldout_ranks on a synthetic fold of 96,000 train and 24,000 test links at P = 1500,
    K = 10, B = 1, end to end on the host clock (24 census calls of at most 1024 thresholds);
  * at P = 300, K = 10 the listed path to the same counts (EMEngine.predict over all C(300, 3) rows
    plus a host sort and searchsorted) against one census of 1000 thresholds, host clock.
Parameters are random normalised theta / p from a seeded generator.
"""
from __future__ import annotations

import argparse
import itertools
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))

from scan_bench import params, random_known, resident  # noqa: E402


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
    return {"median_ms": statistics.median(out), "min_ms": min(out), "max_ms": max(out), "reps": reps}


def quantile_thresholds(eng, P, sample, n, seed):
    """n thresholds at evenly spaced quantiles of the scores of 200,000 random triples."""
    from trigenicinteractionpredictor_amd.scan import rank_order
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.integers(0, P, (220000, 3)), axis=1)
    pos = pos[(pos[:, 0] < pos[:, 1]) & (pos[:, 1] < pos[:, 2])][:200000]
    probs = eng.predict(rank_order(P)[pos].astype(np.int32))
    s = probs[0] if sample is not None else probs.mean(axis=0)
    return np.quantile(s, (np.arange(n) + 0.5) / n)


def shape_record(K, P, B, n_known, reps, warmup):
    from trigenicinteractionpredictor_amd.engine import EMEngine
    eng = EMEngine(K, P, B=B)
    eng.upload(*params(K, P, B, 1))
    known = random_known(P, n_known, 2)
    sample = None if B > 1 else 0
    triples = P * (P - 1) * (P - 2) // 6
    rec = {"K": K, "P": P, "B": B, "known_keys": int(known.size), "triples": triples}
    os.environ["MMSBM_SCAN_SELECT"] = "0"
    rec["scan_score_only"] = device_ms(lambda: eng.scan_top_async(1000, known, sample), reps, warmup)
    os.environ["MMSBM_SCAN_SELECT"] = "1"
    top, _ = eng.scan_top(1000, known, sample)
    cases = (("one_threshold_above_all", np.array([2.0])), ("scan_top_1000_scores", top),
             ("quantiles_1024", quantile_thresholds(eng, P, sample, 1024, 4)))
    base = rec["scan_score_only"]["median_ms"]
    for label, thresholds in cases:
        r = device_ms(lambda: eng.census_async(thresholds, known, sample), reps, warmup)
        counts, total = eng.census(thresholds, known, sample)
        r["ratio_over_scan_score_only"] = r["median_ms"] / base
        r["thresholds"] = int(thresholds.size)
        r["count_max"], r["count_min"], r["total"] = int(counts.max()), int(counts.min()), total
        rec[label] = r
    # where the single-threshold call's time goes: the same pair without a known-key table, and
    # the bare C call on resident tensors (no upload of keys or thresholds, no unsort of the counts)
    os.environ["MMSBM_SCAN_SELECT"] = "0"
    rec["no_known_keys"] = {"scan_score_only": device_ms(lambda: eng.scan_top_async(1000, None, sample), reps, warmup)}
    os.environ["MMSBM_SCAN_SELECT"] = "1"
    rec["no_known_keys"]["one_threshold_above_all"] = device_ms(
        lambda: eng.census_async(np.array([2.0]), None, sample), reps, warmup)
    rec["one_threshold_above_all"]["c_call_on_resident_tensors"] = device_ms(resident_call(eng, known, sample),
                                                                            reps, warmup)
    eng.close()
    return rec


def resident_call(eng, known, sample):
    import torch
    thr_d = torch.tensor([2.0], dtype=torch.float64, device=eng.device)
    out = torch.empty(2, dtype=torch.int64, device=eng.device)
    return resident(eng, known, sample)("census", (1,), (thr_d, 1), (out,))


def heldout_record(K, P, n_train, n_test, reps):
    """Model.heldout_ranks end to end on a synthetic fold (host clock; the first call, which builds
    the engine, is not counted)."""
    import torch
    from trigenicinteractionpredictor_amd import Model
    import random
    rng = np.random.default_rng(6)
    t = np.sort(rng.integers(0, P, (2 * (n_train + n_test), 3)), axis=1)
    t = np.unique(t[(t[:, 0] < t[:, 1]) & (t[:, 1] < t[:, 2])], axis=0)
    t = t[rng.permutation(t.shape[0])[:n_train + n_test]]
    with tempfile.TemporaryDirectory() as d:
        paths = []
        for name, rows in (("train.dat", t[:n_train]), ("test.dat", t[n_train:])):
            paths.append(os.path.join(d, name))
            with open(paths[-1], "w", encoding="utf-8") as f:
                for i, (a, b, c) in enumerate(rows):
                    f.write("g%d_g%d_g%d\t%d\n" % (a, b, c, i % 2))
        m = Model()
        m.get_traintest(*paths)
    random.seed(1)
    m.initialize_parameters(K)
    rows = m.heldout_ranks()
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows = m.heldout_ranks()
        times.append(time.perf_counter() - t0)
    return {"K": K, "P": m.P, "B": 1, "train_links": n_train, "test_links": len(rows),
            "census_calls": -(-len(rows) // 1024), "end_to_end_ms": statistics.median(times) * 1e3,
            "min_ms": min(times) * 1e3, "max_ms": max(times) * 1e3, "reps": reps,
            "best_rank": rows[0][0], "worst_rank": rows[-1][0]}


def listed_comparison(K, P, M, reps, warmup):
    """The way to these counts without the census: predict every row, sort, searchsorted."""
    import torch
    from trigenicinteractionpredictor_amd.engine import EMEngine
    from trigenicinteractionpredictor_amd.scan import rank_order
    eng = EMEngine(K, P, B=1)
    eng.upload(*params(K, P, 1, 3))
    ids = rank_order(P)[np.array(list(itertools.combinations(range(P), 3)), dtype=np.int32)]
    thresholds = np.sort(eng.scan_top(M, None, 0)[0])
    listed, census = [], []
    same = True
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scores = np.sort(eng.predict(ids)[0])
        want = scores.size - np.searchsorted(scores, thresholds, side="left")
        t1 = time.perf_counter()
        got, total = eng.census(thresholds, None, 0)
        t2 = time.perf_counter()
        if i >= warmup:
            listed.append(t1 - t0)
            census.append(t2 - t1)
        # the predict kernel sums in another order: a count may differ by the ties it moves
        same = same and total == scores.size and int(np.abs(got - want).max()) <= 1
    eng.close()
    lm, cm = statistics.median(listed) * 1e3, statistics.median(census) * 1e3
    return {"K": K, "P": P, "thresholds": M, "triples": int(ids.shape[0]), "listed_total_ms": lm,
            "census_ms": cm, "ratio_listed_over_census": lm / cm, "counts_agree_within_1": bool(same),
            "reps": reps}


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
        raise SystemExit("census_bench needs the GPU")
    torch.cuda.set_device(0)
    rec = {"metric": "score census, median ms per call", "build_id": _lib.build_id(),
           "device": torch.cuda.get_device_name(0), "dtype": "f64",
           "timing": "HIP events around one call's launches (uploads of the known keys and thresholds "
                     "included); medians over reps after a warm-up",
           "shapes": [shape_record(10, 1500, 1, a.known, a.reps, a.warmup),
                      shape_record(10, 1500, 8, a.known, a.reps, a.warmup),
                      shape_record(30, 1500, 1, a.known, a.reps, a.warmup)],
           "heldout_ranks": heldout_record(10, 1500, 96000, 24000, max(2, a.reps // 4)),
           "listed_vs_census": listed_comparison(10, 300, 1000, max(3, a.reps // 3), 1)}
    text = json.dumps(rec, indent=1)
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
