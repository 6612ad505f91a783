#!/usr/bin/env python3
"""Partner scan timings (EMEngine.partners_top, include/mmsbm.h mmsbm_partners_topn), one GPU.

    python tools/partners_bench.py [--reps 20] [--warmup 3] [--out profiles/partners_bench.json]

Prints (and with --out writes) one JSON record stamped with mmsbm_build_id():
  * the fold0 shape (P = 1500, K = 10) at B = 1 and as the B = 8 ensemble, and K = 30, P = 1500,
    B = 1, each for Q = 1, Q = 32 and Q = P queries with N = 100 and the partner pairs of 100,000
    random known triples: the median device time of a call (HIP events around the call's launches,
    after a warm-up), and the same call with selection flagged out (MMSBM_PARTNERS_SELECT=0: the
    bare score phase), with the score phase's 2 K Q (P-1)(P-2)/2 B FLOP over each time against the
    78.6 TFLOP/s FP64 matrix peak (Q = P: 2 K 3 C(P,3) B);
  * for Q = P, the genome-wide scan's score-only time at the same shape (MMSBM_SCAN_SELECT=0; a
    third of the partner scan's scores) and the ratio of the two score-only times;
  * for Q = 1 at each single-sample shape, the listed-triplet path to the same list: the gene's
    enumerated (P-1)(P-2)/2 id rows through EMEngine.predict plus a host sort under the same order,
    against partners_top (host wall clock, both ending with the list on the host).
Parameters are random normalised theta / p from a seeded generator (timing does not depend on
their values beyond the selection's flush count).
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

FP64_PEAK_TFLOPS = 78.6


def params(K, P, B, seed):
    rng = np.random.default_rng(seed)
    th = rng.random((B, P, K))
    th /= th.sum(axis=2, keepdims=True)
    pr = rng.random((B, K, K, K, 2))
    pr /= pr.sum(axis=4, keepdims=True)
    return th, pr


def random_known_ids(P, n, seed):
    """n random triples of distinct genes as gene ids in key order."""
    from trigenicinteractionpredictor_amd.scan import rank_order
    rng = np.random.default_rng(seed)
    t = np.sort(rng.integers(0, P, (n + n // 8, 3)), axis=1).astype(np.int64)
    t = t[(t[:, 0] < t[:, 1]) & (t[:, 1] < t[:, 2])][:n]
    return rank_order(P)[t]


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


def stats(ms, flop):
    med = statistics.median(ms)
    return {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "reps": len(ms),
            "score_tflops": flop / (med * 1e-3) / 1e12,
            "share_of_fp64_peak": flop / (med * 1e-3) / 1e12 / FP64_PEAK_TFLOPS}


def shape_record(K, P, B, N, n_known, reps, warmup):
    from trigenicinteractionpredictor_amd.engine import EMEngine
    from trigenicinteractionpredictor_amd.scan import known_keys, partner_known
    eng = EMEngine(K, P, B=B)
    eng.upload(*params(K, P, B, 1))
    ids = random_known_ids(P, n_known, 2)
    sample = None if B > 1 else 0
    pairs_per_query = (P - 1) * (P - 2) // 2
    rec = {"K": K, "P": P, "B": B, "N": N, "known_triples": int(ids.shape[0]), "queries": []}
    rng = np.random.default_rng(4)
    for Q in (1, 32, P):
        queries = list(range(P)) if Q == P else rng.choice(P, Q, replace=False).tolist()
        known = partner_known((P, ids, None), queries)
        flop = 2.0 * K * Q * pairs_per_query * B
        r = {"Q": Q, "scores": Q * pairs_per_query, "known_pairs": int(known[1].size), "score_flop": flop}
        for label, flag in (("partners", "1"), ("score_only", "0")):
            os.environ["MMSBM_PARTNERS_SELECT"] = flag
            r[label] = stats(device_ms(lambda: eng.partners_top_async(queries, N, known, sample), reps, warmup),
                             flop)
        os.environ["MMSBM_PARTNERS_SELECT"] = "1"
        r["selection_ms"] = r["partners"]["median_ms"] - r["score_only"]["median_ms"]
        rec["queries"].append(r)
    # the genome-wide scan's bare score phase at the same shape: C(P,3) scores, a third of Q = P's
    triples = P * (P - 1) * (P - 2) // 6
    os.environ["MMSBM_SCAN_SELECT"] = "0"
    scan_known = known_keys((P, ids, None))
    rec["scan_score_only"] = stats(device_ms(lambda: eng.scan_top_async(N, scan_known, sample), reps, warmup),
                                   2.0 * K * triples * B)
    os.environ["MMSBM_SCAN_SELECT"] = "1"
    rec["ratio_partners_over_scan_score_only"] = (rec["queries"][-1]["score_only"]["median_ms"] /
                                                  rec["scan_score_only"]["median_ms"])
    eng.close()
    return rec


def listed_comparison(K, P, N, reps, warmup):
    """What the listed-triplet entry point needs for one gene's list, against partners_top."""
    import torch
    from trigenicinteractionpredictor_amd.engine import EMEngine
    from trigenicinteractionpredictor_amd.scan import pack_keys, rank_of, rank_order
    eng = EMEngine(K, P, B=1)
    eng.upload(*params(K, P, 1, 3))
    order = rank_order(P)
    rank = rank_of(order)
    g = P // 3
    t0 = time.perf_counter()
    q = int(rank[g])
    b, c = np.triu_indices(P, k=1)
    keep = (b != q) & (c != q)
    pos = np.sort(np.stack([np.full(keep.sum(), q), b[keep], c[keep]], axis=1), axis=1)
    ids = order[pos].astype(np.int32)
    keys = pack_keys(ids, rank, P)
    enum_s = time.perf_counter() - t0
    listed, mine = [], []
    top = got = None
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scores = eng.predict(ids)[0]
        t1 = time.perf_counter()
        top = np.lexsort((keys, -scores))[:N]
        t2 = time.perf_counter()
        ((_, got),) = eng.partners_top([g], N, None, 0)
        t3 = time.perf_counter()
        if i >= warmup:
            listed.append((t1 - t0, t2 - t1))
            mine.append(t3 - t2)
    same = bool((ids[top] == got).all())
    eng.close()
    pm = statistics.median(a for a, _ in listed) * 1e3
    sm = statistics.median(b for _, b in listed) * 1e3
    tm = statistics.median(a + b for a, b in listed) * 1e3
    cm = statistics.median(mine) * 1e3
    return {"K": K, "P": P, "N": N, "rows": int(ids.shape[0]), "id_table_bytes": int(ids.nbytes),
            "enumerate_ids_s_not_counted": enum_s, "predict_ms": pm, "host_sort_ms": sm,
            "listed_total_ms": tm, "partners_top_ms": cm, "ratio_listed_over_partners": tm / cm,
            "same_id_list": same, "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--top", type=int, default=100)
    ap.add_argument("--known", type=int, default=100000)
    ap.add_argument("--genes", type=int, default=1500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from trigenicinteractionpredictor_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("partners_bench needs the GPU")
    torch.cuda.set_device(0)
    P = a.genes
    rec = {"metric": "partner scan, median ms per call", "build_id": _lib.build_id(),
           "device": torch.cuda.get_device_name(0), "dtype": "f64", "fp64_peak_tflops": FP64_PEAK_TFLOPS,
           "timing": "HIP events around one call's launches; medians over reps after a warm-up",
           "shapes": [shape_record(10, P, 1, a.top, a.known, a.reps, a.warmup),
                      shape_record(10, P, 8, a.top, a.known, a.reps, a.warmup),
                      shape_record(30, P, 1, a.top, a.known, a.reps, a.warmup)],
           "listed_vs_partners": [listed_comparison(10, P, a.top, a.reps, a.warmup),
                                  listed_comparison(30, P, a.top, a.reps, a.warmup)]}
    text = json.dumps(rec, indent=1)
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
