#!/usr/bin/env python3
"""Genome-wide scan timings (EMEngine.scan_top, include/mmsbm.h mmsbm_scan_topn), one GPU.

    python tools/scan_bench.py [--reps 20] [--warmup 3] [--out profiles/scan_bench.json]

Prints (and with --out writes) one JSON record stamped with mmsbm_build_id():
  * the fold0 shape (P = 1500, K = 10) at B = 1 and as the B = 8 ensemble, and K = 30, P = 1500,
    B = 1, each with N = 1000 and a known-key table of 100,000 random triples: the median device
    time of a scan (HIP events around the call's launches, after a warm-up), and the same scan with
    selection flagged out (MMSBM_SCAN_SELECT=0: the bare score phase), with the score phase's
    2 K C(P,3) B FLOP over each time against the 78.6 TFLOP/s FP64 matrix peak;
  * one comparison against the listed-triplet path: at P = 300, K = 10 (4,455,100 triples)
    EMEngine.predict over the enumerated id table plus a host sort, against scan_top (host wall
    clock, both ending with the result on the host).
Parameters are random normalised theta / p from a seeded generator (timing does not depend on
their values beyond the selection's flush count).
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

FP64_PEAK_TFLOPS = 78.6


def params(K, P, B, seed):
    rng = np.random.default_rng(seed)
    th = rng.random((B, P, K))
    th /= th.sum(axis=2, keepdims=True)
    pr = rng.random((B, K, K, K, 2))
    pr /= pr.sum(axis=4, keepdims=True)
    return th, pr


def random_known(P, n, seed):
    rng = np.random.default_rng(seed)
    t = np.sort(rng.integers(0, P, (n + n // 8, 3)), axis=1).astype(np.int64)
    t = t[(t[:, 0] < t[:, 1]) & (t[:, 1] < t[:, 2])][:n]
    return np.unique((t[:, 0] * P + t[:, 1]) * P + t[:, 2])


ENTRY = {"census": "mmsbm_scan_census", "pair_census": "mmsbm_pair_census", "scan_above": "mmsbm_scan_above",
         "scan_votes": "mmsbm_scan_votes", "scan": "mmsbm_scan_topn", "scan_quorum": "mmsbm_scan_quorum_topn",
         "scan_spread": "mmsbm_scan_spread_topn"}


def resident(eng, known, sample):
    """The bare C calls of the key-table families on resident tensors (no upload, nothing done to
    the outputs): -> bind(family, size_args, mid, outs), which gives the call as a function of no
    arguments.  size_args: what the family's workspace size asks (EMEngine.scan_workspace); mid: the
    entry's arguments between the sample and the workspace, outs: its output tensors (tensors go by
    pointer)."""
    import torch
    known_d = torch.from_numpy(known).to(eng.device)
    head = (eng.ctx, eng.scan_order.data_ptr(), known_d.data_ptr(), int(known.size), eng.theta.data_ptr(),
            eng.pr.data_ptr(), -1 if sample is None else sample)

    def bind(family, size_args, mid, outs):
        ws = eng.scan_workspace(family, *size_args)
        entry = getattr(eng.lib, ENTRY[family])
        args = (*head, *[m.data_ptr() if torch.is_tensor(m) else m for m in mid], ws.data_ptr(), ws.numel(),
                *[o.data_ptr() for o in outs])
        keep = (known_d, mid, outs)

        def call():
            assert entry(*args, eng._stream()) == 0, keep
        return call
    return bind


def device_ms(eng, N, known, sample, reps, warmup):
    import torch
    for _ in range(warmup):
        eng.scan_top_async(N, known, sample)
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.scan_top_async(N, known, sample)
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def shape_record(K, P, B, N, n_known, reps, warmup):
    from trigenicinteractionpredictor_amd.engine import EMEngine
    eng = EMEngine(K, P, B=B)
    eng.upload(*params(K, P, B, 1))
    known = random_known(P, n_known, 2)
    triples = P * (P - 1) * (P - 2) // 6
    flop = 2.0 * K * triples * B
    rec = {"K": K, "P": P, "B": B, "N": N, "known_keys": int(known.size), "triples": triples,
           "score_flop": flop}
    for label, flag in (("scan", "1"), ("score_only", "0")):
        os.environ["MMSBM_SCAN_SELECT"] = flag
        ms = device_ms(eng, N, known, None if B > 1 else 0, reps, warmup)
        med = statistics.median(ms)
        rec[label] = {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "reps": reps,
                      "score_tflops": flop / (med * 1e-3) / 1e12,
                      "share_of_fp64_peak": flop / (med * 1e-3) / 1e12 / FP64_PEAK_TFLOPS}
    os.environ["MMSBM_SCAN_SELECT"] = "1"
    rec["selection_ms"] = rec["scan"]["median_ms"] - rec["score_only"]["median_ms"]
    eng.close()
    return rec


def listed_comparison(K, P, N, reps, warmup):
    """What the listed-triplet entry point needs for the same answer, against the scan."""
    import torch
    from trigenicinteractionpredictor_amd.engine import EMEngine
    from trigenicinteractionpredictor_amd.scan import rank_order
    eng = EMEngine(K, P, B=1)
    eng.upload(*params(K, P, 1, 3))
    t0 = time.perf_counter()
    order = rank_order(P)
    ids = order[np.array(list(itertools.combinations(range(P), 3)), dtype=np.int32)]
    enum_s = time.perf_counter() - t0
    listed, scan = [], []
    top = None
    for i in range(warmup + reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        scores = eng.predict(ids)[0]
        t1 = time.perf_counter()
        top = np.argsort(-scores, kind="stable")[:N]      # rows are in packed-key order
        t2 = time.perf_counter()
        s, got = eng.scan_top(N, None, 0)
        t3 = time.perf_counter()
        if i >= warmup:
            listed.append((t1 - t0, t2 - t1))
            scan.append(t3 - t2)
    same = bool((ids[top] == got).all())
    eng.close()
    pm = statistics.median(a for a, _ in listed) * 1e3
    sm = statistics.median(b for _, b in listed) * 1e3
    tm = statistics.median(a + b for a, b in listed) * 1e3
    cm = statistics.median(scan) * 1e3
    return {"K": K, "P": P, "N": N, "triples": int(ids.shape[0]), "id_table_bytes": int(ids.nbytes),
            "enumerate_ids_s_not_counted": enum_s, "predict_ms": pm, "host_sort_ms": sm,
            "listed_total_ms": tm, "scan_top_ms": cm, "ratio_listed_over_scan": tm / cm,
            "same_id_list": same, "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--top", type=int, default=1000)
    ap.add_argument("--known", type=int, default=100000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from trigenicinteractionpredictor_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("scan_bench needs the GPU")
    torch.cuda.set_device(0)
    rec = {"metric": "genome-wide scan, median ms per call", "build_id": _lib.build_id(),
           "device": torch.cuda.get_device_name(0), "dtype": "f64", "fp64_peak_tflops": FP64_PEAK_TFLOPS,
           "timing": "HIP events around one call's launches; medians over reps after a warm-up",
           "shapes": [shape_record(10, 1500, 1, a.top, a.known, a.reps, a.warmup),
                      shape_record(10, 1500, 8, a.top, a.known, a.reps, a.warmup),
                      shape_record(30, 1500, 1, a.top, a.known, a.reps, a.warmup)],
           "listed_vs_scan": listed_comparison(10, 300, a.top, max(3, a.reps // 4), 1)}
    text = json.dumps(rec, indent=1)
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
