#!/usr/bin/env python3
"""Pair-masked top-N scan and partner scan timings (include/mmsbm.h mmsbm_scan_topn_masked,
mmsbm_partners_topn_masked), one GPU.

    python tools/scan_topn_masked_bench.py [--reps 10] [--warmup 2] [--out profiles/scan_topn_masked_bench.json]

Prints (and with --out writes) one JSON record stamped with mmsbm_build_id(): for K = 10 at B = 1 and
B = 8 and K = 30 at B = 3, all at P = 1500 without a key table, under the three masks of
tools/scan_masked_bench.py ((i) all zero, (ii) 10 % of the pairs at random, (iii) 300 allowed genes),
  * mmsbm_scan_topn_masked at N = 1000 next to mmsbm_scan_topn of the same build: the median device
    time (HIP events around the whole bare C call on resident tensors, after a warm-up, the calls of
    a case taking turns inside every repetition), each masked call's ratio over the unmasked one and
    the unmasked call's own min-max spread;
  * on the host clock, EMEngine.scan_top(1000, mask=(ii)) next to the route it replaces, restated
    here (masked censuses bracket the cut from 1.0, the masked threshold scan lists above it, the
    host sorts and cuts), and next to the unmasked EMEngine.scan_top(1000); the two masked lists
    must be the same bytes;
  * mmsbm_partners_topn_masked at N = 100 next to mmsbm_partners_topn under (i) and (iii), for one
    query (an allowed gene: Q = 1, the query spread over the device) and for every gene (Q = P).
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

from scan_bench import params  # noqa: E402
from scan_masked_bench import masks  # noqa: E402
from scan_votes_bench import host_ms, taking_turns_ms  # noqa: E402


def ratios(c):
    base = c["unmasked"]
    c["unmasked_spread_ms"] = base["max_ms"] - base["min_ms"]
    for label, v in c.items():
        if label.startswith("masked_"):
            v["over_unmasked_median"] = v["median_ms"] / base["median_ms"]
    return c


def census_route(eng, n, sample, mask):
    """EMEngine.scan_top_any(n, mask=) as it was before the masked top-N kernel."""
    from trigenicinteractionpredictor_amd.scan import bracket_threshold
    lo = bracket_threshold(n, 1.0, lambda t: eng.census(t, None, sample, mask=mask)[0])
    scores, ids = eng.scan_above(lo, None, sample, mask=mask)
    return scores[:n], ids[:n]


def shape_record(K, P, B, reps, warmup):
    import torch
    from trigenicinteractionpredictor_amd.engine import EMEngine
    eng = EMEngine(K, P, B=B)
    eng.upload(*params(K, P, B, 1))
    sample = 0 if B == 1 else None
    rec = {"K": K, "P": P, "B": B, "triples": P * (P - 1) * (P - 2) // 6}
    host = masks(P, 7)
    dev = {label: torch.from_numpy(m.view(np.int32)).to(eng.device) for label, m in host.items()}
    tail = (eng.theta.data_ptr(), eng.pr.data_ptr(), -1 if sample is None else sample)
    keep = []

    def empty(shape, dtype):
        keep.append(torch.empty(shape, dtype=dtype, device=eng.device))
        return keep[-1]

    # the genome-wide scan, N = 1000
    N = 1000
    ws = eng.scan_workspace("scan", N)
    outs = [empty(N, torch.float64), empty((N, 3), torch.int32), empty(1, torch.int64)]

    def bind_scan(label):
        entry = eng.lib.mmsbm_scan_topn_masked if label else eng.lib.mmsbm_scan_topn
        args = (eng.ctx, eng.scan_order.data_ptr(), None, 0, *((dev[label].data_ptr(),) if label else ()), *tail, N,
                ws.data_ptr(), ws.numel(), *[o.data_ptr() for o in outs])

        def call():
            assert entry(*args, eng._stream()) == 0
        return call

    calls = {"unmasked": bind_scan(None)}
    for label in host:
        calls["masked_" + label] = bind_scan(label)
    rec["scan_top_1000"] = ratios(taking_turns_ms(calls, reps, warmup))
    n_host = max(3, reps // 3)
    top_ms, (s0, _) = host_ms(lambda: eng.scan_top(N, None, sample), n_host)
    new_ms, (s1, i1) = host_ms(lambda: eng.scan_top(N, None, sample, mask=host["random_10pct"]), n_host)
    old_ms, (s2, i2) = host_ms(lambda: census_route(eng, N, sample, host["random_10pct"]), n_host)
    assert s1.tobytes() == s2.tobytes() and i1.tobytes() == i2.tobytes()
    rec["top_1000_host_clock"] = {"scan_top_unmasked_ms": top_ms, "scan_top_masked_random_10pct_ms": new_ms,
                                  "census_route_masked_random_10pct_ms": old_ms, "same_list": True,
                                  "rows": [int(s0.size), int(s1.size), int(s2.size)]}

    # the partner scan, N = 100
    N = 100
    from trigenicinteractionpredictor_amd.scan import rank_order
    # a query inside the allowed universe: the gene whose mask row blocks the fewest pairs
    blocked_per_row = np.unpackbits(np.ascontiguousarray(host["allowed_300"][:P]).view(np.uint8), axis=1).sum(axis=1)
    q_allowed = int(rank_order(P)[int(np.argmin(blocked_per_row))])
    for label_q, queries in (("Q1", np.array([q_allowed], dtype=np.int32)), ("QP", np.arange(P, dtype=np.int32))):
        Q = int(queries.size)
        wsp = eng.scan_workspace("partners", Q, N)
        pouts = [empty((Q, N), torch.float64), empty((Q, N, 3), torch.int32), empty(Q, torch.int64)]
        keep.append(queries)

        def bind_part(label, queries=queries, Q=Q, wsp=wsp, pouts=pouts):
            entry = eng.lib.mmsbm_partners_topn_masked if label else eng.lib.mmsbm_partners_topn
            args = (eng.ctx, eng.scan_order.data_ptr(), queries.ctypes.data, Q, None, None,
                    *((dev[label].data_ptr(),) if label else ()), *tail, N, wsp.data_ptr(), wsp.numel(),
                    *[o.data_ptr() for o in pouts])

            def call():
                assert entry(*args, eng._stream()) == 0
            return call

        calls = {"unmasked": bind_part(None), "masked_zero": bind_part("zero"),
                 "masked_allowed_300": bind_part("allowed_300")}
        c = ratios(taking_turns_ms(calls, reps, warmup))
        torch.cuda.synchronize()
        c["rows_under_allowed_300"] = int(pouts[2].sum().cpu())
        rec["partners_top_100_" + label_q] = c
    eng.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    from trigenicinteractionpredictor_amd import _lib
    if not torch.cuda.is_available():
        raise SystemExit("scan_topn_masked_bench needs the GPU")
    torch.cuda.set_device(0)
    shapes = [shape_record(K, 1500, B, a.reps, a.warmup) for K, B in ((10, 1), (10, 8), (30, 3))]
    rec = {"metric": "pair-masked top-N scan and partner scan, median ms per call", "build_id": _lib.build_id(),
           "device": torch.cuda.get_device_name(0), "dtype": "f64",
           "timing": "HIP events around one whole bare C call on resident tensors; the calls of one case take "
                     "turns inside every repetition; medians over reps after a warm-up; *_host_clock: "
                     "perf_counter around the EMEngine call, synchronised, median after one warm-up call",
           "shapes": shapes}
    print(json.dumps(rec), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
