"""Generate the reference fixtures above K = 10 by importing the REFERENCE implementation.

Run by hand on the build machine (the reference is mounted read-only at /root/reference and
never travels to the GPU box):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_largek_golden.py [--jobs N]   # write
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_largek_golden.py --check      # compare

tests/golden/make_golden.py and make_joint_golden.py stop at K in {1, 2, 3, 10}.  This one runs
the same two reference models on three of their committed input folds (it writes no `.dat`) at
the K where the kernels change: 11 and 12 (four gene stretches per unit), 13 (first large K), 16
and 17 (two against up to four X groups), 20, 24 and 25 (either side of BIG_K), 30 and 32
(MMSBM_MAX_K), and the joint model at 13, 20 and 32.

p has K^3 * 2 entries, 512 KiB at K = 32, so a file holds for every snapshot `it`:
theta_<it> in full, L_<it> (and LT_<it>; the joint files the one joint L_<it> and qr_<it> in full),
pr_sha_<it>, the SHA-256 of p (golden_util.pr_digest), and pr_sub_<it>, p at the flat indices
`pr_idx` (golden_util.pr_index, a rule of K alone).  Up to K = 17 it also holds pr_<last>, the
whole p of the last snapshot.  The test-set table and metrics are stored as the two older
generators store them.  The `.json` beside it holds K, seed, iters, fold, P and the link counts;
the link tables are in the input folds' own metadata.

`--check` runs everything again and compares every array with the files, byte for byte.
"""
from __future__ import annotations

import contextlib
import io
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))      # tests/: golden_util
sys.dont_write_bytecode = True

from golden_util import (GOLDEN, JOINT, LARGEK, LARGEK_JOINT, PR_FULL_MAX_K, pr_digest,  # noqa: E402
                         pr_index)

REF_SRC = "/root/reference/src"

# fold: [(K, seed, iterations at which a snapshot is taken)]
CASES = {
    "tiny": [(11, 1, [0, 1, 5]), (12, 1, [0, 1, 5, 25]), (13, 1, [0, 1, 5, 25]), (13, 2, [0, 1, 5]),
             (16, 1, [0, 1, 5]), (17, 1, [0, 1, 5]), (20, 1, [0, 1, 5, 25]), (24, 1, [0, 1, 5]),
             (25, 1, [0, 1, 5]), (30, 1, [0, 1, 5]), (32, 1, [0, 1, 5])],
    "multi": [(13, 3, [0, 1, 5]), (20, 3, [0, 1, 5]), (30, 4, [0, 1, 5])],
}
# the joint model, interaction `all`
JOINT_CASES = {
    "tiny": [(13, 1, [0, 1, 5]), (20, 1, [0, 1, 5]), (32, 1, [0, 1])],
}


def _import_reference(joint):
    if REF_SRC not in sys.path:
        sys.path.insert(0, REF_SRC)
    if not joint:
        import TrigenicInteractionPredictor as ref
        return ref
    import TrigenicInteractionPredictor_23 as ref
    if not hasattr(ref.DataType, "ALL"):
        # the spec fix of make_joint_golden.py: ALL is the member the code means by `all`
        type.__setattr__(ref.DataType, "ALL", ref.DataType.all)
    return ref


def run_case(joint, fold, K, seed, iters):
    """-> (arrays of the .npz, dict of the .json)."""
    ref = _import_reference(joint)
    src = os.path.join(JOINT if joint else GOLDEN, fold)
    train, test = os.path.join(src, "train.dat"), os.path.join(src, "test.dat")
    with contextlib.redirect_stdout(io.StringIO()):
        m = ref.Model()
        (m.get_train_test if joint else m.get_traintest)(train, test)
    random.seed(seed)
    if joint:
        m.initialize_parameters(K, ref.DataType.all)
    else:
        m.initialize_parameters(K)
    idx = pr_index(K)
    out = {"pr_idx": idx}
    done = 0
    for it in iters:
        while done < it:
            m.make_iteration()
            done += 1
        pr = np.array(m.pr, dtype=np.float64)
        assert pr.shape == (K, K, K, 2)
        out["theta_%d" % it] = np.array(m.theta, dtype=np.float64)
        out["pr_sha_%d" % it] = pr_digest(pr)
        out["pr_sub_%d" % it] = pr.reshape(-1)[idx]
        if joint:
            out["qr_%d" % it] = np.array(m.qr, dtype=np.float64)
            out["L_%d" % it] = np.float64(m.compute_likelihood())
        else:
            out["L_%d" % it] = np.float64(m.compute_likelihood("train"))
            out["LT_%d" % it] = np.float64(m.compute_likelihood("test"))
    if K <= PR_FULL_MAX_K:
        out["pr_%d" % iters[-1]] = pr
    m.calculate_test_set_results()
    out["pred"] = np.array([row[0] for row in m.results], dtype=np.float64)
    out["pred_key"] = np.array([row[1] for row in m.results])
    out["pred_real"] = np.array([row[2] for row in m.results], dtype=np.int64)
    try:
        out["metrics"] = np.array(m.calculate_metrics(), dtype=np.float64)
    except ZeroDivisionError:
        out["metrics"] = np.array([np.nan] * 4)
    meta = {"K": K, "seed": seed, "iters": iters, "fold": ("joint/" if joint else "") + fold,
            "P": m.P, "n_links": len(m.links), "n_test_links": len(m.test_links)}
    if joint:
        meta.update(interaction="all", n_dlinks=len(m.dlinks), n_dtest_links=len(m.dtest_links))
    return out, meta


def all_cases():
    """(joint, fold, K, seed, iters) of every file, the slowest first."""
    runs = [(False, fold, *c) for fold, cs in CASES.items() for c in cs]
    runs += [(True, fold, *c) for fold, cs in JOINT_CASES.items() for c in cs]
    return sorted(runs, key=lambda r: -(r[2] ** 3) * max(r[4][-1], 1))


def paths(joint, fold, K, seed):
    stem = os.path.join(LARGEK_JOINT if joint else LARGEK, fold, "K%d_s%d" % (K, seed))
    return stem + ".npz", stem + ".json"


def _do(job):
    check, run = job
    joint, fold, K, seed, iters = run
    out, meta = run_case(*run)
    npz, js = paths(joint, fold, K, seed)
    if check:
        with open(js, encoding="utf-8") as f:
            assert json.load(f) == meta, js
        got = np.load(npz, allow_pickle=False)
        assert sorted(got.files) == sorted(out), npz
        for key, want in out.items():
            want = np.asarray(want)
            assert got[key].dtype == want.dtype and got[key].shape == want.shape, (npz, key)
            assert got[key].tobytes() == want.tobytes(), (npz, key)
        return "%s: reproduced" % npz
    os.makedirs(os.path.dirname(npz), exist_ok=True)
    np.savez_compressed(npz, **out)
    with open(js, "w", encoding="utf-8") as f:
        json.dump(meta, f)
    return "%s: L_final=%r, %d bytes" % (npz, float(out["L_%d" % iters[-1]]), os.path.getsize(npz))


def main():
    check = "--check" in sys.argv
    jobs = int(sys.argv[sys.argv.index("--jobs") + 1]) if "--jobs" in sys.argv else 1
    work = [(check, run) for run in all_cases()]
    if jobs > 1:
        import multiprocessing
        with multiprocessing.get_context("spawn").Pool(jobs) as pool:
            for line in pool.imap_unordered(_do, work):
                print("  " + line, flush=True)
    else:
        for job in work:
            print("  " + _do(job), flush=True)


if __name__ == "__main__":
    main()
