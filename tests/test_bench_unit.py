"""bench.py's host-side accounting (no GPU): the per-kernel work table is keyed by the labels the
engine times (EMEngine.LABELS) for every plan family, and the roofline record follows the
headline rule (SURVEY 8d credit, or the executed FLOPs where the credit exceeds the peak)."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import bench  # noqa: E402


def _labels():
    import ast
    src = open(os.path.join(REPO, "trigenicinteractionpredictor_amd", "engine.py")).read()
    tree = ast.parse(src)
    for node in ast.walk(tree):
        if isinstance(node, ast.Assign) and getattr(node.targets[0], "id", None) == "LABELS":
            return ast.literal_eval(node.value)
    raise AssertionError("EMEngine.LABELS not found")


PLAN = {"rows_stream0": 76000, "rows": 76000, "partial_rows": 3200, "partial_rows_stream0": 3200,
        "v_genes": 3000, "wg_stream0": 190, "wg_spartial": 200, "y_entries": 144000}


def test_kernel_work_keys_match_engine_labels():
    for fam, labels in _labels().items():
        work = bench.kernel_work(dict(PLAN, small_k=fam), 10, 1500, 2, 1, 72000)
        assert set(work) == set(labels), (fam, work.keys(), labels)
        assert all(f > 0 and b > 0 for f, b in work.values())


def test_roofline_headline_basis():
    plan = dict(PLAN, small_k=0)
    b2b = {"pass_a": 0.1, "gene": 0.05, "fin": 0.01}
    slow = bench.roofline_record(20, 1500, 2, 8, 72000, plan, 1e-3, b2b, "none")
    assert slow["frac_basis"].startswith("SURVEY") and slow["frac"] == slow["credited"]["frac"]
    fast = bench.roofline_record(20, 1500, 2, 8, 72000, plan, 1e-6, b2b, "none")
    assert fast["frac_basis"].startswith("executed") and fast["frac"] == fast["executed"]["frac"]
    assert fast["credited"]["frac"] > 1.0
    assert fast["dominant_kernel"]["kernel"].startswith("pass_kernel<20")


class _Runner:
    """Stands in for EMEngine.download(): a small theta and a pr over the dump's per-array share."""
    def __init__(self, n_pr):
        import numpy as np
        self.theta = np.arange(2 * 5 * 3, dtype=np.float64).reshape(2, 5, 3)
        self.pr = np.arange(n_pr, dtype=np.float64)

    def download(self):
        return self.theta, self.pr


def test_dump_outputs_whole_arrays_and_bounded_sample(tmp_path, monkeypatch):
    import numpy as np
    monkeypatch.setattr(bench, "DUMP_BUDGET", 2 * 2 ** 20 + 2 * 8 * 1000)   # 1,000 values per array
    r = _Runner(5000)
    L = np.array([-1.5, -2.5])
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), r, L, 1, 0)
    got = {f: np.load(str(tmp_path / "a" / f)) for f in sorted(os.listdir(str(tmp_path / "a")))}
    assert sorted(got) == ["loglik.npy", "pr.npy", "theta.npy"]
    assert all(a.dtype == np.float64 for a in got.values())
    np.testing.assert_array_equal(got["theta.npy"], r.theta)          # under the share: whole, shaped
    np.testing.assert_array_equal(got["loglik.npy"], L)
    pr = got["pr.npy"]                                                # over it: a fixed sorted sample
    assert pr.shape == (1000,) and np.all(np.diff(pr) > 0) and set(pr) <= set(r.pr)
    for f, a in got.items():                                          # the same from run to run
        np.testing.assert_array_equal(np.load(str(tmp_path / "b" / f)), a)
    assert sum(a.nbytes for a in got.values()) <= 64 * 2 ** 20
