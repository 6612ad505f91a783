"""A plain `bench.py` run on the GPU: it prints the headline without the `--full` records, and
`--dump-outputs` writes the parameters and the log-likelihood its timed iterations left, which
equal an engine run of warmup + steps iterations from the same seeded start bit for bit."""
import contextlib
import io
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, E, K, B, SEED, STEPS, WARMUP = 300, 6000, 10, 2, 3, 4, 2


def test_plain_run_dumps_what_the_timed_steps_left(tmp_path):
    import torch

    import bench
    from trigenicinteractionpredictor_amd import EMEngine, Model
    from trigenicinteractionpredictor_amd.restarts import family_for_batch, fixed_run, init_samples
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    out = str(tmp_path / "dump")
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(STEPS),
                        "--warmup", str(WARMUP), "--P", str(P), "--E", str(E), "--K", str(K), "--samples",
                        str(B), "--seed", str(SEED), "--dump-outputs", out], cwd=REPO, env=env,
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    rec = json.loads(p.stdout.strip().splitlines()[-1])
    assert rec["steps"] == STEPS and rec["warmup"] == WARMUP and rec["full"] is False
    assert rec["ms_per_step"] > 0 and rec["value"] == pytest.approx(B * 1e3 / rec["ms_per_step"])
    assert rec["unit"] == "EM-iterations/s" and rec["higher_is_better"] is True and rec["dtype"] == "f64"
    for moved in ("roofline", "kernel_us", "cpu_baseline", "vs_cpu_baseline"):
        assert moved not in rec
    got = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    assert sorted(got) == ["loglik", "pr", "theta"]
    assert all(a.dtype == np.float64 for a in got.values())

    train, test = bench.make_fold(P, E, 0)
    with contextlib.redirect_stdout(io.StringIO()):
        host = Model()
        host.get_traintest(train, test)
    thetas, prs = init_samples(host, K, list(range(B)), SEED)
    eng = EMEngine(K, host.P, B=B, device=torch.device("cuda", 0), family=family_for_batch(B))
    eng.set_links(0, *host._link_arrays(0))
    eng.set_links(1, *host._link_arrays(1))
    L = fixed_run(eng, thetas, prs, WARMUP + STEPS)
    theta, pr = eng.download()
    for name, want in (("theta", theta), ("pr", pr), ("loglik", L)):
        assert got[name].shape == want.shape, name
        assert np.array_equal(got[name].view(np.int64), want.view(np.int64)), name
    assert rec["final_loglik"] == L[0] and np.isfinite(L).all()
