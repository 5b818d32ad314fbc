"""bench.py without --full: the headline line only, and --dump-outputs writes what the timed steps computed -- the same
arrays on every run with the same arguments, equal to the model driven through the same number of update_once() calls
in this process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

STEPS, WARMUP, M, F, T, K = 3, 2, 4, 129, 512, 4


def _run_bench(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
           "--bins", str(F), "--frames", str(T), "--prewarm-ms", "20", "--dump-outputs", str(out_dir)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_plain_bench_line_and_dumped_outputs(tmp_path):
    out = _run_bench(tmp_path / "a")
    assert out["steps"] == STEPS and out["warmup"] == WARMUP and out["full"] is False
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["unit"] == "iterations/s" and out["dtype"] == "f64"
    assert out["roofline"] is None and out["roofline_b8"] is None and out["cpu_baseline"] is None
    assert not [k for k in out if k.startswith("value_") or k in ("other_configs", "config5")]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["activation.npy", "basis.npy", "demix_filter.npy", "estimation.npy"]
    dumped = {n[:-4]: np.load(tmp_path / "a" / n) for n in names}
    assert all(a.dtype == np.float64 and np.isfinite(a).all() for a in dumped.values())
    assert sum(a.nbytes for a in dumped.values()) <= 64 << 20

    # a second run with the same arguments: the same arrays, bit for bit (the pre-warm's length does not leak into them)
    _run_bench(tmp_path / "b")
    for n in names:
        assert np.array_equal(np.load(tmp_path / "b" / n), dumped[n[:-4]]), n

    # the timed path itself: WARMUP + STEPS update_once() calls from the seeded state of bench.py's model
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from audio_source_separation_amd.bss.ilrma import GaussILRMA
    dev = torch.device("cuda", 0)
    X = bench.synth_mixture(torch, dev, 1, M, F, T, seed=1000).to(torch.complex128).contiguous()
    np.random.seed(111)
    m = GaussILRMA(n_basis=K, recordable_loss=False, dtype="float64", device=dev, power_statistic="covariance")
    m.input = X
    m._reset()
    for _ in range(WARMUP + STEPS):
        m.update_once()
    Y = m._engine.demix(m._X, m._Wd)
    expect = {"demix_filter": torch.view_as_real(m._Wd), "basis": m._Td, "activation": m._Vd,
              "estimation": torch.view_as_real(Y)}
    for n, t in expect.items():
        assert np.array_equal(t.cpu().numpy(), dumped[n]), n
