"""bench.py's command line: a plain run is only the headline loop (the extra legs and the CPU baseline need --full), --steps sets the
number of timed steps, and --dump-outputs writes what the timed path computed in its last step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 0x5EED0001


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "ISX_FORCE_DIST", "ISX_BENCH_CONFIGS3")}


def test_options_and_step_count_are_checked_before_any_gpu_call():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], env=_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--full" in r.stdout and "--dump-outputs" in r.stdout
    for bad in (["--steps", "0"], ["--warmup", "-1"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *bad], env=_env(), capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and r.stdout.strip() == "" and "--steps must be >= 1" in r.stderr


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(isx, tmp_path):
    """A plain N = 1 run at the default workload (5e7 rays per step): one JSON line with the headline keys and none of the --full
    legs; the dumped histogram and census are those isx.fluxmap gives for the ray indices of the last timed step."""
    steps, warmup = 3, 1
    out_dir = tmp_path / "outputs"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", str(out_dir)], env=_env(), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    out = json.loads(lines[0])
    assert out["unit"] == "Mrays/s" and out["higher_is_better"] is True and out["dtype"] == "f64" and out["steps"] == steps
    rays = out["config"]["rays_per_gpu_per_step"]
    assert rays == 50_000_000
    assert abs(out["value"] - rays / (out["ms_per_step"] * 1e3)) < 1e-6 * out["value"]
    assert "cpu_baseline" not in out
    for key in ("configs0", "configs2", "configs3", "configs4", "perpos_8p1e8", "size_sweep", "surfaces", "chord_mode"):
        assert out[key] is None, key
    assert sorted(os.listdir(out_dir)) == ["census.npy", "fluxmap.npy"]
    hist, census = np.load(out_dir / "fluxmap.npy"), np.load(out_dir / "census.npy")
    assert hist.dtype == np.float64 and census.dtype == np.float64
    first, count = isx.step_slice(warmup + steps - 1, 0, 1, rays)
    h, st = isx.fluxmap(isx.default_config(), count, SEED, first)
    assert hist.shape == h.shape and np.array_equal(hist, h.astype(np.float64))
    assert census.tolist() == [float(v) for v in (st.launched, st.exited, st.counted_below_z, st.absorbed, st.suspended,
                                                   st.bin_increments, st.wall_hits)]
    assert out["hist_sum_last_step"] == int(h.sum())
