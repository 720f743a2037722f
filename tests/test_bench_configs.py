"""`python bench.py --config c1|c2|c3` print ONE JSON line each in the driver's format, with `roofline`
and `cpu_baseline` (BASELINE.json configs[0..2]; c4 = the default line, tests/test_bench_spawn.py)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
        "vs_baseline", "dtype", "data", "config")


def _line(*argv, timeout=900):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "SOIL_BENCH_GRID")}
    res = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + list(argv), cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    out = json.loads(lines[0])
    for k in KEYS:
        assert k in out, k
    assert "workload" in out["config"] and "model" not in out["config"]
    return out


def test_config1_line_runs_on_the_host():
    """configs[0] is a CPU path in the reference and here: the line exists without a GPU (its roofline
    block — the device twin of the operator — is then null)."""
    out = _line("--config", "c1", "--steps", "10", "--warmup", "1")
    assert out["value"] > 0 and out["config"]["grid"] == [256, 256] and out["unit"] == "Mcells/s"
    cb = out["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] == 1 and cb["equals_product"] is True


@pytest.mark.gpu
def test_config_lines_on_gpu(hip):
    c1 = _line("--config", "c1", "--steps", "20")
    r = c1["roofline"]
    assert r["bound"] == "hbm" and r["algorithmic_bytes_per_cell"] == 16 and r["device_equals_host_bit_for_bit"] is True
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    c2 = _line("--config", "c2", "--steps", "20", "--warmup", "3", "--cpu-size", "256")
    assert c2["config"]["grid"] == [1024, 1024] and c2["config"]["baseline_config"] == "configs[1]"
    assert c2["config"]["particle_arithmetic"].startswith("exact") and "fast_arithmetic" in c2
    assert c2["roofline"]["kernel"] == "k_erode_cells_fused" and c2["cpu_baseline"]["value"] > 0
    c3 = _line("--config", "c3", "--size", "512", "--steps", "16", "--warmup", "2")
    assert c3["config"]["K"] == 16 and c3["config"]["grid"] == [512, 512] and c3["value"] > 0
    r = c3["roofline"]
    assert r["bound"] == "hbm" and r["avg_launch_ms"] > 0 and r["algorithmic_bytes_per_cell"] > 0
    assert c3["config"]["mean_upstream_area_min_max"][0] >= 1.0        # every cell drains at least itself
    assert c3["cpu_baseline"]["cores"] == 1


def test_dump_outputs_takes_one_seeded_sample(tmp_path):
    """bench.py --dump-outputs: a grid above DUMP_CELLS is written at the same seeded cells every time,
    within 64 MB; a grid of at most DUMP_CELLS cells is written whole."""
    import numpy as np
    import bench
    H, W = 1536, 1024
    full = {k: np.random.default_rng(7).random((H, W, 2) if k in ("layers", "velocity", "debrisVelocity") else (H, W),
                                                 np.float32) for k in bench.DUMP_PLANES}
    one, again = str(tmp_path / "one"), str(tmp_path / "again")
    bench.dump_outputs(one, lambda k: full[k], H, W)
    bench.dump_outputs(again, lambda k: full[k], H, W)
    cells = np.sort(np.random.default_rng(0).choice(H * W, bench.DUMP_CELLS, replace=False))
    total = 0
    for k in bench.DUMP_PLANES:
        a = np.load(os.path.join(one, k + ".npy"))
        assert a.dtype == np.float32 and a.shape == (bench.DUMP_CELLS,) + full[k].shape[2:], (k, a.shape)
        assert np.array_equal(a, np.load(os.path.join(again, k + ".npy"))), k
        assert np.array_equal(a, full[k].reshape((H * W,) + full[k].shape[2:])[cells]), k
        total += os.path.getsize(os.path.join(one, k + ".npy"))
    assert total <= 64 * 2**20
    small = str(tmp_path / "small")
    bench.dump_outputs(small, lambda k: full[k][:512], 512, W)
    for k in bench.DUMP_PLANES:
        assert np.array_equal(np.load(os.path.join(small, k + ".npy")), full[k][:512]), k


@pytest.mark.gpu
def test_dump_outputs_of_two_runs_agree(hip, tmp_path):
    """The default line with --dump-outputs, with 2 and with 4 timed steps.  Every step of such a run computes
    from the same primed state, so the loop really ran --steps steps when the particle steps it counted are in
    the ratio 1:2, and the planes of the last step (float32, whole at 1024^2) are the same in both runs but for
    the order of the fp32 deposits."""
    import numpy as np
    runs, walked = [], []
    for k in (2, 4):
        d = str(tmp_path / str(k))
        out = _line("--size", "1024", "--steps", str(k), "--warmup", "1", "--no-cpu-baseline", "--dump-outputs", d)
        assert out["steps"] == k and out["ms_per_step"] > 0 and out["config"]["grid"] == [1024, 1024]
        assert out["config"]["step_inputs"].startswith("every step from the state one step")
        walked.append(out["particle_steps_timed"])
        runs.append({p: np.load(os.path.join(d, p + ".npy")) for p in
                     ("layers", "height", "waterHeight", "velocity", "debris", "debrisVelocity")})
    assert walked[0] > 0 and walked[1] == 2 * walked[0], walked
    a, b = runs
    for k in a:
        assert a[k].dtype == np.float32 and a[k].shape[:2] == (1024, 1024), (k, a[k].shape)
        np.testing.assert_allclose(a[k], b[k], rtol=1e-5, atol=1e-6 * np.nanmax(np.abs(a[k])), err_msg=k)
    # the terrain stays finite; the flow planes may not (the reference's NaN walkers)
    assert np.isfinite(a["layers"]).all() and np.isfinite(a["height"]).all()
    assert np.abs(a["waterHeight"][np.isfinite(a["waterHeight"])]).max() > 0
    assert np.abs(a["velocity"][np.isfinite(a["velocity"])]).max() > 0
