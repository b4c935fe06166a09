"""bench.py's command line: a plain run measures the headline figure only,
--full adds the legs measured beside it, --dump-outputs writes the state after
the last timed step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
NAMES = ["log_weights", "map_offsets", "map_particles", "map_sizes", "maps", "poses"]


def _state(n, lo, hi, seed):
    from phdslam.types import GAUSSIAN2D, POSE
    rng = np.random.default_rng(seed)
    offs = np.zeros(n + 1, np.int32)
    offs[1:] = np.cumsum(rng.integers(lo, hi, n))
    maps = np.zeros(offs[-1], GAUSSIAN2D)
    maps["weight"] = rng.random(offs[-1])
    maps["mean"] = rng.normal(0, 30, (offs[-1], 2))
    maps["cov"] = rng.random((offs[-1], 4))
    poses = np.zeros(n, POSE)
    for k in POSE.names:
        poses[k] = rng.normal(size=n)
    return poses, rng.normal(size=n).astype(np.float32), maps, offs


def _load(d):
    assert sorted(os.listdir(d)) == [f"{k}.npy" for k in NAMES]
    return {k: np.load(os.path.join(d, f"{k}.npy")) for k in NAMES}


def _check_dump(out, poses, lw, maps, offs):
    """The dump holds every pose, log-weight and map size, and the sampled
    particles' maps exactly as the state has them."""
    assert all(a.dtype in (np.float32, np.float64) for a in out.values())
    np.testing.assert_array_equal(out["poses"], np.stack([poses[k] for k in poses.dtype.names], 1))
    np.testing.assert_array_equal(out["log_weights"], lw)
    np.testing.assert_array_equal(out["map_sizes"], np.diff(offs))
    picked, so = out["map_particles"].astype(np.int64), out["map_offsets"].astype(np.int64)
    assert len(so) == len(picked) + 1 and so[0] == 0 and so[-1] == len(out["maps"])
    assert (np.diff(picked) > 0).all()
    np.testing.assert_array_equal(np.diff(so), np.diff(offs)[picked])
    for i, p in enumerate(picked):
        g = maps[offs[p]:offs[p + 1]]
        want = np.concatenate([g["weight"][:, None], g["mean"], g["cov"]], 1)
        np.testing.assert_array_equal(out["maps"][so[i]:so[i + 1]], want)


def test_dump_outputs_whole_state(tmp_path):
    """A state within the byte budget is written whole."""
    sys.path.insert(0, REPO)
    import bench
    state = _state(37, 0, 9, 1)
    bench.dump_outputs(tmp_path / "d", state, seed=5)
    out = _load(tmp_path / "d")
    np.testing.assert_array_equal(out["map_particles"], np.arange(37))
    _check_dump(out, *state)


def test_dump_outputs_sample_is_bounded_and_fixed(tmp_path, monkeypatch):
    """Past the byte budget the maps of a sample of particles are written: as
    many as fit, the same ones for the same seed."""
    sys.path.insert(0, REPO)
    import bench
    monkeypatch.setattr(bench, "DUMP_MAP_BYTES", 40 * 28)
    state = _state(50, 1, 6, 2)
    bench.dump_outputs(tmp_path / "a", state, seed=5)
    bench.dump_outputs(tmp_path / "b", state, seed=5)
    bench.dump_outputs(tmp_path / "c", state, seed=6)
    a, b, c = _load(tmp_path / "a"), _load(tmp_path / "b"), _load(tmp_path / "c")
    for k in NAMES:
        assert a[k].tobytes() == b[k].tobytes()
    assert a["map_particles"].tolist() != c["map_particles"].tolist()
    assert 0 < len(a["maps"]) <= 40 and len(a["maps"]) + 5 > 40  # (no further particle would have fitted for sure)
    _check_dump(a, *state)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["plain", "full", "full-config2"])
def test_bench_command_line(gpu, tmp_path, kind):
    """One short run of each kind at 64 particles: the result line's headline
    fields, --steps timed steps, the dumped state of the plain run, and the
    legs that only --full measures (config 3: config 4's model, its CPHD oracle
    leg left out as too slow for a test; config 2: the CPU oracle's rate)."""
    full = kind != "plain"
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--particles", "64"]
    cmd += {"plain": ["--dump-outputs", str(tmp_path / "d")], "full": ["--full", "--no-cpu-baseline"],
            "full-config2": ["--full", "--config", "2", "--cpu-budget", "0.5"]}[kind]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, PHD_BENCH_CLOCK_WARMUP="0"))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert all(k in d for k in HEADLINE)
    assert d["steps"] == 3 and d["unit"] == "steps/s" and d["dtype"] == "f32" and d["higher_is_better"] is True
    assert d["value"] > 0 and abs(d["ms_per_step"] - 1e3 / d["value"]) <= 1e-3 * d["ms_per_step"] + 1e-4
    assert d["config"]["slow_paths"]["particle_updates"] == 3 * 64
    if full:
        assert d["roofline"]["copy_ceiling_gbs"] > 0
        if kind == "full":
            assert d["config4_model"]["filter_steps_per_s"] > 0 and d["config4_model"]["steps"] == 3
        else:
            assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["value_1thread"] > 0
    else:
        assert "cpu_baseline" not in d and "config4_model" not in d and "copy_ceiling_gbs" not in d["roofline"]
        out = _load(tmp_path / "d")
        assert out["poses"].shape == (64, 6) and out["log_weights"].shape == (64,)
        assert out["maps"].shape == (int(out["map_sizes"].sum()), 7) and len(out["maps"]) > 0
        assert all(np.isfinite(a).all() for a in out.values())
        np.testing.assert_allclose(np.exp(out["log_weights"].astype(np.float64)).sum(), 1.0, rtol=1e-4)
