"""Cost of the mixed-model estimate trace (phd_trace_enable_mixed): K free-running
phd_step calls of a feature_model 2 context at the largest shape of
tests/test_gpu_mixed.py (6 particles, 300 static + 90 dynamic components, 24
measurements; capacities 512 / 192 / 1536), trace off and on, same seed and
inputs (the trace does not perturb the chain, so both runs do the same work).

    python scripts/trace_mixed_overhead.py [--steps 200] [--only on|off]

Prints one JSON line per run: wall time per step over the K steps (one
synchronisation at the end) and the update kernel's time from the context's
event pairs (phd_update_timing).  For per-kernel times run it with --only on
under `rocprofv3 --kernel-trace --stats` (no counters).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cuda-phdslam_amd"))

import phdslam  # noqa: E402
from phdslam.scenario import mixed_config, mixed_scenario  # noqa: E402


def run(traced, steps, warmup=20):
    cfg = mixed_config()
    cfg.motionType = 0
    cfg.resampleThresh = 0.5
    n = 6
    poses, sm, sof, dm, dof, z = mixed_scenario(cfg, n, 300, 90, 24, seed=991)
    f = phdslam.PHDFilter(n, cfg, map_capacity=512, max_measurements=32, candidate_capacity=1536,
                          survivor_capacity=256)
    f.set_seed(77)
    f.enable_dynamic(192)
    f.set_check_each_update(False)
    f.load(poses, np.full(n, -np.log(n), np.float32), sm, sof)
    f.load_dynamic(dm, dof)
    f.set_measurements(z)
    if traced:
        f.enable_trace_mixed(steps + warmup, 64, 192)
    f.enable_timing(steps + warmup)
    for k in range(warmup):
        f.step(None, do_predict=k > 0, step=k, readback=False)
    f.synchronize()
    f.update_timing()
    t0 = time.perf_counter()
    for k in range(warmup, warmup + steps):
        f.step(None, do_predict=True, step=k, readback=False)
    f.synchronize()
    wall = time.perf_counter() - t0
    ms, cnt = f.update_timing()
    out = dict(traced=traced, steps=steps, wall_us_per_step=1e6 * wall / steps,
               update_us_per_step=1e3 * ms / max(cnt, 1), status_errors=f.status_errors())
    if traced:
        drec = f.read_trace_dynamic()[0]
        out["dyn_map_size_last"] = int(drec[-1]["map_size"])
    f.close()
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--only", choices=["on", "off"])
    a = ap.parse_args()
    for traced in (False, True, False, True):
        if a.only and traced != (a.only == "on"):
            continue
        print(json.dumps(run(traced, a.steps)), flush=True)
        if a.only:
            break
