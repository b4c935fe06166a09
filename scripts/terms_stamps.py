"""Per-phase cycle shares of the CPHD terms launch's fast form (cphd_fast64;
diagnostic PHD_STAMPS build, `python cuda-phdslam_amd/build.py --stamps`).

    python scripts/terms_stamps.py [--config 3]
Stamps 35..39 of each particle's wave: entry, setup (logs, λ', β'), the h = 1
half (64 forward + 32 backward chain steps, four batched sums), the h = 0 half
(32 + 32 steps, four sums), the tails.  Read the shares, not the absolute time.
"""
import argparse
import ctypes
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cuda-phdslam_amd"))
os.environ.setdefault("PHDSLAM_LIB", os.path.join(REPO, "cuda-phdslam_amd", "phdslam", "libphdslam_stamps.so"))

import phdslam  # noqa: E402
from phdslam import _lib  # noqa: E402
from phdslam.scenario import bench_capacities  # noqa: E402

SLOTS = 52
PHASES = [(35, 36, "setup: logs, lambda', beta'"), (36, 37, "half h=1: 64 + 32 chain steps, 4 sums"),
          (37, 38, "half h=0: 32 + 32 chain steps, 4 sums"), (38, 39, "tails: hypothesis terms, lse, factors")]

ap = argparse.ArgumentParser()
ap.add_argument("--config", type=int, default=3)
a = ap.parse_args()
cfg, n, G, M, df = phdslam.preset(a.config)
c, poses, lw, maps, offs, z = phdslam.config_scenario(a.config, n=n, G=G, M=M)
f = phdslam.PHDFilter(n, c, **bench_capacities(a.config, G, M))
f.load(poses, lw, maps, offs)
f.set_measurements(z)
f.set_replay(True)
f.set_step_births(-1)
_lib.check(_lib.lib().phd_debug_stamps(f.handle, None, 1), "stamps")
for k in range(6):
    if f.step_births():
        f.predict_update(None, 0, do_predict=False)
    else:
        f.update()
buf = np.zeros(n * SLOTS, np.uint64)
_lib.check(_lib.lib().phd_debug_stamps(f.handle, ctypes.c_void_p(buf.ctypes.data), 0), "stamps")
st = buf.reshape(n, SLOTS).astype(np.int64)
keep = np.all(st[:, 35:40] != 0, axis=1)
if not keep.any():
    raise SystemExit("no fast-form stamps recorded (not a PHD_STAMPS build, or the general form ran)")
st = st[keep]
tot = st[:, 39] - st[:, 35]
print(f"config {a.config}: N={n} G={G} M={M}; {keep.sum()} of {n} particles on the fast form; "
      f"per-wave cycles mean {tot.mean():.0f} p50 {np.median(tot):.0f} max {tot.max()}")
for k0, k1, label in PHASES:
    d = st[:, k1] - st[:, k0]
    print(f"  {label:42s} mean {d.mean():8.0f} cyc ({100 * d.mean() / tot.mean():5.1f} %)  max {d.max():8d}")
