"""Cost of the estimate trace on the sharded step of the mixed model (DESIGN.md
§6 "Mixed model", *Trace*): the (world, n, K) = (2, 24, 4) shape of that
section's timing — mixed_scenario with 30 static and 10 dynamic components, 10
measurements, a resample every step, both ranks on one device under
phdslam.dist.LocalWorld (the collectives as device copies) — untraced and traced with snapshots (8, 16);
host wall clock around a synchronised step, 40 steps after 5, min / median /
max in ms and the bytes of one trace block, one JSON line.

    python scripts/time_trace_mixed_sharded.py
"""
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "cuda-phdslam_amd")]

import torch  # noqa: E402
import phdslam  # noqa: E402
from phdslam.dist import LocalWorld, ShardedFilter  # noqa: E402
from phdslam.scenario import mixed_config, mixed_scenario  # noqa: E402

SEED = 0x5eed


def run(world, n, K, trace, steps=40, warm=5):
    cfg = mixed_config(motionType=0, resampleThresh=1.0)
    N = world * n
    poses, sm, sof, dm, dof, z = mixed_scenario(cfg, N, 30, 10, 10)
    lw = np.full(N, -np.log(N), np.float32)
    dev = torch.device("cuda", 0)
    shards = []
    for r in range(world):
        f = phdslam.PHDFilter(n, cfg, map_capacity=128, max_measurements=32, candidate_capacity=4096,
                              survivor_capacity=256)
        f.set_seed(SEED)
        f.enable_dynamic(64)
        f.set_check_each_update(False)
        f.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        so, do = sof[r * n:(r + 1) * n + 1], dof[r * n:(r + 1) * n + 1]
        f.load(poses[r * n:(r + 1) * n], lw[r * n:(r + 1) * n], sm[so[0]:so[-1]], (so - so[0]).astype(np.int32))
        f.load_dynamic(dm[do[0]:do[-1]], (do - do[0]).astype(np.int32))
        f.set_measurements(z)
        sf = ShardedFilter(f, None, dev, world=world, rank=r, seed=SEED, block_records=K)
        if trace:
            sf.enable_trace_mixed(64, *trace)
        shards.append(sf)
    ranks = LocalWorld(shards)
    ts = []
    for k in range(1, warm + steps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        ranks.step(None, k)
        torch.cuda.synchronize()
        if k > warm:
            ts.append((time.perf_counter() - t0) * 1e3)
    ranks.flush()
    torch.cuda.synchronize()
    res = {"min_ms": round(min(ts), 4), "median_ms": round(statistics.median(ts), 4), "max_ms": round(max(ts), 4),
           "steps": steps, "resamples": shards[0].stats["resamples"]}
    if trace:
        res["block_bytes"] = shards[0].trace_block.numel()
        res["records"] = shards[0].f.trace_count()
    for sf in shards:
        sf.f.close()
    return res


if __name__ == "__main__":
    out = {"shape": [2, 24, 4], "snapshots": [8, 16]}
    out["untraced"], out["traced"] = [], []
    for _ in range(3):  # alternating, so that a drift of the machine shows in both
        out["untraced"].append(run(2, 24, 4, None))
        out["traced"].append(run(2, 24, 4, (8, 16)))
    print(json.dumps(out))
