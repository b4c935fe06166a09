"""Times of the dynamic EAP's blocks form on a sharded mixed filter against the
single context holding the same components (DESIGN.md §6 "Mixed model",
*Expected maps*): eap_dyn_count, eap_dyn_pack, eap_dyn_finish on rank 0 of
`world` ranks emulated on one device, and PHDFilter.expected_map_dynamic; host
wall clock around synchronised calls, median / min / max in ms, one JSON line.

    python scripts/time_eap_dynamic.py
"""
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(REPO, "cuda-phdslam_amd"), os.path.join(REPO, "tests")]

import torch  # noqa: E402
import phdslam  # noqa: E402
from phdslam.dist import ShardedFilter  # noqa: E402
from phdslam.scenario import mixed_config, mixed_scenario  # noqa: E402


def filt(cfg, n, dcap, kcap):
    f = phdslam.PHDFilter(n, cfg, map_capacity=128, max_measurements=32, candidate_capacity=kcap, survivor_capacity=256)
    f.set_seed(0x5eed)
    f.enable_dynamic(dcap)
    return f


def timed(fn, reps, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4),
            "reps": reps}


def shape(world, n, gd, dcap, kcap, reps):
    cfg = mixed_config()
    N = world * n
    poses, sm, sof, dm, dof, z = mixed_scenario(cfg, N, 30, gd, 10)
    lw = np.random.default_rng(1).normal(-np.log(N), 0.3, N).astype(np.float32)
    dev = torch.device("cuda", 0)
    shards = []
    for r in range(world):
        f = filt(cfg, n, dcap, kcap)
        f.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        so, do = sof[r * n:(r + 1) * n + 1], dof[r * n:(r + 1) * n + 1]
        f.load(poses[r * n:(r + 1) * n], lw[r * n:(r + 1) * n], sm[so[0]:so[-1]], (so - so[0]).astype(np.int32))
        f.load_dynamic(dm[do[0]:do[-1]], (do - do[0]).astype(np.int32))
        shards.append(ShardedFilter(f, None, dev, world=world, rank=r, block_records=1))
    counts = [sf.eap_dyn_count() for sf in shards]
    k_max, total = max(counts), sum(counts)
    for sf in shards:
        sf.eap_dyn_pack(k_max)
    blocks = torch.cat([sf.eap_dyn_block for sf in shards])
    sf = shards[0]
    sf.eap_dyn_blocks.copy_(blocks)
    res = {"world": world, "n": n, "components": total, "k_max": k_max}
    res["count"] = timed(sf.eap_dyn_count, reps)
    res["pack"] = timed(lambda: sf.eap_dyn_pack(k_max), reps)
    got = sf.eap_dyn_finish(k_max, total)
    res["blocks_reduce"] = timed(lambda: sf.eap_dyn_finish(k_max, total), reps)
    single = filt(cfg, N, dcap, kcap)
    single.load(poses, lw, sm, sof)
    single.load_dynamic(dm, dof)
    want = single.expected_map_dynamic()
    res["single_context"] = timed(single.expected_map_dynamic, reps)
    res["out_components"] = len(want)
    res["equal"] = got.tobytes() == want.tobytes()
    single.close()
    for s in shards:
        s.f.close()
    return res


if __name__ == "__main__":
    out = [shape(2, 24, 10, 64, 4096, 30), shape(8, 512, 10, 16, 256, 7)]
    print(json.dumps(out))
