"""Times of the dynamic EAP's blocks form on a sharded mixed filter against the
single context holding the same components (DESIGN.md §6 "Mixed model",
*Expected maps*): eap_dyn_count, eap_dyn_pack, eap_dyn_finish on rank 0 of
`world` ranks emulated on one device, and PHDFilter.expected_map_dynamic; host
wall clock around synchronised calls, median / min / max in ms, one JSON line.

    python scripts/time_eap_dynamic.py

The two forms of the reduce itself (DESIGN.md §6 "Mixed model", *Decision
rounds*): `rounds` builds a mixed store of n particles x 64 dynamic components
drawn from 3 000 landmarks spread over a 400 x 400 square (so the map has a few
thousand components), and calls expected_map_dynamic() in mode 1 (the one
workgroup) and mode 0 (the decision rounds) alternately: the median of five
calls after the first, with rounds, cells and the output count, and whether
the two maps are the same bytes.  Two shapes, n = 256 and n = 4 096.  The
mode-1 calls of a shape stop once they have used MODE1_BUDGET_S in all; a
shape that could not finish its six is reported "exceeded".  --tree names
another checkout (a built worktree of the parent commit) whose library is
timed instead; one without the mode switch is timed as it is.

    timeout -k 10 900 python scripts/time_eap_dynamic.py rounds
    timeout -k 10 300 python scripts/time_eap_dynamic.py rounds --tree ../parent --shapes 256
"""
import json
import os
import statistics
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--tree" in sys.argv:  # (before the import of phdslam: the other checkout's package and library)
    REPO = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1])
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


MODE1_BUDGET_S = 240.0
LANDMARKS, PER, CALLS = 3000, 64, 6


def rounds_store(n, seed=9):
    """n particles x PER components, each a jittered copy of one of LANDMARKS
    landmarks (a particle sees a random subset), weights and log-weights random."""
    from phdslam.types import GAUSSIAN4D
    rng = np.random.default_rng(seed)
    base = np.concatenate([rng.uniform(-200, 200, (LANDMARKS, 2)), rng.normal(0, 1.5, (LANDMARKS, 2))], 1)
    K = n * PER
    pick = np.concatenate([rng.choice(LANDMARKS, PER, replace=False) for _ in range(n)])
    d = np.zeros(K, GAUSSIAN4D)
    d["mean"] = (base[pick] + rng.normal(0, 0.1, (K, 4))).astype(np.float32)
    cov = np.zeros((K, 4, 4))
    cov[:, 0, 0], cov[:, 1, 1] = rng.uniform(0.05, 0.3, K), rng.uniform(0.05, 0.3, K)
    cov[:, 2, 2], cov[:, 3, 3] = rng.uniform(0.2, 1.0, K), rng.uniform(0.2, 1.0, K)
    cov[:, 0, 2] = cov[:, 2, 0] = rng.uniform(-0.02, 0.02, K)
    cov[:, 1, 3] = cov[:, 3, 1] = rng.uniform(-0.02, 0.02, K)
    d["cov"] = cov.transpose(0, 2, 1).reshape(K, 16)
    d["weight"] = rng.uniform(0.2, 1.0, K)
    lw = rng.normal(-np.log(n), 0.3, n).astype(np.float32)
    return d, np.arange(n + 1, dtype=np.int32) * PER, lw


def rounds_shape(n):
    cfg = mixed_config()
    poses, sm, sof, _, _, _ = mixed_scenario(cfg, n, 3, 1, 4)
    dm, dof, lw = rounds_store(n)
    f = filt(cfg, n, PER, 256)
    f.load(poses, lw, sm, sof)
    f.load_dynamic(dm, dof)
    modes = (1, 0) if hasattr(f, "set_expected_map_dynamic_mode") else (None,)
    ts, maps, diag = {m: [] for m in modes}, {}, {}
    spent1 = 0.0
    for _ in range(CALLS):
        for m in modes:
            if m == 1 and spent1 > MODE1_BUDGET_S:
                continue
            if m is not None:
                f.set_expected_map_dynamic_mode(m)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            maps[m] = f.expected_map_dynamic()
            torch.cuda.synchronize()
            ts[m].append((time.perf_counter() - t0) * 1e3)
            if m == 1:
                spent1 += ts[m][-1] * 1e-3
            if m is not None:
                diag[m] = f.expected_map_dynamic_groups()
    res = {"n": n, "components": n * PER, "tree": "--tree" if "--tree" in sys.argv else "this tree"}
    for m in modes:
        name = {1: "one_workgroup", 0: "rounds", None: "as_built"}[m]
        t = ts[m][1:]
        if len(ts[m]) < CALLS:
            res[name] = {"exceeded": True, "calls_ms": [round(x, 2) for x in ts[m]], "budget_s": MODE1_BUDGET_S}
        else:
            res[name] = {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3),
                         "max_ms": round(max(t), 3), "first_ms": round(ts[m][0], 3), "reps": len(t)}
        if m in maps:
            res[name]["out_components"] = len(maps[m])
        if m in diag:
            res[name]["rounds"], res[name]["cells"] = diag[m]
    if 0 in maps and 1 in maps:
        res["equal"] = maps[0].tobytes() == maps[1].tobytes()
    f.close()
    return res


if __name__ == "__main__":
    if "rounds" in sys.argv[1:]:
        ns = [256, 4096]
        if "--shapes" in sys.argv:
            ns = [int(x) for x in sys.argv[sys.argv.index("--shapes") + 1].split(",")]
        for n in ns:
            print(json.dumps(rounds_shape(n)), flush=True)
    else:
        out = [shape(2, 24, 10, 64, 4096, 30), shape(8, 512, 10, 16, 256, 7)]
        print(json.dumps(out))
