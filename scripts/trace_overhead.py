"""Cost of the per-scan estimate trace (phd_trace_enable) on the bench workload.

    python scripts/trace_overhead.py [--config 3] [--steps 200] [--warmup 20] [--runs 3]
                                     [--out profiles/trace_overhead.json] [--leg NAME]

bench.py's scenario of --config in replay mode (same capacities, seed, control,
clock warm-up), --steps steps per leg, --runs runs of each leg:
  off        phd_step, trace off                    (bench.py's own loop)
  records    phd_step, trace on, records only
  full       phd_step, trace on, a 64-component map snapshot and (CPHD) the
             cardinality distribution
  host_loop  what phdslam_run's device loop does per scan without the trace:
             phd_predict_update, phd_normalize, phd_export_particles, nEff on
             the host, phd_resample when it decides so
Writes steps/s of every run and leg (median, min, max) as JSON.  --leg runs one
leg once, untimed by this script's JSON (for a profiler's kernel trace of it).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "cuda-phdslam_amd"))

LEGS = ("off", "records", "full", "host_loop")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "trace_overhead.json"))
    ap.add_argument("--leg", choices=LEGS, default=None)
    args = ap.parse_args()

    import torch
    import phdslam
    from phdslam.scenario import SEED_BASE, bench_capacities

    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    cfg, n, G, M, df = phdslam.preset(args.config)
    seed = SEED_BASE + args.config
    _, poses, lw, maps, offs, z = phdslam.config_scenario(args.config, n=n, G=G, M=M, seed=seed)
    cphd = cfg.filterType == 1
    control = (2.0, 0.05) if cfg.motionType == 1 else None

    def make_filter():
        f = phdslam.PHDFilter(n, cfg, device=0, **bench_capacities(args.config, G, M, False))
        f.set_seed(seed)
        f.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        f.load(poses, lw, maps, offs)
        f.set_measurements(z)
        f.set_replay(True)
        f.set_check_each_update(False)
        return f

    def clock_warmup():
        x = torch.randn(8192, 8192, device=dev, dtype=torch.bfloat16)
        for _ in range(40):
            x = (x @ x).clamp_(-1, 1)
        torch.cuda.synchronize(dev)

    def run_leg(leg):
        f = make_filter()
        if leg == "records":
            f.enable_trace(args.steps + args.warmup)
        elif leg == "full":
            f.enable_trace(args.steps + args.warmup, 64, cphd)

        if leg == "host_loop":
            def one(k):
                f.predict_update(control, k)
                f.normalize()
                w = f.export(with_maps=False)[1].astype(np.float64)
                if 1.0 / np.sum(np.exp(2.0 * w)) / n <= cfg.resampleThresh:
                    f.resample(step=k, return_indices=False)
        else:
            def one(k):
                f.step(control, step=k, readback=False)
        clock_warmup()
        for k in range(args.warmup):
            one(k)
        torch.cuda.synchronize(dev)
        f.check_errors()
        t0 = time.perf_counter()
        for k in range(args.steps):
            one(args.warmup + k)
        torch.cuda.synchronize(dev)
        dt = time.perf_counter() - t0
        f.check_errors()
        extra = {}
        if leg in ("records", "full"):
            assert f.trace_count() == args.steps + args.warmup
            out = f.read_trace()
            rec = out[0] if isinstance(out, tuple) else out
            extra = {"resampled": int(rec["resampled"][args.warmup:].sum()), "neff": float(rec["neff"][-1])}
        f.close()
        return args.steps / dt, extra

    if args.leg:
        print(json.dumps({"leg": args.leg, "steps_per_s": run_leg(args.leg)[0]}))
        return 0
    res = {"config": args.config, "particles": n, "steps": args.steps, "warmup": args.warmup, "mode": "replay",
           "device": torch.cuda.get_device_name(0), "legs": {}}
    for leg in LEGS:
        runs, extra = [], {}
        for _ in range(args.runs):
            r, extra = run_leg(leg)
            runs.append(round(r, 1))
        res["legs"][leg] = dict(steps_per_s=runs, median=float(np.median(runs)), min=min(runs), max=max(runs), **extra)
    off = res["legs"]["off"]["median"]
    for leg in ("records", "full", "host_loop"):
        res["legs"][leg]["vs_off"] = round(res["legs"][leg]["median"] / off, 4)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
