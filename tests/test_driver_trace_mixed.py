"""phdslam_run --trace under feature_model 2: the driver's per-scan dynamic
cardinality file equals what the Python binding's read_trace_dynamic returns
for the same run (same configuration file, seed, capacities and call sequence)."""
import os
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N, SCANS = 8, 4


def _write_run(tmp_path):
    from phdslam.scenario import mixed_config, mixed_scenario
    c = mixed_config()
    z = mixed_scenario(c, N, 10, 6, 10, seed=41)[5]
    rng = np.random.default_rng(3)
    scans = []
    for _ in range(SCANS):
        zk = z.copy()
        zk["range"] += rng.normal(0, 0.05, len(zk)).astype(np.float32)
        scans.append(zk)
    data = tmp_path / "data"
    data.mkdir()
    with open(data / "measurements.txt", "w") as f:
        for zk in scans:
            f.write(" ".join(f"{float(m['range'])!r} {float(m['bearing'])!r} {int(m['label'])}" for m in zk) + "\n")
    (data / "controls.txt").write_text("".join("0, 0\n" for _ in range(SCANS)))
    cfg = tmp_path / "mixed.cfg"
    cfg.write_text("motion_type = 0\nfeature_model = 2\nfilter_type = 0\nparticle_weighting = 0\n"
                   "distance_metric = 0\nmax_range = 20\nmin_range = 0\nmax_bearing = 3.141593\n"
                   "std_range = 0.3\nstd_bearing = 0.02\npd = 0.9\nclutter_rate = 5\nbirth_weight = 0.05\n"
                   "birth_noise_factor = 1.5\nmin_feature_weight = 0.00001\nmin_separation = 4\n"
                   "cov_vx_birth = 1\ncov_vy_birth = 1\nstd_ax_features = 0.5\nstd_ay_features = 0.5\n"
                   "ps = 0.98\ntau = 1.5\nbeta = 4\ndt = 0.1\nlabeled_measurements = 1\n"
                   f"resample_threshold = 0.5\nn_particles = {N}\ndata_directory = {data}/\n")
    return cfg, scans


@pytest.mark.gpu
def test_driver_trace_mixed(gpu, tmp_path):
    import phdslam
    from phdslam.types import GAUSSIAN2D, POSE
    cfg, scans = _write_run(tmp_path)
    out = tmp_path / "out"
    out.mkdir()
    exe = os.path.join(REPO, "cuda-phdslam_amd", "phdslam", "phdslam_run")
    env = dict(os.environ)
    env.pop("PHDSLAM_SEED", None)
    r = subprocess.run([exe, str(cfg), "--triples", "--trace", "--log", str(out)], capture_output=True, text=True,
                       timeout=100, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rows = np.loadtxt(out / "trajectory_dynamic.txt", comments="%", ndmin=2)
    traj = np.loadtxt(out / "trajectory.txt", comments="%", ndmin=2)
    assert rows.shape == (SCANS, 4) and traj.shape[0] == SCANS
    # the same run through the binding: the driver's capacities, seed, initial state and step numbers
    c = phdslam.load_config(cfg)[0]
    assert c.featureModel == 2 and c.motionType == 0 and c.n_particles == N
    f = phdslam.PHDFilter(N, c, map_capacity=1024, candidate_capacity=2048)
    poses = np.zeros(N, POSE)
    for fld, v in (("px", c.x0), ("py", c.y0), ("ptheta", c.yaw0), ("vx", c.vx0), ("vy", c.vy0), ("vtheta", c.vyaw0)):
        poses[fld] = v
    f.load(poses, np.full(N, -np.log(np.float32(N)), np.float32), np.zeros(0, GAUSSIAN2D), np.zeros(N + 1, np.int32))
    f.set_seed(0x5eed5eed)
    f.set_check_each_update(False)
    f.enable_dynamic(256)
    f.enable_trace_mixed(SCANS)
    for k, zk in enumerate(scans):
        f.set_measurements(zk)
        f.step((0.0, 0.0), do_predict=k > 0, step=max(k - 1, 0), readback=False)
    rec = f.read_trace()
    drec = f.read_trace_dynamic()
    f.check_errors()
    f.close()
    assert any(d["map_size"] > 0 for d in drec), "the run builds dynamic maps"
    for k in range(SCANS):
        # to the printed precision: %.9g round-trips a float
        assert int(rows[k][0]) == k and int(rows[k][3]) == drec[k]["map_size"], k
        assert np.float32(rows[k][1]) == drec[k]["card_expected"], (k, rows[k][1], drec[k]["card_expected"])
        assert np.float32(rows[k][2]) == drec[k]["card_map"], (k, rows[k][2], drec[k]["card_map"])
        assert np.float32(traj[k][13]) == rec[k]["neff"] and int(traj[k][17]) == rec[k]["map_size"], k
