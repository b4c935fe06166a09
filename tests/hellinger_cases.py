"""Inputs and expected outputs shared by the Hellinger-merge tests
(tests/test_hellinger_ref.py on the CPU, tests/test_gpu_hellinger.py on the
device): each case's scenario is built once, its expected update
(hellinger_ref.expected_update) once, and both are handed out unchanged.

TEST INFRASTRUCTURE ONLY.
"""
import functools
import os

import numpy as np

import hellinger_ref as H

GOLDEN_PAIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hellinger_directed_pair.npz")

# name -> (config id, n, G, M, overrides of the preset, minSeparation values)
CASES = {
    "phd_small": (2, 16, 64, 16, {}, (0.3, 0.7, 0.95)),
    "phd_large": (2, 8, 300, 40, {}, (0.3, 0.7, 0.95)),
    "merge_stress": (5, 8, 256, 64, {"pd": 0.7}, (0.7,)),
    "cphd": (3, 8, 64, 16, {"maxCardinality": 127}, (0.7,)),
    "collapse": (2, 8, 32, 8, {}, (1.5,)),
    "zero_cov": (2, 8, 32, 8, {}, (0.7,)),
}
MAX_SKIP = 8  # at most 1 particle in MAX_SKIP may hold a near decision


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(cfg with distanceMetric 1, poses, log-weights, maps, offsets, measurements)."""
    import phdslam
    cid, n, G, M, over, _ = CASES[name]
    cfg, poses, lw, maps, offs, z = phdslam.config_scenario(cid, n=n, G=G, M=M)
    for k, v in over.items():
        setattr(cfg, k, v)
    cfg.distanceMetric = 1
    if name == "zero_cov":  # as test_singular_covariance_takes_serial_fallback
        maps["cov"][offs[6] + 1] = (0.0, 0.0, 0.0, 0.0)
    for a in (poses, lw, maps, offs, z):
        a.setflags(write=False)
    return cfg, poses, lw, maps, offs, z


def config(name, T):
    c = inputs(name)[0].copy()
    c.minSeparation = T
    return c


@functools.lru_cache(maxsize=None)
def expected(name, T):
    """hellinger_ref.expected_update of the case at minSeparation T (read-only arrays)."""
    cfg, poses, lw, maps, offs, z = inputs(name)
    r = H.expected_update(config(name, T), poses, maps, offs, z, T, cardinality=cfg.filterType == 1)
    for a in r:
        a.setflags(write=False)
    return r


def all_case_keys():
    return [(name, T) for name, c in CASES.items() for T in c[5]]


def find_directed_pair(seed=7, tries=200000):
    """Search random pairs for d(a, b) != d(b, a).  With symmetric covariances
    the distance is bitwise symmetric (device_math.cuh:405-408: the entries of
    a b and of b a are then the same sums, transposed), so the pairs carry the
    asymmetry real candidates have: off-diagonals a few ulps apart, as the
    rounded covariance updates of detection terms.  Returns (mean_a, cov_a,
    mean_b, cov_b, d_ab, d_ba) of the first pair with both distances in
    (0.2, 0.8); means laid 55 m out on the x axis (the nearly-in-range ring of
    config 2's 50 m sensor for a pose at the origin)."""
    rng = np.random.default_rng(seed)
    th = rng.uniform(0, np.pi, (tries, 2))
    l1 = rng.uniform(0.05, 0.5, (tries, 2))
    l2 = l1 * rng.uniform(0.1, 1.0, (tries, 2))
    c, s = np.cos(th), np.sin(th)
    b = (c * s * (l1 - l2)).astype(np.float32)
    b2 = b.copy()
    for _ in range(3):
        b2 = np.nextafter(b2, np.float32(np.inf))
    cov = np.stack([(c * c * l1 + s * s * l2).astype(np.float32), b, b2, (s * s * l1 + c * c * l2).astype(np.float32)], -1)
    ma = np.tile(np.array([55.0, 0.0], np.float32), (tries, 1))
    mb = (ma + rng.uniform(-0.6, 0.6, (tries, 2))).astype(np.float32)
    dab = H.hellinger(ma, cov[:, 0], mb, cov[:, 1])
    dba = H.hellinger(mb, cov[:, 1], ma, cov[:, 0])
    hit = np.flatnonzero((dab != dba) & (dab > 0.2) & (dab < 0.8))
    if len(hit) == 0:
        return None
    i = hit[0]
    return ma[i], cov[i, 0], mb[i], cov[i, 1], dab[i], dba[i]


def directed_scenario(mirrored=False):
    """One particle at the origin whose map is the saved pair as class-2 (nearly
    in range) components, the heavier one first — or second when mirrored, so
    that priority order and index order disagree and a merge that evaluated
    d(lower index, higher index) would decide wrongly; one measurement close to
    the sensor.  T = the larger of the pair's two distances, so the seed-first
    and the candidate-first test decide differently."""
    import phdslam
    from phdslam.types import GAUSSIAN2D, MEASUREMENT, POSE
    g = np.load(GOLDEN_PAIR)
    cfg = phdslam.config_scenario(2, n=1, G=2, M=1)[0]
    assert cfg.maxRange < 55.0 - 1.0 and 1.2 * cfg.maxRange > 55.0 + 1.0
    poses = np.zeros(1, POSE)
    maps = np.zeros(2, GAUSSIAN2D)
    ia, ib = (1, 0) if mirrored else (0, 1)
    maps[ia]["mean"], maps[ia]["cov"], maps[ia]["weight"] = g["mean_a"], g["cov_a"], 0.6
    maps[ib]["mean"], maps[ib]["cov"], maps[ib]["weight"] = g["mean_b"], g["cov_b"], 0.5
    z = np.zeros(1, MEASUREMENT)
    z[0]["range"], z[0]["bearing"] = 5.0, -2.0
    cfg.distanceMetric = 1
    cfg.minSeparation = float(max(g["d_ab"], g["d_ba"]))
    return cfg, poses, np.zeros(1, np.float32), maps, np.array([0, 2], np.int32), z, g
