"""Inputs, float64 reference results and measured oracle distances of the pose
prediction, the estimates and the static EAP map, shared by
tests/test_state_ref64.py (CPU) and tests/test_gpu_state_ref64.py (device):
each case's inputs are built once, its reference (state_ref64) once, and both
are handed out unchanged.

Maps are compared per field class as mixed_ref64_cases compares the dynamic
ones (FIELD_CLASSES: weight, noncancel, cancel; field_deviations here is its
2-D form on update_ref64_cases.map_deviations' measures, in emission order,
NaN matching NaN).  Pose fields: relative deviation with a scale floor of 1
(predicted poses) or 1e-3 (the expected pose), as the oracle-parity tests call
parity.close; headings by circular difference.

TEST INFRASTRUCTURE ONLY.
"""
import collections
import functools
import zlib

import numpy as np

import parity
import state_ref64 as R
import update_ref64_cases as U
import weighting_ref
from mixed_ref64_cases import CONTRACT, FIELD_CLASSES  # noqa: F401

PI32 = np.float32(np.pi)
MODELS = ("ack", "cv")
PREDICT_CASES = tuple(f"{m}_{k}" for m in MODELS
                      for k in ("n1_s1", "n1_s4", "n257_s1", "n257_s4", "n1000_s1", "n1000_s4", "still", "npp3", "fused"))
POSE_CLASSES = ("pos", "heading", "vel")
PREDICT_CLASSES = POSE_CLASSES + ("noise",)
EP_CASES = ("ep_n1", "ep_n1023_tie0_5", "ep_n1024_tie63_64", "ep_n1025_last", "ep_n4097_tie7_1031", "ep_n4097_last")
EP_CLASSES = POSE_CLASSES
EAP_CASES = ("sum_edges", "big_cell", "borders", "wide_lambda", "chains", "duplicates", "zero_weights", "fallback",
             "single", "empty")
CARD_SIZES = (0, 1, 63, 64, 65, 128)
CARD_CAP = 128
CARD_RTOL = 2.0 ** -23  # a double sum rounded to float32 once

# D_oracle(case, class): the worst deviation of the oracle (pyoracle.predict_* /
# noise_* / expected_pose / expected_map) from state_ref64, measured on the CPU
# (tests/test_state_ref64.py prints the figures) and rounded up to two
# significant figures.  test_state_ref64.py asserts the oracle stays within
# it; test_gpu_state_ref64.py holds the device to D_oracle + 1e-5.
D_ORACLE = {
    "ack_n1_s1": dict(pos=5.5e-08, heading=5.7e-08, vel=0, noise=0),
    "ack_n1_s4": dict(pos=3.6e-08, heading=2.1e-08, vel=0, noise=0),
    "ack_n257_s1": dict(pos=7.9e-08, heading=5.9e-08, vel=0, noise=0),
    "ack_n257_s4": dict(pos=5.8e-08, heading=5.5e-08, vel=0, noise=0),
    "ack_n1000_s1": dict(pos=6.8e-08, heading=6e-08, vel=0, noise=0),
    "ack_n1000_s4": dict(pos=6e-08, heading=5.9e-08, vel=0, noise=0),
    "ack_still": dict(pos=0, heading=2.1e-08, vel=0, noise=0),
    "ack_npp3": dict(pos=5.8e-08, heading=6e-08, vel=0, noise=0),
    "ack_fused": dict(pos=5.7e-08, heading=5.7e-08, vel=0, noise=0),
    "cv_n1_s1": dict(pos=4.4e-08, heading=2.6e-08, vel=3.4e-08, noise=0),
    "cv_n1_s4": dict(pos=4.4e-08, heading=2.2e-08, vel=3.7e-08, noise=0),
    "cv_n257_s1": dict(pos=1.1e-07, heading=8.9e-08, vel=6e-08, noise=0),
    "cv_n257_s4": dict(pos=1.1e-07, heading=1.1e-07, vel=5.9e-08, noise=0),
    "cv_n1000_s1": dict(pos=1.1e-07, heading=1.2e-07, vel=6.1e-08, noise=0),
    "cv_n1000_s4": dict(pos=1.1e-07, heading=1.1e-07, vel=5.9e-08, noise=0),
    "cv_still": dict(pos=0, heading=2.1e-08, vel=0, noise=0),
    "cv_npp3": dict(pos=1.2e-07, heading=6.6e-08, vel=5.9e-08, noise=0),
    "cv_fused": dict(pos=1.1e-07, heading=9.5e-08, vel=5.6e-08, noise=0),
    "ep_n1": dict(pos=0, heading=0, vel=0),
    "ep_n1023_tie0_5": dict(pos=6e-08, heading=1.8e-07, vel=2.4e-08),
    "ep_n1024_tie63_64": dict(pos=3.2e-08, heading=6.7e-09, vel=2.9e-07),
    "ep_n1025_last": dict(pos=1.9e-08, heading=1.3e-07, vel=9.3e-08),
    "ep_n4097_tie7_1031": dict(pos=3.6e-09, heading=9.1e-07, vel=5e-08),
    "ep_n4097_last": dict(pos=4.2e-08, heading=2e-08, vel=1.2e-07),
    "sum_edges": dict(weight=2e-07, noncancel=3.4e-07, cancel=2e-08),
    "big_cell": dict(weight=2.9e-07, noncancel=5.2e-07, cancel=9.4e-09),
    "borders": dict(weight=6.8e-08, noncancel=1.5e-07, cancel=4e-08),
    "wide_lambda": dict(weight=8e-08, noncancel=1.5e-07, cancel=3.7e-08),
    "chains": dict(weight=1.1e-07, noncancel=1.8e-07, cancel=1.9e-10),
    "duplicates": dict(weight=1.7e-07, noncancel=2.8e-07, cancel=2.2e-07),
    "zero_weights": dict(weight=1.4e-07, noncancel=2.9e-07, cancel=6.2e-08),
    "fallback": dict(weight=1.5e-07, noncancel=1.2e-06, cancel=2.2e-08),
    "single": dict(weight=0, noncancel=0, cancel=5.1e-08),
    "empty": dict(weight=0, noncancel=0, cancel=0),
}


def _rng(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def _freeze(t):
    for a in t:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return t


# ---- predict -----------------------------------------------------------

PCase = collections.namedtuple("PCase", "cfg model poses lw maps offs z control npp seed step offsets host fused")

# (seed, step) of the device draws; one case with the seed's high word and one
# with the step's high word in use
_DRAWS = {"n257_s4": (4242, 2 ** 33 + 5), "n1000_s1": (2 ** 40 + 12345, 11)}


def _predict_build(name):
    import phdslam
    from phdslam.types import ACKERMAN_NOISE, CV_NOISE, POSE
    model, kind = name.split("_", 1)
    rng = _rng(name)
    n = {"still": 64, "npp3": 40, "fused": 64}.get(kind) or int(kind.split("_")[0][1:])
    sub = int(kind.split("_s")[1]) if "_s" in kind else 1
    fused = kind == "fused"
    G, M = (16, 4) if fused else (1, 1)
    cfg, _, lw, maps, offs, z = phdslam.config_scenario(2 if model == "ack" else 3, n=n, G=G, M=M)
    cfg.subdividePredict = sub
    cfg.ay = 0.3  # (the presets have ay = 0: the ay terms would go unchecked)
    npp = 3 if kind == "npp3" else 1
    cfg.nPredictParticles = npp
    if fused:
        cfg.resampleThresh = 0.0  # no resample: the exported poses are the predicted ones
    dt = float(cfg.dt) / sub
    poses = np.zeros(n, POSE)
    poses["px"], poses["py"] = rng.uniform(-50, 50, n), rng.uniform(-50, 50, n)
    poses["ptheta"] = rng.uniform(-np.pi, np.pi, n)
    poses["vx"], poses["vy"] = rng.uniform(-3, 3, n), rng.uniform(-3, 3, n)
    poses["vtheta"] = rng.uniform(-0.5, 0.5, n)
    # Ackerman inputs stay within |tan(alpha + n_alpha) h / l| <= 0.5 (asserted
    # below), so the quotient 1 / (1 - tan h / l) has a conditioning of at most 2:
    # the pole is not a float64-versus-float32 question
    v, alpha = (2.5, 0.1 if sub == 1 else -0.1)
    rate = abs(v * np.tan(alpha) / float(cfg.l)) if model == "ack" else 0.4
    # headings whose step crosses +pi upwards and -pi downwards (and their
    # mirror images, which do not): within 1.5 steps of the cut, both signs
    k = n // 2 if n > 1 else 1
    s = np.where(rng.uniform(size=k) < 0.5, -1.0, 1.0)
    poses["ptheta"][:k] = s * (np.pi - rng.uniform(0.05, 1.5, k) * dt * rate)
    if model == "cv":
        poses["vtheta"][:k] = np.where(rng.uniform(size=k) < 0.75, s, -s) * 0.4
    if n >= 8:
        poses["ptheta"][k:k + 3] = (PI32, -PI32, 0.0)
        if model == "cv":
            poses["vtheta"][k:k + 3] = (0.4, -0.4, 0.0)
    assert np.all(np.abs(poses["ptheta"]) <= PI32)
    m = n * npp
    if model == "ack":
        host = np.zeros(m, ACKERMAN_NOISE)
        host["n_alpha"] = float(cfg.stdAlpha) * rng.normal(size=m)
        host["n_encoder"] = float(cfg.stdEncoder) * rng.normal(size=m)
    else:
        host = np.zeros(m, CV_NOISE)
        host["ax"] = 3 * float(cfg.ax) * rng.normal(size=m)
        host["ay"] = 3 * float(cfg.ay) * rng.normal(size=m)
        host["atheta"] = 3 * float(cfg.ayaw) * rng.normal(size=m)
    offsets = (0, 4096)
    if kind == "still":  # zero control, zero noise: the pose is unchanged apart from the wrap
        v, alpha = 0.0, 0.0
        host[:] = 0
        if model == "cv":
            poses["vx"] = poses["vy"] = poses["vtheta"] = 0
        offsets = ()
    seed, step = _DRAWS.get(kind, (77, 5))
    return PCase(cfg, model, poses, lw, maps, offs, z, (v, alpha), npp, seed, step, offsets, host, fused)


@functools.lru_cache(maxsize=None)
def predict_inputs(name):
    return _freeze(_predict_build(name))


def _predict(c, poses, noise):
    if c.model == "ack":
        assert np.all(np.abs(np.tan(c.control[1] + noise["n_alpha"].astype(np.float64))) * float(c.cfg.h)
                      / float(c.cfg.l) <= 0.5)
        return R.predict_ackerman(c.cfg, poses, c.control[0], c.control[1], noise)
    return R.predict_cv(c.cfg, poses, noise)


PRef = collections.namedtuple("PRef", "host lw parent noise rng")


@functools.lru_cache(maxsize=None)
def predict_reference(name):
    """PRef: the prediction with the host noise; the children's log-weights and
    parents; per index offset the reference draw and the prediction with it."""
    c = predict_inputs(name)
    noise, out = {}, {}
    for off in c.offsets:
        ep, _, _, ids = R.expand(c.poses, c.lw, c.npp, off)
        noise[off] = (R.noise_ackerman if c.model == "ack" else R.noise_cv)(c.cfg, c.seed, ids, c.step)
        out[off] = _predict(c, ep, noise[off])
    ep, w, parent, _ = R.expand(c.poses, c.lw, c.npp)
    return PRef(_predict(c, ep, c.host), w, parent, noise, out)


def pose_deviations(ref, got, scale=1.0):
    """Worst deviations per class of pose records (or one record) in the same order."""
    ref, got = np.atleast_1d(ref), np.atleast_1d(got)
    assert len(ref) == len(got)
    a, b = ref["ptheta"].astype(np.float64), got["ptheta"].astype(np.float64)
    d = np.abs(R.wrap(a - b))
    return dict(pos=max(U._rel(ref[k], got[k], scale=scale) for k in ("px", "py")),
                heading=float(np.max(d / np.maximum(np.maximum(np.abs(a), np.abs(b)), scale))),
                vel=max(U._rel(ref[k], got[k], scale=scale) for k in ("vx", "vy", "vtheta")))


def noise_deviation(ref, got):
    return max(U._rel(ref[k], got[k]) for k in ref.dtype.names)


# ---- expected pose -------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ep_inputs(name):
    """(poses, float32 log-weights, the indices that share the maximum)."""
    from phdslam.types import POSE
    parts = name.split("_")
    n = int(parts[1][1:])
    ties = (n - 1,) if len(parts) < 3 or parts[2] == "last" else (int(parts[2][3:]), int(parts[3]))
    rng = _rng(name)
    w = rng.normal(0, 1, n)
    if n > 400:
        w[100:164] = -np.inf  # a block of particles without weight
    w[list(ties)] = 6.0 if n > 1 else 0.0
    lw = weighting_ref.normalize(w)[0].astype(np.float32)
    assert len(set(lw[list(ties)])) == 1 and np.sum(lw == lw[ties[0]]) == len(ties) and lw.max() == lw[ties[0]]
    poses = np.zeros(n, POSE)
    for k in POSE.names:
        poses[k] = rng.uniform(-3, 3, n)  # both signs: the sums cancel
    poses["px"] += 40
    return _freeze((poses, lw, ties))


@functools.lru_cache(maxsize=None)
def ep_reference(name):
    poses, lw, _ = ep_inputs(name)
    return R.expected_pose(lw, poses)


# ---- cardinalities -------------------------------------------------------

@functools.lru_cache(maxsize=None)
def card_inputs():
    """(cfg, poses, lw, maps, offsets, z): slabs of CARD_SIZES components (twice,
    in two orders) of weights 1e-6 .. 1.  The scan is labelled dynamic, so the
    static update adds neither detections nor births: no map outgrows its slab."""
    import phdslam
    sizes = np.array(CARD_SIZES + CARD_SIZES[::-1][1:] + CARD_SIZES[:1])
    n = len(sizes)
    cfg, poses, _, maps, offs, z = phdslam.config_scenario(2, n=n, G=CARD_CAP, M=4)
    maps, offs = U._subset(maps, offs, sizes)
    rng = _rng("card")
    maps["weight"] = 10.0 ** rng.uniform(-6, 0, len(maps))
    cfg.labeledMeasurements = True
    z["label"] = 1
    lw = np.log(rng.dirichlet(np.ones(n))).astype(np.float32)
    return _freeze((cfg, poses, lw, maps, offs.astype(np.int32), z))


# ---- the static EAP map --------------------------------------------------

ECase = collections.namedtuple("ECase", "cfg poses lw maps offs cap extra")
T_EAP = 10.0


def _spd(rng, k, lam_lo, lam_hi, cond_hi):
    """k covariances with the larger eigenvalue in [lam_lo, lam_hi], a condition in [1, cond_hi], any orientation."""
    l1 = rng.uniform(lam_lo, lam_hi, k)
    l2 = l1 / rng.uniform(1.0, cond_hi, k)
    th = rng.uniform(0, np.pi, k)
    c, s = np.cos(th), np.sin(th)
    off = (l1 - l2) * c * s
    return np.stack([l1 * c * c + l2 * s * s, off, off, l1 * s * s + l2 * c * c], 1).astype(np.float32)


def _iso(k, lam):
    return np.tile(np.array([lam, 0, 0, lam], np.float32), (k, 1))


def _grid_weights(rng, K):
    """K distinct weights in 0.2 .. 0.2 (1 + K / 1000), neighbours at least 2e-4 K / (K + 1000) apart relatively."""
    return 0.2 * (1.0 + 1e-3 * rng.permutation(K))


def _clusters(rng, centres, counts, lam=(0.05, 0.15), cond=30.0, sigma=0.01):
    """Tight clusters: every member within a small fraction of the merge radius of every other."""
    mean = np.concatenate([np.asarray(c)[None] + rng.normal(0, sigma, (k, 2)) for c, k in zip(centres, counts)])
    return mean, _spd(rng, len(mean), lam[0], lam[1], cond), np.repeat(np.arange(len(counts)), counts)


def _assemble(rng, n, W, mean, cov, dead=(), shuffle=True, extra=None):
    """K components in n particles of nearly equal sizes.  W: the weight each
    component is to have AFTER the scaling by its particle's weight (the
    float32 weight loaded is W / exp(lw), so the products keep W's spacing);
    particles of `dead` have log-weight -inf and carry W itself."""
    import phdslam
    from phdslam.types import GAUSSIAN2D, POSE
    K = len(W)
    order = rng.permutation(K) if shuffle else np.arange(K)
    sizes = np.full(n, K // n)
    sizes[:K % n] += 1
    offs = np.zeros(n + 1, np.int32)
    offs[1:] = np.cumsum(sizes)
    lw = np.log(rng.dirichlet(np.ones(n) * 4)).astype(np.float32) if n > 1 else np.zeros(1, np.float32)
    lw[list(dead)] = -np.inf
    ew = np.repeat(np.where(np.isfinite(lw), np.exp(lw.astype(np.float64)), 1.0), sizes)
    maps = np.zeros(K, GAUSSIAN2D)
    maps["weight"] = np.asarray(W, np.float64)[order] / ew
    maps["mean"] = np.asarray(mean)[order]
    maps["cov"] = np.asarray(cov)[order]
    cfg = phdslam.default_config()
    cfg.minSeparation = T_EAP
    return ECase(cfg, np.zeros(n, POSE), lw, maps, offs, max(64, int(sizes.max())), extra)


def lattice_side(cov, T=T_EAP):
    """R = sqrt(1.05 T Lambda), Lambda the largest covariance eigenvalue of the set."""
    P = R._mat(np.asarray(cov, np.float64))
    return float(np.sqrt(1.05 * T * np.linalg.eigvalsh(P).max()))


SUM_EDGES = (0, 1, 62, 63, 64, 65, 127, 128, 129)
_DIRS = [(1, 0), (-1, 0), (0, 1), (0, -1), (1, 1), (-1, -1), (1, -1), (-1, 1)]


def _borders(rng, wide):
    cov1 = _iso(1, 0.1)
    side = lattice_side(cov1)
    half = 0.5 * np.sqrt(0.5 * T_EAP * float(cov1[0, 0]))  # d = T / 2 between the two
    corners = [(i, j) for i in (0, -10, 5, -5, 10) for j in (0, -5, 10, -10, 5)]  # lattice corners, 5 cells apart
    mean, pair = [], []
    for q, u in enumerate(_DIRS):
        un = np.array(u, np.float64) / np.hypot(*u)
        for r in range(3):
            c = np.array(corners[3 * q + r], np.float64) * side
            if 0 in u:  # an edge, not the corner: move along the border
                c = c + 0.4 * side * np.array([u[1], u[0]], np.float64)
            mean += [c - half * un, c + half * un]
            pair += [len(pair) // 2] * 2
    c = np.array(corners[24], np.float64) * side + 0.5 * side
    mean += [c, c + np.array([3 * side, 0.0])]  # three cells apart: no merge
    mean = np.array(mean)
    cov = _iso(len(mean), 0.1)
    if wide:  # one far component 400 times wider: the cells grow, almost everything shares few of them
        mean = np.concatenate([mean, [[500.0, 500.0]]])
        cov = np.concatenate([cov, _iso(1, 40.0)])
    return _assemble(rng, 4, _grid_weights(rng, len(mean)), mean, cov, extra=dict(side=side, pairs=24))


def _eap_build(name):
    rng = _rng("eap_" + name)
    if name == "sum_edges":
        counts = [m + 1 for m in SUM_EDGES]
        centres = [(10.0 * (i % 3) - 7.0, 10.0 * (i // 3) - 12.0) for i in range(len(counts))]
        mean, cov, _ = _clusters(rng, centres, counts)
        return _assemble(rng, 8, _grid_weights(rng, len(mean)), mean, cov)
    if name == "big_cell":
        lam_set = _iso(1, 0.15)  # sets Lambda, hence the lattice
        side = lattice_side(lam_set)
        centres = [((cx + 0.5) * side + 0.4 * i, 3.5 * side + 0.4 * j) for cx in (2, 4) for i in (-1, 0, 1)
                   for j in (-1, 0, 1)]
        mean, cov, _ = _clusters(rng, centres, [78] * 18, lam=(0.004, 0.008), cond=3.0, sigma=0.005)
        mean = np.concatenate([mean, [[-40.0, -40.0]]])
        cov = np.concatenate([cov, lam_set])
        return _assemble(rng, 12, _grid_weights(rng, len(mean)), mean, cov, extra=dict(side=side))
    if name in ("borders", "wide_lambda"):
        return _borders(rng, name == "wide_lambda")
    if name == "chains":
        # covariance 0.1 I: merge radius sqrt(T 0.1) = 1; neighbours 0.9 apart (d = 8.1), the
        # next but one 1.8 (d = 32.4); weights descending along every line
        L, per = 8, 40
        t = np.tile(np.arange(per), L)
        line = np.repeat(np.arange(L), per)
        mean = np.stack([0.9 * t - 100.0 + 0.37 * line, 5.0 * line], 1)
        W = -np.sort(-_grid_weights(rng, L * per).reshape(L, per), axis=1).ravel()
        return _assemble(rng, 8, W, mean, _iso(L * per, 0.1))
    if name in ("duplicates", "zero_weights"):
        counts = rng.integers(3, 40, 24)
        centres = [(9.0 * (i % 5) - 20.0, 9.0 * (i // 5) - 20.0) for i in range(len(counts))]
        mean, cov, _ = _clusters(rng, centres, counts)
        n = 32 if name == "duplicates" else 20
        c = _assemble(rng, n, _grid_weights(rng, len(mean)), mean, cov,
                      dead=range(0, n, 5) if name == "zero_weights" else ())
        if name == "zero_weights":
            # components without weight that no weighted seed absorbs: a group of three and
            # a single one, whose merged weight is 0 (moments 0 / 0)
            c.maps["mean"][c.offs[0]:c.offs[0] + 3] = [(200.0, 200.0), (200.01, 200.0), (200.0, 200.01)]
            c.maps["mean"][c.offs[5]] = (-200.0, 200.0)
            return c
        # the state after a resample of this one: the parents of fixed uniforms
        c.maps["weight"] = _grid_weights(rng, len(mean))  # (every particle weighs the same afterwards)
        u = rng.uniform(size=n)
        par = weighting_ref.parents(c.lw, u)
        idx = par.parent
        assert len(set(idx)) < n
        m2 = np.concatenate([c.maps[c.offs[p]:c.offs[p + 1]] for p in idx])
        o2 = np.zeros(n + 1, np.int32)
        o2[1:] = np.cumsum(np.diff(c.offs)[idx])
        base = dict(lw=c.lw, maps=c.maps, offs=c.offs, u=u, parents=idx, near=int(par.near.sum()))
        return ECase(c.cfg, c.poses, np.full(n, np.float32(-np.log(float(n)))), m2, o2, c.cap, base)
    if name == "fallback":
        counts = [1100, 30, 7, 1]
        centres = [(0.0, 0.0), (12.0, 3.0), (-9.0, 14.0), (20.0, -20.0)]
        mean, cov, _ = _clusters(rng, centres, counts)
        mean[-1, 0] = np.nan  # a component without a position: the one-workgroup greedy
        return _assemble(rng, 8, _grid_weights(rng, len(mean)), mean, cov)
    if name == "single":
        return _assemble(rng, 1, [0.7], [[3.0, -4.0]], _spd(rng, 1, 0.05, 0.15, 30.0))
    if name == "empty":
        return _assemble(rng, 4, np.zeros(0), np.zeros((0, 2)), np.zeros((0, 4), np.float32))
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def eap_inputs(name):
    c = _eap_build(name)
    if isinstance(c.extra, dict):
        _freeze(tuple(c.extra.values()))
    return ECase(*_freeze(tuple(c)))


@functools.lru_cache(maxsize=None)
def eap_reference(name):
    """(records in emission order, near decisions, members absorbed by every seed)."""
    c = eap_inputs(name)
    groups = []
    out, near = R.expected_map(c.cfg.copy(), c.lw, c.maps, c.offs, groups)
    out.setflags(write=False)
    return out, near, tuple(groups)


def field_deviations(A, B):
    """Per-class worst deviations of two static maps in the same (emission)
    order; None when the sizes differ or a NaN faces a number."""
    if len(A) != len(B):
        return None
    out = dict(weight=U._rel(A["weight"], B["weight"], floor=1e-12), noncancel=0.0, cancel=0.0)
    if len(A) == 0:
        return out
    fa, fb = parity._fields(A), parity._fields(B)
    nan = np.isnan(fa)
    if not np.array_equal(nan, np.isnan(fb)):
        return None
    fa, fb = np.where(nan, 0.0, fa), np.where(nan, 0.0, fb)
    nc = (parity.noncancellation_mask(fa, fb) & ~nan)[:, 1:]
    fa, fb = fa[:, 1:], fb[:, 1:]
    sa = np.sqrt(np.abs(fa[:, 2] * fa[:, 5]))[:, None]
    ms = np.maximum(np.abs(fa[:, :2]).max(1, keepdims=True), 1.0)
    scale = np.concatenate([np.repeat(ms, 2, 1), np.repeat(sa, 4, 1)], 1)
    ref = np.maximum(np.abs(fa), np.abs(fb))
    d = np.abs(fa - fb)
    rel = np.where(d > 0, d / np.maximum(ref, 1e-300), 0.0)
    srel = np.where(d > 0, d / np.maximum(np.maximum(ref, scale), 1e-300), 0.0)
    out["noncancel"] = float(rel[nc].max()) if nc.any() else 0.0
    out["cancel"] = float(srel[~nc].max()) if (~nc).any() else 0.0
    return out


round_up = U.round_up
