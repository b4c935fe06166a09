"""Inputs, float64 reference results and measured oracle distances of the mixed
static + dynamic model, shared by tests/test_mixed_ref64.py (CPU) and
tests/test_gpu_mixed_ref64.py (device): each case's scenario is built once,
its reference (mixed_ref64) once, and both are handed out unchanged.

TEST INFRASTRUCTURE ONLY.
"""
import collections
import functools

import numpy as np
from scipy.optimize import linear_sum_assignment
from scipy.special import logsumexp

import mixed_ref64 as R
import parity
import update_ref64_cases as U

CASES = ("mx_tiny", "mx_mid", "mx_unlabelled", "mx_chunks", "mx_manyz", "mx_cut", "mx_fov", "mx_ragged",
         "mx_predicted", "mx_cluster", "mx_ties", "mx_noscan")
CLASSES = ("weight_s", "weight_d", "noncancel", "cancel", "delta", "lognorm")
PREDICT_CASES = ("pred_dt0.1", "pred_dt1.0")
EAP_CASES = tuple(f"eap_{c}_{w}" for c in ("mx_mid", "mx_predicted", "mx_cluster") for w in ("in", "post"))
FIELDS = ("weight", "mean", "cov")
CONTRACT = 1e-5

Case = collections.namedtuple("Case", "cfg poses lw smaps soffs dmaps doffs z caps")

# name -> seed of phdslam.scenario.mixed_scenario (default SEED_BASE + 100), chosen so
# that the excluded share meets the caps (test_mixed_ref64.py asserts them with
# the reference alone)
SEEDS = {"mx_manyz": 5, "mx_predicted": 4, "mx_cluster": 3}

# device capacities of a case: map, dynamic map, measurements, candidates
_SMALL = dict(cap=128, dcap=64, M=32, K=4096)
_LARGE = dict(cap=512, dcap=320, M=32, K=4096)

# D_oracle(case, class): the worst deviation of the oracle (orc_update_mixed /
# orc_predict_dynamic / orc_expected_map_dynamic) from mixed_ref64 over the
# particles compared, measured on the CPU by deviations() / field_deviations()
# and rounded up to two significant figures.  test_mixed_ref64.py asserts the
# oracle stays within it; test_gpu_mixed_ref64.py holds the device to
# D_oracle + 1e-5.
D_ORACLE = {
    "mx_tiny": dict(weight_s=9.7e-08, weight_d=4.7e-08, noncancel=5.8e-07, cancel=3.4e-07, delta=2e-07, lognorm=0),
    "mx_mid": dict(weight_s=1.4e-05, weight_d=4.3e-06, noncancel=3.4e-06, cancel=1.6e-06, delta=3.4e-07, lognorm=6.7e-07),
    "mx_unlabelled": dict(weight_s=1.4e-05, weight_d=1.3e-05, noncancel=3.5e-06, cancel=1.6e-06, delta=3.4e-07, lognorm=7.9e-07),
    "mx_chunks": dict(weight_s=5.7e-06, weight_d=1.4e-05, noncancel=1.1e-06, cancel=3.3e-07, delta=6.6e-08, lognorm=1.2e-07),
    "mx_manyz": dict(weight_s=1.1e-05, weight_d=1.1e-05, noncancel=1.7e-06, cancel=1.7e-06, delta=9.2e-07, lognorm=4.4e-05),
    "mx_cut": dict(weight_s=1.7e-05, weight_d=6.1e-06, noncancel=7.4e-06, cancel=2.8e-06, delta=6.9e-07, lognorm=3.4e-06),
    "mx_fov": dict(weight_s=5.9e-07, weight_d=4.7e-06, noncancel=1.7e-06, cancel=7.1e-07, delta=2.4e-07, lognorm=0),
    "mx_ragged": dict(weight_s=3.4e-05, weight_d=4.3e-06, noncancel=2.9e-06, cancel=1.2e-06, delta=4.5e-07, lognorm=1.2e-06),
    "mx_predicted": dict(weight_s=1.5e-05, weight_d=1.1e-05, noncancel=2.9e-06, cancel=2.1e-06, delta=5.1e-07, lognorm=1.1e-06),
    "mx_cluster": dict(weight_s=6.3e-06, weight_d=1.9e-06, noncancel=2.4e-06, cancel=1.5e-06, delta=9.6e-08, lognorm=1.7e-06),
    "mx_ties": dict(weight_s=1.4e-05, weight_d=6.6e-06, noncancel=8.7e-06, cancel=2e-06, delta=8.1e-07, lognorm=7.4e-07),
    "mx_noscan": dict(weight_s=0, weight_d=0, noncancel=0, cancel=0, delta=0, lognorm=0),
    "pred_dt0.1": dict(weight=2.6e-07, noncancel=1.3e-07, cancel=1.3e-08),
    "pred_dt1.0": dict(weight=2.6e-07, noncancel=9.3e-08, cancel=7.1e-08),
    "eap_mx_mid_in": dict(weight=1.7e-07, noncancel=3.2e-07, cancel=1.1e-08),
    "eap_mx_mid_post": dict(weight=1.4e-07, noncancel=3.8e-07, cancel=4.4e-08),
    "eap_mx_predicted_in": dict(weight=1.2e-07, noncancel=2.5e-07, cancel=9.4e-08),
    "eap_mx_predicted_post": dict(weight=2.4e-07, noncancel=4.1e-07, cancel=9.4e-08),
    "eap_mx_cluster_in": dict(weight=3.4e-07, noncancel=1.1e-06, cancel=2.5e-08),
    "eap_mx_cluster_post": dict(weight=1.1e-07, noncancel=2e-07, cancel=6.3e-09),
}


def max_left_out(name):
    """Particles that may be left out whole (a near classification): 2 of 16, 1 of 2, 4 or 8."""
    return 2 if len(inputs(name).poses) >= 16 else 1


def _subset(maps, offs, sizes):
    parts = [maps[offs[p]:offs[p] + sizes[p]] for p in range(len(sizes))]
    o = np.zeros(len(sizes) + 1, np.int32)
    o[1:] = np.cumsum(sizes)
    return np.ascontiguousarray(np.concatenate(parts)), o


def to32(rec, maps):
    """float64 records -> the project's float32 records."""
    out = np.zeros(len(maps), rec)
    for f in FIELDS:
        out[f] = maps[f]
    return out


def _clear_chains(cfg, poses, sm, so, dm, do, n_chains=2, step=0.7):
    """(range, bearing) of n_chains radial chains of three measurements `step`
    apart, each so far from every component of every particle that its
    likelihood terms vanish beside kappa + 2 beta in float64 and in float32
    (sum of q below 1e-20): the birth weights of the six are then equal
    exactly.  Neighbours of a chain merge (d^2 = step^2 / (1.5 stdRange)^2 =
    2.4 < 4), its ends do not (9.7)."""
    from phdslam.types import MEASUREMENT
    found = []
    ok = np.ones(1, bool)
    for b in np.linspace(-3.0, 3.0, 241):
        for r0 in np.arange(4.0, float(cfg.maxRange) - 2 * step - 0.5, 0.5):
            if any(abs(b - fb) < 0.5 for _, fb in found):
                continue
            worst = -np.inf
            for k in range(3):
                z = np.zeros(1, MEASUREMENT)
                z["range"], z["bearing"] = r0 + k * step, b
                for p in range(len(poses)):
                    for comps, D in ((sm[so[p]:so[p + 1]], 2), (dm[do[p]:do[p + 1]], 4)):
                        lq = R._map_terms(cfg, poses[p], comps, z, ok, D, D == 2)["logq"]
                        if lq.size:
                            worst = max(worst, float(lq.max()))
                if worst > -50.0:
                    break
            if worst <= -50.0:
                found.append((r0, b))
                if len(found) == n_chains:
                    return [(r0 + k * step, b) for r0, b in found for k in range(3)]
    raise AssertionError("no clear chain found")


def _build(name):
    from phdslam.scenario import mixed_config, mixed_scenario
    seed = SEEDS.get(name)
    kw = {} if seed is None else dict(seed=seed)
    caps = dict(_SMALL)

    def ms(n, Gs, Gd, M, **cfgkw):
        cfg = mixed_config(**cfgkw)
        return (cfg,) + mixed_scenario(cfg, n, Gs, Gd, M, **kw)

    if name == "mx_tiny":
        cfg, poses, sm, so, dm, do, z = ms(4, 3, 2, 2)
    elif name in ("mx_mid", "mx_noscan"):
        cfg, poses, sm, so, dm, do, z = ms(16, 40, 16, 12)
        if name == "mx_noscan":
            z = z[:0]
    elif name == "mx_unlabelled":
        cfg, poses, sm, so, dm, do, z = ms(16, 40, 16, 12, labeledMeasurements=False)
    elif name == "mx_chunks":
        cfg, poses, sm, so, dm, do, z = ms(4, 300, 257, 4)
        sm, so = _subset(sm, so, [255, 256, 257, 300])
        dm, do = _subset(dm, do, [63, 64, 65, 257])
        caps = dict(_LARGE)
    elif name == "mx_manyz":
        cfg, poses, sm, so, dm, do, z = ms(2, 8, 4, 257)
        caps = dict(_LARGE, M=256)
    elif name == "mx_cut":  # headings at +-pi, both signs; the scan turned with them
        cfg, poses, sm, so, dm, do, z = ms(16, 40, 16, 12)
        poses["ptheta"] = R.wrap(poses["ptheta"].astype(np.float64) + np.pi).astype(np.float32)
        z["bearing"] = R.wrap(z["bearing"].astype(np.float64) - np.pi).astype(np.float32)
        assert (poses["ptheta"] > 3).any() and (poses["ptheta"] < -3).any()
    elif name == "mx_fov":
        cfg, poses, sm, so, dm, do, z = ms(16, 40, 16, 12)
        cfg.maxBearing = 2.0
        cfg.minRange = 5.0
        cfg.update_clutter_density()
    elif name == "mx_ragged":
        cfg, poses, sm, so, dm, do, z = ms(16, 40, 16, 12)
        sm, so = _subset(sm, so, [0, 1, 2, 3, 7, 13, 21, 31, 32, 33, 40, 0, 1, 40, 5, 11])
        dm, do = _subset(dm, do, [16, 0, 1, 2, 3, 5, 8, 13, 15, 16, 7, 0, 16, 1, 4, 9])
    elif name == "mx_predicted":
        from phdslam.types import GAUSSIAN4D
        cfg, poses, sm, so, dm, do, z = ms(16, 40, 16, 12, dt=0.5)
        rng = np.random.default_rng(4242 if seed is None else seed)
        speed = rng.uniform(0.0, 2.0 * float(cfg.tau), len(dm))
        ang = rng.uniform(-np.pi, np.pi, len(dm))
        dm["mean"][:, 2], dm["mean"][:, 3] = speed * np.cos(ang), speed * np.sin(ang)
        for _ in range(3):
            dm = to32(GAUSSIAN4D, R.predict(cfg, dm))
    elif name == "mx_cluster":
        cfg, poses, sm, so, dm, do, z = ms(8, 260, 210, 6)
        rng = np.random.default_rng(99 if seed is None else seed)
        cs = np.array([[8.0, 3.0], [-6.0, -9.0]])
        cd = np.array([[3.0, -10.0, 1.0, 0.5], [-11.0, 5.0, -0.8, 1.2], [12.0, -4.0, 0.3, -1.0]])
        sm["mean"] = np.repeat(cs, 130, 0)[np.arange(len(sm)) % 260] + rng.normal(0, 0.05, (len(sm), 2))
        dm["mean"] = np.repeat(cd, 70, 0)[np.arange(len(dm)) % 210] + rng.normal(0, 0.05, (len(dm), 4))
        for k, (c, lab) in enumerate([(cs[0], 0), (cs[1], 0), (cd[0], 1), (cd[1], 1), (cd[2], 1)]):
            z[k]["range"] = np.hypot(c[0], c[1]) + rng.normal(0, 0.1)
            z[k]["bearing"] = np.arctan2(c[1], c[0]) + rng.normal(0, 0.01)
            z[k]["label"] = lab
        caps = dict(_LARGE)
    elif name == "mx_ties":
        cfg, poses, sm, so, dm, do, z = ms(16, 12, 6, 10, labeledMeasurements=False)
        for k, (r, b) in enumerate(_clear_chains(cfg, poses, sm, so, dm, do)):
            z[4 + k]["range"], z[4 + k]["bearing"] = r, b
    else:
        raise KeyError(name)
    n = len(poses)
    lw = np.log(np.random.default_rng(5).dirichlet(np.ones(n) * 4)).astype(np.float32)
    return Case(cfg, poses, lw, sm, so.astype(np.int32), dm, do.astype(np.int32), z, caps)


def _freeze(t):
    for a in t:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return t


@functools.lru_cache(maxsize=None)
def inputs(name):
    """Case(cfg, poses, log-weights, static maps, offsets, dynamic maps, offsets,
    measurements, device capacities), arrays read-only."""
    return _freeze(_build(name))


def config(name):
    return inputs(name).cfg.copy()


@functools.lru_cache(maxsize=None)
def _reference(name):
    c = inputs(name)
    counts = []
    r = R.update(config(name), c.poses, c.smaps, c.soffs, c.dmaps, c.doffs, c.z, counts)
    k = np.array(counts, np.int64).reshape(-1, 6)
    return _freeze(r), _freeze((k,))[0]


def reference(name):
    """mixed_ref64.update of the case (read-only arrays)."""
    return _reference(name)[0]


def candidate_counts(name):
    """(n, 2): the reference's static and dynamic candidate counts after the prune."""
    return _reference(name)[1][:, :2]


def merge_shape(name):
    """((n, 2) members of the widest merge set per map, (n, 2) the widest span of
    candidate indices within one merge set), from the reference."""
    k = _reference(name)[1]
    return k[:, 2:4], k[:, 4:6]


def shares(name):
    """(particles left out whole, particles with any near decision, particles)."""
    r = reference(name)
    return int(np.sum(r.cls > 0)), int(np.sum((r.cls > 0) | (r.pm > 0))), len(r.cls)


# ---- comparison -------------------------------------------------------

_DIAG4 = np.zeros(16, bool)
_DIAG4[[0, 5, 10, 15]] = True


def match4(A, B):
    """Match two dynamic maps as multisets (index arrays), as parity.match_maps."""
    if len(A) != len(B):
        raise AssertionError(f"map sizes differ: {len(A)} vs {len(B)}")
    if len(A) == 0:
        return np.zeros(0, int), np.zeros(0, int)
    ia = np.lexsort((A["weight"], A["mean"][:, 1], A["mean"][:, 0]))
    ib = np.lexsort((B["weight"], B["mean"][:, 1], B["mean"][:, 0]))
    fa, fb = parity._fields(A[ia]), parity._fields(B[ib])
    scale = np.maximum(np.maximum(np.abs(fa), np.abs(fb)), 1e-3)
    if np.all(np.abs(fa - fb) <= 1e-4 * scale):
        return ia, ib
    ma, mb = A["mean"].astype(np.float64), B["mean"].astype(np.float64)
    cost = np.sum((ma[:, None, :] - mb[None, :, :]) ** 2, -1)
    cost += (np.log(np.maximum(A["weight"], 1e-30))[:, None].astype(np.float64)
             - np.log(np.maximum(B["weight"], 1e-30))[None, :].astype(np.float64)) ** 2
    return linear_sum_assignment(cost)


def _scales4(a):
    ms = np.maximum(np.abs(a["mean"]).max(1, keepdims=True), 1.0).astype(np.float64)
    cs = np.abs(a["cov"]).max(1, keepdims=True).astype(np.float64)
    return ms, cs


def ordered_deviations4(a, b):
    """Two dynamic maps in the same order: weights (1e-12 floor), non-cancellation
    entries per element (covariance diagonals, mean coordinates with |x| >= 1),
    the other entries on test_gpu_mixed._cmp4's scaled measure."""
    out = dict(weight=U._rel(a["weight"], b["weight"], floor=1e-12), noncancel=0.0, cancel=0.0)
    if len(a) == 0:
        return out
    fa = np.concatenate([a["mean"], a["cov"]], 1).astype(np.float64)
    fb = np.concatenate([b["mean"], b["cov"]], 1).astype(np.float64)
    ref = np.maximum(np.abs(fa), np.abs(fb))
    nc = np.concatenate([ref[:, :4] >= 1.0, np.broadcast_to(_DIAG4, (len(a), 16))], 1)
    ms, cs = _scales4(a)
    scale = np.concatenate([np.repeat(ms, 4, 1), np.repeat(cs, 16, 1)], 1)
    d = np.abs(fa - fb)
    rel = np.where(d > 0, d / np.maximum(ref, 1e-300), 0.0)
    srel = np.where(d > 0, d / np.maximum(np.maximum(ref, scale), 1e-300), 0.0)
    out["noncancel"] = float(rel[nc].max()) if nc.any() else 0.0
    out["cancel"] = float(srel[~nc].max()) if (~nc).any() else 0.0
    return out


def map_deviations4(A, B):
    ia, ib = match4(A, B)
    return ordered_deviations4(A[ia], B[ib])


def unmatched4(A, B, rtol):
    """parity.unmatched for dynamic maps, on _cmp4's scales."""
    if len(A) == 0 or len(B) == 0:
        return len(A), len(B)
    wb, mb, cb = (B[f].astype(np.float64) for f in FIELDS)
    used = np.zeros(len(B), bool)
    miss = 0
    for i in range(len(A)):
        wa, ma, ca = (np.float64(A[f][i]) for f in FIELDS)
        ms, cs = max(np.abs(ma).max(), 1.0), np.abs(ca).max()
        ok = (~used & (np.abs(wb - wa) <= rtol * np.maximum(np.abs(wb), abs(wa)) + 1e-12)
              & np.all(np.abs(mb - ma) <= rtol * np.maximum(np.maximum(np.abs(mb), np.abs(ma)), ms), 1)
              & np.all(np.abs(cb - ca) <= 5 * rtol * np.maximum(np.maximum(np.abs(cb), np.abs(ca)), cs) + 1e-30, 1))
        j = np.flatnonzero(ok)
        if len(j):
            used[j[0]] = True
        else:
            miss += 1
    return miss, int((~used).sum())


def deviations(name, smaps, soffs, dmaps, doffs, logw, lognorm, tol=None, skip=()):
    """Compare one implementation's result with the reference of the case.
    smaps / soffs, dmaps / doffs: its posterior maps; logw: its lw + delta (not
    normalised); lognorm: the same normalised by its own normalise routine over
    every particle (when particles are left out, both sides are shifted to the
    logsumexp over the particles kept).  Particles with a near classification
    (and those of `skip`) are left out; particles with a near prune / merge of a
    map have that map compared component by component (at most 3 unmatched per
    near decision, at rtol max(tol) or the contract's) and the others whole.
    Returns (worst deviation per class, disagreements in sizes / decisions,
    particles compared)."""
    c = inputs(name)
    ref = reference(name)
    keep = ref.cls == 0
    keep[list(skip)] = False
    worst = dict.fromkeys(CLASSES, 0.0)
    bad = []
    rt = CONTRACT if tol is None else max(tol["weight_s"], tol["weight_d"], tol["noncancel"], tol["cancel"])
    for p in np.flatnonzero(keep):
        for m, (A, B, dev, unm) in enumerate((
                (ref.smaps[ref.soffs[p]:ref.soffs[p + 1]], smaps[soffs[p]:soffs[p + 1]], U.map_deviations,
                 parity.unmatched),
                (ref.dmaps[ref.doffs[p]:ref.doffs[p + 1]], dmaps[doffs[p]:doffs[p + 1]], map_deviations4, unmatched4))):
            which = "static" if m == 0 else "dynamic"
            if ref.pm2[p, m] == 0:
                if len(A) != len(B):
                    bad.append((int(p), which, "size", len(A), len(B)))
                    continue
                v = dev(A, B)
                worst["weight_s" if m == 0 else "weight_d"] = max(worst["weight_s" if m == 0 else "weight_d"], v["weight"])
                worst["noncancel"] = max(worst["noncancel"], v["noncancel"])
                worst["cancel"] = max(worst["cancel"], v["cancel"])
            else:
                ua, ub = unm(A, B, rt)
                if max(ua, ub) > 3 * ref.pm2[p, m]:
                    bad.append((int(p), which, "near-threshold components", ua, ub, int(ref.pm2[p, m])))
    lw = np.asarray(c.lw, np.float64)
    worst["delta"] = U._rel(np.asarray(logw, np.float64)[keep] - lw[keep], ref.delta[keep])
    lr = lw + ref.delta
    a = np.asarray(lognorm, np.float64)
    if not keep.all():
        a = a - logsumexp(a[keep])
    worst["lognorm"] = U.lognorm_deviation(a, lr - logsumexp(lr[keep]), keep)
    return worst, bad, int(keep.sum())


# ---- predict ----------------------------------------------------------

@functools.lru_cache(maxsize=None)
def predict_inputs(name):
    """(cfg, poses, static maps, offsets, dynamic maps, offsets, dcap): three
    particles with 0, 1 and dcap dynamic components, speeds 0 .. 2 tau, one of
    them tau exactly."""
    from phdslam.scenario import mixed_config, mixed_scenario
    dcap = 64
    cfg = mixed_config(dt=float(name[len("pred_dt"):]))
    poses, sm, so, dm, do, z = mixed_scenario(cfg, 3, 2, dcap, 2, seed=31)
    dm, do = _subset(dm, do, [0, 1, dcap])
    tau = float(cfg.tau)
    speed = np.linspace(0.0, 2.0 * tau, len(dm))
    ang = np.linspace(-3.0, 3.0, len(dm))
    dm["mean"][:, 2], dm["mean"][:, 3] = speed * np.cos(ang), speed * np.sin(ang)
    dm["mean"][7, 2:] = (tau, 0.0)
    dm["mean"][8, 2:] = (0.0, 0.0)
    assert dm["mean"][7, 2] == np.float32(tau)
    return _freeze((cfg, poses, sm, so, dm, do.astype(np.int32), dcap))


@functools.lru_cache(maxsize=None)
def predict_reference(name):
    cfg, _, _, _, dm, _, _ = predict_inputs(name)
    return _freeze((R.predict(cfg.copy(), dm),))[0]


def field_deviations(A, B):
    """Per-field worst deviations of two dynamic maps in the same order."""
    if len(A) != len(B):
        return None
    v = ordered_deviations4(A, B)
    return dict(weight=v["weight"], noncancel=v["noncancel"], cancel=v["cancel"])


FIELD_CLASSES = ("weight", "noncancel", "cancel")


# ---- EAP --------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def eap_inputs(name):
    """(cfg, poses, log-weights, static maps, offsets, dynamic maps, offsets,
    dcap): the dynamic maps of a case as loaded, or its reference posterior
    (float32 records) with the reference's normalised log-weights."""
    from phdslam.types import GAUSSIAN4D
    case, which = name[len("eap_"):].rsplit("_", 1)
    c = inputs(case)
    if which == "in":
        lw = c.lw.astype(np.float64)
        dm, do = c.dmaps, c.doffs
    else:
        r = reference(case)
        lw = c.lw.astype(np.float64) + r.delta
        dm, do = to32(GAUSSIAN4D, r.dmaps), r.doffs.astype(np.int32)
    lw = (lw - logsumexp(lw)).astype(np.float32)
    return _freeze((c.cfg, c.poses, lw, c.smaps, c.soffs, dm, do, c.caps))


@functools.lru_cache(maxsize=None)
def eap_reference(name):
    """(records in emission order, near decisions)."""
    cfg, _, lw, _, _, dm, do, _ = eap_inputs(name)
    out, near = R.expected_map(cfg.copy(), lw, dm, do)
    out.setflags(write=False)
    return out, near


round_up = U.round_up
