"""Inputs, float64 reference results and measured oracle distances shared by
tests/test_update_ref64.py (CPU) and tests/test_gpu_ref64.py (device): each
case's scenario is built once, its reference (update_ref64.update) once, and
both are handed out unchanged.

TEST INFRASTRUCTURE ONLY.
"""
import functools

import numpy as np
from scipy.special import logsumexp

import parity
import update_ref64 as R

CASES = ("tiny", "phd_mid", "phd_wide", "phd_cut", "phd_fov", "phd_ragged", "phd_lowclutter", "phd_labeled",
         "cphd_small", "cphd_mid", "cphd_empty", "hell_mid")
CLASSES = ("weight", "noncancel", "cancel", "delta", "lognorm", "card")
CONTRACT = 1e-5

# name -> scenario seed (phdslam.config_scenario's default is SEED_BASE + config id);
# chosen so that the excluded share meets the caps below (test_update_ref64.py
# asserts them with the reference alone)
SEEDS = {}

# D_oracle(case, class): the worst deviation of the oracle (oracle/scphd_cpu.cpp;
# hell_mid: its candidates through hellinger_ref.greedy) from update_ref64 over
# the particles compared, measured on the CPU by deviations() below and rounded
# up to two significant figures.  test_update_ref64.py asserts the oracle stays
# within it; test_gpu_ref64.py holds the device to D_oracle + 1e-5.
D_ORACLE = {
    "tiny": dict(weight=1.4e-05, noncancel=2.8e-06, cancel=1.5e-06, delta=6.5e-06, lognorm=2.4e-06, card=0),
    "phd_mid": dict(weight=4.8e-05, noncancel=1.3e-05, cancel=6.7e-06, delta=6.7e-07, lognorm=4.4e-06, card=0),
    "phd_wide": dict(weight=0.00012, noncancel=1.7e-05, cancel=1.3e-05, delta=9.6e-07, lognorm=4.6e-05, card=0),
    "phd_cut": dict(weight=7.9e-05, noncancel=2.2e-05, cancel=1.3e-05, delta=1.6e-06, lognorm=7.2e-06, card=0),
    "phd_fov": dict(weight=4.2e-05, noncancel=5.4e-06, cancel=3.6e-06, delta=7.5e-07, lognorm=4.2e-06, card=0),
    "phd_ragged": dict(weight=4.2e-05, noncancel=5.2e-06, cancel=4.2e-06, delta=1.1e-06, lognorm=7.3e-06, card=0),
    "phd_lowclutter": dict(weight=3.9e-05, noncancel=5.5e-06, cancel=3e-06, delta=5.9e-07, lognorm=2.5e-06, card=0),
    "phd_labeled": dict(weight=4.8e-05, noncancel=1.3e-05, cancel=6.7e-06, delta=5e-07, lognorm=1.7e-06, card=0),
    "cphd_small": dict(weight=5.8e-05, noncancel=7.5e-06, cancel=4.6e-06, delta=9.7e-07, lognorm=1.1e-06, card=0),
    "cphd_mid": dict(weight=7.4e-05, noncancel=2.5e-05, cancel=2e-05, delta=0.00025, lognorm=3.3e-06, card=0),
    "cphd_empty": dict(weight=2.4e-05, noncancel=8.1e-07, cancel=4.5e-07, delta=2.3e-06, lognorm=0, card=0),
    "hell_mid": dict(weight=4.8e-05, noncancel=1.3e-05, cancel=3e-06, delta=6.7e-07, lognorm=4.4e-06, card=0),
}


def max_left_out(name):
    """Particles that may be left out whole (a near classification): 2 of 16, 1 of 4."""
    return 1 if name == "tiny" else 2


def _subset(maps, offs, sizes):
    from phdslam.types import csr_from_maps
    return csr_from_maps([maps[offs[p]:offs[p] + sizes[p]] for p in range(len(sizes))])


def _build(name):
    import phdslam
    seed = SEEDS.get(name)
    cs = lambda cid, n, G, M: phdslam.config_scenario(cid, n=n, G=G, M=M, seed=seed)  # noqa: E731
    if name == "tiny":
        return cs(2, 4, 3, 2)
    if name == "phd_mid":
        return cs(2, 16, 64, 16)
    if name == "phd_wide":
        return cs(2, 16, 200, 40)
    if name == "phd_cut":  # headings at +-pi, both signs; the scan turned with them
        c, poses, lw, maps, offs, z = cs(2, 16, 64, 16)
        th = poses["ptheta"].astype(np.float64) + np.pi
        poses["ptheta"] = R.wrap(th).astype(np.float32)
        z["bearing"] = R.wrap(z["bearing"].astype(np.float64) - np.pi).astype(np.float32)
        assert (poses["ptheta"] > 3).any() and (poses["ptheta"] < -3).any()
        return c, poses, lw, maps, offs, z
    if name == "phd_fov":
        c, poses, lw, maps, offs, z = cs(2, 16, 64, 16)
        c.maxBearing = 2.0
        c.minRange = 5.0
        c.update_clutter_density()
        return c, poses, lw, maps, offs, z
    if name == "phd_ragged":
        c, poses, lw, maps, offs, z = cs(2, 16, 64, 8)
        sizes = np.array([0, 1, 64, 0, 1, 64, 2, 3, 7, 13, 21, 31, 32, 33, 47, 63])
        maps, offs = _subset(maps, offs, sizes)
        return c, poses, lw, maps, offs, z
    if name == "phd_lowclutter":
        c, poses, lw, maps, offs, z = cs(2, 16, 64, 16)
        c.clutterRate = 0.0
        c.update_clutter_density()
        c.birthWeight = 1e-12
        return c, poses, lw, maps, offs, z
    if name == "phd_labeled":
        c, poses, lw, maps, offs, z = cs(2, 16, 64, 16)
        c.labeledMeasurements = True
        z["label"][::3] = 1
        return c, poses, lw, maps, offs, z
    if name in ("cphd_small", "cphd_mid"):
        c, poses, lw, maps, offs, z = cs(3, 16, 64, 8 if name == "cphd_small" else 16)
        c.maxCardinality = 127 if name == "cphd_small" else 300
        return c, poses, lw, maps, offs, z
    if name == "cphd_empty":
        c, poses, lw, maps, offs, z = cs(3, 16, 4, 4)
        c.maxCardinality = 127
        maps, offs = _subset(maps, offs, np.arange(16) % 2)
        return c, poses, lw, maps, offs, z
    if name == "hell_mid":
        c, poses, lw, maps, offs, z = cs(2, 16, 64, 16)
        c.distanceMetric = 1
        c.minSeparation = 0.7
        return c, poses, lw, maps, offs, z
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(cfg, poses, log-weights, maps, offsets, measurements), arrays read-only."""
    r = _build(name)
    for a in r[1:]:
        a.setflags(write=False)
    return r


def config(name):
    return inputs(name)[0].copy()


@functools.lru_cache(maxsize=None)
def reference(name):
    """update_ref64.update of the case (read-only arrays)."""
    cfg, poses, lw, maps, offs, z = inputs(name)
    r = R.update(config(name), poses, maps, offs, z)
    for a in r:
        if a is not None:
            a.setflags(write=False)
    return r


def shares(name):
    """(particles left out whole, particles with any near decision, particles)."""
    r = reference(name)
    return int(np.sum(r.cls > 0)), int(np.sum((r.cls > 0) | (r.pm > 0))), len(r.cls)


def normalised(lw, delta, keep):
    """lw + delta normalised by logsumexp over the particles kept, in float64."""
    v = np.asarray(lw, np.float64) + np.asarray(delta, np.float64)
    return v - logsumexp(v[keep])


def _rel(a, b, scale=None, floor=0.0):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    ref = np.maximum(np.abs(a), np.abs(b))
    if scale is not None:
        ref = np.maximum(ref, scale)
    d = np.abs(a - b)
    d = np.where(d <= floor, 0.0, d)
    return float(np.max(np.where(d > 0, d / np.maximum(ref, 1e-300), 0.0)))


def map_deviations(A, B):
    """Worst deviations of two matched maps per field class: weights (1e-12
    floor), non-cancellation entries per element (parity.noncancellation_mask),
    cancellation entries on compare_maps' scaled measure."""
    ia, ib = parity.match_maps(A, B)
    a, b = A[ia], B[ib]
    out = dict(weight=_rel(a["weight"], b["weight"], floor=1e-12), noncancel=0.0, cancel=0.0)
    if len(a) == 0:
        return out
    fa, fb = parity._fields(a)[:, 1:], parity._fields(b)[:, 1:]
    nc = parity.noncancellation_mask(parity._fields(a), parity._fields(b))[:, 1:]
    sa = np.sqrt(np.abs(a["cov"][:, 0] * a["cov"][:, 3])).astype(np.float64)[:, None]
    ms = np.maximum(np.abs(a["mean"]).max(1, keepdims=True), 1.0).astype(np.float64)
    scale = np.concatenate([np.repeat(ms, 2, 1), np.repeat(sa, 4, 1)], 1)
    ref = np.maximum(np.abs(fa), np.abs(fb))
    d = np.abs(fa - fb)
    rel = np.where(d > 0, d / np.maximum(ref, 1e-300), 0.0)
    srel = np.where(d > 0, d / np.maximum(np.maximum(ref, scale), 1e-300), 0.0)
    out["noncancel"] = float(rel[nc].max()) if nc.any() else 0.0
    out["cancel"] = float(srel[~nc].max()) if (~nc).any() else 0.0
    return out


def deviations(name, maps, offs, logw, lognorm, cn=None, tol=None):
    """Compare one implementation's result with the reference of the case.
    maps / offs: its posterior maps; logw: its lw + delta (not normalised);
    lognorm: the same normalised by its own normalise routine over every
    particle (when particles are left out, both sides are shifted to the
    logsumexp over the particles kept); cn: its log cardinality rows (CPHD).
    Particles with a near classification are left out; particles with a near prune / merge are compared component by
    component (parity.unmatched, at most 3 per near decision, at rtol tol["..."]
    or the contract's) and the others whole.  Returns (worst deviation per
    class, list of disagreements in sizes / decisions, particles compared)."""
    cfg, poses, lw, _, _, _ = inputs(name)
    ref = reference(name)
    n = len(poses)
    keep = ref.cls == 0
    worst = dict.fromkeys(CLASSES, 0.0)
    bad = []
    rt = CONTRACT if tol is None else max(tol["weight"], tol["noncancel"], tol["cancel"])
    for p in np.flatnonzero(keep):
        A = ref.maps[ref.offsets[p]:ref.offsets[p + 1]]
        B = maps[offs[p]:offs[p + 1]]
        if ref.pm[p] == 0:
            if len(A) != len(B):
                bad.append((int(p), "size", len(A), len(B)))
                continue
            for k, v in map_deviations(A, B).items():
                worst[k] = max(worst[k], v)
        else:
            ua, ub = parity.unmatched(A, B, rt)
            if max(ua, ub) > 3 * ref.pm[p]:
                bad.append((int(p), "near-threshold components", ua, ub, int(ref.pm[p])))
    lr = np.asarray(lw, np.float64) + ref.delta
    worst["delta"] = _rel(np.asarray(logw, np.float64)[keep] - np.asarray(lw, np.float64)[keep], ref.delta[keep])
    a = np.asarray(lognorm, np.float64)
    if not keep.all():
        a = a - logsumexp(a[keep])
    worst["lognorm"] = lognorm_deviation(a, lr - logsumexp(lr[keep]), keep)
    if cn is not None:
        g = np.asarray(cn, np.float64)[keep]
        r = ref.cn[keep]
        sig = r > -60.0  # probabilities above ~1e-26
        d = np.abs(g[sig] - r[sig])
        d = np.where(d <= 1e-4, 0.0, d)  # the absolute floor of the cardinality comparison
        worst["card"] = float(np.max(d / np.maximum(np.maximum(np.abs(g[sig]), np.abs(r[sig])), 1e-300))) if d.size else 0.0
        if not np.all(g[~sig] < -50.0):
            bad.append(("cardinality", "mass where the reference has none"))
    return worst, bad, int(keep.sum())


def lognorm_deviation(a, b, keep):
    """Worst |a - b| / max(|a|, |b|) of normalised log-weights beyond the 1e-5
    absolute floor (compared after normalisation)."""
    a, b = np.asarray(a, np.float64)[keep], np.asarray(b, np.float64)[keep]
    d = np.abs(a - b)
    d = np.where(d <= 1e-5, 0.0, d - 1e-5)
    return float(np.max(d / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300))) if d.size else 0.0


def round_up(x):
    """x rounded up to two significant figures."""
    if x <= 0:
        return 0.0
    e = int(np.floor(np.log10(x))) - 1
    return float(np.ceil(x / 10.0 ** e - 1e-9) * 10.0 ** e)
