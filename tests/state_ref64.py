"""What enters and leaves a static step, in float64, from the model: the pose
prediction (Ackerman and constant velocity), the
device-noise contract ("RNG" row of its deviations table), the
n_predict_particles expansion, the expected pose with the MAP index, the
per-particle cardinalities and the static EAP map (every
particle's map with its weights scaled by the particle weight, reduced by the
greedy merge of Appendix A.4 over the concatenation).

Written from those statements and from neither implementation's instruction
order, with update_ref64's rules:

  * no import of pyoracle, no routine of include/phd_detmath.h or
    include/phd_rng.h (Philox is weighting_ref's, pinned to the Random123
    known answers);
  * every input is converted to float64 on entry, no float32 intermediate
    except where the contract itself rounds (the noise handed to the model);
  * quotients stay quotients: a / b, np.linalg.solve on the 2 x 2.

Layout: a covariance is stored cov[0..3] column-major, (P00, P10, P01, P11).

Near decisions of the EAP map follow update_ref64: a merge distance d is near
its threshold T = minSeparation when

    |d - T| <= max(NEAR * T, C * bound(d)),       NEAR = 1e-4, C = 2,

bound(d) a first-order float32 forward-error bound of d = D' S^-1 D,
D = a - b, S = (A + B) / 2, from EXACT float32 inputs (the maps as loaded),
eps = 2^-24 per rounding, g = S^-1 D:

  the mean difference: one subtraction per coordinate, delta_D_k = eps |D_k|,
    and d moves by 2 |g| . delta_D;
  the averaged covariance: one sum per entry (the halving is exact),
    delta_S_ij = eps |S_ij|, and d moves by |g|' |delta_S| |g|;
  the factorisation and the substitution (two roots, three quotients, a
    product and a difference, two squares and a sum): each rounds relative to
    its operands, never to the determinant, so the difference s11 - l10^2
    carries eps s11 against a value of det / s00 — an amplification of
    s00 s11 / det <= (1 + kappa)^2 / (4 kappa) <= kappa, kappa = lambda_max /
    lambda_min of S: 8 eps kappa d.

  bound(d) = 2 eps |g| . |D| + eps |g|' |S| |g| + 8 eps kappa(S) d.

A weight gap between neighbours of the priority order that is not 0 and at
most 1e-6 of the weight is one near decision when the order can matter: the
two would absorb each other, or a common third component (as update_ref64
counts merge ties).  Weights that are EQUAL are not near: the lower
concatenation index goes first in every precision.

TEST INFRASTRUCTURE ONLY.
"""
import numpy as np

import weighting_ref
from update_ref64 import C, EPS32, G64, NEAR, _flat, _mat, wrap  # noqa: F401

STREAM_PREDICT = 0x50524544  # 'PRED'
POSE_FIELDS = ("px", "py", "ptheta", "vx", "vy", "vtheta")
POSE64 = np.dtype([(k, np.float64) for k in POSE_FIELDS])
ACKERMAN_NOISE32 = np.dtype([("n_alpha", np.float32), ("n_encoder", np.float32)])
CV_NOISE32 = np.dtype([("ax", np.float32), ("ay", np.float32), ("atheta", np.float32)])
WEIGHT_GAP = 1e-6


def _f(x, k):
    return np.asarray(x[k], np.float64)


def _dt(cfg):
    sub = int(cfg.subdividePredict)
    return float(cfg.dt) / (sub if sub > 0 else 1)


# ---- pose prediction -----------------------------------------------------

def predict_ackerman(cfg, poses, v_encoder, alpha, noise):
    """SURVEY A.1, one pose per noise entry: ve = v + n_enc, al = alpha + n_alpha,
    vc = ve / (1 - tan(al) h / l) (the encoder sits h beside the axle centre),
    heading rate vc tan(al) / l, the sensor a ahead and b beside the axle:
    x' = x + Dt (vc cos th - rate (a sin th + b cos th)),
    y' = y + Dt (vc sin th + rate (a cos th - b sin th)), th' = wrap(th + Dt rate),
    Dt = dt / subdivide; the velocities are zeroed."""
    l, h, a, b = float(cfg.l), float(cfg.h), float(cfg.a), float(cfg.b)
    dt = _dt(cfg)
    ve = float(v_encoder) + _f(noise, "n_encoder")
    ta = np.tan(float(alpha) + _f(noise, "n_alpha"))
    vc = ve / (1.0 - ta * h / l)
    rate = vc * ta / l
    x, y, th = _f(poses, "px"), _f(poses, "py"), _f(poses, "ptheta")
    s, c = np.sin(th), np.cos(th)
    out = np.zeros(len(ve), POSE64)
    out["px"] = x + dt * (vc * c - rate * (a * s + b * c))
    out["py"] = y + dt * (vc * s + rate * (a * c - b * s))
    out["ptheta"] = wrap(th + dt * rate)
    return out


def predict_cv(cfg, poses, noise):
    """The constant-velocity step: the body-frame velocity (vx, vy) and the
    body-frame acceleration noise rotated by the heading, x' = x + Dt R v +
    Dt^2 / 2 R a, th' = wrap(th + Dt vth + Dt^2 / 2 ath), v' = v + Dt a."""
    dt = _dt(cfg)
    x, y, th = _f(poses, "px"), _f(poses, "py"), _f(poses, "ptheta")
    vx, vy, vth = _f(poses, "vx"), _f(poses, "vy"), _f(poses, "vtheta")
    ax, ay, ath = _f(noise, "ax"), _f(noise, "ay"), _f(noise, "atheta")
    s, c = np.sin(th), np.cos(th)
    out = np.zeros(len(ax), POSE64)
    out["px"] = x + dt * (vx * c - vy * s) + 0.5 * dt * dt * (ax * c - ay * s)
    out["py"] = y + dt * (vx * s + vy * c) + 0.5 * dt * dt * (ax * s + ay * c)
    out["ptheta"] = wrap(th + dt * vth + 0.5 * dt * dt * ath)
    out["vx"] = vx + dt * ax
    out["vy"] = vy + dt * ay
    out["vtheta"] = vth + dt * ath
    return out


def _normals(seed, ids, step):
    """Four standard normals per id.  The contract: Philox4x32-10 with key
    (seed low word, seed high word) and counter (global particle id, step low
    word, step high word, stream 'PRED'); its output words (x0, x1) and (x2, x3)
    each give two normals by Box-Muller with u1 = (a + 1) 2^-32 in (0, 1] and
    u2 = b 2^-32 in [0, 1): sqrt(-2 ln u1) (cos, sin)(2 pi u2)."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    ids = np.asarray(ids, np.uint64)
    x = weighting_ref.philox4x32_10([ids, step & 0xFFFFFFFF, step >> 32, STREAM_PREDICT],
                                    [seed & 0xFFFFFFFF, seed >> 32])
    out = []
    for a, b in ((x[0], x[1]), (x[2], x[3])):
        u1 = (a.astype(np.float64) + 1.0) * 2.0 ** -32
        u2 = b.astype(np.float64) * 2.0 ** -32
        rad = np.sqrt(-2.0 * np.log(u1))
        out += [rad * np.cos(2.0 * np.pi * u2), rad * np.sin(2.0 * np.pi * u2)]
    return out


def noise_ackerman(cfg, seed, ids, step):
    """The device-noise contract of the Ackerman model: the first normal times
    stdAlpha is the steering noise, the second times stdEncoder the encoder
    noise (_normals has the draw), each rounded to float32 once, where the noise
    is handed to the model."""
    g = _normals(seed, ids, step)
    out = np.zeros(len(g[0]), ACKERMAN_NOISE32)
    out["n_alpha"] = (float(cfg.stdAlpha) * g[0]).astype(np.float32)
    out["n_encoder"] = (float(cfg.stdEncoder) * g[1]).astype(np.float32)
    return out


def noise_cv(cfg, seed, ids, step):
    """The device-noise contract of the constant-velocity model: the first three
    normals times 3 ax, 3 ay, 3 ayaw, each rounded to float32 once."""
    g = _normals(seed, ids, step)
    out = np.zeros(len(g[0]), CV_NOISE32)
    out["ax"] = (3.0 * float(cfg.ax) * g[0]).astype(np.float32)
    out["ay"] = (3.0 * float(cfg.ay) * g[1]).astype(np.float32)
    out["atheta"] = (3.0 * float(cfg.ayaw) * g[2]).astype(np.float32)
    return out


def expand(poses, lw, npp, index_offset=0):
    """n_predict_particles: parent i has the children i npp .. i npp + npp - 1,
    each with its pose and the weight w_i - log npp.  Returns (child poses,
    child log-weights, parent of every child, global noise id of every child:
    its own index plus the index offset)."""
    npp = max(1, int(npp))
    parent = np.repeat(np.arange(len(lw)), npp)
    w = np.asarray(lw, np.float64)[parent] - np.log(float(npp))
    return poses[parent], w, parent, np.arange(len(parent), dtype=np.int64) + int(index_offset)


# ---- estimates -----------------------------------------------------------

def expected_pose(lw, poses):
    """(sum over particles of exp(w_i) state_i per field, the first index of the maximum log-weight)."""
    w = np.asarray(lw, np.float64)
    e = np.exp(w)
    out = np.zeros((), POSE64)
    for k in POSE_FIELDS:
        out[k] = np.sum(e * _f(poses, k))
    return out, int(np.argmax(w))


def cardinalities(maps, offs):
    """The sum of the component weights of every particle."""
    w = maps["weight"].astype(np.float64)
    return np.array([np.sum(w[offs[p]:offs[p + 1]]) for p in range(len(offs) - 1)], np.float64)


def _kappa(S):
    h = 0.5 * (S[..., 0, 0] + S[..., 1, 1])
    q = 0.5 * (S[..., 0, 0] - S[..., 1, 1])
    rt = np.sqrt(q * q + S[..., 0, 1] * S[..., 1, 0])
    with np.errstate(all="ignore"):
        return (h + rt) / (h - rt)


def distance(am, ac, bm, bc):
    """d = (a - b)' ((A + B) / 2)^-1 (a - b) of a seed against candidates, by
    np.linalg.solve, and its float32 bound (module text)."""
    am, bm = np.asarray(am, np.float64), np.asarray(bm, np.float64)
    D = am - bm
    S = (_mat(ac) + _mat(bc)) / 2
    with np.errstate(all="ignore"):
        g = np.linalg.solve(S, D[..., None])[..., 0]
        d = np.sum(D * g, -1)
        ag = np.abs(g)
        bound = EPS32 * (2 * np.sum(ag * np.abs(D), -1) + np.einsum("...i,...ij,...j->...", ag, np.abs(S), ag)
                         + 8 * _kappa(S) * np.abs(d))
    return d, bound


def expected_map(cfg, lw, maps, offs, groups=None):
    """The EAP map: component weights times exp(log w_n), a stable descending
    order, every seed absorbs each later unmerged component with d <
    minSeparation; the merged mean first, then the covariance about it.  A
    component with a non-finite mean has no distance to anything: it merges
    with nothing.  A merged weight of 0 leaves 0 / 0 = NaN moments.  Returns
    (G64 records in emission order, near decisions); groups: a list that
    receives the number of members every seed absorbed."""
    T = float(cfg.minSeparation)
    n = len(lw)
    offs = np.asarray(offs, np.int64)
    lo, hi = int(offs[0]), int(offs[n])
    ew = np.repeat(np.exp(np.asarray(lw, np.float64)), np.diff(offs))
    w = maps["weight"][lo:hi].astype(np.float64) * ew
    m = maps["mean"][lo:hi].astype(np.float64).reshape(-1, 2)
    c = maps["cov"][lo:hi].astype(np.float64).reshape(-1, 4)
    order = np.argsort(-w, kind="stable")
    near = 0
    ws = w[order]
    gap = ws[:-1] - ws[1:]
    for k in np.flatnonzero((gap > 0) & (gap <= WEIGHT_GAP * ws[:-1])):
        a, b = order[k], order[k + 1]
        with np.errstate(invalid="ignore"):
            da = distance(m[a], c[a], m, c)[0] < T
            db = distance(m[b], c[b], m, c)[0] < T
        near += int(da[b] or db[a] or np.any(da & db))
    used = np.zeros(len(w), bool)
    out = []
    for oi, a in enumerate(order):
        if used[a]:
            continue
        used[a] = True
        later = order[oi + 1:]
        later = later[~used[later]]
        d, bd = distance(m[a], c[a], m[later], c[later])
        with np.errstate(invalid="ignore"):
            near += int(np.sum(np.abs(d - T) <= np.maximum(NEAR * T, C * bd)))
            grp = later[d < T]
        used[grp] = True
        mem = np.concatenate([[a], grp]).astype(int)
        with np.errstate(all="ignore"):
            W = np.sum(w[mem])
            mu = np.sum(w[mem, None] * m[mem], 0) / W
            dm = mu - m[mem]
            P = np.sum(w[mem, None, None] * (_mat(c[mem]) + dm[:, :, None] * dm[:, None, :]), 0) / W
        g = np.zeros((), G64)
        g["weight"], g["mean"], g["cov"] = W, mu, _flat(P)
        out.append(g)
        if groups is not None:
            groups.append(len(grp))
    return (np.array(out, G64) if out else np.zeros(0, G64)), near
