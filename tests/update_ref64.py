"""The static PHD / CPHD update of one particle set in float64, from the model.

A plain numpy / scipy evaluation of the equations SURVEY.md states (Appendix
A.2 classification, "Births", A.3 EKF and weights, A.4 merge; the CPHD terms as
the oracle's cphd_terms comment documents them: Vo, Vo & Cantoni's analytic
GM-CPHD with a Poisson predicted cardinality).  It is written from those
equations and from neither implementation's instruction order:

  * no import of pyoracle, no routine of include/phd_detmath.h;
  * every input is converted to float64 on entry, no float32 intermediate;
  * quotients stay quotients (np.linalg.inv / solve on 2x2 stacks, a / b), sums
    are numpy sums, log / exp / sin / cos / arctan2 are numpy's, log-sums are
    scipy.special.logsumexp.

Layout (notation): a covariance is stored cov[0..3]
column-major, cov = (P00, P10, P01, P11).

update() returns a Result: maps (G64 records, CSR), delta (the change of the
particle log-weight), cn (CPHD: the log cardinality rows), and two per-particle
counts of near decisions: cls (range / bearing classification) and pm (prune /
merge).

Near decisions
--------------
A float32 pipeline and this one may decide differently when a decided value v
sits at its threshold T.  A decision is near when

    |v - T| <= max(NEAR * T, C * bound(v)),       NEAR = 1e-4, C = 2,

bound(v) a first-order float32 forward-error bound of v from the float32
inputs, eps = 2^-24 per rounding:

  range r = |mu - p|: two subtractions, two squares, a sum and a root, each
    relative: bound = 3 eps r.
  bearing phi = wrap(atan2(dy, dx) - theta): the rounded differences move the
    angle by <= 2 eps, the arctangent, the subtraction and the wrap round at
    their magnitudes: bound = eps (|atan2| + |theta| + |phi| + 2).
  non-detection weight (1 - pd) w: bound = 2 eps v.
  detection / birth weight q / eta, evaluated in logs by a float32 pipeline:
    log v = log pd + log w - d / 2 - log 2 pi - log|S| / 2 - log eta, each
    addend rounded at its magnitude, and d = nu' S^-1 nu inherits the
    innovation's error delta_nu = (eps (3 r + |z_r|), eps (|b_z| + |phi| + 5)):
    delta_d = 2 |S^-1 nu| . delta_nu + 8 eps d.  bound = v (eps (|log pd w| +
    |g| + |log q| + 2 |log eta| + 2) + delta_d / 2); births: v eps (|log beta|
    + 2 |log eta| + 2).
  merge distance d = D' ((A + B) / 2)^-1 D, D = a - b: the means are float32
    results (an updated mean carries eps of its own size and of the innovation
    mapped through K, about eps times its distance to the pose), so each
    coordinate of D moves by delta_D_k = 2 eps (|a_k| + |b_k| + |a - p| +
    |b - p|) — the eps (|a| + |b|) / |a - b| per coordinate of the mean
    difference, doubled by the square in delta_d = 2 |Sigma^-1 D| . delta_D —
    plus 8 eps d for the covariance average, determinant and quotients.
  Hellinger distance 1 - c e^(-q / 4) (metric 1): delta = (1 - d) (delta_q / 4
    + 16 eps), delta_q the Mahalanobis form's bound on (A + B).

C: each bound is the sum of the itemised first-order terms at their worst
case, so a float32 pipeline that makes exactly those roundings stays within
1 x bound; C = 2 leaves the same again for what the itemisation leaves out —
a quotient taken as a reciprocal and a product (one more rounding each),
contraction of a * b + c, and elementary functions within an ulp of the
correctly rounded value instead of at it.  NEAR is the oracle's own band
(Margin::NEAR, oracle/scphd_cpu.cpp), kept as the floor.

A weight tie at a merge selection — candidates within C * bound of the maximum
— counts as one near decision when its order can matter: two of the tied
candidates would absorb a common candidate (as hellinger_ref.greedy counts it).

TEST INFRASTRUCTURE ONLY.
"""
import collections

import numpy as np
from scipy.special import logsumexp

import hellinger_ref

EPS32 = 2.0 ** -24
NEAR = 1e-4
C = 2.0

G64 = np.dtype([("cov", np.float64, (4,)), ("mean", np.float64, (2,)), ("weight", np.float64)])
Result = collections.namedtuple("Result", "maps offsets delta cn cls pm")
TWO_PI = 2.0 * np.pi


def wrap(a):
    """wrapAngle (notation): the remainder of a / 2 pi, moved into [-pi, pi]."""
    r = np.fmod(np.asarray(a, np.float64), TWO_PI)
    return np.where(r > np.pi, r - TWO_PI, np.where(r < -np.pi, r + TWO_PI, r))


def _near(v, T, bound):
    v = np.asarray(v, np.float64)
    return np.abs(v - T) <= np.maximum(NEAR * abs(T), C * np.asarray(bound, np.float64))


def _mat(cov):
    """(..., 4) column-major -> (..., 2, 2)."""
    cov = np.asarray(cov, np.float64)
    return np.swapaxes(cov.reshape(cov.shape[:-1] + (2, 2)), -1, -2)


def _flat(P):
    return np.swapaxes(P, -1, -2).reshape(P.shape[:-2] + (4,))


def classify(cfg, pose, mean):
    """SURVEY A.2.  Returns (class per component: 1 in range, 2 nearly, 0 far;
    r; phi; number of near classifications)."""
    p = np.array([pose["px"], pose["py"]], np.float64)
    th = float(pose["ptheta"])
    d = np.asarray(mean, np.float64).reshape(-1, 2) - p
    r = np.sqrt(np.sum(d * d, 1))
    at = np.arctan2(d[:, 1], d[:, 0])
    phi = wrap(at - th)
    ab = np.abs(phi)
    minR, maxR, maxB = float(cfg.minRange), float(cfg.maxRange), float(cfg.maxBearing)
    inr = (r >= minR) & (r <= maxR) & (ab <= maxB)
    nearly = ~inr & (r >= 0.8 * minR) & (r <= 1.2 * maxR) & (ab <= 1.2 * maxB)
    cls = np.where(inr, 1, np.where(nearly, 2, 0))
    br = 3 * EPS32 * r
    bb = EPS32 * (np.abs(at) + abs(th) + ab + 2)
    near = _near(r, maxR, br)
    if minR > 0:
        near |= _near(r, minR, br)
    if maxB < np.pi:
        near |= _near(ab, maxB, bb)
    out = ~inr  # the second test is made for these only
    near |= out & _near(r, 1.2 * maxR, br)
    if minR > 0:
        near |= out & _near(r, 0.8 * minR, br)
    if 1.2 * maxB < np.pi:
        near |= out & _near(ab, 1.2 * maxB, bb)
    return cls, r, phi, int(np.sum(near))


def ekf(cfg, pose, mean, cov):
    """the range-bearing EKF of in-range components.  Returns a dict
    of stacks: r, phi, H, S (symmetrised), Sinv, K, Pp (Joseph form), logdet."""
    p = np.array([pose["px"], pose["py"]], np.float64)
    d = np.asarray(mean, np.float64).reshape(-1, 2) - p
    dx, dy = d[:, 0], d[:, 1]
    r2 = dx * dx + dy * dy
    r = np.sqrt(r2)
    phi = wrap(np.arctan2(dy, dx) - float(pose["ptheta"]))
    H = np.stack([np.stack([dx / r, dy / r], -1), np.stack([-dy / r2, dx / r2], -1)], -2)
    P = _mat(cov).reshape(-1, 2, 2)
    R = np.diag([float(cfg.stdRange) ** 2, float(cfg.stdBearing) ** 2])
    Ht = np.swapaxes(H, -1, -2)
    S = H @ P @ Ht + R
    S = (S + np.swapaxes(S, -1, -2)) / 2
    Sinv = np.linalg.inv(S) if len(S) else S
    K = P @ Ht @ Sinv
    A = np.eye(2) - K @ H
    Pp = A @ P @ np.swapaxes(A, -1, -2) + K @ R @ np.swapaxes(K, -1, -2)
    logdet = np.log(np.linalg.det(S)) if len(S) else np.zeros(0)
    return dict(r=r, phi=phi, H=H, S=S, Sinv=Sinv, K=K, Pp=Pp, logdet=logdet)


def births(cfg, pose, z):
    """SURVEY Appendix A "Births": the inverse measurement model.  (means, covariance matrices)."""
    zr = z["range"].astype(np.float64)
    tb = float(pose["ptheta"]) + z["bearing"].astype(np.float64)
    dx, dy = zr * np.cos(tb), zr * np.sin(tb)
    mean = np.stack([float(pose["px"]) + dx, float(pose["py"]) + dy], -1)
    J = np.stack([np.stack([dx / zr, -dy], -1), np.stack([dy / zr, dx], -1)], -2)
    f = float(cfg.birthNoiseFactor)
    V = np.diag([(float(cfg.stdRange) * f) ** 2, (float(cfg.stdBearing) * f) ** 2])
    return mean, J @ V @ np.swapaxes(J, -1, -2)


def esf_log(lam):
    """log elementary symmetric functions e_0..e_M of exp(lam), by the positive
    recursion e_k <- e_k + lambda e_(k-1) in logs."""
    lam = np.asarray(lam, np.float64)
    e = np.full(len(lam) + 1, -np.inf)
    e[0] = 0.0
    with np.errstate(all="ignore"):
        for k, l in enumerate(lam):
            e[1:k + 2] = logsumexp(np.stack([e[1:k + 2], l + e[0:k + 1]]), axis=0)
    return e


def _lse(a, axis=None):
    with np.errstate(all="ignore"):
        return logsumexp(a, axis=axis)


def cphd_terms(cfg, M, lam, w_in, pd, W):
    """The CPHD update's scalar terms of one particle (the formulas documented
    at cphd_terms, oracle/scphd_cpu.cpp; Vo, Vo & Cantoni 2007 with
    p(n) = Poisson(W)): lam[m] = log Lambda_m, w_in the in-range weights, W the
    whole predicted mass.  Returns (<Psi0,p>, <Psi1,p>, <Psi1d_m,p> per m, the
    updated log cardinality row), all logs."""
    Nmax = int(cfg.maxCardinality)
    rate = float(cfg.clutterRate)
    lrate = np.log(rate)
    lf = np.concatenate([[0.0], np.cumsum(np.log(np.arange(1, max(Nmax, M) + 2, dtype=np.float64)))])
    win = float(np.sum(w_in))
    qd = float(np.sum((1 - pd) * w_in))
    n = np.arange(Nmax + 1, dtype=np.float64)
    if W > 0:
        cn_pred = n * np.log(W) - W - lf[:Nmax + 1]
    else:  # an empty predicted map: cardinality delta_0 (D10)
        cn_pred = np.where(n == 0, 0.0, -np.inf)
    live = np.isfinite(cn_pred)
    if win <= 0 and np.any(live[1:]):
        raise NotImplementedError("predicted mass with no in-range component: <q_D,w>/<1,w> is 0/0")
    lw = np.log(win) if win > 0 else 0.0
    lq = np.log(qd) if qd > 0 else -np.inf

    def inner(e, Mx, shift):
        """log <Psi, p> rows: sum over j of (Mx - j)! clutter(Mx - j) e_j n! / (n - j - shift)!
        qd^(n - j - shift) / win^n, for n - j - shift >= 0; returns Psi[n]."""
        j = np.arange(len(e), dtype=np.float64)
        k = Mx - j
        aux = lf[k.astype(int)] + (k * lrate - rate - lf[k.astype(int)]) + e  # (Mx-j)! * Poisson(Mx-j)
        left = n[:, None] - j[None, :] - shift
        ok = left >= 0
        li = np.where(ok, left, 0).astype(int)
        with np.errstate(all="ignore"):
            pw = np.where(left > 0, left * lq, 0.0) - n[:, None] * lw
            t = aux[None, :] + lf[:Nmax + 1][:, None] - lf[li] + pw
        t = np.where(ok & live[:, None] & np.isfinite(e)[None, :], t, -np.inf)
        return _lse(t, axis=1)

    e = esf_log(lam)
    psi0 = inner(e, M, 0)
    psi1 = inner(e, M, 1)
    with np.errstate(all="ignore"):
        ip0 = _lse(np.where(live, psi0 + cn_pred, -np.inf))
        ip1 = _lse(np.where(live, psi1 + cn_pred, -np.inf))
        cn = np.where(live, cn_pred + psi0 - ip0, -np.inf)
        ip1d = np.full(M, -np.inf)
        for m in range(M):
            ed = esf_log(np.delete(lam, m))
            ip1d[m] = _lse(np.where(live, inner(ed, M - 1, 1) + cn_pred, -np.inf))
    return float(ip0), float(ip1), ip1d, cn


def _mahal_bound(D, Sinv, q, am, bm, p):
    L = (np.abs(am) + np.abs(bm) + np.linalg.norm(am - p, axis=-1, keepdims=True)
         + np.linalg.norm(bm - p, axis=-1, keepdims=True))
    g = np.abs(np.einsum("...ij,...j->...i", Sinv, D))
    return 2 * np.sum(g * (2 * EPS32 * L), -1) + 8 * EPS32 * np.abs(q)


def distance(metric, am, ac, bm, bc, p):
    """d(seed a, candidates b) and its float32 bound: Mahalanobis on the averaged
    covariance (metric 0) or hellinger_ref.hellinger64 (metric 1)."""
    am = np.asarray(am, np.float64)
    bm = np.asarray(bm, np.float64)
    D = am - bm
    A, B = _mat(ac), _mat(bc)
    with np.errstate(all="ignore"):
        if metric == 0:
            Sinv = np.linalg.inv((A + B) / 2)
            d = np.einsum("...i,...ij,...j->...", D, Sinv, D)
            return d, _mahal_bound(D, Sinv, d, am, bm, p)
        Sinv = np.linalg.inv(A + B)
        q = np.einsum("...i,...ij,...j->...", D, Sinv, D)
        d = hellinger_ref.hellinger64(am, ac, bm, bc)
        return d, (1 - d) * (_mahal_bound(D, Sinv, q, am, bm, p) / 4 + 16 * EPS32)


def merge(cfg, w, mean, cov, wbound, p):
    """the greedy merge of one particle's candidates (update-array
    order).  Returns (G64 outputs in selection order, near decisions)."""
    T = float(cfg.minSeparation)
    metric = int(cfg.distanceMetric)
    n = len(w)
    merged = np.zeros(n, bool)
    out = []
    near = 0
    while True:
        live = np.flatnonzero(~merged)
        if len(live) == 0:
            break
        best = live[np.argmax(w[live])]  # first maximum (D1)
        d, bd = distance(metric, mean[best], cov[best], mean[live], cov[live], p)
        with np.errstate(invalid="ignore"):
            take = d < T
            others = live != best
            near += int(np.sum(_near(d[others], T, bd[others])))
        tied = live[(w[best] - w[live]) <= C * (wbound[best] + wbound[live])]
        if len(tied) > 1:
            with np.errstate(invalid="ignore"):
                sets = [distance(metric, mean[t], cov[t], mean[live], cov[live], p)[0] < T for t in tied]
            near += int(np.any(np.sum(sets, 0) > 1))
        mem = live[take]
        W = float(np.sum(w[mem]))
        if W == 0:
            break
        g = np.zeros((), G64)
        if len(mem) == 1:  # a one-member set is emitted as its member
            Pm = _mat(cov[mem[0]])
            g["weight"], g["mean"] = w[mem[0]], mean[mem[0]]
        else:
            mu = np.sum(w[mem, None] * mean[mem], 0) / W
            dm = mu - mean[mem]
            Pm = np.sum(w[mem, None, None] * (_mat(cov[mem]) + dm[:, :, None] * dm[:, None, :]), 0) / W
            g["weight"], g["mean"] = W, mu
        g["cov"] = _flat((Pm + Pm.T) / 2)
        merged[mem] = True
        out.append(g)
    return (np.array(out, G64) if out else np.zeros(0, G64)), near


def update_particle(cfg, pose, comps, z):
    """One particle.  Returns (G64 map, delta, cn row or None, cls, pm)."""
    cphd = int(cfg.filterType) == 1
    M = len(z)
    w = comps["weight"].astype(np.float64)
    mean = comps["mean"].astype(np.float64).reshape(-1, 2)
    cov = comps["cov"].astype(np.float64).reshape(-1, 4)
    p = np.array([pose["px"], pose["py"]], np.float64)
    cls, _, _, ncls = classify(cfg, pose, mean)
    i1 = np.flatnonzero(cls == 1)
    G = len(i1)
    pd = float(cfg.pd)
    kappa, beta, minw = float(cfg.clutterDensity), float(cfg.birthWeight), float(cfg.minFeatureWeight)
    e = ekf(cfg, pose, mean[i1], cov[i1])
    wi = w[i1]
    zr, zb = z["range"].astype(np.float64), z["bearing"].astype(np.float64)
    static = (z["label"] == 0) | (not bool(cfg.labeledMeasurements))
    # innovations (G, M, 2), Mahalanobis term, log g, log q  (A.3)
    nu = np.stack([zr[None, :] - e["r"][:, None], wrap(zb[None, :] - e["phi"][:, None])], -1)
    Sn = np.einsum("gij,gmj->gmi", e["Sinv"], nu)
    d = np.sum(nu * Sn, -1)
    with np.errstate(divide="ignore"):
        logpw = np.log(pd) + np.log(np.where(wi > 0, wi, 0.0))
        lg = -0.5 * d - np.log(TWO_PI) - 0.5 * e["logdet"][:, None]
        logq = np.where(static[None, :], logpw[:, None] + lg, -np.inf)
    q = np.exp(logq)
    mu_det = mean[i1][:, None, :] + np.einsum("gij,gmj->gmi", e["K"], nu)
    dnu = np.stack([np.broadcast_to(EPS32 * (3 * e["r"][:, None] + np.abs(zr)[None, :]), d.shape),
                    EPS32 * (np.abs(zb)[None, :] + np.abs(e["phi"])[:, None] + 5)], -1)
    dd = 2 * np.sum(np.abs(Sn) * dnu, -1) + 8 * EPS32 * d
    cn = None
    if cphd:
        W = float(np.sum(w))
        with np.errstate(divide="ignore"):
            lam = np.log(np.sum(q, 0)) + np.log(float(cfg.clutterRate)) - np.log(kappa) if G else np.full(M, -np.inf)
        ip0, ip1, ip1d, cn = cphd_terms(cfg, M, lam, wi, np.full(G, pd), W)
        delta = ip0
        leta = (ip0 - ip1d) - (np.log(float(cfg.clutterRate)) - np.log(kappa))
        w_nd = wi * (1 - pd) * np.exp(ip1 - ip0)
        b_nd = w_nd * EPS32 * (abs(ip1 - ip0) + 4)
    else:
        eta = np.sum(q, 0) + kappa + beta
        leta = np.log(eta)
        delta = float(np.sum(leta) - (np.sum(pd * wi) + M * beta))
        w_nd = wi * (1 - pd)
        b_nd = 2 * EPS32 * w_nd
    with np.errstate(all="ignore"):
        w_det = np.exp(logq - leta[None, :])
        b_det = w_det * (EPS32 * (np.abs(logpw)[:, None] + np.abs(lg) + np.abs(np.where(np.isfinite(logq), logq, 0))
                                  + 2 * np.abs(leta)[None, :] + 2) + dd / 2)
    cw, cm, cc, cb = [], [], [], []
    pm = 0

    def push(wv, mv, cv, bv):
        nonlocal pm
        wv, bv = np.asarray(wv, np.float64).ravel(), np.asarray(bv, np.float64).ravel()
        pm += int(np.sum(_near(wv, minw, bv)))
        keep = ~(wv < minw)
        cw.append(wv[keep])
        cm.append(np.asarray(mv).reshape(-1, 2)[keep])
        cc.append(np.asarray(cv).reshape(-1, 4)[keep])
        cb.append(bv[keep])

    push(w_nd, mean[i1], cov[i1], b_nd)  # non-detection
    Pp = _flat(e["Pp"])
    push(w_det.T, np.swapaxes(mu_det, 0, 1), np.broadcast_to(Pp[None], (M, G, 4)), b_det.T)  # measurement-major
    if not cphd:  # births are not part of the CPHD candidate list
        bm, bP = births(cfg, pose, z)
        w_b = np.where(static, beta / eta, 0.0)
        push(w_b, bm, _flat(bP), w_b * EPS32 * (abs(np.log(beta)) + 2 * np.abs(leta) + 2))
    i2 = np.flatnonzero(cls == 2)  # nearly in range: join the merge as they are
    cw.append(w[i2])
    cm.append(mean[i2])
    cc.append(cov[i2])
    cb.append(np.zeros(len(i2)))
    out, nm = merge(cfg, np.concatenate(cw), np.concatenate(cm), np.concatenate(cc), np.concatenate(cb), p)
    i0 = np.flatnonzero(cls == 0)  # far: appended unmerged
    far = np.zeros(len(i0), G64)
    far["weight"], far["mean"], far["cov"] = w[i0], mean[i0], cov[i0]
    return np.concatenate([out, far]), float(delta), cn, ncls, pm + nm


def update(cfg, poses, maps, offsets, z):
    """The update of every particle (inputs as pyoracle.update takes them)."""
    z = z[:256]
    n = len(poses)
    outs, delta, cns, cls, pm = [], np.zeros(n), [], np.zeros(n, np.int64), np.zeros(n, np.int64)
    for i in range(n):
        m, delta[i], cn, cls[i], pm[i] = update_particle(cfg, poses[i], maps[offsets[i]:offsets[i + 1]], z)
        outs.append(m)
        cns.append(cn)
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum([len(m) for m in outs])
    cn = np.stack(cns) if int(cfg.filterType) == 1 else None
    return Result(np.concatenate(outs) if outs else np.zeros(0, G64), offs, delta, cn, cls, pm)
