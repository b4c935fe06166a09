"""The mixed static + dynamic feature model (feature_model 2) in float64, from
the model.

A plain numpy evaluation of the equations SURVEY.md states (Appendix A.2
classification, "Births", A.3 EKF and weights, A.4 merge) for a static
(2-D, position) and a dynamic (4-D, position + velocity) Gaussian mixture that
share one scan, and of the routines phd_mixed.hip's header cites: the
constant-velocity prediction with the speed-gated survival, and the EAP
reduction of the dynamic maps.  Written from those equations and from neither
implementation's instruction order:

  * no import of pyoracle, no routine of include/phd_detmath.h, nothing of
    include/phd_mixed.h or oracle/mixed_ref.h;
  * every input is converted to float64 on entry, no float32 intermediate;
  * quotients stay quotients: np.linalg.inv / solve on stacks, a / b.

Layout: a covariance is stored column-major, cov[i + D j] = P[i, j], D = 2
(static) or 4 (dynamic, state (x, y, vx, vy)).

update() returns a Result: both posterior maps (CSR; G64 / G64_4 records),
delta (the change of the particle log-weight) and per-particle counts of near
decisions: cls (range / bearing classification) and pm (prune / merge; pm2
holds the static and the dynamic count apart, pm their sum).

Near decisions follow update_ref64 (its module text has the bounds): a decided
value v is near its threshold T when |v - T| <= max(1e-4 T, 2 bound(v)), bound
a first-order float32 forward-error bound.  The 4-D merge distance uses the
same bound with the velocity coordinates carried like the position ones.  A
seed choice between candidates whose weights differ, by no more than that band,
counts as one near decision when its order can matter (two of them would
absorb a common candidate).  Weights that are EQUAL in float64 are not near:
the lowest index is the seed (D1) in every precision.

A scan without measurements: the reference's driver runs no update then
(main.cpp:1260, `if ZZ.size() > 0`), so update() returns its inputs, delta 0.

TEST INFRASTRUCTURE ONLY.
"""
import collections

import numpy as np

from update_ref64 import C, EPS32, G64, NEAR, TWO_PI, _near, wrap  # noqa: F401

G64_4 = np.dtype([("cov", np.float64, (16,)), ("mean", np.float64, (4,)), ("weight", np.float64)])
Result = collections.namedtuple("Result", "smaps soffs dmaps doffs delta cls pm pm2")
STATIC, DYNAMIC = 0, 1  # measurement labels


def mat(cov, D):
    """(..., D D) column-major -> (..., D, D)."""
    cov = np.asarray(cov, np.float64)
    return np.swapaxes(cov.reshape(cov.shape[:-1] + (D, D)), -1, -2)


def flat(P):
    D = P.shape[-1]
    return np.swapaxes(P, -1, -2).reshape(P.shape[:-2] + (D * D,))


def _T(A):
    return np.swapaxes(A, -1, -2)


def classify(cfg, pose, xy, second):
    """SURVEY A.2 on positions xy (n, 2).  Returns (class: 1 in range, 2 nearly,
    0 out; r; phi; near classifications).  second: the nearly / out boundary
    matters (static maps; a dynamic component that is not in range is dropped
    either way)."""
    p = np.array([pose["px"], pose["py"]], np.float64)
    th = float(pose["ptheta"])
    d = np.asarray(xy, np.float64).reshape(-1, 2) - p
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
    if second:
        out = ~inr
        near |= out & _near(r, 1.2 * maxR, br)
        if minR > 0:
            near |= out & _near(r, 0.8 * minR, br)
        if 1.2 * maxB < np.pi:
            near |= out & _near(ab, 1.2 * maxB, bb)
    return cls, r, phi, int(np.sum(near))


def ekf(cfg, pose, mean, cov, D):
    """SURVEY A.3 for D-dimensional components observed in range and bearing:
    H is the 2 x 2 Jacobian of (r, phi) in the position, zero in the velocity
    columns.  Returns stacks r, phi, S, Sinv, K (D x 2), Pp (Joseph form), logdet."""
    mean = np.asarray(mean, np.float64).reshape(-1, D)
    n = len(mean)
    p = np.array([pose["px"], pose["py"]], np.float64)
    d = mean[:, :2] - p
    dx, dy = d[:, 0], d[:, 1]
    r2 = dx * dx + dy * dy
    r = np.sqrt(r2)
    phi = wrap(np.arctan2(dy, dx) - float(pose["ptheta"]))
    H = np.zeros((n, 2, D))
    H[:, 0, 0], H[:, 0, 1] = dx / r, dy / r
    H[:, 1, 0], H[:, 1, 1] = -dy / r2, dx / r2
    P = mat(np.asarray(cov, np.float64).reshape(-1, D * D), D)
    R = np.diag([float(cfg.stdRange) ** 2, float(cfg.stdBearing) ** 2])
    S = H @ P @ _T(H) + R
    S = (S + _T(S)) / 2
    Sinv = np.linalg.inv(S) if n else S
    K = P @ _T(H) @ Sinv
    A = np.eye(D) - K @ H
    Pp = A @ P @ _T(A) + K @ R @ _T(K)
    logdet = np.log(np.linalg.det(S)) if n else np.zeros(0)
    return dict(r=r, phi=phi, H=H, S=S, Sinv=Sinv, K=K, Pp=Pp, logdet=logdet)


def births(cfg, pose, z, D):
    """The inverse measurement model (SURVEY Appendix A "Births"): mean pose +
    r (cos, sin)(theta + b), covariance J diag(sr^2, sb^2) factor^2 J'; a 4-D
    birth is at rest with the velocity variances covVxBirth / covVyBirth."""
    zr = z["range"].astype(np.float64)
    tb = float(pose["ptheta"]) + z["bearing"].astype(np.float64)
    dx, dy = zr * np.cos(tb), zr * np.sin(tb)
    M = len(zr)
    mean = np.zeros((M, D))
    mean[:, 0], mean[:, 1] = float(pose["px"]) + dx, float(pose["py"]) + dy
    J = np.stack([np.stack([dx / zr, -dy], -1), np.stack([dy / zr, dx], -1)], -2)
    f = float(cfg.birthNoiseFactor)
    V = np.diag([(float(cfg.stdRange) * f) ** 2, (float(cfg.stdBearing) * f) ** 2])
    P = np.zeros((M, D, D))
    P[:, :2, :2] = J @ V @ _T(J)
    if D == 4:
        P[:, 2, 2] = float(cfg.covVxBirth)
        P[:, 3, 3] = float(cfg.covVyBirth)
    return mean, P


def distance(am, ac, bm, bc, p, D):
    """d = (a - b)' ((A + B) / 2)^-1 (a - b) of a seed against candidates, by
    np.linalg.solve, and its float32 bound (update_ref64._mahal_bound's terms)."""
    am, bm = np.asarray(am, np.float64), np.asarray(bm, np.float64)
    Dv = am - bm
    Sg = (mat(ac, D) + mat(bc, D)) / 2
    with np.errstate(all="ignore"):
        g = np.linalg.solve(Sg, Dv[..., None])[..., 0]
        d = np.sum(Dv * g, -1)
    L = (np.abs(am) + np.abs(bm) + np.linalg.norm(am[..., :2] - p, axis=-1, keepdims=True)
         + np.linalg.norm(bm[..., :2] - p, axis=-1, keepdims=True))
    bound = 2 * np.sum(np.abs(g) * (2 * EPS32 * L), -1) + 8 * EPS32 * np.abs(d)
    return d, bound


def merge(cfg, w, mean, cov, wbound, p, D):
    """the greedy merge of one map's candidates (update-array order).
    Returns (records in selection order, near decisions, (members of the widest
    merge set, the widest span of candidate indices in one set))."""
    T = float(cfg.minSeparation)
    widest = span = 0
    rec = G64 if D == 2 else G64_4
    n = len(w)
    merged = np.zeros(n, bool)
    out = []
    near = 0
    while True:
        live = np.flatnonzero(~merged)
        if len(live) == 0:
            break
        best = live[np.argmax(w[live])]  # first maximum (D1)
        d, bd = distance(mean[best], cov[best], mean[live], cov[live], p, D)
        with np.errstate(invalid="ignore"):
            take = d < T
            others = live != best
            near += int(np.sum(_near(d[others], T, bd[others])))
        gap = w[best] - w[live]
        tied = live[(gap > 0) & (gap <= np.maximum(NEAR * w[best], C * (wbound[best] + wbound[live])))]
        if len(tied):
            tied = np.concatenate([[best], tied])
            with np.errstate(invalid="ignore"):
                sets = [distance(mean[t], cov[t], mean[live], cov[live], p, D)[0] < T for t in tied]
            near += int(np.any(np.sum(sets, 0) > 1))
        mem = live[take]
        W = float(np.sum(w[mem]))
        if W == 0:
            break
        g = np.zeros((), rec)
        mu = np.sum(w[mem, None] * mean[mem], 0) / W
        dm = mu - mean[mem]
        Pm = np.sum(w[mem, None, None] * (mat(cov[mem], D) + dm[:, :, None] * dm[:, None, :]), 0) / W
        g["weight"], g["mean"] = W, mu
        g["cov"] = flat((Pm + Pm.T) / 2)
        merged[mem] = True
        widest, span = max(widest, len(mem)), max(span, int(mem.max() - mem.min()))
        out.append(g)
    return (np.array(out, rec) if out else np.zeros(0, rec)), near, (widest, span)


def _records(rec, w, mean, cov):
    out = np.zeros(len(w), rec)
    out["weight"], out["mean"], out["cov"] = w, mean, cov
    return out


def _map_terms(cfg, pose, comps, z, ok, D, second):
    """Classification, EKF and the detection terms log q (G, M) of one map."""
    w = comps["weight"].astype(np.float64)
    mean = comps["mean"].astype(np.float64).reshape(-1, D)
    cov = comps["cov"].astype(np.float64).reshape(-1, D * D)
    cls, _, _, ncls = classify(cfg, pose, mean[:, :2], second)
    i1 = np.flatnonzero(cls == 1)
    e = ekf(cfg, pose, mean[i1], cov[i1], D)
    zr, zb = z["range"].astype(np.float64), z["bearing"].astype(np.float64)
    nu = np.stack([zr[None, :] - e["r"][:, None], wrap(zb[None, :] - e["phi"][:, None])], -1)
    Sn = np.einsum("gij,gmj->gmi", e["Sinv"], nu)
    d = np.sum(nu * Sn, -1)
    wi = w[i1]
    with np.errstate(divide="ignore"):
        logpw = np.log(float(cfg.pd)) + np.log(np.where(wi > 0, wi, 0.0))
        lg = -0.5 * d - np.log(TWO_PI) - 0.5 * e["logdet"][:, None]
        logq = np.where(ok[None, :], logpw[:, None] + lg, -np.inf)
    dnu = np.stack([np.broadcast_to(EPS32 * (3 * e["r"][:, None] + np.abs(zr)[None, :]), d.shape),
                    EPS32 * (np.abs(zb)[None, :] + np.abs(e["phi"])[:, None] + 5)], -1)
    dd = 2 * np.sum(np.abs(Sn) * dnu, -1) + 8 * EPS32 * d
    mu_det = mean[i1][:, None, :] + np.einsum("gij,gmj->gmi", e["K"], nu)
    return dict(w=w, mean=mean, cov=cov, cls=cls, ncls=ncls, i1=i1, e=e, wi=wi, logpw=logpw, lg=lg, logq=logq, dd=dd,
                mu_det=mu_det)


def _candidates(cfg, pose, t, z, ok, leta, D):
    """[non-detect | detect, measurement-major | births | nearly in range (static)]
    after the prune w < minFeatureWeight.  Returns (w, mean, cov, bound, near prunes)."""
    minw, pd, beta = float(cfg.minFeatureWeight), float(cfg.pd), float(cfg.birthWeight)
    M = len(z)
    G = len(t["i1"])
    cw, cm, cc, cb = [], [], [], []
    pm = 0

    def push(wv, mv, cv, bv):
        nonlocal pm
        wv, bv = np.asarray(wv, np.float64).ravel(), np.asarray(bv, np.float64).ravel()
        pm += int(np.sum(_near(wv, minw, bv)))
        keep = ~(wv < minw)
        cw.append(wv[keep])
        cm.append(np.asarray(mv).reshape(-1, D)[keep])
        cc.append(np.asarray(cv).reshape(-1, D * D)[keep])
        cb.append(bv[keep])

    w_nd = t["wi"] * (1 - pd)
    push(w_nd, t["mean"][t["i1"]], t["cov"][t["i1"]], 2 * EPS32 * w_nd)
    with np.errstate(all="ignore"):
        logq = t["logq"]
        w_det = np.exp(logq - leta[None, :])
        b_det = w_det * (EPS32 * (np.abs(t["logpw"])[:, None] + np.abs(t["lg"])
                                  + np.abs(np.where(np.isfinite(logq), logq, 0)) + 2 * np.abs(leta)[None, :] + 2)
                         + t["dd"] / 2)
    Pp = flat(t["e"]["Pp"]) if G else np.zeros((0, D * D))
    push(w_det.T, np.swapaxes(t["mu_det"], 0, 1), np.broadcast_to(Pp[None], (M, G, D * D)), b_det.T)
    bm, bP = births(cfg, pose, z, D)
    w_b = np.where(ok, beta / np.exp(leta), 0.0)
    push(w_b, bm, flat(bP), w_b * EPS32 * (abs(np.log(beta)) + 2 * np.abs(leta) + 2))
    if D == 2:  # nearly in range: join the merge as they are, never pruned
        i2 = np.flatnonzero(t["cls"] == 2)
        cw.append(t["w"][i2])
        cm.append(t["mean"][i2])
        cc.append(t["cov"][i2])
        cb.append(np.zeros(len(i2)))
    return np.concatenate(cw), np.concatenate(cm), np.concatenate(cc), np.concatenate(cb), pm


def update_particle(cfg, pose, scomps, dcomps, z):
    """One particle.  Returns (static map, dynamic map, delta, cls, (pm static, pm dynamic),
    (static candidates, dynamic candidates, widest merge set of each, widest index span of each))."""
    labeled = bool(cfg.labeledMeasurements)
    p = np.array([pose["px"], pose["py"]], np.float64)
    ok_s = (z["label"] == STATIC) | (not labeled)
    ok_d = (z["label"] == DYNAMIC) | (not labeled)
    s = _map_terms(cfg, pose, scomps, z, ok_s, 2, True)
    d = _map_terms(cfg, pose, dcomps, z, ok_d, 4, False)
    kappa, beta, pd = float(cfg.clutterDensity), float(cfg.birthWeight), float(cfg.pd)
    eta = np.sum(np.exp(s["logq"]), 0) + np.sum(np.exp(d["logq"]), 0) + kappa + beta
    if not labeled:
        eta = eta + beta  # a birth into each map
    leta = np.log(eta)
    delta = float(np.sum(leta) - pd * (np.sum(s["wi"]) + np.sum(d["wi"])))
    sw, sm, sc, sb, pms = _candidates(cfg, pose, s, z, ok_s, leta, 2)
    dw, dm, dc, db, pmd = _candidates(cfg, pose, d, z, ok_d, leta, 4)
    sout, ns, shs = merge(cfg, sw, sm, sc, sb, p, 2)
    dout, nd, shd = merge(cfg, dw, dm, dc, db, p, 4)
    i0 = np.flatnonzero(s["cls"] == 0)  # static out of range: appended in order
    far = _records(G64, s["w"][i0], s["mean"][i0], s["cov"][i0])
    return (np.concatenate([sout, far]), dout, delta, s["ncls"] + d["ncls"], (pms + ns, pmd + nd),
            (len(sw), len(dw), shs[0], shd[0], shs[1], shd[1]))


def update(cfg, poses, smaps, soffs, dmaps, doffs, z, counts=None):
    """The mixed update of every particle (inputs as pyoracle.update_mixed takes
    them).  counts: a list that receives update_particle's last tuple per particle."""
    z = z[:256]  # the scan is cut to 256 measurements (phdUpdateSynth)
    n = len(poses)
    if len(z) == 0:  # no update is run for an empty scan
        so = _records(G64, smaps["weight"], smaps["mean"], smaps["cov"])
        do = _records(G64_4, dmaps["weight"], dmaps["mean"], dmaps["cov"])
        zi = np.zeros(n, np.int64)
        if counts is not None:
            counts.extend([(0,) * 6] * n)
        return Result(so, np.asarray(soffs, np.int64).copy(), do, np.asarray(doffs, np.int64).copy(), np.zeros(n),
                      zi, zi.copy(), np.zeros((n, 2), np.int64))
    so, do = [], []
    delta, cls, pm2 = np.zeros(n), np.zeros(n, np.int64), np.zeros((n, 2), np.int64)
    for i in range(n):
        a, b, delta[i], cls[i], pm2[i], k = update_particle(cfg, poses[i], smaps[soffs[i]:soffs[i + 1]],
                                                            dmaps[doffs[i]:doffs[i + 1]], z)
        so.append(a)
        do.append(b)
        if counts is not None:
            counts.append(k)
    soo, doo = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    soo[1:] = np.cumsum([len(m) for m in so])
    doo[1:] = np.cumsum([len(m) for m in do])
    return Result(np.concatenate(so) if so else np.zeros(0, G64), soo,
                  np.concatenate(do) if do else np.zeros(0, G64_4), doo, delta, cls, pm2.sum(1), pm2)


def cv_model(cfg):
    """(F, Q) of the constant-velocity model on (x, y, vx, vy) at dt with white
    accelerations of standard deviations stdAxMap / stdAyMap."""
    dt = float(cfg.dt)
    F = np.eye(4)
    F[0, 2] = F[1, 3] = dt
    G = np.array([[dt * dt / 2, 0], [0, dt * dt / 2], [dt, 0], [0, dt]])
    Q = G @ np.diag([float(cfg.stdAxMap) ** 2, float(cfg.stdAyMap) ** 2]) @ G.T
    return F, Q


def predict(cfg, dmaps):
    """One prediction of a flat array of dynamic components: F m, F P F' + Q, the
    weight times ps / (1 + exp(beta (tau - |v|)))."""
    F, Q = cv_model(cfg)
    m = dmaps["mean"].astype(np.float64).reshape(-1, 4)
    P = mat(dmaps["cov"].astype(np.float64).reshape(-1, 16), 4)
    v = np.sqrt(m[:, 2] ** 2 + m[:, 3] ** 2)
    surv = float(cfg.ps) / (1 + np.exp(float(cfg.beta) * (float(cfg.tau) - v)))
    return _records(G64_4, dmaps["weight"].astype(np.float64) * surv, m @ F.T, flat(F @ P @ F.T + Q))


def expected_map(cfg, logw, dmaps, doffs):
    """The EAP map of the dynamic maps: component weights times exp(log w_n),
    stable descending order, every seed absorbs each later unmerged component
    inside minSeparation; the merged mean first, then the covariance about it.
    Returns (records in emission order, near decisions: a distance within the
    1e-4 band of minSeparation, or two neighbours of the priority order whose
    weights a float32 evaluation could exchange (relative gap <= 1e-6, not 0))."""
    T = float(cfg.minSeparation)
    n = len(logw)
    sizes = np.diff(np.asarray(doffs, np.int64))
    ew = np.repeat(np.exp(np.asarray(logw, np.float64)), sizes)
    lo, hi = int(doffs[0]), int(doffs[n])
    w = dmaps["weight"][lo:hi].astype(np.float64) * ew
    m = dmaps["mean"][lo:hi].astype(np.float64).reshape(-1, 4)
    c = dmaps["cov"][lo:hi].astype(np.float64).reshape(-1, 16)
    order = np.argsort(-w, kind="stable")
    ws = w[order]
    gap = ws[:-1] - ws[1:]
    near = int(np.sum((gap > 0) & (gap <= 1e-6 * ws[:-1])))
    used = np.zeros(len(w), bool)
    out = []
    for oi, a in enumerate(order):
        if used[a]:
            continue
        used[a] = True
        later = order[oi + 1:]
        later = later[~used[later]]
        d, _ = distance(m[a], c[a], m[later], c[later], np.zeros(2), 4)
        near += int(np.sum(np.abs(d - T) <= NEAR * T))
        grp = later[d < T]
        used[grp] = True
        mem = np.concatenate([[a], grp]).astype(int)
        W = np.sum(w[mem])
        mu = np.sum(w[mem, None] * m[mem], 0) / W
        dm = mu - m[mem]
        P = np.sum(w[mem, None, None] * (mat(c[mem], 4) + dm[:, :, None] * dm[:, None, :]), 0) / W
        g = np.zeros((), G64_4)
        g["weight"], g["mean"], g["cov"] = W, mu, flat(P)
        out.append(g)
    return (np.array(out, G64_4) if out else np.zeros(0, G64_4)), near
