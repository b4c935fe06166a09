"""Reference of the Hellinger merge (distance_metric = 1) in numpy float32.

A restatement of the reference's computeHellingerDist for 2-D Gaussians
(device_math.cuh:373-413) and of the greedy merge of phdUpdateMergeKernel
(phdfilter.cu:2739-2890) with the test d(seed, i) < minSeparation
(phdfilter.cu:2802-2806, :2844-2848), the seed always the first argument.
The greedy follows the project's oracle (oracle/scphd_cpu.cpp,
merge_candidates) in everything but the distance: first maximum of the
weights (D1), moments summed in double in candidate order (D3), one
reciprocal of the merged weight (D18), a one-member set emitted as its member
(D15), the covariance symmetrised at the end (device_math.cuh:710-725).

Every float operation is one numpy float32 operation (no contraction), and the
exponential is the project's deterministic one (include/phd_detmath.h,
phd_det_expf) restated in IEEE double operations, so the distances are the
device's bit for bit.

TEST INFRASTRUCTURE ONLY.
"""
import numpy as np

F = np.float32
FLT_MIN = np.float32(np.finfo(np.float32).tiny)
NEAR = 1e-4  # the band of pyoracle.near_counts: |d - T| <= NEAR T


def det_expf(x):
    """phd_det_expf (include/phd_detmath.h) on a float32 array."""
    xf = np.asarray(x, F)
    x = xf.astype(np.float64)
    with np.errstate(all="ignore"):
        xc = np.where(np.isfinite(x), np.clip(x, -120.0, 100.0), 0.0)
        k = np.floor(xc * 1.4426950408889634 + 0.5)
        r = (xc - k * 0.693147180369123816490) - k * 1.90821492927058770002e-10
        p = np.full_like(r, 1.0 / 6227020800.0)
        for c in (1.0 / 479001600.0, 1.0 / 39916800.0, 1.0 / 3628800.0, 1.0 / 362880.0, 1.0 / 40320.0, 1.0 / 5040.0,
                  1.0 / 720.0, 1.0 / 120.0, 1.0 / 24.0, 1.0 / 6.0, 0.5, 1.0, 1.0):
            p = p * r + c
        out = np.ldexp(p, k.astype(np.int64)).astype(F)
    out = np.where(x < -110.0, F(0), out)
    out = np.where(x > 89.0, F(np.inf), out)
    out = np.where(np.isnan(x), xf, out)
    return out.astype(F)


def hellinger(am, ac, bm, bc):
    """computeHellingerDist(a, b), device_math.cuh:373-413: means (..., 2) and
    covariances (..., 4) as float32 arrays that broadcast; returns float32."""
    am, ac, bm, bc = (np.asarray(v, F) for v in (am, ac, bm, bc))
    with np.errstate(all="ignore"):
        i0 = am[..., 0] - bm[..., 0]  # :381-382
        i1 = am[..., 1] - bm[..., 1]
        s0 = ac[..., 0] + bc[..., 0]  # :383-386
        s1 = ac[..., 1] + bc[..., 1]
        s2 = ac[..., 2] + bc[..., 2]
        s3 = ac[..., 3] + bc[..., 3]
        det = s0 * s3 - s2 * s1  # det2, :387 (device_math.cuh:37-39)
        ok = det > FLT_MIN  # :388
        v0 = np.where(ok, s3 / det, F(1))  # :390-393, else the identity of :380
        v1 = np.where(ok, -s1 / det, F(0))
        v2 = np.where(ok, -s2 / det, F(0))
        v3 = np.where(ok, s0 / det, F(1))
        q = i0 * i0 * v0 + i0 * i1 * (v1 + v2) + i1 * i1 * v3  # :396-398, float
        eps = (-0.25 * q.astype(np.float64)).astype(F)  # :395: a double constant, stored to float
        d4 = det / F(4)  # :401
        dist = F(1) / d4  # :402
        p0 = ac[..., 0] * bc[..., 0] + ac[..., 2] * bc[..., 1]  # :405-408
        p1 = ac[..., 1] * bc[..., 0] + ac[..., 3] * bc[..., 1]
        p2 = ac[..., 0] * bc[..., 2] + ac[..., 2] * bc[..., 3]
        p3 = ac[..., 1] * bc[..., 2] + ac[..., 3] * bc[..., 3]
        dp = p0 * p3 - p2 * p1  # :409
        dist = dist * np.sqrt(dp)  # :410
        return (F(1) - np.sqrt(dist) * det_expf(eps)).astype(F)  # :411


def hellinger64(am, ac, bm, bc):
    """The closed form in float64: 1 - sqrt(sqrt(|A||B|) / |(A+B)/2|) exp(-d' (A+B)^-1 d / 4)."""
    am, ac, bm, bc = (np.asarray(v, np.float64) for v in (am, ac, bm, bc))
    A = ac.reshape(ac.shape[:-1] + (2, 2))
    B = bc.reshape(bc.shape[:-1] + (2, 2))
    S = A + B
    d = am - bm
    q = np.einsum("...i,...ij,...j->...", d, np.linalg.inv(S), d)
    c = np.sqrt(np.linalg.det(A) * np.linalg.det(B)) / np.linalg.det(S / 2)
    return 1 - np.sqrt(c) * np.exp(-0.25 * q)


def mahal64(am, ac, bm, bc):
    """d' ((A+B)/2)^-1 d in float64 (computeMahalDist, device_math.cuh:309-325)."""
    am, ac, bm, bc = (np.asarray(v, np.float64) for v in (am, ac, bm, bc))
    S = (ac + bc).reshape(np.broadcast(ac, bc).shape[:-1] + (2, 2)) / 2
    d = am - bm
    return np.einsum("...i,...ij,...j->...", d, np.linalg.inv(S), d)


def cull_threshold(T):
    """T_M = -8 ln(1 - T): d_H < T implies d' ((A+B)/2)^-1 d < T_M (c <= 1)."""
    return -8.0 * np.log1p(-np.asarray(T, np.float64))


def greedy(cand, T):
    """The greedy merge of one particle's candidates (a GAUSSIAN2D array in
    update-array order) under the Hellinger distance.  Returns (merged, near):
    the outputs in selection order, and the number of near decisions — tests
    d(seed, i) it performed with |d - T| <= 1e-4 T (the seed's own included,
    unlike the oracle's Mahalanobis count, whose own distance is exactly 0),
    plus the weight ties at a selection whose order can matter (see below)."""
    T = F(T)
    n = len(cand)
    w = cand["weight"].astype(F)
    mean = cand["mean"].astype(F)
    cov = cand["cov"].astype(F)
    merged = np.zeros(n, bool)
    out = []
    near = 0
    while True:
        live = np.flatnonzero(~merged)
        if len(live) == 0:
            break
        best = live[np.argmax(w[live])]  # first maximum (D1)
        d = hellinger(mean[best], cov[best], mean[live], cov[live])
        tied = live[w[live] == w[best]]
        if len(tied) > 1:
            # a weight tie at the selection is near when the order of the tied
            # candidates can matter: two of them would absorb a common candidate
            # (or one another).  Ties whose merge sets are disjoint (the births
            # of clutter measurements: equal weights by construction, D17, far
            # apart) give the same outputs in any order.
            with np.errstate(invalid="ignore"):
                sets = [hellinger(mean[t], cov[t], mean[live], cov[live]) < T for t in tied]
            near += int(np.any(np.sum(sets, 0) > 1))
        with np.errstate(invalid="ignore"):
            near += int(np.sum(np.abs(d.astype(np.float64) - float(T)) <= NEAR * float(T)))
            take = d < T  # (a NaN distance never merges)
        mem = live[take]
        W = F(np.sum(w[mem].astype(np.float64)))
        if W == 0:
            break
        if len(mem) == 1 and mem[0] == best:  # the seed alone (D15)
            g = cand[best].copy()
            g["cov"][1] = (g["cov"][1] + g["cov"][2]) / F(2)
            g["cov"][2] = g["cov"][1]
            merged[best] = True
            out.append(g)
            continue
        rW = F(1) / W
        gx = F(np.sum((w[mem] * mean[mem, 0]).astype(np.float64))) * rW
        gy = F(np.sum((w[mem] * mean[mem, 1]).astype(np.float64))) * rW
        d0 = gx - mean[mem, 0]
        d1 = gy - mean[mem, 1]
        c = [F(np.sum((w[mem] * (cov[mem, 0] + d0 * d0)).astype(np.float64))) * rW,
             F(np.sum((w[mem] * (cov[mem, 1] + d0 * d1)).astype(np.float64))) * rW,
             F(np.sum((w[mem] * (cov[mem, 2] + d1 * d0)).astype(np.float64))) * rW,
             F(np.sum((w[mem] * (cov[mem, 3] + d1 * d1)).astype(np.float64))) * rW]
        c[1] = (c[1] + c[2]) / F(2)
        c[2] = c[1]
        g = np.zeros((), cand.dtype)
        g["weight"] = W
        g["mean"] = (gx, gy)
        g["cov"] = c
        merged[mem] = True
        out.append(g)
    return (np.array(out, cand.dtype) if out else np.zeros(0, cand.dtype)), near


def n_out_of_range(cfg, pose, comps):
    """Number of class-0 components of one particle's map: neither in range nor
    nearly in range (computeInRangeKernel, phdfilter.cu:1328-1346, as
    oracle/scphd_cpu.cpp states it).  They follow the merged ones unchanged."""
    import pyoracle
    n0 = 0
    for g in comps:
        dx = F(g["mean"][0]) - F(pose["px"])
        dy = F(g["mean"][1]) - F(pose["py"])
        r = np.sqrt(dx * dx + dy * dy)
        ab = abs(F(pyoracle.wrap_angle(F(F(pyoracle.atan2f(dy, dx)) - F(pose["ptheta"])))))
        inr = r >= F(cfg.minRange) and r <= F(cfg.maxRange) and ab <= F(cfg.maxBearing)
        nearly = (float(r) >= 0.8 * cfg.minRange and float(r) <= 1.2 * cfg.maxRange
                  and float(ab) <= 1.2 * cfg.maxBearing)
        n0 += int(not inr and not nearly)
    return n0


def _oracle_candidates(cfg, pose, comps, z):
    """The merge candidates of one particle as the oracle builds them
    (orc_debug_select / orc_debug_candidates of oracle/scphd_cpu.cpp)."""
    import ctypes

    import pyoracle
    L = pyoracle.lib()
    L.orc_debug_select.argtypes = [ctypes.c_int]
    L.orc_debug_candidates.restype = ctypes.c_long
    L.orc_debug_candidates.argtypes = [ctypes.c_void_p, ctypes.c_long]
    L.orc_debug_select(0)
    try:
        pyoracle.update(cfg, pose, comps, np.array([0, len(comps)], np.int32), z)
    finally:
        L.orc_debug_select(-1)
    buf = np.zeros(len(comps) * (len(z) + 1) + len(z) + 16, comps.dtype)
    n = L.orc_debug_candidates(ctypes.c_void_p(buf.ctypes.data), len(buf))
    assert 0 <= n <= len(buf)
    return buf[:n].copy()


def expected_update(cfg, poses, maps, offs, z, T, cardinality=False):
    """Expected device output of an update under metric 1 at minSeparation T:
    the oracle's unmerged candidates (its update at minSeparation 1e-12, where
    every candidate is its own output, in selection order: a stable order of the
    candidates by weight) through greedy(), the class-0 components appended.
    near per particle: greedy()'s count plus the oracle's near range
    classifications and near prunes (either changes the candidate list).
    Returns (maps, offsets, delta, near per particle[, cardinalities])."""
    import pyoracle
    c0 = cfg.copy()
    c0.minSeparation = 1e-12
    c0.distanceMetric = 0
    r = pyoracle.update(c0, poses, maps, offs, z, cardinality=cardinality)
    um, uo, delta = r[0], r[1], r[2]
    cls, pm = pyoracle.near_counts()  # near range classifications, near prunes (no merge is near at 1e-12)
    out, oo, near = [], [0], []
    for p in range(len(poses)):
        comps = maps[offs[p]:offs[p + 1]]
        n0 = n_out_of_range(cfg, poses[p], comps)
        mine = um[uo[p]:uo[p + 1]]
        cand, tail = mine[:len(mine) - n0], mine[len(mine) - n0:]
        cv = comps["cov"].astype(np.float64)
        if np.any(cv[:, 0] * cv[:, 3] - cv[:, 2] * cv[:, 1] <= 0):
            # a singular covariance: the oracle's own greedy stops at that
            # candidate's NaN own-distance, so its output at 1e-12 is cut short;
            # the full list is the oracle's candidate dump (update-array order)
            cand = _oracle_candidates(c0, poses[p:p + 1], comps, z)
        g, nr = greedy(cand, T)
        out += [g, tail]
        oo.append(oo[-1] + len(g) + len(tail))
        near.append(nr + int(cls[p]) + int(pm[p]))
    res = (np.concatenate(out) if out else np.zeros(0, um.dtype), np.array(oo, np.int32), delta,
           np.array(near, np.int32))
    return res + (r[4],) if cardinality else res
