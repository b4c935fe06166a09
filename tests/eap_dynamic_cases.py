"""Hand-built dynamic (Gaussian4D) stores for the decision rounds of the dynamic
expected map (k_eap4_lfmis and its stages, phd_mixed.hip), shared by
tests/test_eap_dynamic_cases.py (CPU: the oracle on every case gives what the
case is named for), tests/test_gpu_eap_dynamic_rounds.py and
tests/test_eap_dynamic_rounds_sharded.py.

A case is a dict: comps (Gaussian4D, concatenation order), sizes (components
per particle, in order), lw (log-weight per particle), T (minSeparation),
n_out (what the greedy must emit, None: not fixed by construction), fallback
(the one-workgroup form must serve it: cells == 0), cells (the exact occupied
cell count, or None), multi_cell (cells > 1).

The sizes follow the kernel's constants: CHUNK = TILE = 256 (EAP4R_NT: the
positions of a work item and the records of a streamed tile) and PASS = 64
(EAP4_PASS: the members one LDS staging pass of the sums holds).
"""
import math

import numpy as np

from phdslam.types import GAUSSIAN4D

CHUNK = 256
TILE = 256
PASS = 64
DCAP = 64
T0 = 4.0

THIN = 1e-4  # variance of the coordinates a case does not use


def comps(means, cov, w):
    """len(means) components of one covariance (4 x 4, row-major = column-major: symmetric)."""
    means = np.asarray(means, np.float64).reshape(-1, 4)
    d = np.zeros(len(means), GAUSSIAN4D)
    d["mean"] = means.astype(np.float32)
    d["cov"] = np.asarray(cov, np.float64).T.reshape(16).astype(np.float32)
    d["weight"] = np.asarray(w, np.float32)
    return d


def diag(a, b, c, e):
    return np.diag([a, b, c, e]).astype(np.float64)


POS = diag(0.1, 0.1, 0.5, 0.5)  # d = |dpos|^2 / 0.1 + |dvel|^2 / 0.5


def lam_of(c):
    """Λ as k_eap4_bound computes it: the largest float trace c0 + c5 + c10 + c15."""
    cv = c["cov"].astype(np.float32)
    tr = ((cv[:, 0] + cv[:, 5]) + cv[:, 10]) + cv[:, 15]
    return float(tr.max()) if len(tr) else 0.0


def side(c, T=T0):
    """The lattice cell side R of a case (eap4_rounds)."""
    return math.sqrt(1.05 * float(np.float32(T)) * lam_of(c)) * 1.0001


def cell_keys(c, T=T0):
    """Cell (cx, cy) of every component, as k_eap_poskey computes it."""
    inv = float(np.float32(1.0 / side(c, T)))
    return np.floor(c["mean"][:, :2].astype(np.float64) * inv).astype(np.int64)


def mahal4(a, b):
    """float64 distance of two components (LLT of the averaged covariance);
    nan when the average is not positive definite."""
    s = 0.5 * (a["cov"].astype(np.float64).reshape(4, 4).T + b["cov"].astype(np.float64).reshape(4, 4).T)
    s = np.tril(s) + np.tril(s, -1).T
    try:
        L = np.linalg.cholesky(s)
    except np.linalg.LinAlgError:
        return float("nan")
    x = np.linalg.solve(L, a["mean"].astype(np.float64) - b["mean"].astype(np.float64))
    return float(x @ x)


def case(c, sizes=None, lw=None, T=T0, n_out=None, fallback=False, cells=None, multi_cell=False, per=DCAP):
    K = len(c)
    if sizes is None:  # consecutive particles of `per` components, the last one short
        sizes = [per] * (K // per) + ([K % per] if K % per or K == 0 else [])
    sizes = np.asarray(sizes, np.int64)
    assert sizes.sum() == K and (sizes <= DCAP).all()
    n = len(sizes)
    lw = np.full(n, -math.log(n), np.float32) if lw is None else np.asarray(lw, np.float32)
    assert len(lw) == n
    return dict(comps=c, sizes=sizes, lw=lw, T=T, n_out=n_out, fallback=fallback, cells=cells, multi_cell=multi_cell)


def offsets(cs):
    return np.concatenate([[0], np.cumsum(cs["sizes"])]).astype(np.int32)


# ------------------------------------------------------------------ the cases

def k1():
    return case(comps([[1, 2, 0.5, -0.5]], POS, [0.7]), n_out=1, cells=1)


def k2_merging():
    return case(comps([[1, 2, 0, 0], [1.3, 2, 0, 0]], POS, [0.7, 0.6]), n_out=1, cells=1)


def k2_apart():
    return case(comps([[1, 2, 0, 0], [2.0, 2, 0, 0]], POS, [0.7, 0.6]), n_out=2, cells=1)


def one_cell(npos):
    """npos positions in one lattice cell (a box well inside [0, R)^2), many
    seeds among them: the cell is split over ceil(npos / CHUNK) workgroups."""
    rng = np.random.default_rng(100 + npos)
    m = np.concatenate([rng.uniform(0.1, 2.1, (npos, 2)), rng.normal(0, 0.3, (npos, 2))], 1)
    c = comps(m, POS, rng.uniform(0.2, 1.0, npos))
    assert side(c) > 2.2 and len(np.unique(cell_keys(c), axis=0)) == 1
    return case(c, cells=1)


def neighbour_stream(nrec):
    """A cell of nrec heavy records beside a cell of five light ones close to
    the border: the light ones' workgroup streams the neighbour's nrec records."""
    rng = np.random.default_rng(200 + nrec)
    R = math.sqrt(1.05 * T0 * 1.2) * 1.0001
    heavy = np.concatenate([rng.uniform([0.1, 0.1], [R - 0.05, R - 0.1], (nrec, 2)), rng.normal(0, 0.3, (nrec, 2))], 1)
    light = np.concatenate([rng.uniform([R + 0.01, 0.1], [R + 0.4, R - 0.1], (5, 2)), rng.normal(0, 0.3, (5, 2))], 1)
    c = np.concatenate([comps(heavy, POS, rng.uniform(0.5, 1.0, nrec)), comps(light, POS, rng.uniform(0.1, 0.4, 5))])
    keys = cell_keys(c)
    assert (keys[:nrec] == [0, 0]).all() and (keys[nrec:] == [1, 0]).all()
    return case(c, cells=2, multi_cell=True)


def stream_ends_early():
    """One seed and 599 light copies of it within T: after the first tile every
    thread has its decider, so the second and third tiles are never streamed."""
    rng = np.random.default_rng(7)
    m = np.array([1.0, 1.0, 0.2, -0.2]) + rng.normal(0, 0.02, (600, 4))
    w = np.concatenate([[0.9], rng.uniform(0.1, 0.5, 599)])
    return case(comps(m, POS, w), n_out=1, cells=1)


def chain(axis):
    """A - B - C with B within T of A, C within T of B only, weights A > B > C:
    A absorbs B, C (whose first candidate is B) is a seed.  Two outputs.  Along
    x, y and the diagonal the three lie in three cells; in velocity only they
    share the position, so the cell."""
    w = [0.9, 0.6, 0.3]
    if axis == "x":
        cov, m = diag(0.1, THIN, THIN, THIN), [[0.6, 0.3, 0, 0], [1.2, 0.3, 0, 0], [1.8, 0.3, 0, 0]]
    elif axis == "y":
        cov, m = diag(THIN, 0.1, THIN, THIN), [[0.3, -0.1, 0, 0], [0.3, -0.7, 0, 0], [0.3, -1.3, 0, 0]]
    elif axis == "diagonal":
        cov = diag(0.05, 0.05, THIN, THIN)
        cov[0, 1] = cov[1, 0] = 0.0499
        m = [[0.6, 0.6, 0, 0], [1.02, 1.02, 0, 0], [1.44, 1.44, 0, 0]]
    else:
        cov, m = diag(THIN, THIN, 0.1, THIN), [[0.3, 0.3, 0.0, 1], [0.3, 0.3, 0.6, 1], [0.3, 0.3, 1.2, 1]]
    c = comps(m, cov, w)
    dAB, dBC, dAC = mahal4(c[0], c[1]), mahal4(c[1], c[2]), mahal4(c[0], c[2])
    assert dAB < T0 * 0.95 and dBC < T0 * 0.95 and dAC > T0 * 1.5, (dAB, dBC, dAC)
    ncell = len(np.unique(cell_keys(c), axis=0))
    assert ncell == (1 if axis == "velocity" else 3), cell_keys(c)
    # one component per particle, and a far bystander
    far = comps([[30, 30, 0, 0]], cov, [0.5])
    return case(np.concatenate([c, far]), sizes=[1, 1, 1, 1], n_out=3, cells=ncell + 1, multi_cell=True)


def ties(order):
    """Equal weights and equal log-weights: X, Y, Z 0.5 apart in a row (d = 2.5
    between neighbours, 10 between X and Z), each in a particle of its own.  In
    the order X, Y, Z the first (X) absorbs Y alone: Z stays.  With Y first it
    absorbs both.  Five exact duplicates elsewhere merge into one."""
    xs = {"XYZ": [10.0, 10.5, 11.0], "YXZ": [10.5, 10.0, 11.0]}[order]
    row = comps([[x, 3.0, 0.5, -0.5] for x in xs], POS, [0.7] * 3)
    dup = comps([[-4.0, -7.0, 0.1, 0.1]] * 5, POS, [0.4] * 5)
    c = np.concatenate([row[:1], dup[:2], row[1:2], dup[2:], row[2:]])
    return case(c, sizes=[1, 2, 1, 3, 1], n_out=(2 if order == "XYZ" else 1) + 1, multi_cell=True)


def around_T():
    """Pairs 0.63 apart (d = 3.969: merge) and 0.635 apart (d = 4.03: do not),
    inside a cell and across the borders at -2R .. 2R, and pairs whose heavier
    component lies exactly on a float multiple of R; rows 10 apart in y
    (positive and negative), so the pairs do not meet."""
    R = math.sqrt(1.05 * T0 * 1.2) * 1.0001
    m, n_out = [], 0
    row = 0
    for mult in (-2, -1, 0, 1, 2):
        for gap, merges in ((0.63, True), (0.635, False)):
            for x0 in (mult * R - 0.3, mult * R + 0.5, float(np.float32(mult * R))):
                y = 10.0 * (row - 14)
                row += 1
                m += [[x0, y, 0, 0], [x0 + gap, y, 0, 0]]
                n_out += 1 if merges else 2
    c = comps(m, POS, np.tile([0.8, 0.5], len(m) // 2))
    assert abs(side(c) - R) < 1e-5 and (c["mean"][:, 1] < 0).any() and (c["mean"][:, 0] < 0).any()
    return case(c, n_out=n_out, multi_cell=True, per=7)


def rank_one(cond):
    """Nearly rank-1 position covariances (condition `cond`), thick axis at 30
    degrees: partners along the thick axis at 1.5 and 2.5 sigma and along the
    thin axis at 1.5 and 3 thin sigmas.  (What merges at this conditioning is the
    float LLT's own answer: every form must give the same.)"""
    th = math.radians(30.0)
    u, v = np.array([math.cos(th), math.sin(th)]), np.array([-math.sin(th), math.cos(th)])
    cov = np.zeros((4, 4))
    cov[:2, :2] = 1.0 * np.outer(u, u) + (1.0 / cond) * np.outer(v, v)
    cov[2, 2] = cov[3, 3] = 0.01
    ts = 1.0 / math.sqrt(cond)
    m, w = [], []
    for g, base in enumerate(([0.0, 0.0], [40.0, -25.0], [-33.0, 18.0], [7.0, 60.0])):
        b = np.array(base)
        for off in (0 * u, 1.5 * u, 2.5 * u, 1.5 * ts * v, 3.0 * ts * v, -1.5 * u + 1.5 * ts * v):
            m.append(list(b + off) + [0.0, 0.0])
            w.append(0.9 - 0.025 * len(w))
    return case(comps(m, cov, w), multi_cell=True, per=5)


def huge_velocity_variance():
    """One component's velocity variance is 1e6: Λ, so the cell side, grows
    until the whole store (positions within +-18) shares one cell."""
    rng = np.random.default_rng(11)
    m = np.concatenate([rng.uniform(1.0, 18.0, (150, 2)), rng.normal(0, 1.0, (150, 2))], 1)
    c = comps(m, POS, rng.uniform(0.2, 1.0, 150))
    c[17]["cov"] = diag(0.1, 0.1, 1e6, 1e6).reshape(16).astype(np.float32)
    assert side(c) > 2000 and len(np.unique(cell_keys(c), axis=0)) == 1
    return case(c, cells=1, per=30)


def not_positive_definite():
    """Three copies of a finite covariance that is not positive definite
    (variances 0.1, covariance 0.2), and ordinary components at the same mean
    and near it: no pair with a copy merges (the averaged covariance has a
    non-positive pivot), the two ordinary ones do.  Stays on the rounds."""
    bad = diag(0.1, 0.1, 0.5, 0.5)
    bad[0, 1] = bad[1, 0] = 0.2
    c = np.concatenate([comps([[2, 2, 0, 0]] * 3, bad, [0.9, 0.8, 0.7]),
                        comps([[2, 2, 0, 0], [2.1, 2, 0, 0]], POS, [0.6, 0.5])])
    assert all(not mahal4(c[i], c[j]) < T0 for i in range(3) for j in range(5) if i != j)
    return case(c, sizes=[2, 3], n_out=4, cells=1)


def _spread(K, seed):
    rng = np.random.default_rng(seed)
    m = np.concatenate([rng.uniform(-18, 18, (K, 2)), rng.normal(0, 1.0, (K, 2))], 1)
    return comps(m, POS, rng.uniform(0.2, 1.0, K))


def fallback(kind):
    """Inputs the lattice bound does not cover: the one-workgroup form serves
    them (cells == 0), with the same output."""
    c = _spread(40, 31)
    c["mean"][5] = c["mean"][4]  # (a few that merge)
    c["mean"][6] = c["mean"][4]
    T = T0
    if kind == "nan_mean":
        c["mean"][9, 1] = np.nan
    elif kind == "inf_cov":
        c["cov"][12, 10] = np.inf
    elif kind == "zero_trace":
        c["cov"][:] = 0.0
    elif kind == "T_zero":
        T = 0.0
    elif kind == "negative_variance":
        c["cov"][3, 15] = -0.5
    elif kind == "tiny_variance":
        c["cov"][3, 15] = 1e-30
    return case(c, T=T, fallback=True, per=8, n_out=40 if kind in ("zero_trace", "T_zero") else None)


def zero_weights():
    """Zero-weight components: some within T of a heavier one (absorbed, adding
    nothing), one on its own far away (a seed of weight 0, last in priority)."""
    c = _spread(30, 41)
    for i in (3, 8, 20):
        c["mean"][i] = c["mean"][i - 1] + np.float32(0.05)
        c["weight"][i] = 0.0
    c["mean"][29] = (60.0, 60.0, 0.0, 0.0)
    c["weight"][29] = 0.0
    return case(c, multi_cell=True, per=6)


def empty_store():
    return case(np.zeros(0, GAUSSIAN4D), sizes=[0, 0, 0], n_out=0)


def empty_between():
    """Particles with empty dynamic maps between full ones."""
    c = _spread(2 * DCAP + 3, 51)
    return case(c, sizes=[0, DCAP, 0, 0, 3, DCAP, 0], multi_cell=True)


def big_group(members):
    """A seed with `members` absorbed components (PASS - 1, PASS, PASS + 1: the
    sums' staging passes), beside a few others."""
    rng = np.random.default_rng(300 + members)
    m = np.array([5.0, -3.0, 0.4, 0.1]) + rng.normal(0, 0.02, (members + 1, 4))
    grp = comps(m, POS, np.concatenate([[0.95], rng.uniform(0.1, 0.5, members)]))
    c = np.concatenate([grp, _spread(6, 61) ])
    c["mean"][members + 1:, :2] += 40.0
    return case(c, multi_cell=True, per=33)


CASES = {
    "k1": k1, "k2_merging": k2_merging, "k2_apart": k2_apart,
    **{f"one_cell_{n}": (lambda n=n: one_cell(n)) for n in (CHUNK - 1, CHUNK, CHUNK + 1)},
    **{f"neighbour_stream_{n}": (lambda n=n: neighbour_stream(n)) for n in (TILE - 1, TILE, TILE + 1)},
    "stream_ends_early": stream_ends_early,
    **{f"chain_{a}": (lambda a=a: chain(a)) for a in ("x", "y", "diagonal", "velocity")},
    "ties_XYZ": lambda: ties("XYZ"), "ties_YXZ": lambda: ties("YXZ"),
    "around_T": around_T,
    **{f"rank_one_{c:g}": (lambda c=c: rank_one(c)) for c in (1e5, 1e6, 1e8)},
    "huge_velocity_variance": huge_velocity_variance,
    "not_positive_definite": not_positive_definite,
    **{f"fallback_{k}": (lambda k=k: fallback(k)) for k in ("nan_mean", "inf_cov", "zero_trace", "T_zero",
                                                           "negative_variance", "tiny_variance")},
    "zero_weights": zero_weights,
    "empty_store": empty_store, "empty_between": empty_between,
    **{f"big_group_{m}": (lambda m=m: big_group(m)) for m in (PASS - 1, PASS, PASS + 1)},
}
