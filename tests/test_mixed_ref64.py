"""The float64 reference of the mixed static + dynamic model
(tests/mixed_ref64.py) on the CPU:

1. closed forms for the reference itself, to 1e-9;
2. the input condition of every shared case (tests/mixed_ref64_cases.py): how
   many particles carry a near decision, from the reference alone, and that the
   case reaches what it is there for;
3. the oracle (orc_update_mixed / orc_predict_dynamic /
   orc_expected_map_dynamic, oracle/mixed_ref.h) against the reference on every
   case: the same sizes and decisions, and per class a worst deviation within
   the committed table D_ORACLE.
"""
import math

import numpy as np
import pytest

import mixed_ref64 as R
import mixed_ref64_cases as C
from phdslam.scenario import mixed_config
from phdslam.types import GAUSSIAN2D, GAUSSIAN4D, MEASUREMENT, POSE


def _one(cfg, s=None, d=None, z=()):
    """One particle at the origin, heading 0, with the given components and measurements."""
    sm = np.zeros(0 if s is None else len(s), GAUSSIAN2D)
    for i, (w, m, P) in enumerate(s or ()):
        sm[i]["weight"], sm[i]["mean"], sm[i]["cov"] = w, m, np.asarray(P, np.float64).T.ravel()
    dm = np.zeros(0 if d is None else len(d), GAUSSIAN4D)
    for i, (w, m, P) in enumerate(d or ()):
        dm[i]["weight"], dm[i]["mean"], dm[i]["cov"] = w, m, np.asarray(P, np.float64).T.ravel()
    zz = np.zeros(len(z), MEASUREMENT)
    for i, (r, b, lab) in enumerate(z):
        zz[i]["range"], zz[i]["bearing"], zz[i]["label"] = r, b, lab
    so, do = np.array([0, len(sm)], np.int32), np.array([0, len(dm)], np.int32)
    return R.update(cfg, np.zeros(1, POSE), sm, so, dm, do, zz)


def test_ref_one_static_feature_scalar_by_hand():
    """A feature on the x axis with a diagonal covariance, a measurement along the
    axis: range and bearing decouple into two scalar Kalman updates."""
    cfg = mixed_config(minSeparation=1e-12)
    w, x, a, b = 0.75, 8.0, 0.25, 0.5
    zr, zb = 8.5, 0.03125
    r = _one(cfg, s=[(w, (x, 0.0), np.diag([a, b]))], z=[(zr, zb, 0)])
    vr, vb = float(cfg.stdRange) ** 2, float(cfg.stdBearing) ** 2
    sr, sb = a + vr, b / x ** 2 + vb
    kr, kb = a / sr, (b / x) / sb
    q = cfg.pd * w * math.exp(-0.5 * ((zr - x) ** 2 / sr + zb ** 2 / sb)) / (2 * math.pi * math.sqrt(sr * sb))
    eta = q + float(cfg.clutterDensity) + float(cfg.birthWeight)
    assert abs(r.delta[0] - (math.log(eta) - cfg.pd * w)) <= 1e-9
    out = r.smaps
    assert len(out) == 3 and len(r.dmaps) == 0
    det = out[np.argmin(np.abs(out["weight"] - q / eta))]
    np.testing.assert_allclose(det["weight"], q / eta, rtol=1e-9)
    np.testing.assert_allclose(det["mean"], [x + kr * (zr - x), kb * zb], rtol=1e-9)
    np.testing.assert_allclose(det["cov"], [a - kr * a, 0, 0, b - kb * b / x], rtol=1e-9, atol=1e-15)
    nd = out[np.argmin(np.abs(out["weight"] - w * (1 - cfg.pd)))]
    np.testing.assert_allclose(nd["weight"], w * (1 - float(cfg.pd)), rtol=1e-9)
    birth = out[np.argmin(np.abs(out["weight"] - cfg.birthWeight / eta))]
    np.testing.assert_allclose(birth["mean"], [zr * math.cos(zb), zr * math.sin(zb)], rtol=1e-9)


def test_ref_one_dynamic_feature_along_the_axis_decouples():
    """A dynamic feature on the x axis whose covariance couples x with vx and y
    with vy only: the 4-D update is two 2-D (position, velocity) updates with
    scalar innovations."""
    cfg = mixed_config(minSeparation=1e-12)
    w, x = 0.625, 10.0
    Px = np.array([[0.5, 0.25], [0.25, 0.75]])   # (x, vx)
    Py = np.array([[0.375, -0.125], [-0.125, 0.625]])  # (y, vy)
    P = np.zeros((4, 4))
    P[np.ix_([0, 2], [0, 2])] = Px
    P[np.ix_([1, 3], [1, 3])] = Py
    zr, zb = 10.5, -0.03125
    r = _one(cfg, d=[(w, (x, 0.0, 1.0, -0.5), P)], z=[(zr, zb, 1)])
    vr, vb = float(cfg.stdRange) ** 2, float(cfg.stdBearing) ** 2
    sr, sb = Px[0, 0] + vr, Py[0, 0] / x ** 2 + vb
    q = cfg.pd * w * math.exp(-0.5 * ((zr - x) ** 2 / sr + zb ** 2 / sb)) / (2 * math.pi * math.sqrt(sr * sb))
    eta = q + float(cfg.clutterDensity) + float(cfg.birthWeight)
    assert abs(r.delta[0] - (math.log(eta) - cfg.pd * w)) <= 1e-9
    assert len(r.smaps) == 0 and len(r.dmaps) == 3
    det = r.dmaps[np.argmin(np.abs(r.dmaps["weight"] - q / eta))]
    np.testing.assert_allclose(det["weight"], q / eta, rtol=1e-9)
    kx = Px[:, 0] / sr             # gain of (x, vx) on the range innovation
    ky = (Py[:, 0] / x) / sb       # gain of (y, vy) on the bearing innovation
    np.testing.assert_allclose(det["mean"], [x + kx[0] * (zr - x), ky[0] * zb, 1.0 + kx[1] * (zr - x), -0.5 + ky[1] * zb],
                               rtol=1e-9)
    want = np.zeros((4, 4))
    want[np.ix_([0, 2], [0, 2])] = Px - np.outer(kx, Px[0])
    want[np.ix_([1, 3], [1, 3])] = Py - np.outer(ky, Py[0] / x)
    np.testing.assert_allclose(R.mat(det["cov"], 4), want, rtol=1e-9, atol=1e-15)
    birth = r.dmaps[np.argmin(np.abs(r.dmaps["weight"] - cfg.birthWeight / eta))]
    np.testing.assert_allclose(birth["mean"], [zr * math.cos(zb), zr * math.sin(zb), 0, 0], rtol=1e-9, atol=1e-15)
    assert birth["cov"][10] == float(cfg.covVxBirth) and birth["cov"][15] == float(cfg.covVyBirth)


def test_ref_two_equal_4d_components_merge():
    """Two components of equal weight and covariance P at m -+ e merge into
    weight 2 w, mean m, covariance P + e e'."""
    cfg = mixed_config(minSeparation=1e9)
    P = np.diag([0.25, 0.5, 1.0, 2.0]) + 0.125
    m, e = np.array([3.0, 4.0, 0.5, -0.25]), np.array([0.25, -0.125, 0.5, 0.0625])
    w = np.array([0.5, 0.5])
    out, near, _ = R.merge(cfg, w, np.stack([m - e, m + e]), np.stack([R.flat(P)] * 2), np.zeros(2), np.zeros(2), 4)
    assert len(out) == 1
    np.testing.assert_allclose(out[0]["weight"], 1.0, rtol=1e-9)
    np.testing.assert_allclose(out[0]["mean"], m, rtol=1e-9)
    np.testing.assert_allclose(R.mat(out[0]["cov"], 4), P + np.outer(e, e), rtol=1e-9)
    d, _ = R.distance(m - e, R.flat(P), (m + e)[None], R.flat(P)[None], np.zeros(2), 4)
    np.testing.assert_allclose(d[0], 4 * e @ np.linalg.inv(P) @ e, rtol=1e-9)


def test_ref_predict_one_component_written_out():
    cfg = mixed_config(dt=0.5)
    dt, qx, qy = 0.5, float(cfg.stdAxMap) ** 2, float(cfg.stdAyMap) ** 2
    g = np.zeros(1, GAUSSIAN4D)
    P = np.array([[0.5, 0.0625, 0.25, 0.0], [0.0625, 0.75, 0.0, -0.125], [0.25, 0.0, 1.0, 0.03125],
                  [0.0, -0.125, 0.03125, 2.0]])
    g[0]["weight"], g[0]["mean"], g[0]["cov"] = 0.5, (1.0, -2.0, 1.5, 2.0), P.T.ravel()
    o = R.predict(cfg, g)[0]
    np.testing.assert_allclose(o["mean"], [1.0 + dt * 1.5, -2.0 + dt * 2.0, 1.5, 2.0], rtol=1e-9)
    Po = R.mat(o["cov"], 4)
    np.testing.assert_allclose(Po[0, 0], P[0, 0] + 2 * dt * P[0, 2] + dt * dt * P[2, 2] + dt ** 4 / 4 * qx, rtol=1e-9)
    np.testing.assert_allclose(Po[1, 1], P[1, 1] + 2 * dt * P[1, 3] + dt * dt * P[3, 3] + dt ** 4 / 4 * qy, rtol=1e-9)
    np.testing.assert_allclose(Po[0, 2], P[0, 2] + dt * P[2, 2] + dt ** 3 / 2 * qx, rtol=1e-9)
    np.testing.assert_allclose(Po[1, 3], P[1, 3] + dt * P[3, 3] + dt ** 3 / 2 * qy, rtol=1e-9)
    np.testing.assert_allclose(Po[0, 1], P[0, 1] + dt * (P[2, 1] + P[0, 3]) + dt * dt * P[2, 3], rtol=1e-9)
    np.testing.assert_allclose(Po[0, 3], P[0, 3] + dt * P[2, 3], rtol=1e-9)
    np.testing.assert_allclose(Po[2, 2], P[2, 2] + dt * dt * qx, rtol=1e-9)
    np.testing.assert_allclose(Po[3, 3], P[3, 3] + dt * dt * qy, rtol=1e-9)
    np.testing.assert_allclose(Po[2, 3], P[2, 3], rtol=1e-9)
    np.testing.assert_allclose(Po, Po.T, rtol=0, atol=1e-15)
    v = 2.5
    np.testing.assert_allclose(o["weight"], 0.5 * cfg.ps / (1 + math.exp(cfg.beta * (cfg.tau - v))), rtol=1e-9)
    g[0]["mean"][2:] = (float(cfg.tau), 0.0)  # |v| = tau: the gate is one half
    np.testing.assert_allclose(R.predict(cfg, g)[0]["weight"], 0.25 * float(cfg.ps), rtol=1e-9)


def test_ref_two_particle_eap():
    """Two particles with one component each, P equal, at m -+ e, particle
    weights 1/4 and 3/4: W = w (1/4 + 3/4), the mean m + e / 2, the covariance
    P + (3/4) e e'; with a small minSeparation both come out, the heavier first."""
    cfg = mixed_config(minSeparation=1e9)
    P = np.diag([0.25, 0.5, 1.0, 2.0]) + 0.0625
    m, e = np.array([3.0, 4.0, 0.5, -0.25]), np.array([0.25, -0.125, 0.5, 0.0625])
    g = np.zeros(2, GAUSSIAN4D)
    g["weight"] = 0.5
    g["mean"] = np.stack([m - e, m + e])
    g["cov"] = P.T.ravel()
    lw = np.log([0.25, 0.75])
    out, near = R.expected_map(cfg, lw, g, np.array([0, 1, 2]))
    assert len(out) == 1 and near == 0
    np.testing.assert_allclose(out[0]["weight"], 0.5, rtol=1e-9)
    np.testing.assert_allclose(out[0]["mean"], m + e / 2, rtol=1e-9)
    np.testing.assert_allclose(R.mat(out[0]["cov"], 4), P + 0.75 * np.outer(e, e), rtol=1e-9)
    cfg.minSeparation = 1e-9
    out, _ = R.expected_map(cfg, lw, g, np.array([0, 1, 2]))
    np.testing.assert_allclose(out["weight"], [0.375, 0.125], rtol=1e-9)
    np.testing.assert_allclose(out["mean"], np.stack([m + e, m - e]), rtol=1e-9)


def test_ref_label_selects_the_map():
    """A labelled measurement contributes to the map of its label only; unlabelled
    scans add a second birth weight to the normaliser and births to both maps."""
    P4 = np.diag([0.25, 0.25, 0.5, 0.5])
    s, d = [(0.75, (10.0, 0.0), np.eye(2) * 0.25)], [(0.75, (10.0, 0.0, 0.0, 0.0), P4)]
    zr, zb = 10.5, 0.03125
    cfg = mixed_config(minSeparation=1e-12)
    a = _one(cfg, s=s, d=d, z=[(zr, zb, 0)])
    assert len(a.smaps) == 3 and len(a.dmaps) == 1  # static: non-detect, detect, birth; dynamic: non-detect
    cfg.labeledMeasurements = False
    b = _one(cfg, s=s, d=d, z=[(zr, zb, 0)])
    assert len(b.smaps) == 3 and len(b.dmaps) == 3
    k, beta = float(cfg.clutterDensity), float(cfg.birthWeight)
    vr, vb = float(cfg.stdRange) ** 2, float(cfg.stdBearing) ** 2
    sr, sb = 0.25 + vr, 0.25 / 100 + vb
    qs = float(cfg.pd) * 0.75 * math.exp(-0.5 * (0.25 / sr + zb * zb / sb)) / (2 * math.pi * math.sqrt(sr * sb))
    np.testing.assert_allclose(a.delta[0], math.log(qs + k + beta) - float(cfg.pd) * 1.5, rtol=1e-9)
    np.testing.assert_allclose(b.delta[0], math.log(2 * qs + k + 2 * beta) - float(cfg.pd) * 1.5, rtol=1e-9)


@pytest.mark.parametrize("name", C.CASES)
def test_case_input_condition(name):
    """At most 2 of 16 particles (1 of the smaller sets) left out whole, at most a
    quarter with any near decision; the device capacities of the case hold the
    reference's candidate and map counts."""
    out, any_near, n = C.shares(name)
    print(f"{name}: {out} of {n} left out, {any_near} of {n} with a near decision")
    assert out <= C.max_left_out(name)
    assert 4 * any_near <= n
    c, r = C.inputs(name), C.reference(name)
    assert C.candidate_counts(name).max() <= c.caps["K"]
    assert np.diff(r.soffs).max() <= c.caps["cap"] and np.diff(r.doffs).max() <= c.caps["dcap"]
    assert np.diff(c.soffs).max() <= c.caps["cap"] and np.diff(c.doffs).max() <= c.caps["dcap"]


def test_cases_reach_what_they_are_for():
    fov = C.inputs("mx_fov")
    cls_s = np.concatenate([R.classify(fov.cfg, fov.poses[p], fov.smaps[fov.soffs[p]:fov.soffs[p + 1]]["mean"], True)[0]
                            for p in range(16)])
    cls_d = np.concatenate([R.classify(fov.cfg, fov.poses[p], fov.dmaps[fov.doffs[p]:fov.doffs[p + 1]]["mean"][:, :2],
                                       False)[0] for p in range(16)])
    assert all((cls_s == k).any() and (cls_d == k).any() for k in (0, 1, 2))
    ch = C.inputs("mx_chunks")
    assert np.diff(ch.soffs).tolist() == [255, 256, 257, 300] and np.diff(ch.doffs).tolist() == [63, 64, 65, 257]
    assert C.candidate_counts("mx_chunks").max() > 256
    assert len(C.inputs("mx_manyz").z) == 257
    rg = C.inputs("mx_ragged")
    assert ((np.diff(rg.soffs) == 0) & (np.diff(rg.doffs) == 0)).any()
    pr = C.inputs("mx_predicted")
    P = R.mat(pr.dmaps["cov"].astype(np.float64), 4)
    rho = P[:, 0, 2] / np.sqrt(P[:, 0, 0] * P[:, 2, 2])
    assert np.median(rho) > 0.5 and np.linalg.cond(P).max() > 30
    sp = np.hypot(pr.dmaps["mean"][:, 2], pr.dmaps["mean"][:, 3])
    assert (sp < pr.cfg.tau).any() and (sp > pr.cfg.tau).any()
    # mx_cluster: merge sets wider than a wave whose members lie more than a chunk apart
    widest, span = C.merge_shape("mx_cluster")
    assert (widest > 64).all() and (span > 256).all(), (widest, span)
    # mx_ties: six births of exactly equal weight in each map, not counted as near
    ti, rt = C.inputs("mx_ties"), C.reference("mx_ties")
    assert not ti.cfg.labeledMeasurements
    eta0 = float(ti.cfg.clutterDensity) + 2 * float(ti.cfg.birthWeight)
    for p in range(len(ti.poses)):
        for m in (rt.smaps[rt.soffs[p]:rt.soffs[p + 1]], rt.dmaps[rt.doffs[p]:rt.doffs[p + 1]]):
            assert np.sum(m["weight"] == 2 * float(ti.cfg.birthWeight) / eta0) == 2  # two merged pairs
            assert np.sum(m["weight"] == float(ti.cfg.birthWeight) / eta0) == 2      # and the chains' far ends


def test_noscan_is_the_identity():
    """mx_noscan: the reference's driver runs no update on an empty scan
    (main.cpp:1260), so maps and weights are unchanged — reference and oracle."""
    import pyoracle
    c, r = C.inputs("mx_noscan"), C.reference("mx_noscan")
    assert np.array_equal(r.soffs, c.soffs) and np.array_equal(r.doffs, c.doffs) and not r.delta.any()
    os_, oso, od, odo, odelta, _ = pyoracle.update_mixed(C.config("mx_noscan"), c.poses, c.smaps, c.soffs, c.dmaps,
                                                         c.doffs, c.z)
    assert os_.tobytes() == c.smaps.tobytes() and od.tobytes() == c.dmaps.tobytes()
    assert np.array_equal(oso, c.soffs) and np.array_equal(odo, c.doffs) and not odelta.any()


def oracle_result(name):
    """(static maps, offsets, dynamic maps, offsets, lw + delta, the same normalised by the oracle)."""
    import pyoracle
    c = C.inputs(name)
    os_, oso, od, odo, odelta, _ = pyoracle.update_mixed(C.config(name), c.poses, c.smaps, c.soffs, c.dmaps, c.doffs,
                                                         c.z)
    olw = (c.lw + odelta).astype(np.float32)
    return os_, oso, od, odo, olw, pyoracle.normalize(olw)[0]


def _assert_table(label, worst, table, classes):
    for k in classes:
        assert worst[k] <= table[k], (label, k, worst[k], table[k])
        # the table is the measurement, not a bound above it
        assert table[k] <= 2 * worst[k] + 1e-12, (label, k, "table entry is stale", worst[k])


@pytest.mark.parametrize("name", C.CASES)
def test_oracle_against_reference(name):
    os_, oso, od, odo, olw, onorm = oracle_result(name)
    worst, bad, compared = C.deviations(name, os_, oso, od, odo, olw, onorm)
    print(f"{name}: " + ", ".join(f"{k} {worst[k]:.3g}" for k in C.CLASSES) + f" ({compared} particles)")
    assert not bad, bad
    assert compared >= len(olw) - C.max_left_out(name)
    _assert_table(name, worst, C.D_ORACLE[name], C.CLASSES)


@pytest.mark.parametrize("name", C.PREDICT_CASES)
def test_oracle_predict_against_reference(name):
    import pyoracle
    cfg, _, _, _, dm, _, _ = C.predict_inputs(name)
    worst = C.field_deviations(C.predict_reference(name), pyoracle.predict_dynamic(cfg.copy(), dm))
    print(f"{name}: " + ", ".join(f"{k} {worst[k]:.3g}" for k in C.FIELD_CLASSES))
    _assert_table(name, worst, C.D_ORACLE[name], C.FIELD_CLASSES)


@pytest.mark.parametrize("name", C.EAP_CASES)
def test_oracle_eap_against_reference(name):
    import pyoracle
    cfg, _, lw, _, _, dm, do, _ = C.eap_inputs(name)
    ref, near = C.eap_reference(name)
    assert near == 0, "the case has a near decision: pick another seed"
    worst = C.field_deviations(ref, pyoracle.expected_map_dynamic(cfg.copy(), lw, dm, do))
    assert worst is not None, "the oracle's EAP map has another size"
    print(f"{name}: " + ", ".join(f"{k} {worst[k]:.3g}" for k in C.FIELD_CLASSES) + f" ({len(ref)} components)")
    _assert_table(name, worst, C.D_ORACLE[name], C.FIELD_CLASSES)
