"""The float64 reference of the update (tests/update_ref64.py) on the CPU:

1. closed forms for the reference itself (the targets of
   tests/test_oracle_closed_form.py, held here to float64 accuracy);
2. the input condition of every shared case (tests/update_ref64_cases.py): how
   many particles carry a near decision, from the reference alone;
3. the oracle (oracle/scphd_cpu.cpp) against the reference on every case: the
   same sizes and decisions, and per field class a worst deviation within the
   committed table D_ORACLE — the measured distance of the oracle's float32
   arithmetic and of the shared include/phd_detmath.h routines from plain
   double arithmetic.
"""
import math

import numpy as np
import pytest

import parity
import test_oracle_closed_form as OC
import update_ref64 as R
import update_ref64_cases as C
from phdslam.types import GAUSSIAN2D, MEASUREMENT, POSE


def _update1(cfg, poses, maps, offs, z):
    r = R.update(cfg, poses, maps, offs, z)
    return r.maps, r.offsets, r.delta


def test_ref_measurement_at_the_predicted_range_and_bearing():
    """One component, one measurement exactly at its predicted (r, b): nu = 0, so
    q = pd w / (2 pi sqrt|S|), the mean stays, the covariance is the Joseph form.
    (minSeparation 1e-30: the three candidates lie within the float32 rounding
    of the bearing of one another and must still come out unmerged.)"""
    cfg = OC._cfg(minSeparation=1e-30)
    P = np.array([[0.1, 0.02], [0.02, 0.15]])
    poses, maps, offs, z = OC._one_particle([3.0, 4.0], P, 0.8, [(5.0, math.atan2(4.0, 3.0))])
    Pf = maps[0]["cov"].astype(np.float64).reshape(2, 2).T
    zr, zb = float(z[0]["range"]), float(z[0]["bearing"])
    cf = OC._closed_form(cfg, [3.0, 4.0], Pf, float(maps[0]["weight"]), zr, zb)
    out, oo, delta = _update1(cfg, poses, maps, offs, z)
    assert oo[1] == 3
    np.testing.assert_allclose(delta[0], cf["delta"], rtol=1e-12)
    w = float(maps[0]["weight"])
    want = sorted([w * (1 - cfg.pd), cf["q"] / cf["eta"], cfg.birthWeight / cf["eta"]], reverse=True)
    np.testing.assert_allclose(sorted(out["weight"], reverse=True), want, rtol=1e-12)
    det = out[np.argmin(np.abs(out["weight"] - cf["q"] / cf["eta"]))]
    np.testing.assert_allclose(det["mean"], cf["mu"], rtol=1e-12)
    np.testing.assert_allclose(det["mean"], [3.0, 4.0], atol=1e-6)  # nu = 0 up to the float32 bearing
    np.testing.assert_allclose(det["cov"].reshape(2, 2).T, cf["P"], rtol=1e-10, atol=1e-15)


def test_ref_off_centre_measurement_closed_form():
    cfg = OC._cfg(minSeparation=1e-12)
    P = np.array([[0.1, 0.02], [0.02, 0.15]])
    poses, maps, offs, z = OC._one_particle([10.0, 1.0], P, 0.8, [(10.2, 0.11)])
    Pf = maps[0]["cov"].astype(np.float64).reshape(2, 2).T
    cf = OC._closed_form(cfg, [10.0, 1.0], Pf, float(maps[0]["weight"]), float(z[0]["range"]), float(z[0]["bearing"]))
    out, oo, delta = _update1(cfg, poses, maps, offs, z)
    assert oo[1] == 3
    np.testing.assert_allclose(delta[0], cf["delta"], rtol=1e-12)
    det = out[np.argmin(np.abs(out["weight"] - cf["q"] / cf["eta"]))]
    np.testing.assert_allclose(det["weight"], cf["q"] / cf["eta"], rtol=1e-11)
    np.testing.assert_allclose(det["mean"], cf["mu"], rtol=1e-12)
    np.testing.assert_allclose(det["cov"].reshape(2, 2).T, cf["P"], rtol=1e-10, atol=1e-15)


def test_ref_full_merge():
    """minSeparation 1e9: everything merges (the oracle's full-merge case); two
    identical nearly-in-range components merge into one of twice the weight."""
    cfg = OC._cfg(minSeparation=1e9)
    P = np.array([[0.1, 0.0], [0.0, 0.1]])
    poses, maps, offs, z = OC._one_particle([10.0, 0.0], P, 0.8, [(10.1, 0.005)])
    Pf = maps[0]["cov"].astype(np.float64).reshape(2, 2).T
    w = float(maps[0]["weight"])
    cf = OC._closed_form(cfg, [10.0, 0.0], Pf, w, float(z[0]["range"]), float(z[0]["bearing"]))
    out, oo, _ = _update1(cfg, poses, maps, offs, z)
    assert oo[1] == 1
    W = w * (1 - cfg.pd) + cf["q"] / cf["eta"] + cfg.birthWeight / cf["eta"]
    np.testing.assert_allclose(out[0]["weight"], W, rtol=1e-12)
    assert out[0]["cov"][1] == out[0]["cov"][2]
    cfg = OC._cfg(maxRange=20.0, minSeparation=1.0)
    maps = np.zeros(2, GAUSSIAN2D)
    maps["mean"] = (22.0, 1.0)
    maps["cov"] = (0.1, 0.02, 0.02, 0.3)
    maps["weight"] = 0.25
    z = np.zeros(1, MEASUREMENT)
    z[0]["range"], z[0]["bearing"] = 5.0, 1.0
    out, oo, _ = _update1(cfg, np.zeros(1, POSE), maps, np.array([0, 2], np.int32), z)
    twin = out[np.argmax(out["weight"])]
    assert twin["weight"] == 0.5 and np.array_equal(twin["mean"], [22.0, 1.0])
    np.testing.assert_allclose(twin["cov"], maps[0]["cov"].astype(np.float64), rtol=1e-15)


def test_ref_out_of_range_passthrough_and_near_range_merge():
    cfg = OC._cfg(maxRange=20.0)
    maps = np.zeros(3, GAUSSIAN2D)
    for i, (x, y) in enumerate([(10.0, 0.0), (22.0, 0.0), (60.0, 0.0)]):  # in, nearly (<= 1.2 maxR), far
        maps[i]["mean"] = (x, y)
        maps[i]["cov"] = (0.1, 0.0, 0.0, 0.1)
        maps[i]["weight"] = 0.7
    z = np.zeros(1, MEASUREMENT)
    z[0]["range"], z[0]["bearing"] = 5.0, 1.0
    r = R.update(cfg, np.zeros(1, POSE), maps, np.array([0, 3], np.int32), z)
    assert r.maps[-1]["mean"][0] == 60.0 and r.maps[-1]["weight"] == float(np.float32(0.7))
    assert any(g["mean"][0] == 22.0 and g["weight"] == float(np.float32(0.7)) for g in r.maps[:-1])
    assert r.cls[0] == 0
    cls = R.classify(cfg, np.zeros(1, POSE)[0], maps["mean"])[0]
    assert cls.tolist() == [1, 2, 0]


def test_ref_labelled_dynamic_measurement_gets_no_detection_or_birth():
    cfg = OC._cfg(labeledMeasurements=True, minSeparation=1e-12)
    poses, maps, offs, z = OC._one_particle([10.0, 0.0], np.eye(2) * 0.1, 0.8, [(10.0, 0.0)])
    z[0]["label"] = 1
    out, oo, delta = _update1(cfg, poses, maps, offs, z)
    assert oo[1] == 1
    w = float(maps[0]["weight"])
    np.testing.assert_allclose(out[0]["weight"], w * (1 - cfg.pd), rtol=1e-15)
    # eta = kappa + beta: no likelihood term joins it
    np.testing.assert_allclose(delta[0], math.log(cfg.clutterDensity + cfg.birthWeight) - (cfg.pd * w + cfg.birthWeight),
                               rtol=1e-12)


def test_ref_cphd_poisson_equivalence():
    """As test_cphd_poisson_equivalence: with a Poisson predicted cardinality
    whose mean is the in-range mass the GM-CPHD update is the GM-PHD update,
    <Psi0,p> = sum_m log(kappa + sum_j q_jm) - pd W - lambda_c + M log(lambda_c / kappa)."""
    c, poses, lw, maps, offs, z = OC._cphd_case()
    c.filterType = 0
    a = R.update(c, poses, maps, offs, z)
    c.filterType = 1
    b = R.update(c, poses, maps, offs, z)
    assert np.array_equal(a.offsets, b.offsets)
    for p in range(len(poses)):
        ok, worst = parity.compare_maps(a.maps[a.offsets[p]:a.offsets[p + 1]], b.maps[b.offsets[p]:b.offsets[p + 1]],
                                        rtol=1e-9)
        assert ok, (p, worst)
    lam = float(c.clutterRate)
    expect = a.delta - lam + len(z) * math.log(lam / c.clutterDensity)
    np.testing.assert_allclose(b.delta, expect, rtol=0, atol=1e-9 * np.abs(expect).max())
    np.testing.assert_allclose(np.log(np.sum(np.exp(b.cn), 1)), 0.0, atol=1e-12)
    W = np.array([maps[offs[p]:offs[p + 1]]["weight"].astype(np.float64).sum() for p in range(len(poses))])
    assert np.all(np.sum(np.exp(b.cn) * np.arange(b.cn.shape[1]), 1) > W * (1 - c.pd))


def test_ref_cphd_empty_map():
    """D10: an empty predicted map has cardinality delta_0 and delta = M log lambda_c - lambda_c."""
    c, poses, lw, maps, offs, z = OC._cphd_case(n=2, M=5)
    c.filterType = 1
    r = R.update(c, poses, maps[:0], np.zeros(3, np.int32), z)
    lam = float(c.clutterRate)
    np.testing.assert_allclose(r.delta, 5 * math.log(lam) - lam, rtol=1e-14)
    assert np.all(r.cn[:, 0] == 0) and np.all(np.isneginf(r.cn[:, 1:])) and r.offsets[-1] == 0


@pytest.mark.parametrize("M", [1, 2, 5, 8])
def test_ref_esf_against_polynomial_coefficients(M):
    lam = np.random.default_rng(M).uniform(0.01, 30.0, M)
    want = np.poly(-lam)  # prod (x + lambda_m) = sum_k e_k x^(M-k)
    np.testing.assert_allclose(np.exp(R.esf_log(np.log(lam))), want, rtol=1e-12)
    for m in range(M):
        np.testing.assert_allclose(np.exp(R.esf_log(np.log(np.delete(lam, m)))), np.poly(-np.delete(lam, m)), rtol=1e-12)
    with_zero = np.concatenate([np.log(lam), [-np.inf]])
    np.testing.assert_allclose(np.exp(R.esf_log(with_zero)), np.concatenate([want, [0.0]]), rtol=1e-12)


def test_ref_near_band():
    """The band is max(NEAR T, C bound): the oracle's 1e-4 floor, widened where
    the float32 bound of the decided value is larger."""
    assert R._near(10.0009, 10.0, 0.0) and not R._near(10.0011, 10.0, 0.0)
    assert R._near(10.004, 10.0, 0.0021) and not R._near(10.0043, 10.0, 0.0021)
    # a pair far from the origin and close together: the mean difference cancels
    d, b = R.distance(0, np.array([4000.0, 0.0]), np.array([1e-4, 0, 0, 1e-4]), np.array([[4000.03, 0.0]]),
                      np.array([[1e-4, 0, 0, 1e-4]]), np.zeros(2))
    assert abs(d[0] - 9.0) < 1e-6 and b[0] > 1e-3 * d[0]


@pytest.mark.parametrize("name", C.CASES)
def test_case_input_condition(name):
    """At most 2 of 16 particles (1 of 4) left out whole, at least half without any near decision."""
    out, any_near, n = C.shares(name)
    print(f"{name}: {out} of {n} left out, {any_near} of {n} with a near decision")
    assert n == (4 if name == "tiny" else 16)
    assert out <= C.max_left_out(name)
    assert 2 * (n - any_near) >= n


def oracle_result(name):
    """(maps, offsets, lw + delta, the same normalised by the oracle, cn rows or None)."""
    import hellinger_ref
    import pyoracle
    cfg, poses, lw, maps, offs, z = C.inputs(name)
    cn = None
    if cfg.distanceMetric == 1:
        om, oo, od = hellinger_ref.expected_update(C.config(name), poses, maps, offs, z, cfg.minSeparation)[:3]
    elif cfg.filterType == 1:
        om, oo, od, _, cn = pyoracle.update(C.config(name), poses, maps, offs, z, cardinality=True)
    else:
        om, oo, od, _ = pyoracle.update(C.config(name), poses, maps, offs, z)
    olw = (lw + od).astype(np.float32)
    return om, oo, olw, pyoracle.normalize(olw)[0], cn


@pytest.mark.parametrize("name", C.CASES)
def test_oracle_against_reference(name):
    om, oo, olw, onorm, cn = oracle_result(name)
    worst, bad, compared = C.deviations(name, om, oo, olw, onorm, cn)
    print(f"{name}: " + ", ".join(f"{k} {worst[k]:.3g}" for k in C.CLASSES) + f" ({compared} particles)")
    assert not bad, bad
    assert compared >= len(olw) - C.max_left_out(name)
    for k in C.CLASSES:
        assert worst[k] <= C.D_ORACLE[name][k], (name, k, worst[k], C.D_ORACLE[name][k])
        # the table is the measurement, not a bound above it
        assert C.D_ORACLE[name][k] <= 2 * worst[k] + 1e-12, (name, k, "table entry is stale", worst[k])
