"""The float64 reference of the pose prediction, the estimates and the static
EAP map (tests/state_ref64.py) on the CPU:

1. closed forms for the reference itself, and its Philox against the Random123
   known answers;
2. the input condition of every shared case (tests/state_ref64_cases.py), from
   the reference alone: no near decision in any EAP case, and that each case
   reaches what it is there for;
3. the oracle (pyoracle.predict_* / noise_* / expected_pose / expected_map)
   against the reference on every case: the same counts and order, and per
   class a worst deviation within the committed table D_ORACLE.
"""
import math

import numpy as np
import pytest

import state_ref64 as R
import state_ref64_cases as C
import weighting_ref
from phdslam.types import ACKERMAN_NOISE, CV_NOISE, GAUSSIAN2D, POSE


def _cfg(**kw):
    import phdslam
    c = phdslam.config_scenario(2, n=1, G=1, M=1)[0]
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def _pose(**kw):
    p = np.zeros(1, POSE)
    for k, v in kw.items():
        p[k] = v
    return p


# ---------------------------------------------------------------- closed forms

def test_ref_ackerman_straight_line_and_standstill():
    cfg = _cfg(subdividePredict=2)
    dt = float(cfg.dt) / 2
    p = _pose(px=1.0, py=-2.0, ptheta=0.75, vx=9.0, vy=9.0, vtheta=9.0)
    o = R.predict_ackerman(cfg, p, 3.0, 0.0, np.zeros(1, ACKERMAN_NOISE))[0]
    np.testing.assert_allclose([o["px"], o["py"], o["ptheta"]],
                               [1.0 + dt * 3.0 * math.cos(0.75), -2.0 + dt * 3.0 * math.sin(0.75), 0.75], rtol=1e-12)
    assert o["vx"] == 0 and o["vy"] == 0 and o["vtheta"] == 0
    o = R.predict_ackerman(cfg, p, 0.0, 0.3, np.zeros(1, ACKERMAN_NOISE))[0]
    assert (o["px"], o["py"], o["ptheta"]) == (1.0, -2.0, 0.75)


def test_ref_ackerman_sensor_offset_terms():
    """Heading 0: the sensor, a ahead and b beside the axle, moves with the axle
    centre plus the turn: x' = x + Dt (vc - rate b), y' = y + Dt rate a."""
    cfg = _cfg()
    dt, l, h, a, b = (float(getattr(cfg, k)) for k in ("dt", "l", "h", "a", "b"))
    nz = np.zeros(1, ACKERMAN_NOISE)
    nz["n_alpha"], nz["n_encoder"] = 0.05, -0.5
    ta = math.tan(0.25 + float(nz["n_alpha"][0]))
    vc = (2.0 + float(nz["n_encoder"][0])) / (1 - ta * h / l)
    o = R.predict_ackerman(cfg, _pose(), 2.0, 0.25, nz)[0]
    np.testing.assert_allclose([o["px"], o["py"], o["ptheta"]],
                               [dt * (vc - vc * ta / l * b), dt * vc * ta / l * a, dt * vc * ta / l], rtol=1e-12)
    assert b > 0 and a > 0 and o["py"] > 0


def test_ref_cv_straight_line_and_heading_ramp():
    cfg = _cfg(motionType=0, subdividePredict=4)
    dt = float(cfg.dt) / 4
    nz = np.zeros(1, CV_NOISE)
    p = _pose(px=1.0, py=2.0, ptheta=0.5, vx=2.0, vy=-1.0)
    o = R.predict_cv(cfg, p, nz)[0]
    c, s = math.cos(0.5), math.sin(0.5)
    np.testing.assert_allclose([o["px"], o["py"], o["ptheta"], o["vx"], o["vy"], o["vtheta"]],
                               [1.0 + dt * (2.0 * c + s), 2.0 + dt * (2.0 * s - c), 0.5, 2.0, -1.0, 0.0], rtol=1e-12)
    o = np.array([(0, 0, 3.0, 0, 0, 0.5)], R.POSE64)
    for k in range(40):  # a constant yaw rate: a heading ramp, through +pi and wrapped once
        o = R.predict_cv(cfg, o, nz)
    assert 3.0 + 40 * dt * 0.5 > math.pi
    np.testing.assert_allclose(o["ptheta"][0], 3.0 + 40 * dt * 0.5 - 2 * math.pi, rtol=1e-12)
    assert o["px"][0] == 0 and o["vtheta"][0] == 0.5
    nz["ax"], nz["ay"], nz["atheta"] = 0.5, -0.25, 0.125
    o = R.predict_cv(cfg, _pose(), nz)[0]
    np.testing.assert_allclose([o["px"], o["py"], o["ptheta"], o["vx"], o["vy"], o["vtheta"]],
                               [0.25 * dt * dt, -0.125 * dt * dt, 0.0625 * dt * dt, 0.5 * dt, -0.25 * dt, 0.125 * dt],
                               rtol=1e-12)


def _g2(*rows):
    g = np.zeros(len(rows), GAUSSIAN2D)
    for i, (w, m, P) in enumerate(rows):
        g[i]["weight"], g[i]["mean"], g[i]["cov"] = w, m, np.asarray(P, np.float64).T.ravel()
    return g


def test_ref_eap_identical_far_and_symmetric_pairs():
    cfg = _cfg(minSeparation=10.0)
    P = np.array([[0.25, 0.0625], [0.0625, 0.5]])
    offs = np.array([0, 1, 2])
    lw = np.log([0.5, 0.5])
    out, near = R.expected_map(cfg, lw, _g2((0.5, (3, 4), P), (0.5, (3, 4), P)), offs)
    assert len(out) == 1 and near == 0
    np.testing.assert_allclose(out[0]["weight"], 0.5, rtol=1e-12)  # twice 0.25
    np.testing.assert_allclose(out[0]["mean"], (3, 4), rtol=1e-12)
    np.testing.assert_allclose(R._mat(out[0]["cov"]), P, rtol=1e-12)
    # two far components: both come out, the heavier (after the particle weights) first
    out, near = R.expected_map(cfg, np.log([0.25, 0.75]), _g2((0.5, (3, 4), P), (0.5, (30, 4), P)), offs)
    assert near == 0
    np.testing.assert_allclose(out["weight"], [0.375, 0.125], rtol=1e-12)
    np.testing.assert_allclose(out["mean"], [(30, 4), (3, 4)], rtol=1e-12)
    # a symmetric pair m -+ e of equal weight: mean m, covariance P + e e'
    m, e = np.array([3.0, 4.0]), np.array([0.25, -0.125])
    out, near = R.expected_map(cfg, lw, _g2((0.5, m - e, P), (0.5, m + e, P)), offs)
    assert len(out) == 1 and near == 0
    np.testing.assert_allclose(out[0]["mean"], m, rtol=1e-12)
    np.testing.assert_allclose(R._mat(out[0]["cov"]), P + np.outer(e, e), rtol=1e-12)
    d, bound = R.distance(m - e, P.T.ravel(), (m + e)[None], P.T.ravel()[None])
    np.testing.assert_allclose(d[0], 4 * e @ np.linalg.inv(P) @ e, rtol=1e-12)
    assert 0 < bound[0] < 1e-5 * d[0]


def test_ref_eap_near_decisions_are_counted():
    cfg = _cfg(minSeparation=10.0)
    P = np.eye(2) * 0.1
    offs = np.array([0, 2])
    g = _g2((0.5, (0, 0), P), (0.25, (np.sqrt(10.0 * 0.1) * (1 + 2e-5), 0), P))
    assert R.expected_map(cfg, [0.0], g, offs)[1] == 1  # a distance inside the band
    g = _g2((0.5, (0, 0), P), (0.5 * (1 - 5e-7), (0.5, 0), P))
    assert R.expected_map(cfg, [0.0], g, offs)[1] == 1  # a weight gap that can matter
    g = _g2((0.5, (0, 0), P), (0.5 * (1 - 5e-7), (50, 0), P))
    assert R.expected_map(cfg, [0.0], g, offs)[1] == 0  # the same gap between strangers
    g = _g2((0.5, (0, 0), P), (0.5, (0.5, 0), P))
    assert R.expected_map(cfg, [0.0], g, offs)[1] == 0  # an exact tie: broken by index


def test_ref_bound_scales_with_the_conditioning():
    m = np.array([0.3, 0.2])
    b1 = R.distance(np.zeros(2), [0.1, 0, 0, 0.1], m[None], np.array([[0.1, 0, 0, 0.1]]))
    b2 = R.distance(np.zeros(2), [0.1, 0, 0, 0.001], m[None], np.array([[0.1, 0, 0, 0.001]]))
    assert b2[1][0] / b2[0][0] > 20 * b1[1][0] / b1[0][0]


def test_ref_box_muller_moments():
    cfg = _cfg(motionType=0, ax=1.0 / 3, ay=1.0 / 3, ayaw=1.0 / 3)
    n = 100000
    nz = R.noise_cv(cfg, 99, np.arange(n), 3)
    a = R.noise_ackerman(_cfg(stdAlpha=1.0, stdEncoder=1.0), 99, np.arange(n), 3)
    for x in (nz["ax"], nz["ay"], nz["atheta"], a["n_alpha"], a["n_encoder"]):
        x = x.astype(np.float64)
        assert abs(x.mean()) <= 4 / math.sqrt(n)
        assert abs(x.var() - 1) <= 4 * math.sqrt(2 / n)
        assert abs(np.mean(x ** 3)) <= 4 * math.sqrt(15 / n)
        assert abs(np.mean(x ** 4) - 3) <= 4 * math.sqrt(96 / n)
    assert abs(np.corrcoef(nz["ax"], nz["ay"])[0, 1]) <= 4 / math.sqrt(n)
    assert abs(np.corrcoef(nz["ax"], nz["atheta"])[0, 1]) <= 4 / math.sqrt(n)
    # one draw per id: both models read the same normals (3 float32(1 / 3) is 1 to a rounding)
    np.testing.assert_allclose(a["n_alpha"], nz["ax"], rtol=1e-6)
    np.testing.assert_allclose(a["n_encoder"], nz["ay"], rtol=1e-6)


def test_ref_philox_known_answers():
    # Random123 kat_vectors, philox4x32 with 10 rounds (as tests/test_weighting_ref.py)
    kat = [([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
           ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
            [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
    for ctr, key, want in kat:
        got = [int(x[0]) for x in weighting_ref.philox4x32_10(ctr, key)]
        assert got == want, (ctr, [hex(g) for g in got])
    # the draw's words are (id, step low, step high, 'PRED') under (seed low, seed high)
    seed, step, i = 2 ** 40 + 12345, 2 ** 33 + 5, 4099
    x = weighting_ref.philox4x32_10([i, step & 0xFFFFFFFF, step >> 32, 0x50524544], [seed & 0xFFFFFFFF, seed >> 32])
    u1, u2 = (float(x[0][0]) + 1) * 2.0 ** -32, float(x[1][0]) * 2.0 ** -32
    g0 = math.sqrt(-2 * math.log(u1)) * math.cos(2 * math.pi * u2)
    cfg = _cfg()
    got = R.noise_ackerman(cfg, seed, [i], step)
    assert got["n_alpha"][0] == np.float32(float(cfg.stdAlpha) * g0)
    assert not np.array_equal(got, R.noise_ackerman(cfg, seed, [i], step & 0xFFFFFFFF))  # the high word counts


def test_ref_expand_expected_pose_cardinalities():
    p = np.zeros(3, POSE)
    p["px"] = (1, 2, 3)
    ep, w, parent, ids = R.expand(p, np.log([0.2, 0.3, 0.5]), 3, 4096)
    assert parent.tolist() == [0, 0, 0, 1, 1, 1, 2, 2, 2] and ids.tolist() == list(range(4096, 4105))
    np.testing.assert_allclose(np.exp(w), np.repeat([0.2, 0.3, 0.5], 3) / 3, rtol=1e-12)
    assert ep["px"].tolist() == [1, 1, 1, 2, 2, 2, 3, 3, 3]
    e, mi = R.expected_pose(np.log([0.25, 0.5, 0.25]), p)
    assert mi == 1 and abs(e["px"] - 2.0) <= 1e-12
    assert R.expected_pose([-1.0, -0.5, -0.5, -np.inf], np.zeros(4, POSE))[1] == 1  # the first maximum
    g = _g2((0.5, (0, 0), np.eye(2)), (0.25, (0, 0), np.eye(2)), (1e-6, (0, 0), np.eye(2)))
    cn = R.cardinalities(g, [0, 0, 2, 3])
    assert cn[0] == 0 and cn[1] == 0.75 and cn[2] == float(np.float32(1e-6))


# ------------------------------------------------------ the cases' conditions

@pytest.mark.parametrize("name", C.EAP_CASES)
def test_eap_case_has_no_near_decision(name):
    """No distance and no weight gap that a float32 evaluation could decide
    otherwise: a flipped greedy decision changes everything after it, so no
    component may be left out.  From the reference alone."""
    c = C.eap_inputs(name)
    out, near, groups = C.eap_reference(name)
    print(f"{name}: {len(c.maps)} components in {len(c.lw)} particles -> {len(out)}, near {near}")
    assert near == 0
    assert len(c.maps) <= 4096 and np.diff(c.offs).max(initial=0) <= c.cap
    P = R._mat(c.maps["cov"].astype(np.float64))
    if len(P):
        ev = np.linalg.eigvalsh(P)
        assert (ev[:, 1] / ev[:, 0]).max() <= 100.0


def test_eap_cases_reach_what_they_are_for():
    _, _, g = C.eap_reference("sum_edges")
    assert sorted(g) == sorted(C.SUM_EDGES)  # the 64-member staging boundaries of the sums
    # big_cell: two cells of ~700 components each, two cells apart, nine seeds in each, whose
    # members are spread over the whole priority order (absorbed mass between live candidates)
    c = C.eap_inputs("big_cell")
    side = c.extra["side"]
    assert abs(side - C.lattice_side(c.maps["cov"])) <= 1e-12
    cell = np.floor(c.maps["mean"].astype(np.float64) / side).astype(int)
    keys, cnt = np.unique(cell, axis=0, return_counts=True)
    big = keys[cnt > 600]
    assert len(big) == 2 and abs(big[0, 0] - big[1, 0]) == 2 and big[0, 1] == big[1, 1] and (cnt > 3 * 256 - 100).sum() == 2
    out, _, g = C.eap_reference("big_cell")
    assert len(out) == 19 and sorted(g) == [0] + [77] * 18
    # borders: every pair merges across its border — the two lie in different cells, in each of
    # the 8 directions, among them cells of negative index and the cells around the origin
    for name in ("borders", "wide_lambda"):
        c = C.eap_inputs(name)
        out, _, g = C.eap_reference(name)
        extra = 1 if name == "wide_lambda" else 0
        assert sorted(g) == [0] * (2 + extra) + [1] * 24 and len(out) == 26 + extra
    c = C.eap_inputs("borders")
    assert abs(c.extra["side"] - C.lattice_side(c.maps["cov"])) <= 1e-12
    cell = np.floor(c.maps["mean"].astype(np.float64) / c.extra["side"]).astype(int)
    dirs = set()
    for a in range(len(cell)):
        d = np.sum((c.maps["mean"][a].astype(np.float64) - c.maps["mean"].astype(np.float64)) ** 2, 1)
        b = np.argsort(d)[1]
        if d[b] < 1.0:
            dirs.add(tuple(cell[b] - cell[a]))
            assert tuple(cell[b]) != tuple(cell[a])
    assert dirs == {(i, j) for i in (-1, 0, 1) for j in (-1, 0, 1)} - {(0, 0)}
    assert (cell < 0).any() and (np.abs(cell).max(1) == 0).any() and ((cell == -1).any(1) & (cell.max(1) <= 0)).any()
    w = C.eap_inputs("wide_lambda")
    assert C.lattice_side(w.maps["cov"]) > 19 * c.extra["side"]
    out, _, g = C.eap_reference("chains")
    assert sorted(g) == [1] * 160  # every seed takes its neighbour, never the next but one
    d = C.eap_inputs("duplicates")
    assert d.extra["near"] == 0 and len(set(d.extra["parents"])) < len(d.lw)
    z = C.eap_inputs("zero_weights")
    assert np.isneginf(z.lw[::5]).all() and np.isfinite(np.delete(z.lw, np.s_[::5])).all()
    out, _, _ = C.eap_reference("zero_weights")
    assert np.isnan(out["mean"]).any() and (out["weight"][np.isnan(out["mean"][:, 0])] == 0).all()
    f = C.eap_inputs("fallback")
    out, _, g = C.eap_reference("fallback")
    assert max(g) > 1024 and np.isnan(f.maps["mean"]).sum() == 1
    assert np.isnan(out["mean"][:, 0]).sum() == 1 and np.isfinite(out["mean"][:, 1]).all()
    assert len(C.eap_reference("single")[0]) == 1 and len(C.eap_reference("empty")[0]) == 0


def test_predict_cases_reach_what_they_are_for():
    for model in C.MODELS:
        up = down = 0
        for kind in ("n257_s1", "n257_s4", "n1000_s1", "n1000_s4"):
            c, r = C.predict_inputs(f"{model}_{kind}"), C.predict_reference(f"{model}_{kind}")
            for ref in (r.host,) + tuple(r.rng.values()):
                th0 = c.poses["ptheta"].astype(np.float64)
                up += int(np.sum((th0 > 3) & (ref["ptheta"] < -3)))
                down += int(np.sum((th0 < -3) & (ref["ptheta"] > 3)))
                assert np.all(np.abs(ref["ptheta"]) <= np.pi)
            assert (c.poses["ptheta"] == C.PI32).any() and (c.poses["ptheta"] == -C.PI32).any()
            assert (c.poses["ptheta"] == 0).any()
            # the index offset moves the draw
            assert not np.array_equal(r.noise[0], r.noise[4096])
        assert up >= 10 and down >= 10, (model, up, down)
        c, r = C.predict_inputs(f"{model}_still"), C.predict_reference(f"{model}_still")
        for k in ("px", "py"):
            assert np.array_equal(r.host[k], c.poses[k].astype(np.float64))
        assert np.abs(R.wrap(r.host["ptheta"] - c.poses["ptheta"])).max() <= 1e-15
        c, r = C.predict_inputs(f"{model}_npp3"), C.predict_reference(f"{model}_npp3")
        assert len(r.host) == 120 and r.parent.tolist() == np.repeat(np.arange(40), 3).tolist()
        np.testing.assert_allclose(r.lw, np.repeat(c.lw.astype(np.float64), 3) - math.log(3), rtol=1e-15)
    assert any(C.predict_inputs(n).step >= 2 ** 32 for n in C.PREDICT_CASES)
    assert any(C.predict_inputs(n).seed >= 2 ** 32 for n in C.PREDICT_CASES)


# ------------------------------------------------- the oracle against the reference

def _assert_table(label, worst, table, classes):
    for k in classes:
        assert worst[k] <= table[k], (label, k, worst[k], table[k])
        # the table is the measurement, not a bound above it
        assert table[k] <= 2 * worst[k] + 1e-12, (label, k, "table entry is stale", worst[k])


def oracle_predict(name):
    """Worst deviations of the oracle's noise and predictions from the reference's, host noise and every offset."""
    import pyoracle
    c, r = C.predict_inputs(name), C.predict_reference(name)
    m = len(c.poses) * c.npp
    worst = dict.fromkeys(C.PREDICT_CLASSES, 0.0)

    def run(noise):
        if c.model == "ack":
            return pyoracle.predict_ackerman(c.cfg.copy(), c.poses, c.control[0], c.control[1], noise)
        return pyoracle.predict_cv(c.cfg.copy(), c.poses, noise)

    outs = [(r.host, run(c.host))]
    for off in c.offsets:
        draw = (pyoracle.noise_ackerman if c.model == "ack" else pyoracle.noise_cv)(c.cfg.copy(), m + off, c.seed, c.step)
        worst["noise"] = max(worst["noise"], C.noise_deviation(r.noise[off], draw[off:]))
        outs.append((r.rng[off], run(draw[off:])))
    for ref, got in outs:
        assert np.all(np.abs(got["ptheta"]) <= C.PI32)
        for k, v in C.pose_deviations(ref, got).items():
            worst[k] = max(worst[k], v)
    return worst


@pytest.mark.parametrize("name", C.PREDICT_CASES)
def test_oracle_predict_against_reference(built, name):
    worst = oracle_predict(name)
    print(f"{name}: " + ", ".join(f"{k} {worst[k]:.3g}" for k in C.PREDICT_CLASSES))
    _assert_table(name, worst, C.D_ORACLE[name], C.PREDICT_CLASSES)


def oracle_ep(name):
    import pyoracle
    poses, lw, ties = C.ep_inputs(name)
    ref, mi = C.ep_reference(name)
    got, omi = pyoracle.expected_pose(lw, poses)
    assert mi == omi == ties[0]
    return C.pose_deviations(ref, got, scale=1e-3)


@pytest.mark.parametrize("name", C.EP_CASES)
def test_oracle_expected_pose_against_reference(built, name):
    worst = oracle_ep(name)
    print(f"{name}: " + ", ".join(f"{k} {worst[k]:.3g}" for k in C.EP_CLASSES))
    _assert_table(name, worst, C.D_ORACLE[name], C.EP_CLASSES)


def oracle_eap(name):
    import pyoracle
    c = C.eap_inputs(name)
    ref, near, _ = C.eap_reference(name)
    assert near == 0, "the case has a near decision"
    worst = C.field_deviations(ref, pyoracle.expected_map(c.cfg.copy(), c.lw, c.maps, c.offs))
    assert worst is not None, "the oracle's EAP map has another size, or a NaN where the reference has a number"
    return worst


@pytest.mark.parametrize("name", C.EAP_CASES)
def test_oracle_eap_against_reference(built, name):
    """The same count in the same emission order, every field within the table."""
    worst = oracle_eap(name)
    print(f"{name}: " + ", ".join(f"{k} {worst[k]:.3g}" for k in C.FIELD_CLASSES))
    _assert_table(name, worst, C.D_ORACLE[name], C.FIELD_CLASSES)


def test_tables_cover_the_cases():
    assert set(C.D_ORACLE) == set(C.PREDICT_CASES) | set(C.EP_CASES) | set(C.EAP_CASES)
