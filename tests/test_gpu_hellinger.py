"""Hellinger merge distance (distance_metric = 1) on the device update against
the numpy reference (tests/hellinger_ref.py): expected output per particle =
greedy(the oracle's unmerged candidates under metric 1) + the class-0
components; the expected log-weight change is the oracle's (the merge does not
touch it).  A particle with a near decision is skipped (at most 1 in 8 per
case: tests/test_hellinger_ref.py asserts the cap over the same inputs)."""
import numpy as np
import pytest

import hellinger_cases as C
import hellinger_ref as H
import parity
import pyoracle

pytestmark = pytest.mark.gpu


def _filter(cfg, n, **cap):
    import phdslam
    f = phdslam.PHDFilter(n, cfg, **cap)
    f.set_seed(1234)
    return f


def _run(name, T, threads=0, form=0, merge_mode=0):
    cfg, poses, lw, maps, offs, z = C.inputs(name)
    f = _filter(C.config(name, T), len(poses))
    if threads:
        f.set_update_threads(threads)
    if form:
        f.set_update_form(form)
    f.set_merge_mode(merge_mode)
    f.load(poses, lw, maps, offs)
    f.update(z)
    f.check_errors()
    fb = f.merge_fallbacks()
    used = (f.update_threads()[0], f.update_form())
    card = f.cardinality_distribution() if cfg.filterType == 1 else None
    _, glw, gm, go = f.export()
    f.close()
    return glw, gm, go, fb, used, card


def _compare(name, T, glw, gm, go, skip_near=True):
    cfg, poses, lw, maps, offs, z = C.inputs(name)
    exp = C.expected(name, T)
    em, eo, delta, near = exp[:4]
    n = len(poses)
    assert int((near > 0).sum()) * C.MAX_SKIP <= n
    assert parity.close(glw, lw + delta, parity.RTOL, floor=1e-5).all(), "log-weights differ from the oracle's"
    compared = 0
    for p in range(n):
        if skip_near and near[p]:
            continue
        A, B = em[eo[p]:eo[p + 1]], gm[go[p]:go[p + 1]]
        assert len(A) == len(B), (name, T, p, len(A), len(B))
        ok, worst = parity.compare_maps(A, B)
        assert ok, (name, T, p, worst)
        compared += 1
    assert compared * C.MAX_SKIP >= n * (C.MAX_SKIP - 1)
    return compared


def test_metric_1_update_is_accepted(gpu):
    cfg, poses, lw, maps, offs, z = C.inputs("phd_small")
    f = _filter(C.config("phd_small", 0.7), len(poses))
    f.load(poses, lw, maps, offs)
    f.update(z)  # PHD_OK (raises otherwise)
    f.check_errors()
    f.close()


@pytest.mark.parametrize("T", [0.3, 0.7, 0.95])
@pytest.mark.parametrize("name", ["phd_small", "phd_large"])
def test_parity_phd(gpu, name, T):
    glw, gm, go, fb, used, _ = _run(name, T)
    _compare(name, T, glw, gm, go)


@pytest.mark.parametrize("T", [0.3, 0.7, 0.95])
@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("threads", [256, 512, 1024])
def test_parity_phd_threads_and_forms(gpu, threads, form, T):
    glw, gm, go, fb, used, _ = _run("phd_small", T, threads=threads, form=form)
    assert used == (threads, form == 2)
    _compare("phd_small", T, glw, gm, go)


def test_parity_merge_stress(gpu):
    glw, gm, go, fb, used, _ = _run("merge_stress", 0.7)
    _compare("merge_stress", 0.7, glw, gm, go)


def test_parity_cphd(gpu):
    glw, gm, go, fb, used, card = _run("cphd", 0.7)
    _compare("cphd", 0.7, glw, gm, go)
    cn = C.expected("cphd", 0.7)[4]
    gc = np.asarray(card, np.float64)
    sig = cn > -60.0  # probabilities above ~1e-26 (as the metric-0 cardinality test)
    assert parity.close(gc[sig], cn[sig], 1e-5, floor=1e-4).all()
    assert np.all(gc[~sig] < -50.0)


@pytest.mark.parametrize("name,T", [("phd_small", 0.7), ("merge_stress", 0.7), ("cphd", 0.7)])
def test_parallel_equals_serial(gpu, name, T):
    par = _run(name, T, merge_mode=0)
    ser = _run(name, T, merge_mode=1)
    assert par[3] == 0, "the parallel merge fell back to the serial greedy"
    assert np.array_equal(par[2], ser[2])  # offsets
    assert np.array_equal(par[0], ser[0])  # log-weights
    n = len(par[2]) - 1
    for p in range(n):
        A, B = par[1][par[2][p]:par[2][p + 1]], ser[1][ser[2][p]:ser[2][p + 1]]
        ok, worst = parity.compare_maps(A, B, rtol=1e-6)  # (as multisets: the serial greedy emits in selection order)
        assert ok, (p, worst)


@pytest.mark.parametrize("mirrored", [False, True])
def test_directed_edge(gpu, mirrored):
    """The saved pair with d(a, b) != d(b, a) as class-2 components, T the larger
    of the two distances: the device must take the seed-first decision, on the
    parallel and on the serial merge — with the heavier component first (the
    issue's arrangement) and second (mirrored: priority and index order then
    disagree, so evaluating d(lower index, higher index) decides wrongly)."""
    cfg, poses, lw, maps, offs, z, g = C.directed_scenario(mirrored)
    c0 = cfg.copy()
    c0.minSeparation = 1e-12
    c0.distanceMetric = 0
    um, uo, delta, _ = pyoracle.update(c0, poses, maps, offs, z)
    cand = um.copy()
    hits = 0
    for k in (0, 1):  # the oracle's one-member outputs symmetrise the covariance (D15): the pair's own back
        i = np.flatnonzero(np.all(cand["mean"] == maps["mean"][k], 1))
        assert len(i) == 1
        cand["cov"][i[0]] = maps["cov"][k]
        hits += 1
    assert hits == 2 and cand["weight"][0] == np.float32(0.6) and cand["weight"][1] == np.float32(0.5)
    want, _ = H.greedy(cand, cfg.minSeparation)
    merged = bool(g["d_ab"] < np.float32(cfg.minSeparation))  # the seed-first decision
    assert len(want) == len(cand) - (1 if merged else 0)
    for mode in (0, 1):
        f = _filter(cfg, 1)
        f.set_merge_mode(mode)
        f.load(poses, lw, maps, offs)
        f.update(z)
        f.check_errors()
        _, _, gm, go = f.export()
        f.close()
        assert go[1] == len(want), (mode, int(go[1]), len(want))
        ok, worst = parity.compare_maps(want, gm)
        assert ok, (mode, worst)


def test_separation_above_one_collapses_each_map(gpu):
    """T = 1.5: every distance that is not NaN is below T, so each particle's
    candidates collapse into one component (the serial greedy: fallbacks allowed)."""
    glw, gm, go, fb, used, _ = _run("collapse", 1.5)
    assert fb == len(go) - 1  # T >= 1: every particle takes the serial greedy
    _compare("collapse", 1.5, glw, gm, go)


def test_zero_covariance_takes_serial_fallback(gpu):
    glw, gm, go, fb, used, _ = _run("zero_cov", 0.7)
    assert fb >= 1
    _compare("zero_cov", 0.7, glw, gm, go)


@pytest.mark.parametrize("thresh", [1.0, 0.0])
def test_step_over_three_scans_equals_separate_calls(gpu, thresh):
    """step() over 3 scans under metric 1 against the separate predict, update,
    normalize and resample calls, bit for bit: with a resample on every scan
    (threshold 1: the next update then reads its prior through the resample's
    slab references) and without one (threshold 0)."""
    import phdslam
    c, poses, lw, maps, offs, z = phdslam.config_scenario(2, n=64, G=64, M=16)
    c.distanceMetric = 1
    c.minSeparation = 0.7
    c.resampleThresh = thresh
    u = (2.0, 0.05)
    f = _filter(c, 64)
    f.set_seed(77)
    f.load(poses, lw, maps, offs)
    g = _filter(c, 64)
    g.set_seed(77)
    g.load(poses, lw, maps, offs)
    resampled = []
    for k in range(3):
        f.set_measurements(z)
        resampled.append(f.step(control=u, step=k)[1])
        g.predict_ackerman(u[0], u[1], noise=None, step=k)
        g.set_measurements(z)
        g.update()
        g.normalize()
        if thresh > 0:
            g.resample(step=k, return_indices=False)
    f.check_errors()
    g.check_errors()
    a, b = f.export(), g.export()
    f.close()
    g.close()
    assert resampled == [thresh > 0] * 3, resampled
    for x, y, name in zip(a, b, ("poses", "log-weights", "maps", "offsets")):
        assert x.tobytes() == y.tobytes(), f"{name} differ"


@pytest.mark.parametrize("replay", [False, True])
def test_cphd_step_with_births_and_replay_equals_separate_calls(gpu, replay):
    """The CPHD step under metric 1 with the step's births and a resample on
    every scan, fresh and in replay mode, against the separate calls (births by
    add_births), bit for bit — the pattern of the metric-0
    test_step_cphd_overlapped_resample_matches_separate_calls at a small shape."""
    import phdslam
    c, poses, lw, maps, offs, z = phdslam.config_scenario(3, n=64, G=64, M=16)
    c.distanceMetric = 1
    c.minSeparation = 0.7
    c.maxCardinality = 127
    c.resampleThresh = 1.0
    zs = [z, z.copy()]
    zs[1]["range"] = (zs[1]["range"] + 0.05).astype(np.float32)  # a second scan
    f = _filter(c, 64)
    f.load(poses, lw, maps, offs)
    assert f.step_births()
    if replay:
        f.set_measurements(z)
        f.set_replay(True)
    g = _filter(c, 64)
    g.set_step_births(0)
    g.load(poses, lw, maps, offs)
    for k in range(2):
        if not replay:
            f.set_measurements(zs[k])
        f.step(do_predict=True, step=k)
        if replay and k == 0:
            continue
        g.predict_cv(step=k)
        if replay:
            g.add_births(z)
        elif k > 0:
            g.add_births(zs[k - 1])
        g.set_measurements(z if replay else zs[k])
        g.update()
        g.normalize()
        g.resample(step=k, return_indices=False)
    f.check_errors()
    g.check_errors()
    a, b = f.export(), g.export()
    ca, cb = f.cardinality_distribution(), g.cardinality_distribution()
    f.close()
    g.close()
    for x, y, name in zip(a, b, ("poses", "log-weights", "maps", "offsets")):
        assert x.tobytes() == y.tobytes(), f"{name} differ"
    assert ca.tobytes() == cb.tobytes(), "cardinality distributions differ"


def test_rejections(gpu):
    from phdslam import _lib
    from phdslam.scenario import mixed_config
    cfg, poses, lw, maps, offs, z = C.inputs("phd_small")
    c = C.config("phd_small", 0.7)
    c.distanceMetric = 2
    f = _filter(c, len(poses))
    f.load(poses, lw, maps, offs)
    f.set_measurements(z)
    rc = _lib.lib().phd_update(f.handle)
    assert rc == _lib.PHD_E_UNSUPPORTED
    f.close()
    m = mixed_config()
    m.distanceMetric = 1
    f = _filter(m, 4)
    f.enable_dynamic(64)
    f.set_measurements(z[:4])
    rc = _lib.lib().phd_update(f.handle)
    assert rc == _lib.PHD_E_UNSUPPORTED
    assert b"Hellinger" in _lib.lib().phd_last_error()
    f.close()
