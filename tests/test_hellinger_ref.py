"""CPU checks of the Hellinger merge reference (tests/hellinger_ref.py) and of
the bounds the device merge rests on (distance_metric = 1)."""
import numpy as np

import hellinger_cases as C
import hellinger_ref as H
import pyoracle

F = np.float32


def _rand_cov(rng, n, max_cond, dtype=np.float32, scale=(-2, 1), asym=False):
    th = rng.uniform(0, np.pi, n)
    l1 = 10.0 ** rng.uniform(scale[0], scale[1], n)
    l2 = l1 / 10.0 ** rng.uniform(0, np.log10(max_cond), n)
    c, s = np.cos(th), np.sin(th)
    b = c * s * (l1 - l2)
    cov = np.stack([c * c * l1 + s * s * l2, b, b, s * s * l1 + c * c * l2], 1).astype(dtype)
    if asym:  # off-diagonals a few ulps apart, as rounded covariance updates leave them
        for _ in range(3):
            cov[:, 2] = np.nextafter(cov[:, 2], dtype(np.inf))
    return cov, l1


def _rand_pairs(seed, n, max_cond, **kw):
    rng = np.random.default_rng(seed)
    A, la = _rand_cov(rng, n, max_cond, **kw)
    B, lb = _rand_cov(rng, n, max_cond, **kw)
    am = rng.uniform(-50, 50, (n, 2)).astype(F)
    r = np.sqrt(np.maximum(la, lb)) * 10.0 ** rng.uniform(-2, 0.8, n)
    ph = rng.uniform(0, 2 * np.pi, n)
    bm = (am + np.stack([r * np.cos(ph), r * np.sin(ph)], 1)).astype(F)
    return am, A, bm, B


def test_det_expf_restatement_matches_the_shared_helper():
    x = np.concatenate([np.linspace(-30, 2, 400), [-120.0, -110.5, 0.0, -0.0, 88.9, 95.0]]).astype(F)
    got = H.det_expf(x)
    want = np.array([pyoracle.det_expf(v) for v in x], F)
    assert got.tobytes() == want.tobytes()


def test_distance_against_float64_closed_form():
    P = np.array([0.3, 0.05, 0.05, 0.2], F)
    m = np.array([4.0, -2.0], F)
    # identical Gaussians: ~0
    assert abs(float(H.hellinger(m, P, m, P))) < 1e-6
    # equal covariances: 1 - exp(-d' P^-1 d / 8)
    for dm in ([0.3, 0.1], [1.0, -0.7], [0.0, 2.5]):
        m2 = (m + np.array(dm, F)).astype(F)
        d = (m2 - m).astype(np.float64)
        want = 1 - np.exp(-d @ np.linalg.solve(P.astype(np.float64).reshape(2, 2), d) / 8)
        assert abs(float(H.hellinger(m, P, m2, P)) - want) < 2e-6
    # a far pair: 1
    assert float(H.hellinger(m, P, (m + F(100)).astype(F), P)) == 1.0
    # random well-conditioned pairs against the float64 closed form
    am, A, bm, B = _rand_pairs(3, 20000, 30.0)
    assert np.max(np.abs(H.hellinger(am, A, bm, B) - H.hellinger64(am, A, bm, B))) < 5e-5


def test_cull_bound():
    """d_H < T implies d' ((A+B)/2)^-1 d < 1.05 T_M, T_M = -8 ln(1 - T), over
    2 x 10^5 pairs of condition number <= 1e4 and T swept over (0, 1).  The
    bound is one of the exact distance (c <= 1), so d_H is the float64 closed
    form here.  The reference's float32 distance does NOT keep it at condition
    numbers near 1e4 (the determinant of the product cancels: |d32 - d64| up to
    0.4, one violation in 4 x 10^5 pairs at T = 1e-3), which is why the device
    bins only condition numbers below 100 under this metric and adds
    PHD_HELL_SLACK to T: the second half checks that class in float32."""
    Ts = np.concatenate([10.0 ** np.linspace(-3, -1, 5), np.linspace(0.15, 0.95, 9), [0.99, 0.999]])
    am, A, bm, B = _rand_pairs(11, 200000, 1e4)
    d64 = H.hellinger64(am, A, bm, B)
    m64 = H.mahal64(am, A, bm, B)
    for T in Ts:
        below = d64 < T
        assert below.any() or T < 1e-2
        assert np.all(m64[below] < 1.05 * H.cull_threshold(T)), T
    # the device's class: cond < 100, float32 distance within the slack of the exact one
    SLACK = 4e-3  # PHD_HELL_SLACK (phd_devutil.h)
    am, A, bm, B = _rand_pairs(12, 200000, 100.0)
    d32 = H.hellinger(am, A, bm, B)
    d64 = H.hellinger64(am, A, bm, B)
    m64 = H.mahal64(am, A, bm, B)
    assert np.nanmax(np.abs(d32 - d64)) < SLACK / 2
    for T in Ts:
        if T + SLACK >= 1:
            continue
        with np.errstate(invalid="ignore"):
            below = d32 < T
        assert np.all(m64[below] < 1.05 * H.cull_threshold(T + SLACK)), T
    # the class is decided by the eigenvalue ratio alone: eigenvalues from 1e-6
    # to 1e4 (each pair within three decades) and slightly asymmetric covariances
    am, A, bm, B = _rand_pairs(13, 200000, 100.0, scale=(-6, 4), asym=True)
    d32 = H.hellinger(am, A, bm, B)
    assert np.nanmax(np.abs(d32 - H.hellinger64(am, A, bm, B))) < SLACK / 2
    m64 = H.mahal64(am, A, bm, B)
    for T in Ts:
        if T + SLACK >= 1:
            continue
        with np.errstate(invalid="ignore"):
            below = d32 < T
        assert np.all(m64[below] < 1.05 * H.cull_threshold(T + SLACK)), T


def test_near_decision_cap_of_every_gpu_case():
    """The reference alone keeps the cap: at most 1 particle in 8 of each case
    holds a near decision (and is skipped by the device comparison)."""
    for name, T in C.all_case_keys():
        near = C.expected(name, T)[3]
        assert int((near > 0).sum()) * C.MAX_SKIP <= len(near), (name, T, near.tolist())
    cfg, poses, lw, maps, offs, z, g = C.directed_scenario()
    assert len(poses) == 1  # (compared whole: its one decision is near by construction)


def test_directed_pair_search_and_saved_pair():
    """d(a, b) != d(b, a) exists (asymmetric covariances), and with T the larger
    of the two the seed-first and the candidate-first test decide differently."""
    r = C.find_directed_pair()
    assert r is not None
    g = np.load(C.GOLDEN_PAIR)
    for k, v in zip(("mean_a", "cov_a", "mean_b", "cov_b", "d_ab", "d_ba"), r):
        assert np.asarray(v, F).tobytes() == g[k].tobytes(), k  # the saved pair is the one the search finds
    dab = H.hellinger(g["mean_a"], g["cov_a"], g["mean_b"], g["cov_b"])
    dba = H.hellinger(g["mean_b"], g["cov_b"], g["mean_a"], g["cov_a"])
    assert dab == g["d_ab"] and dba == g["d_ba"] and dab != dba
    T = max(dab, dba)
    assert (dab < T) != (dba < T)
    # symmetric covariances: bitwise symmetric (the entries of a b and b a are the same sums)
    am, A, bm, B = _rand_pairs(5, 50000, 100.0)
    assert H.hellinger(am, A, bm, B).tobytes() == H.hellinger(bm, B, am, A).tobytes()


def test_config_file_carries_the_metric(tmp_path):
    import phdslam
    p = tmp_path / "hellinger.cfg"
    p.write_text("distance_metric = 1\nmin_separation = 0.7\n")
    cfg, _ = phdslam.load_config(p)
    assert cfg.distanceMetric == 1 and abs(cfg.minSeparation - 0.7) < 1e-6


def test_greedy_merges_and_counts_near():
    from phdslam.types import GAUSSIAN2D
    cand = np.zeros(3, GAUSSIAN2D)
    cand["cov"] = (0.1, 0.0, 0.0, 0.1)
    cand["mean"] = [(0.0, 0.0), (0.1, 0.0), (5.0, 5.0)]
    cand["weight"] = (0.5, 0.9, 0.2)
    out, near = H.greedy(cand, 0.5)
    assert len(out) == 2 and near == 0
    np.testing.assert_allclose(out[0]["weight"], 1.4, rtol=1e-6)  # the heaviest seed first
    np.testing.assert_allclose(out[0]["mean"], [0.9 * 0.1 / 1.4, 0.0], rtol=1e-5, atol=1e-7)
    assert out[1]["weight"] == F(0.2)
    d01 = float(H.hellinger(cand["mean"][1], cand["cov"][1], cand["mean"][0], cand["cov"][0]))
    assert H.greedy(cand, d01 * (1 + 5e-5))[1] == 1  # a test inside the band is near
