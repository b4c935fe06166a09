"""The float64 reference of the weighting stage (tests/weighting_ref.py) on the
CPU:

1. closed forms for the reference itself, and its Philox against the Random123
   known answers and the oracle's uniforms;
2. the input condition of every shared case (tests/weighting_cases.py), from
   the reference alone: no near decision, at most 1 % near strata;
3. the oracle (normalize, neff, resample_fixed) held to the reference on every
   case: the decision, every stratum that is not near equal to the reference's
   parent, every near one among its admissible parents, and the normalised
   log-weights / nEff within the committed table D_ORACLE.

`python tests/test_weighting_ref.py` prints the table and the (seed, step)
pairs of the `tie` cases from the current oracle.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import weighting_cases as C  # noqa: E402
import weighting_ref as R  # noqa: E402

CASE_IDS = [C.key(c) for c in C.CASES]


# ---------------------------------------------------------------- closed forms

def test_philox_known_answers():
    # Random123 kat_vectors, philox4x32 with 10 rounds (as tests/test_oracle_closed_form.py)
    kat = [([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
           ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
           ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0],
            [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1])]
    for ctr, key, want in kat:
        got = [int(x[0]) for x in R.philox4x32_10(ctr, key)]
        assert got == want, (ctr, [hex(g) for g in got])


@pytest.mark.parametrize("n,seed,step", [(1, 0, 0), (1000, 4242, 11), (5000, 2 ** 63 + 12345, 2 ** 40 + 3)])
def test_philox_uniforms_equal_the_oracles(built, n, seed, step):
    import pyoracle
    np.testing.assert_array_equal(R.resample_uniforms(n, seed, step), pyoracle.resample_uniforms(n, seed, step))


def test_hand_computed_parents():
    """Weights 0.1 / 0.2 / 0.3 / 0.4: c = 0.1, 0.3, 0.6, 1.0; strata (j + u) / 4."""
    w = np.log(np.array([0.1, 0.2, 0.3, 0.4])).astype(np.float32)
    # u = 0.5: r = 0.125, 0.375, 0.625, 0.875 -> 1, 2, 3, 3
    np.testing.assert_array_equal(R.parents(w, [0.5] * 4).parent, [1, 2, 3, 3])
    # u = 0.1: r = 0.025, 0.275, 0.525, 0.775 -> 0, 1, 2, 3
    np.testing.assert_array_equal(R.parents(w, [0.1] * 4).parent, [0, 1, 2, 3])
    # u = 0.9: r = 0.225, 0.475, 0.725, 0.975 -> 1, 2, 3, 3
    p = R.parents(w, [0.9] * 4)
    np.testing.assert_array_equal(p.parent, [1, 2, 3, 3])
    assert not p.near.any() and p.beyond.size == 0 and p.amax == 3
    # two strata over the four entries: r = 0.25, 0.75 -> 1, 3
    np.testing.assert_array_equal(R.parents(w, [0.5, 0.5]).parent, [1, 3])
    # a stratum on an entry's edge is near: r_1 = (1 + 0.2) / 4 = 0.3 = c[1]
    p = R.parents(w, [0.5, 0.2, 0.5, 0.5])
    assert list(p.near) == [False, True, False, False] and (p.lo[1], p.hi[1]) == (1, 2)


def test_flat_weights_are_the_identity():
    """Equal weights: parent j == j for any u away from the stratum's edges (the
    float32 rounding of -log n moves the CDF by parts in 1e7)."""
    for n in (1, 8, 63):
        w = np.full(n, -np.log(n), np.float32)
        for u in (0.01, 0.25, 0.5, 0.99):
            p = R.parents(w, np.full(n, u))
            np.testing.assert_array_equal(p.parent, np.arange(n))
            assert not p.near.any()
        assert abs(R.neff(R.normalize(w)[0]) - 1.0) < 1e-12


def test_one_dominant_particle_takes_every_stratum():
    n = 1000
    w = R.normalize(C.weights("one", n))[0].astype(np.float32)
    p = R.parents(w, R.resample_uniforms(n, 1, 2))
    assert (p.parent == 750).all() and p.amax == 750
    assert abs(R.neff(w) - 1.0 / n) < 1e-9


def test_minus_inf_is_never_a_parent_and_overrun_takes_the_first_maximum():
    with np.errstate(divide="ignore"):
        w = np.log(np.array([0.0, 0.25, 0.0, 0.0, 0.25, 0.125, 0.0, 0.125])).astype(np.float32)  # total 0.75
    u = R.resample_uniforms(8, 5, 6)
    p = R.parents(w, u)
    assert np.isfinite(w[p.parent]).all()
    # strata 6 and 7 lie past the CDF's end 0.75 ((6 + u) / 8 >= 0.75): the first of the equal maxima
    np.testing.assert_array_equal(p.beyond, [6, 7])
    assert p.amax == 1 and list(p.parent[6:]) == [1, 1]
    wrong, outside, near = R.check_parents(p.parent, p)
    assert wrong.size == 0 and outside.size == 0
    bad = p.parent.copy()
    bad[7] = 4  # the second maximum is not admissible
    assert R.check_parents(bad, p)[0].tolist() == [7]


def test_decision_bound_scales():
    d = R.decision(C.weights("normal", 4096), 1.0)
    assert d.resample and not d.near and 0 < d.bound < 1e-5 * d.neff
    assert R.decision(np.zeros(10, np.float32), 1.0).near  # nEff = 1 against 1.0
    assert not R.decision(np.zeros(10, np.float32), 1.5).near
    assert not R.decision(np.zeros(10, np.float32), 1.5, has_meas=False).resample


# ------------------------------------------------------- the cases, the oracle

def uniforms(case, n_out=None):
    seed, step = C.seed_step(case)
    return R.resample_uniforms(case[2] if n_out is None else n_out, seed, step)


def _oracle_delta(config, n):
    import pyoracle
    c, poses, empty, offs0, z = C.scenario(config, n)
    return pyoracle.update(c.copy(), poses, empty, offs0, z)[2]


_DELTA = {}


def oracle_normalised(case):
    """The oracle's normalised float32 log-weights of a case: the input weights
    (standalone), or input + the empty-map update's shift, rounded to float32
    (step), through its normalise."""
    import pyoracle
    path, config, n, dist = case
    w = C.weights(dist, n)
    if path == "step":
        if (config, n) not in _DELTA:
            _DELTA[(config, n)] = _oracle_delta(config, n)
        delta = _DELTA[(config, n)]
        assert np.ptp(delta) == 0, "the empty-map update shifts every particle alike"
        w = (w + delta).astype(np.float32)
    return pyoracle.normalize(w)[0]


def oracle_figures(case):
    import pyoracle
    ow = oracle_normalised(case)
    wn, dec = C.reference(case)
    return ow, C.lognorm_deviation(ow, wn), C.neff_deviation(pyoracle.neff(ow), dec.neff)


@pytest.mark.parametrize("case", C.CASES, ids=CASE_IDS)
def test_case_conditions_from_the_reference_alone(case):
    """No near decision (with a resample asked for, and at threshold 0), and at
    most 1 % near strata on the reference's own float32 normalised weights."""
    wn, dec = C.reference(case)
    assert dec.resample and not dec.near, dec
    d0 = R.decision(C.weights(case[3], case[2]), 0.0)
    assert not d0.resample and not d0.near, d0
    p = R.parents(wn.astype(np.float32), uniforms(case))
    assert p.near.sum() <= 0.01 * len(p.parent), (int(p.near.sum()), len(p.parent))


@pytest.mark.parametrize("case", C.CASES, ids=CASE_IDS)
def test_oracle_against_reference(built, case):
    import pyoracle
    ow, d_w, d_neff = oracle_figures(case)
    wn, dec = C.reference(case)
    k = C.key(case)
    print(f"{k}: lognorm {d_w:.3g}, neff {d_neff:.3g}")
    on = pyoracle.neff(ow)
    assert (on <= C.thresh(case[3], case[2])) == dec.resample
    u = uniforms(case)
    near, n, ref = C.hold_parents(pyoracle.resample_fixed(ow, u), ow, u, k)
    print(f"{k}: {near} of {n} strata near, {ref.beyond.size} past the end")
    for name, got in (("lognorm", d_w), ("neff", d_neff)):
        want = C.D_ORACLE[k][name]
        assert got <= want, (k, name, got, want)
        assert want <= 2 * got + 1e-12, (k, name, "table entry is stale", got)  # the table is the measurement


def _lowered(ow):
    """The standalone `tie` weights with the CDF's total lowered by 2^-10, so the last strata overrun it."""
    return (ow - np.float32(2.0 ** -10)).astype(np.float32)


@pytest.mark.parametrize("n", [1000, 2049, 4097, 20000])
def test_oracle_standalone_tie_overrun(built, n):
    """u[-1] = 1 - 2^-32 over a CDF whose total is 1 - 2^-10: the last strata
    take the first of the two equal maxima, and not as near strata."""
    import pyoracle
    ow = _lowered(oracle_normalised(("standalone", "phd", n, "tie")))
    u = R.resample_uniforms(n, C.SEED, C.STEP)
    u[-1] = 1.0 - 2.0 ** -32
    got = pyoracle.resample_fixed(ow, u)
    near, _, ref = C.hold_parents(got, ow, u, f"tie {n}")
    assert ref.beyond.size >= 1 and not ref.near[ref.beyond].any()
    assert ref.amax == n // 3 and (got[ref.beyond] == n // 3).all()


@pytest.mark.parametrize("n", sorted(C.TIE_SEED_STEP))
def test_tie_pairs_overrun(built, n):
    """The committed (seed, step) of the phd_step `tie` cases: the reference
    reports a stratum past the CDF's end on the oracle's normalised weights."""
    case = ("step", "phd", n, "tie")
    ow = oracle_normalised(case)
    ref = R.parents(ow, uniforms(case))
    assert ref.beyond.size >= 1 and ref.amax == n // 3


def test_live_particles_to_n_particles(built):
    """n_out < n: 1000 strata over 2500 live weights."""
    import pyoracle
    n_live, n_out = C.LIVE
    ow = pyoracle.normalize(C.weights("normal", n_live))[0]
    u = R.resample_uniforms(n_out, C.SEED, C.STEP)
    C.hold_parents(pyoracle.resample_fixed(ow, u), ow, u, "live")


def _find_tie_pairs():
    out = {}
    for n in (1000, 2049, 4097, 20000):
        ow = oracle_normalised(("step", "phd", n, "tie"))
        total = np.cumsum(np.exp(ow.astype(np.float64)))[-1]
        steps = np.arange(1, 2000001, dtype=np.uint64)  # the last stratum's draw at every step
        x0 = R.philox4x32_10([n - 1, steps, 0, R.STREAM_RESAMPLE], [C.SEED & 0xFFFFFFFF, C.SEED >> 32])[0]
        hit = np.flatnonzero((n - 1 + x0.astype(np.float64) * 2.0 ** -32) / n > total)
        out[n] = (C.SEED, int(steps[hit[0]])) if hit.size else None
        print(n, "total", total, "first steps", steps[hit[:3]])
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
    if "--tie" in sys.argv:
        print("TIE_SEED_STEP =", _find_tie_pairs())
    import shard_plan_cases as SC  # the gathered sizes of the sharded plan (tests/test_gpu_shard_plan.py)
    print("D_ORACLE = {")
    for case in C.CASES + SC.WCASES:
        _, d_w, d_neff = oracle_figures(case)
        print(f'    "{C.key(case)}": dict(lognorm={C.round_up(d_w):.2g}, neff={C.round_up(d_neff):.2g}),')
    print("}")
