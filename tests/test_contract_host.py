"""The host half of the CPU / gfx950 bit contract (D5, D6, D8, D14,
D16-D18): the helpers of include/phd_detmath.h, include/phd_rng.h and
csrc/phd_device.h, one function at a time.

  * hipcc's host compiler (tests/contract_probe.hip, probe_host_*), the g++
    oracle and the oracle's optimised build (x86-64-v3) give the same bits on
    every input set of tests/contract_inputs.py (NaN matches NaN);
  * the accuracy bounds of test_oracle_closed_form.py / test_oracle_mixed.py
    hold against mpmath at 80 digits on the adversarial sets and 4096 sweep
    points; the worst measured value is recorded beside each bound;
  * phd_fix_term / phd_fix_stratum equal exact integer / Fraction arithmetic of
    the correctly rounded double operations.

Needs no device.  The device half is tests/test_gpu_contract.py.
"""
from fractions import Fraction

import numpy as np
import pytest

import contract_inputs as ci
import contract_legs as legs
from test_gpu_parity import _record_elementwise


@pytest.fixture(scope="module")
def probe(built):
    return legs.load_probe()


@pytest.fixture(scope="module")
def cases(built):
    return legs.cases()


@pytest.mark.parametrize("name", list(legs.SPEC))
def test_host_legs_same_bits(probe, cases, name):
    x = cases[name]
    cfg = legs.config()
    got = {"hipcc-host": legs.probe(probe, "host", name, x, cfg), "g++": legs.oracle(name, x, cfg)}
    if name != "hellinger":  # (its host leg is the one numpy restatement)
        got["g++ x86-64-v3"] = legs.oracle(name, x, cfg, fast=True)
    n, bad, msg = legs.mismatch(name, x, got)
    _record_elementwise(dict(label=f"contract {name}", legs=list(got), compared=n, mismatches=bad))
    assert bad == 0, msg


def test_philox_known_answers(probe):
    x = ci.philox_set()[:len(ci.PHILOX_KAT)]
    want = np.array([r for _, _, r in ci.PHILOX_KAT], np.uint32)
    np.testing.assert_array_equal(legs.probe(probe, "host", "philox4x32_10", x), want)
    np.testing.assert_array_equal(legs.oracle("philox4x32_10", x), want)


def test_rng_draw_is_philox_of_the_counter(probe):
    """phd_rng_draw = Philox of (index, step lo, step hi, stream) under the key (seed lo, seed hi)."""
    d = ci.rng_draw_set()
    ctr = np.stack([d["index"], (d["step"] & np.uint64(0xffffffff)).astype(np.uint32),
                    (d["step"] >> np.uint64(32)).astype(np.uint32), d["stream"],
                    (d["seed"] & np.uint64(0xffffffff)).astype(np.uint32),
                    (d["seed"] >> np.uint64(32)).astype(np.uint32)], 1).astype(np.uint32)
    np.testing.assert_array_equal(legs.probe(probe, "host", "rng_draw", d),
                                  legs.probe(probe, "host", "philox4x32_10", ctr))


def test_u01_exact(probe):
    x = ci.u01_set()
    np.testing.assert_array_equal(legs.probe(probe, "host", "u01", x), x.astype(np.float64) * 2.0 ** -32)


def test_fix_term_exact(probe):
    """floor(t 2^40): the double product of a float and 2^40 is exact."""
    t = ci.fix_term_set()
    want = np.array([int(Fraction(float(v)) * 2 ** 40) for v in t], np.uint64)
    np.testing.assert_array_equal(legs.probe(probe, "host", "fix_term", t), want)
    np.testing.assert_array_equal(legs.oracle("fix_term", t), want)


def _rn(q):
    """The double nearest to the rational q (ties to even): Python's conversion is correctly rounded."""
    return Fraction(float(q))


def test_fix_stratum_exact(probe):
    """floor(RN(RN(j + u) / n) 2^40) in exact rational arithmetic."""
    s = ci.fix_stratum_set()
    want = np.array([int(_rn(_rn(Fraction(int(j)) + Fraction(float(u))) / int(n)) * 2 ** 40) for u, j, n in s.tolist()],
                    np.uint64)
    np.testing.assert_array_equal(legs.probe(probe, "host", "fix_stratum", s), want)
    np.testing.assert_array_equal(legs.oracle("fix_stratum", s), want)


# ---- accuracy against mpmath ----

def _sample(adv, cap=15000):
    """At most cap adversarial inputs (an even stride) plus 4096 sweep points:
    under 20 000 mpmath evaluations per function."""
    adv = np.asarray(adv)
    if len(adv) > cap:
        adv = adv[::-(-len(adv) // cap)]
    return adv


def _ulp_err(got, ref):
    """|got - ref| in units of the float spacing at |ref| (the measure of the
    existing oracle tests: np.spacing(float32(|ref|))), for mpmath refs."""
    import mpmath
    out = np.zeros(len(ref))
    for i, (g, r) in enumerate(zip(got.tolist(), ref)):
        sp = float(np.spacing(np.float32(abs(float(r))))) if r != 0 else float(np.float32(1e-45))
        out[i] = float(abs(mpmath.mpf(g) - r) / sp)
    return out


def _record_accuracy(name, n, bound, worst):
    print(f"contract accuracy {name}: {n} inputs, bound {bound} ulp, worst measured {worst:.6f} ulp")
    _record_elementwise(dict(label=f"contract accuracy {name}", reference="mpmath 80 digits", compared=n,
                             bound_ulp=bound, worst_ulp=worst))


def test_det_expf_accuracy(probe):
    """test_oracle_closed_form.test_det_expf_accuracy's bound: relative error
    < 1.2e-7 where exp(x) > 1e-37 (about 2 float ulp).  Worst measured here:
    0.500000 ulp, relative 5.83e-8 (an evaluation in double rounded once)."""
    import mpmath
    x = np.concatenate([ci.expf_set(), ci.sweep_sample()])
    x = x[np.isfinite(x) & (np.abs(x) < 200)]
    got = legs.probe(probe, "host", "det_expf", x)
    with mpmath.workdps(80):
        ref = [mpmath.exp(mpmath.mpf(float(v))) for v in x]
        fin = np.isfinite(got)
        # past the overflow threshold the result is inf: there the true value must round to inf
        assert all(ref[i] > mpmath.mpf(2) ** 128 - mpmath.mpf(2) ** 103 for i in np.flatnonzero(~fin))
        idx = np.flatnonzero(fin)
        rel = np.array([float(abs(mpmath.mpf(float(got[i])) - ref[i]) / ref[i]) for i in idx])
        big = np.array([ref[i] > 1e-37 for i in idx])
        ulp = _ulp_err(got[idx], [ref[i] for i in idx])
    assert np.all(rel[big] < 1.2e-7)
    assert np.all(ulp <= 1.0)  # (subnormal results included: one rounding of the double value)
    _record_accuracy("det_expf", len(idx), 1.0, float(ulp.max()))
    print(f"contract accuracy det_expf: worst relative error above 1e-37: {rel[big].max():.3e} (bound 1.2e-7)")


def test_det_logf_accuracy(probe):
    """test_oracle_mixed.test_det_logf_within_one_ulp's bound: 1 ulp.  Worst
    measured here: 0.500000 ulp."""
    import mpmath
    x = np.concatenate([ci.logf_set(), ci.sweep_sample()])
    x = x[np.isfinite(x) & (x > 0)]
    got = legs.probe(probe, "host", "det_logf", x)
    with mpmath.workdps(80):
        ulp = _ulp_err(got, [mpmath.log(mpmath.mpf(float(v))) for v in x])
    assert np.all(ulp <= 1.0)
    _record_accuracy("det_logf", len(x), 1.0, float(ulp.max()))
    edge = legs.probe(probe, "host", "det_logf", np.array([0.0, -0.0, np.inf, -1.0, np.nan], np.float32))
    assert edge[0] == -np.inf and edge[1] == -np.inf and edge[2] == np.inf and np.isnan(edge[3]) and np.isnan(edge[4])


def test_atan2f_accuracy(probe):
    """test_oracle_closed_form.test_shared_atan2f_correctly_rounded's bound: 1
    ulp.  Worst measured here: 0.500000 ulp."""
    import mpmath
    yx = _sample(ci.atan2f_set())
    yx = yx[np.all(np.isfinite(yx), 1)]
    got = legs.probe(probe, "host", "atan2f", yx)
    with mpmath.workdps(80):
        # (mpmath has no signed zero: the sign of y, -0 included, is applied to atan2(|y|, x);
        #  x = -0 with y = 0 gives pi)
        ref = [(-1 if np.signbit(y) else 1) * (mpmath.atan2(mpmath.mpf(abs(float(y))), mpmath.mpf(float(x)))
                                               if (y != 0 or x != 0) else (mpmath.pi if np.signbit(x) else mpmath.mpf(0)))
               for y, x in yx]
        ulp = _ulp_err(got, ref)
    assert np.all(ulp <= 1.0)
    z = np.array(ref, object) == 0
    assert np.all(np.signbit(got[z]) == np.signbit(yx[z, 0]))  # +-0 keeps the sign of y
    _record_accuracy("atan2f", len(yx), 1.0, float(ulp.max()))


def test_sincosf_tanf_accuracy(probe):
    """test_oracle_closed_form.test_shared_sincosf_tanf_correctly_rounded's
    bound for sin and cos: 1 ulp, on |x| < 1.5e6 (the deterministic range).
    tan: the same 1 ulp (the quotient of the two double values, whose relative
    error next to a multiple of pi/2 is that of the reduced argument, < 1e-10
    for a float below 1.5e6, far under the float's half ulp).  Worst measured
    here: sin 0.499992, cos 0.499989, tan 0.499961 ulp."""
    import mpmath
    x = np.concatenate([_sample(ci.trig_set(), 14000), ci.sweep_sample()])
    x = x[np.abs(x) < 1.5e6]
    sc = legs.probe(probe, "host", "det_sincosf", x)
    tn = legs.probe(probe, "host", "det_tanf", x)
    with mpmath.workdps(80):
        mx = [mpmath.mpf(float(v)) for v in x]
        us = _ulp_err(sc[:, 0], [mpmath.sin(v) for v in mx])
        uc = _ulp_err(sc[:, 1], [mpmath.cos(v) for v in mx])
        ut = _ulp_err(tn, [mpmath.tan(v) for v in mx])
    for nm, u in (("det_sincosf sin", us), ("det_sincosf cos", uc), ("det_tanf", ut)):
        assert np.all(u <= 1.0), nm
        _record_accuracy(nm, len(x), 1.0, float(u.max()))
    assert tuple(legs.probe(probe, "host", "det_sincosf", np.zeros(1, np.float32))[0]) == (0.0, 1.0)


def test_box_muller_host_within_structural_bound(probe):
    """phd_box_muller on the host (glibc's double log / cos / sin) within
    1e-13 max(|value|, rad) of the mpmath value: the bound the device is held to
    in tests/test_gpu_contract.py."""
    x, _, _, rad = legs.box_muller_ref()
    for leg, got in (("hipcc-host", legs.probe(probe, "host", "box_muller", x)), ("g++", legs.oracle("box_muller", x))):
        worst = legs.box_muller_worst(got)
        print(f"contract box_muller {leg}: worst distance from mpmath {worst:.3e} of max(|value|, rad)")
        _record_elementwise(dict(label="contract box_muller accuracy", leg=leg, compared=len(x), worst=worst,
                                 bound=legs.BM_BOUND))
        assert worst <= legs.BM_BOUND
        top = np.asarray(got).reshape(-1, 2)[x[:, 0] == 2 ** 32 - 1]
        assert np.all(top == 0)  # u1 = 1: rad = -0
