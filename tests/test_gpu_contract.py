"""The device half of the CPU / gfx950 bit contract (D5, D6, D8,
D14, D16-D18): every helper of include/phd_detmath.h, include/phd_rng.h and
csrc/phd_device.h evaluated alone on the device (tests/contract_probe.hip,
built with the product's flags) and compared bit for bit with hipcc's host
compiler and with the g++ oracle on the input sets of tests/contract_inputs.py.
The expected number of mismatches is 0: the contract as DESIGN states it.

The probe holds the headers under the product's flags, not the instruction
stream of the update kernels; float operations with contraction off do not
depend on the surrounding kernel.

phd_box_muller calls the platform's double log / cos / sin (glibc / ocml), which
are not exact primitives: its device outputs are held to a structural bound
against mpmath, and their distance from the host's is recorded.
"""
import numpy as np
import pytest

import contract_inputs as ci
import contract_legs as legs
from test_gpu_parity import _record_elementwise

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probe(built, gpu):
    return legs.load_probe()


@pytest.fixture(scope="module")
def cases(built):
    return legs.cases()


def _three_legs(probe, name, x):
    cfg = legs.config()
    return {"device": legs.probe(probe, "dev", name, x, cfg), "hipcc-host": legs.probe(probe, "host", name, x, cfg),
            "g++": legs.oracle(name, x, cfg)}


def _assert_same_bits(probe, name, x, mask=None):
    got = _three_legs(probe, name, x)
    n, bad, msg = legs.mismatch(name, x, got, mask)
    print(f"contract {name}: {n} elements, {bad} mismatches (device, hipcc-host, g++)")
    _record_elementwise(dict(label=f"contract {name}", legs=list(got), compared=n, mismatches=bad))
    assert bad == 0, msg
    return got


EXACT = [f for f in legs.SPEC if f not in ("det_sincosf", "det_tanf", "box_muller")]


@pytest.mark.parametrize("name", EXACT)
def test_device_bits(probe, cases, name):
    _assert_same_bits(probe, name, cases[name])


def _f32_ordered(a):
    i = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7fffffff), i)


def _f64_ordered(a):
    i = np.ascontiguousarray(a, np.float64).view(np.int64)
    return np.where(i < 0, -(i & np.int64(0x7fffffffffffffff)), i)


@pytest.mark.parametrize("name", ["det_sincosf", "det_tanf"])
def test_device_bits_trig(probe, cases, name):
    """Bits asserted on |x| < 1.5e6 (the deterministic reduction); beyond it
    (and for NaN) both sides take their platform's function: the device's
    distance from the host there is recorded, not asserted."""
    x = cases[name]
    inside = np.abs(x) < 1.5e6
    got = _assert_same_bits(probe, name, x, inside)
    out = ~inside & np.isfinite(x)
    d, h = np.asarray(got["device"]).reshape(len(x), -1)[out], np.asarray(got["hipcc-host"]).reshape(len(x), -1)[out]
    fin = np.isfinite(d) & np.isfinite(h)
    dist = np.abs(_f32_ordered(d[fin]) - _f32_ordered(h[fin]))
    rec = dict(label=f"contract {name} platform range", compared=int(fin.sum()), differing=int(np.sum(dist > 0)),
               worst_float_ulps=int(dist.max()) if dist.size else 0)
    print(rec)
    _record_elementwise(rec)


def test_philox_known_answers_on_device(probe):
    x = ci.philox_set()[:len(ci.PHILOX_KAT)]
    want = np.array([r for _, _, r in ci.PHILOX_KAT], np.uint32)
    np.testing.assert_array_equal(legs.probe(probe, "dev", "philox4x32_10", x), want)


def test_box_muller_device(probe):
    """phd_box_muller on the device (ocml's double log / cos / sin): within
    1e-13 max(|value|, rad) of the mpmath value (a float32 evaluation or a wrong
    constant shows at >= 6e-8, a double library specified to a few ulp near
    1e-16).  Recorded, not asserted: the worst device-host distance in double
    ulps over the 2^18 LCG pairs and the number of pairs whose float noise
    (float)(sigma g) differs from the host's, for the sigmas of presets 1 and 3.
    Where that number is not 0, each differing value differs by exactly one
    float ulp: device-Philox noise then matches the oracle's to an ulp, not to
    the bit (RNG row)."""
    import phdslam
    x = ci.box_muller_set()
    dev = legs.probe(probe, "dev", "box_muller", x)
    host = legs.oracle("box_muller", x)
    worst = legs.box_muller_worst(dev)
    print(f"contract box_muller device: worst distance from mpmath {worst:.3e} of max(|value|, rad)")
    rec = dict(label="contract box_muller", compared=len(x), mpmath_compared=len(legs.box_muller_ref()[0]),
               worst_vs_mpmath=worst, bound=legs.BM_BOUND)
    assert worst <= legs.BM_BOUND
    assert np.all(dev[x[:, 0] == 2 ** 32 - 1] == 0)  # u1 = 1: rad = -0
    dist = np.abs(_f64_ordered(dev) - _f64_ordered(host))
    rec.update(double_mismatches=int(np.sum(np.any(dist > 0, 1))), worst_double_ulps=int(dist.max()))
    lcg_pairs = slice(ci.BM_CROSSED, None)
    sig = {}
    for preset in (1, 3):
        cfg = phdslam.preset(preset)[0]
        for nm, s in (("stdAlpha", np.float64(np.float32(cfg.stdAlpha))),
                      ("stdEncoder", np.float64(np.float32(cfg.stdEncoder))),
                      ("3 ax", np.float64(np.float32(3) * np.float32(cfg.ax)))):
            nd = (s * dev[lcg_pairs]).astype(np.float32)
            nh = (s * host[lcg_pairs]).astype(np.float32)
            fd = np.abs(_f32_ordered(nd) - _f32_ordered(nh))
            sig[f"preset {preset} {nm}={float(s):.6g}"] = int(np.sum(np.any(fd > 0, 1)))
            assert np.all(fd <= 1), f"float noise more than one ulp from the host's (sigma {nm}, preset {preset})"
    rec["float_noise_pairs_differing"] = sig
    print(rec)
    _record_elementwise(rec)
