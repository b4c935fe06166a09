"""The legs of the CPU / gfx950 bit contract: each covered function over an
array of records on the device and on hipcc's host compiler
(tests/contract_probe.hip), on the g++ oracle in both builds of its Makefile
(oracle/scphd_cpu.cpp, orc_arr_*), and d_hellinger in numpy float32
(tests/hellinger_ref.py).

TEST INFRASTRUCTURE ONLY.
"""
import ctypes
import importlib.util
import os

import numpy as np

import hellinger_ref
import pyoracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# function -> (words per input record, output dtype, output words per record, takes the config)
SPEC = {
    "det_expf": (1, np.float32, 1, False),
    "det_logf": (1, np.float32, 1, False),
    "det_tanf": (1, np.float32, 1, False),
    "det_sincosf": (1, np.float32, 2, False),
    "atan2f": (2, np.float32, 1, False),
    "fix_term": (1, np.uint64, 1, False),
    "fix_stratum": (None, np.uint64, 1, False),
    "philox4x32_10": (6, np.uint32, 4, False),
    "rng_draw": (None, np.uint32, 4, False),
    "u01": (1, np.float64, 1, False),
    "box_muller": (2, np.float64, 2, False),
    "wrap": (1, np.float32, 1, False),
    "det_safe_log": (1, np.float32, 1, False),
    "compute_ekf": (9, np.float32, 16, True),
    "birth": (5, np.float32, 6, True),
    "mahal": (12, np.float32, 1, False),
    "hellinger": (12, np.float32, 1, False),
}
EKF_FIELDS = ("r", "bearing", "pd", "det", "S0", "S1", "S2", "S3", "K0", "K1", "K2", "K3", "cu0", "cu1", "cu2", "cu3")


def load_probe():
    """Build tests/libcontract_probe.so (build_contract_probe of build.py: the
    product's flags) and load it."""
    spec = importlib.util.spec_from_file_location("phd_build", os.path.join(REPO, "cuda-phdslam_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return ctypes.CDLL(mod.build_contract_probe())


def _count(name, x):
    words = SPEC[name][0]
    x = np.ascontiguousarray(x)
    if words is None:
        return x, len(x)
    assert x.size % words == 0 and x.dtype.itemsize == 4, (name, x.dtype, x.shape)
    return x, x.size // words


def _out(name, n):
    _, dt, ow, _ = SPEC[name]
    return np.zeros((n, ow) if ow > 1 else n, dt)


def _call(fn, name, x, cfg):
    x, n = _count(name, x)
    out = _out(name, n)
    vp = ctypes.c_void_p
    args = [vp(x.ctypes.data), vp(out.ctypes.data), ctypes.c_long(n)]
    if SPEC[name][3]:
        args.insert(0, ctypes.cast(ctypes.pointer(cfg), vp))
    fn.restype = ctypes.c_int
    fn.argtypes = [type(a) for a in args]
    rc = fn(*args)
    return rc, out


def probe(lib, leg, name, x, cfg=None):
    """leg 'dev' (one kernel on the GPU) or 'host' (hipcc's host compiler)."""
    rc, out = _call(getattr(lib, f"probe_{leg}_{name}"), name, x, cfg)
    if rc != 0:
        raise RuntimeError(f"probe_{leg}_{name}: HIP status {rc}")
    return out


def oracle(name, x, cfg=None, fast=False):
    """The g++ leg: orc_arr_<name> of liboracle.so (fast: liboracle_fast.so);
    d_hellinger's host leg is the numpy restatement."""
    if name == "hellinger":
        x = np.ascontiguousarray(x, np.float32).reshape(-1, 12)
        return hellinger_ref.hellinger(x[:, 0:2], x[:, 2:6], x[:, 6:8], x[:, 8:12])
    fn = getattr(pyoracle.lib(fast), f"orc_arr_{name}")
    _, out = _call(fn, name, x, cfg)
    return out


def canon(a):
    """The bits of a result array as unsigned integers, every NaN mapped to one
    pattern (NaN matches NaN; payloads are not part of the contract)."""
    a = np.ascontiguousarray(a)
    if a.dtype.kind != "f":
        return a
    u = a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64).copy()
    u[np.isnan(a)] = np.array(0x7fc00000 if a.dtype.itemsize == 4 else 0x7ff8000000000000, u.dtype)
    return u


def _hex(rec):
    rec = np.ascontiguousarray(rec)
    w = rec.reshape(1).view(np.uint32) if rec.dtype.names else np.atleast_1d(rec).view(
        np.uint32 if rec.dtype.itemsize == 4 else np.uint64)
    return " ".join(f"{int(v):#x}" for v in w) + f" ({rec.tolist()})"


def mismatch(name, x, legs, mask=None):
    """Compare the legs {label: result} bit for bit.  Returns (elements
    compared, mismatches, message): an element mismatches when any leg differs
    from the first in any output word; the message names the first differing
    input as hex with every leg's result there.  mask: the elements compared."""
    x, n = _count(name, x)
    xr = x.reshape(n, -1) if not x.dtype.names else x
    labels = list(legs)
    cs = [canon(legs[k]).reshape(n, -1) for k in labels]
    bad = np.zeros(n, bool)
    for c in cs[1:]:
        bad |= np.any(c != cs[0], axis=1)
    if mask is not None:
        bad &= mask
        n = int(np.sum(mask))
    cnt = int(bad.sum())
    msg = ""
    if cnt:
        i = int(np.flatnonzero(bad)[0])
        res = "; ".join(f"{k}: {_hex(np.asarray(legs[k]).reshape(len(bad), -1)[i])}" for k in labels)
        msg = f"contract {name}: {cnt} of {n} differ; first at element {i}, input {_hex(xr[i])}: {res}"
    return n, cnt, msg


def config():
    """The configuration of the d_* helpers' sets: the typical ranges (0.5 ..
    60 m) and bearings (over +-pi) fall on both sides of maxRange / maxBearing,
    so pd takes both values."""
    import phdslam
    c = phdslam.default_config()
    c.minRange, c.maxRange, c.maxBearing = 1.0, 30.0, 2.0
    c.stdRange, c.stdBearing, c.pd = 0.25, 0.008727, 0.95
    c.birthNoiseFactor = 1.5
    return c


def cases():
    """function -> its input records (tests/contract_inputs.py)."""
    import contract_inputs as ci
    sw = ci.sweep()
    trig = np.concatenate([sw, ci.trig_set()])
    ekf, birth, pair = ci.ekf_set()[0], ci.birth_set()[0], ci.pair_set()[0]
    return {
        "det_expf": np.concatenate([sw, ci.expf_set()]),
        "det_logf": np.concatenate([sw, ci.logf_set()]),
        "det_tanf": trig,
        "det_sincosf": trig,
        "atan2f": ci.atan2f_set(),
        "fix_term": ci.fix_term_set(),
        "fix_stratum": ci.fix_stratum_set(),
        "philox4x32_10": ci.philox_set(),
        "rng_draw": ci.rng_draw_set(),
        "u01": ci.u01_set(),
        "box_muller": ci.box_muller_set(),
        "wrap": np.concatenate([sw, ci.near([ci.PI, -ci.PI, 2 * ci.PI, -2 * ci.PI, 3 * ci.PI, -3 * ci.PI], 3)]),
        "det_safe_log": np.concatenate([sw, ci.logf_set()]),
        "compute_ekf": ekf,
        "birth": birth,
        "mahal": pair,
        "hellinger": pair,
    }


_BM_REF = None


def box_muller_ref(m=4096):
    """Box-Muller of the crossed edge words and the first m LCG pairs of
    contract_inputs.box_muller_set() in mpmath at 80 digits, rounded to float64:
    (records, n0, n1, rad).  Computed once."""
    global _BM_REF
    if _BM_REF is None:
        import contract_inputs as ci
        import mpmath
        x = ci.box_muller_set()[:ci.BM_CROSSED + m]
        with mpmath.workdps(80):
            out = []
            for a, b in x.tolist():
                rad = mpmath.sqrt(-2 * mpmath.log(mpmath.mpf(a + 1) / 2 ** 32))
                ang = 2 * mpmath.pi * mpmath.mpf(b) / 2 ** 32
                out.append((float(rad * mpmath.cos(ang)), float(rad * mpmath.sin(ang)), float(rad)))
        o = np.array(out, np.float64)
        _BM_REF = (x, o[:, 0], o[:, 1], o[:, 2])
    return _BM_REF


BM_BOUND = 1e-13  # structural: a float32 evaluation or a wrong constant shows at >= 6e-8, a double library near 1e-16


def box_muller_worst(got, m=4096):
    """Worst |got - reference| / max(|reference|, rad) of a leg's Box-Muller
    outputs over box_muller_ref()'s records (0 where rad = 0: u1 = 1)."""
    x, n0, n1, rad = box_muller_ref(m)
    g = np.asarray(got, np.float64).reshape(-1, 2)[:len(x)]
    worst = 0.0
    for k, ref in ((0, n0), (1, n1)):
        scale = np.maximum(np.abs(ref), rad)
        err = np.abs(g[:, k] - ref)
        assert np.all(err[scale == 0] == 0)
        worst = max(worst, float(np.max(err[scale > 0] / scale[scale > 0])))
    return worst
