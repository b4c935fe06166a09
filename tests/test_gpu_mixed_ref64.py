"""The device's mixed static + dynamic update, prediction and dynamic EAP map
against the float64 reference (tests/mixed_ref64.py), not against the oracle:
the shared cases of tests/mixed_ref64_cases.py through PHDFilter, compared per
class at

    tol(case, class) = D_oracle(case, class) + 1e-5

— the device is contracted to lie within 1e-5 of the oracle, and the oracle
lies D_oracle (measured on the CPU, committed in mixed_ref64_cases.D_ORACLE)
from the reference.  Normalised log-weights (the device's own normalise call)
in SURVEY §8(d)'s form: |a - b| <= tol max(|a|, |b|) + 1e-5.  A particle with a
near classification (the reference's own count) is left out, a map with a near
prune / merge is compared component by component.  The oracle is not called
here.  Every comparison's worst figures go to the parity record under labels
"mixed ref64 ...".
"""
import numpy as np
import pytest

import mixed_ref64_cases as C
from test_gpu_mixed import _filter
from test_gpu_parity import _record_elementwise

pytestmark = pytest.mark.gpu

ST_CANDIDATE_OVERFLOW_MX = 2  # csrc/phd_mixed_k.h
ST_MAP_OVERFLOW_MX = 4


def _run(name, **caps):
    """(lw + delta, the same normalised on the device, static maps, offsets,
    dynamic maps, offsets, status words, whether check_errors raised)."""
    import phdslam
    c = C.inputs(name)
    n = len(c.poses)
    f = _filter(C.config(name), n, **dict(c.caps, **caps))
    f.load(c.poses, c.lw, c.smaps, c.soffs)
    f.load_dynamic(c.dmaps, c.doffs)
    raised = False
    try:  # (an update reports an overflow of its own launch; the results stay readable)
        f.update(c.z)
        f.check_errors()
    except phdslam.PHDError as e:
        assert "capacity" in str(e), e
        raised = True
    status = f.particle_status() if len(c.z) else np.zeros(n, np.int32)
    gp, glw, gs, gso = f.export()
    gd, gdo = f.export_dynamic()
    f.normalize()
    gnorm = f.export(with_maps=False)[1]
    capacity = f.capacity
    f.close()
    assert gp.tobytes() == np.ascontiguousarray(c.poses).tobytes()  # poses untouched by the update
    # every covariance leaves the update symmetric to the bit (the merge symmetrises; the inputs are)
    assert np.array_equal(gs["cov"][:, 1], gs["cov"][:, 2])
    gc = gd["cov"].reshape(-1, 4, 4)
    assert np.array_equal(gc, gc.transpose(0, 2, 1))
    return glw, gnorm, gs, gso, gd, gdo, status, raised, capacity


def _compare(name, label, res, skip=()):
    glw, gnorm, gs, gso, gd, gdo = res[:6]
    tol = {k: C.D_ORACLE[name][k] + C.CONTRACT for k in C.CLASSES}
    worst, bad, compared = C.deviations(name, gs, gso, gd, gdo, glw, gnorm, tol, skip=skip)
    print(f"{label}: " + ", ".join(f"{k} {worst[k]:.3g} (D_oracle {C.D_ORACLE[name][k]:.2g})" for k in C.CLASSES)
          + f"; {compared} particles")
    _record_elementwise(dict(label=label, reference="mixed_ref64", particles=len(glw), compared=compared,
                             **{f"ref64_{k}": worst[k] for k in C.CLASSES},
                             **{f"d_oracle_{k}": C.D_ORACLE[name][k] for k in C.CLASSES}))
    assert not bad, f"{label}: {bad[:5]}"
    assert compared >= len(glw) - C.max_left_out(name) - len(skip)
    for k in C.CLASSES:
        assert worst[k] <= tol[k], f"{label}: {k} deviates {worst[k]:.3g} from the reference, tolerance {tol[k]:.3g}"


@pytest.mark.parametrize("name", C.CASES)
def test_case_matches_reference(gpu, name):
    res = _run(name)
    assert not res[7] and not res[6].any(), f"{name}: status {res[6]}"
    _compare(name, f"mixed ref64 {name}", res)


def _field_check(label, name, ref, got):
    worst = C.field_deviations(ref, got)
    assert worst is not None, f"{label}: {len(got)} components, the reference has {len(ref)}"
    print(f"{label}: " + ", ".join(f"{k} {worst[k]:.3g} (D_oracle {C.D_ORACLE[name][k]:.2g})" for k in C.FIELD_CLASSES))
    _record_elementwise(dict(label=label, reference="mixed_ref64", components=len(ref),
                             **{f"ref64_{k}": worst[k] for k in C.FIELD_CLASSES},
                             **{f"d_oracle_{k}": C.D_ORACLE[name][k] for k in C.FIELD_CLASSES}))
    for k in C.FIELD_CLASSES:
        tol = C.D_ORACLE[name][k] + C.CONTRACT
        assert worst[k] <= tol, f"{label}: {k} deviates {worst[k]:.3g} from the reference, tolerance {tol:.3g}"


@pytest.mark.parametrize("name", C.PREDICT_CASES)
def test_predict_dynamic_matches_reference(gpu, name):
    """Sizes 0, 1 and dcap; speeds 0 .. 2 tau, tau itself among them."""
    cfg, poses, sm, so, dm, do, dcap = C.predict_inputs(name)
    n = len(poses)
    f = _filter(cfg.copy(), n, dcap=dcap)
    f.load(poses, np.zeros(n, np.float32), sm, so)
    f.load_dynamic(dm, do)
    f.predict_dynamic()
    g, go = f.export_dynamic()
    f.close()
    assert np.array_equal(go, do)
    _field_check(f"mixed ref64 {name}", name, C.predict_reference(name), g)


@pytest.mark.parametrize("name", C.EAP_CASES)
def test_expected_map_dynamic_matches_reference(gpu, name):
    cfg, poses, lw, sm, so, dm, do, caps = C.eap_inputs(name)
    n = len(poses)
    f = _filter(cfg.copy(), n, **caps)
    f.load(poses, lw, sm, so)
    f.load_dynamic(dm, do)
    eap = f.expected_map_dynamic()
    f.close()
    ref, near = C.eap_reference(name)
    assert near == 0
    _field_check(f"mixed ref64 {name}", name, ref, eap)


def _overflow_check(label, bit, over, res, capacity_ok):
    status, raised = res[6], res[7]
    assert over.any() and not over.all(), f"{label}: the capacity does not split the particles"
    assert raised, f"{label}: check_errors did not report the overflow"
    assert np.array_equal((status & bit) != 0, over), f"{label}: status {status}, expected on {np.flatnonzero(over)}"
    assert not (status & ~bit).any(), f"{label}: other status bits {status}"
    assert capacity_ok
    _compare("mx_mid", f"mixed ref64 mx_mid {label}", res, skip=tuple(np.flatnonzero(over)))


def test_candidate_overflow_status(gpu):
    """candidate_capacity below some particles' reference candidate count: the bit
    on exactly those particles, every other particle still the reference's."""
    k = C.candidate_counts("mx_mid")
    K = int(np.sort(k.max(1))[len(k) // 2])
    res = _run("mx_mid", K=K)
    assert res[8].candidate_capacity == K
    _overflow_check("candidate overflow", ST_CANDIDATE_OVERFLOW_MX, (k > K).any(1), res, True)


def test_map_overflow_status(gpu):
    """map_capacity / dyn_capacity below some particles' reference merged count:
    the bit on exactly those particles, exported sizes clamped to the capacity,
    every other particle still the reference's."""
    c, r = C.inputs("mx_mid"), C.reference("mx_mid")
    ns, nd = np.diff(r.soffs), np.diff(r.doffs)
    cap = max(int(np.sort(ns)[len(ns) // 2]), int(np.diff(c.soffs).max()))
    dcap = max(int(np.sort(nd)[len(nd) // 2]), int(np.diff(c.doffs).max()))
    over = (ns > cap) | (nd > dcap)
    assert (ns > cap).any() and (nd > dcap).any()
    res = _run("mx_mid", cap=cap, dcap=dcap)
    gso, gdo = res[3], res[5]
    assert res[8].map_capacity == cap
    assert np.array_equal(np.diff(gso), np.minimum(ns, cap)) and np.array_equal(np.diff(gdo), np.minimum(nd, dcap))
    _overflow_check("map overflow", ST_MAP_OVERFLOW_MX, over, res, True)
