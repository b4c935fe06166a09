"""The device update against the float64 reference (tests/update_ref64.py), not
against the oracle: the shared cases of tests/update_ref64_cases.py through the
C ABI, compared per field class at

    tol(case, class) = D_oracle(case, class) + 1e-5

— the device is contracted to lie within 1e-5 of the oracle, and the oracle
lies D_oracle (measured on the CPU, committed in update_ref64_cases.D_ORACLE)
from the reference.  compare_maps' scale floors hold for cancellation entries,
the 1e-12 floor for weights.  Normalised log-weights (the device's own
normalise call) in SURVEY §8(d)'s form: |a - b| <= tol max(|a|, |b|) + 1e-5.
A particle with a near classification (the reference's own count) is left out,
one with a near prune / merge is compared component by component.  The oracle
is not called here.  Every comparison's worst figures go to the parity record.
"""
import numpy as np
import pytest

import update_ref64_cases as C
from test_gpu_parity import _filter, _record_elementwise

pytestmark = pytest.mark.gpu


def _run(name, threads=0, form=0):
    """(lw + delta, the same normalised on the device, maps, offsets, cardinality rows or None)."""
    cfg, poses, lw, maps, offs, z = C.inputs(name)
    n = len(poses)
    f = _filter(C.config(name), n)
    if form:
        f.set_update_form(form)
    if threads:
        f.set_update_threads(threads)
    f.load(poses, lw, maps, offs)
    f.set_step_births(0)
    f.update(z)
    f.check_errors()
    gp, glw, gmaps, goffs = f.export()
    used = (f.update_threads()[0], f.update_form())
    cn = f.cardinality_distribution().astype(np.float64) if cfg.filterType == 1 else None
    f.normalize()
    gnorm = f.export(with_maps=False)[1]
    f.close()
    assert gp.tobytes() == np.ascontiguousarray(poses).tobytes()  # poses untouched by the update
    return glw, gnorm, gmaps, goffs, cn, used


def _check(name, threads=0, form=0):
    glw, gnorm, gmaps, goffs, cn, used = _run(name, threads, form)
    if threads:
        assert used[0] == threads
    if form:
        assert used[1] == (form == 2)
    tol = {k: C.D_ORACLE[name][k] + C.CONTRACT for k in C.CLASSES}
    worst, bad, compared = C.deviations(name, gmaps, goffs, glw, gnorm, cn, tol)
    label = f"ref64 {name} t{threads} f{form}"
    print(f"{label}: " + ", ".join(f"{k} {worst[k]:.3g} (D_oracle {C.D_ORACLE[name][k]:.2g})" for k in C.CLASSES)
          + f"; {compared} particles")
    _record_elementwise(dict(label=label, reference="update_ref64", particles=len(glw), compared=compared,
                             **{f"ref64_{k}": worst[k] for k in C.CLASSES},
                             **{f"d_oracle_{k}": C.D_ORACLE[name][k] for k in C.CLASSES}))
    assert not bad, f"{label}: {bad[:5]}"
    assert compared >= len(glw) - C.max_left_out(name)
    for k in C.CLASSES:
        assert worst[k] <= tol[k], f"{label}: {k} deviates {worst[k]:.3g} from the reference, tolerance {tol[k]:.3g}"


@pytest.mark.parametrize("name", C.CASES)
def test_case_matches_reference(gpu, name):
    _check(name)


@pytest.mark.parametrize("threads", [256, 512, 1024])
@pytest.mark.parametrize("name", ["phd_wide", "cphd_mid"])
def test_workgroup_sizes(gpu, name, threads):
    _check(name, threads=threads)


@pytest.mark.parametrize("form", [1, 2])
@pytest.mark.parametrize("threads", [256, 512, 1024])
def test_phd_update_forms(gpu, threads, form):
    """One fused launch (form 1) and part A + part C (form 2) at every workgroup size."""
    _check("phd_wide", threads=threads, form=form)


@pytest.mark.parametrize("form", [1, 2])
def test_hellinger_forms(gpu, form):
    _check("hell_mid", form=form)
