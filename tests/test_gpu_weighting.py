"""The device's weighting stage — log-sum-exp normalisation, nEff, the resample
decision, the stratified resample and the parent remap — against the float64
reference tests/weighting_ref.py, in every device form and at the edges of each
(the shared cases of tests/weighting_cases.py).  The oracle is not called.

Normalised log-weights (SURVEY §8(d)'s form) and nEff (relative) are held to
D_oracle(case) + 1e-5: the device is contracted to lie within 1e-5 of the
oracle, which lies D_oracle (measured on the CPU, weighting_cases.D_ORACLE)
from the reference.  Parents are held to the reference's rule on the device's
own exported normalised weights: equal to the reference's parent where the
stratum is not near, among the admissible parents where it is, at most 1 % of
the strata near (weighting_ref's band).  Every comparison's worst figures and
near count go to the parity record.
"""
import numpy as np
import pytest

import weighting_cases as C
import weighting_ref as R
from test_gpu_parity import _filter, _record_elementwise

pytestmark = pytest.mark.gpu


def _ids(cases):
    return [C.key(c) for c in cases]


def _weights_close(case, got, label, rec):
    wn, dec = C.reference(case)
    d = C.lognorm_deviation(got, wn)
    tol = C.D_ORACLE[C.key(case)]["lognorm"] + C.CONTRACT
    rec.update(lognorm=d, d_oracle_lognorm=C.D_ORACLE[C.key(case)]["lognorm"])
    print(f"{label}: lognorm {d:.3g} (tolerance {tol:.3g})")
    assert d <= tol, f"{label}: normalised log-weights deviate {d:.3g} from the reference, tolerance {tol:.3g}"


def _neff_close(case, got, label, rec):
    dec = C.reference(case)[1]
    d = C.neff_deviation(got, dec.neff)
    tol = C.D_ORACLE[C.key(case)]["neff"] + C.CONTRACT
    rec.update(neff=d, d_oracle_neff=C.D_ORACLE[C.key(case)]["neff"])
    print(f"{label}: nEff {got:.9g}, reference {dec.neff:.9g}: {d:.3g} (tolerance {tol:.3g})")
    assert d <= tol, f"{label}: nEff deviates {d:.3g} from the reference, tolerance {tol:.3g}"


def _parents_hold(got, w32, u, label, rec, tag):
    near, n, ref = C.hold_parents(got, w32, u, label)
    rec.update({f"{tag}_near": near, f"{tag}_strata": n, f"{tag}_beyond": int(ref.beyond.size)})
    print(f"{label}: {near} of {n} strata near, {ref.beyond.size} past the CDF's end")
    return ref


def _new_logw(n_out):
    return np.float32(-np.log(np.float64(n_out)))


# ------------------------------------------------------------------ standalone

def _standalone(case, n_out=None):
    """normalize(), neff(), resample(uniforms) and resample(device RNG) of one
    case: k_normalize + k_resample (resample_block), one workgroup; the CDF in
    LDS up to RS_LDS_MAX = 8192 entries, in global memory above."""
    _, config, n, dist = case
    n_out = n if n_out is None else n_out
    label = f"weighting {C.key(case)}" + (f" to {n_out}" if n_out != n else "")
    rec = dict(label=label, reference="weighting_ref", form="standalone", particles=n)
    c, poses, empty, offs0, z = C.scenario(config, n)
    f = _filter(C.config(case), n_out, max_particles=n, **C.CAPS)
    f.load(poses, C.weights(dist, n), empty, offs0)
    f.normalize()
    neff = f.neff()
    gw = f.export(with_maps=False)[1]
    if n_out == n:
        _weights_close(case, gw, label, rec)
        _neff_close(case, neff, label, rec)
    u = R.resample_uniforms(n_out, C.SEED, C.STEP)
    if dist == "tie":  # the CDF's total lowered by 2^-10 and the last stratum at its upper end: an overrun
        gw = (gw - np.float32(2.0 ** -10)).astype(np.float32)
        u_dev, u = u, u.copy()
        u[-1] = 1.0 - 2.0 ** -32
    f.load(poses, gw, empty, offs0)
    idx = f.resample(uniforms=u)
    ref = _parents_hold(idx, gw, u, label + " supplied uniforms", rec, "given")
    if dist == "tie":
        assert ref.beyond.size >= 1 and not ref.near[ref.beyond].any(), "the tie case's strata overrun the CDF"
        assert (idx[ref.beyond] == n // 3).all(), "an overrun takes the FIRST of the equal maxima"
    # the device RNG path draws the same uniforms
    f.load(poses, gw, empty, offs0)
    f.set_seed(C.SEED)
    idx2 = f.resample(uniforms=None, step=C.STEP)
    if dist == "tie":
        _parents_hold(idx2, gw, u_dev, label + " device uniforms", rec, "device")
        np.testing.assert_array_equal(idx2[:-1], idx[:-1])
    else:
        np.testing.assert_array_equal(idx2, idx)
    # copy_particles semantics: the parents' poses, every log-weight -log n_out
    assert f.n == n_out
    gp, gw2, _, go = f.export()
    f.close()
    assert gp.tobytes() == np.ascontiguousarray(poses[idx2]).tobytes()
    np.testing.assert_array_equal(gw2, _new_logw(n_out))
    assert go[-1] == 0
    _record_elementwise(rec)


@pytest.mark.parametrize("case", [("standalone", "phd", n, d) for n, d in C.STANDALONE],
                         ids=_ids([("standalone", "phd", n, d) for n, d in C.STANDALONE]))
def test_standalone(gpu, case):
    _standalone(case)


def test_standalone_live_particles_to_n_particles(gpu):
    """2500 live weights, 1000 strata (n_out < n after a predict that spawned children)."""
    _standalone(("standalone", "phd", C.LIVE[0], "normal"), n_out=C.LIVE[1])


# -------------------------------------------------------------------- phd_step

def _step_filter(case, resample, caps):
    _, config, n, dist = case
    c, poses, empty, offs0, z = C.scenario(config, n)
    f = _filter(C.config(case, resample), n, **caps)
    if config == "split":
        f.set_update_form(2)
    f.load(poses, C.weights(dist, n), empty, offs0)
    f.set_measurements(z)
    seed, step = C.seed_step(case)
    f.set_seed(seed)
    return f, poses, step


def _step(case, form, caps=C.CAPS):
    """phd_step of one case in the device form `form` (phd_last_resample_form)."""
    _, config, n, dist = case
    label = f"weighting {C.key(case)}"
    rec = dict(label=label, reference="weighting_ref", form=form, particles=n)
    # the normalised weights: update + normalize through the separate entry
    # points (k_normalize), first held to the reference
    g, poses, step = _step_filter(case, True, caps)
    if config == "cphd":
        g.set_step_births(0)
    g.update()
    g.normalize()
    gw_norm = g.export(with_maps=False)[1]
    g.check_errors()
    g.close()
    _weights_close(case, gw_norm, label, rec)
    # threshold 0: no resample; phd_step leaves exactly those bits in place
    h, _, _ = _step_filter(case, False, caps)
    neff0, resampled0 = h.step(do_predict=False, step=step)
    assert h.last_resample_form() == form
    hp, hw, _, _ = h.export()
    h.check_errors()
    h.close()
    assert not resampled0
    assert hw.tobytes() == gw_norm.tobytes(), "phd_step's normalised weights differ from normalize()'s"
    assert hp.tobytes() == np.ascontiguousarray(poses).tobytes()
    _neff_close(case, neff0, label + " (threshold 0)", rec)
    # with a resample: the decision, nEff, the parents (read back through px), the new weights
    f, _, _ = _step_filter(case, True, caps)
    assert f.last_resample_form() == "none"
    neff, resampled = f.step(do_predict=False, step=step)
    assert f.last_resample_form() == form
    gp, gw, _, _ = f.export()
    f.check_errors()
    f.close()
    dec = C.reference(case)[1]
    assert resampled == dec.resample and resampled
    _neff_close(case, neff, label, rec)
    parents = gp["px"].astype(np.int64)
    assert (parents == gp["px"]).all() and parents.min() >= 0 and parents.max() < n
    ref = _parents_hold(parents, gw_norm, R.resample_uniforms(n, *C.seed_step(case)), label, rec, "step")
    if dist == "tie":
        assert ref.beyond.size >= 1, "the committed (seed, step) overruns the CDF of the device's weights"
        assert (parents[ref.beyond[~ref.near[ref.beyond]]] == n // 3).all()
    assert gp.tobytes() == np.ascontiguousarray(poses[parents]).tobytes()
    assert np.unique(gw).size == 1
    np.testing.assert_allclose(gw, _new_logw(n), rtol=1e-6)
    _record_elementwise(rec)


def _phd(cases):
    return [("step", "phd", n, d) for n, d in cases]


@pytest.mark.parametrize("case", _phd(C.STEP_BLOCK), ids=_ids(_phd(C.STEP_BLOCK)))
def test_step_one_block(gpu, case):
    """n <= 2048: phd_step launches k_normalize_resample, one workgroup
    (norm_resample_regs<1> up to 1024 entries, <2> up to 2048)."""
    _step(case, "block")


@pytest.mark.parametrize("case", _phd(C.STEP_ONE_LAUNCH), ids=_ids(_phd(C.STEP_ONE_LAUNCH)))
def test_step_one_launch(gpu, case):
    """2049 <= n <= 16384 with the fused PHD update: launch_rs_chunks' fused
    branch, k_rs_step on the context's stream, one workgroup per 1024 entries;
    rs_search_block stages the whole CDF up to 4 chunks (n <= 4096) and each
    workgroup's own chunks above — or, when its strata's parents lie 4 or more
    chunks apart (`two_far`, `holes`), reads the CDF from global memory."""
    _step(case, "step")


@pytest.mark.parametrize("case", _phd(C.STEP_MULTI), ids=_ids(_phd(C.STEP_MULTI)))
def test_step_multi_launch(gpu, case):
    """n > 16384: launch_rs_chunks' other branch, k_rs_max / k_rs_sum / k_rs_cdf /
    k_rs_search."""
    _step(case, "chunks")


LEAD = [("step",) + c for c in C.STEP_LEAD]


@pytest.mark.parametrize("case", LEAD, ids=_ids(LEAD))
def test_step_lead_workgroup(gpu, case):
    """A CPHD step, or a split PHD step, above 2048 particles with the benched
    capacities: phd_step arms the overlapped resample and part C's lead
    workgroup runs it (rs_step_block)."""
    _step(case, "lead", C.CAPS_ROOMY)


@pytest.mark.parametrize("case", LEAD, ids=_ids(LEAD))
def test_step_second_stream(gpu, case):
    """The same steps with the small capacities: part C's LDS (a few KB) cannot
    hold rs_step_block's 8.4 KB of tables, so the armed resample is launched as
    k_rs_step on the second stream beside part C.  (Before the LDS check in
    phd_capi_update.hip the lead workgroup ran here all the same, read zeros past its
    allocation and left the log-weights unnormalised: entry 0 of
    `split-4097-two_far` -208.017 against normalize()'s -199.974.)"""
    _step(case, "beside")
