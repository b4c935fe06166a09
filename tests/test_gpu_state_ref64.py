"""The device's pose prediction, expected pose, cardinalities and static EAP map
against the float64 reference (tests/state_ref64.py), not against the oracle:
the shared cases of tests/state_ref64_cases.py through PHDFilter, compared per
class at

    tol(case, class) = D_oracle(case, class) + 1e-5

— the device is contracted to lie within 1e-5 of the oracle, and the oracle
lies D_oracle (measured on the CPU, committed in state_ref64_cases.D_ORACLE)
from the reference.  Cardinalities have no oracle routine: a double sum
rounded once, held to 2^-23.  No case leaves anything out (the EAP cases have
no near decision, by the reference's own count).  The oracle is not called
here.  Every comparison's worst figures go to the parity record under labels
"state ref64 ...".
"""
import numpy as np
import pytest

import state_ref64 as R
import state_ref64_cases as C
from test_gpu_parity import _filter, _record_elementwise

pytestmark = pytest.mark.gpu


def _check(label, name, worst, classes, **info):
    table = C.D_ORACLE[name]
    print(f"{label}: " + ", ".join(f"{k} {worst[k]:.3g} (D_oracle {table[k]:.2g})" for k in classes))
    _record_elementwise(dict(label=label, reference="state_ref64", **info,
                             **{f"ref64_{k}": worst[k] for k in classes},
                             **{f"d_oracle_{k}": table[k] for k in classes}))
    for k in classes:
        tol = table[k] + C.CONTRACT
        assert worst[k] <= tol, f"{label}: {k} deviates {worst[k]:.3g} from the reference, tolerance {tol:.3g}"


def _predicted(c, noise, offset=None):
    """The case through a fresh filter: (poses, log-weights, maps, offsets, live particles)."""
    n = len(c.poses)
    f = _filter(c.cfg.copy(), n, max_particles=n * c.npp)
    f.load(c.poses, c.lw, c.maps, c.offs)
    if offset is not None:
        f.set_seed(c.seed)
        f.set_index_offset(offset)
    if c.fused:
        f.set_measurements(c.z)
        f.step(control=c.control if c.model == "ack" else None, do_predict=True, step=c.step)
    elif c.model == "ack":
        f.predict_ackerman(c.control[0], c.control[1], noise=noise, step=c.step)
    else:
        f.predict_cv(noise=noise, step=c.step)
    live = f.n
    out = f.export()
    f.close()
    return out + (live,)


@pytest.mark.parametrize("name", C.PREDICT_CASES)
def test_predict_matches_reference(gpu, name):
    """Host noise, then the device's own draws at index offsets 0 and 4096 (the
    reference draws at id + offset); n_predict_particles through the expansion,
    the fused case through step()."""
    c, r = C.predict_inputs(name), C.predict_reference(name)
    m = len(c.poses) * c.npp
    runs = [] if c.fused else [("host noise", r.host, _predicted(c, c.host))]
    runs += [(f"device draws at offset {off}", r.rng[off], _predicted(c, None, off)) for off in c.offsets]
    assert runs
    for what, ref, (gp, gw, gm, go, live) in runs:
        assert live == m and len(gp) == m
        assert np.all(np.abs(gp["ptheta"]) <= C.PI32), what
        _check(f"state ref64 predict {name} {what}", name, C.pose_deviations(ref, gp), C.POSE_CLASSES, particles=m)
        if c.fused:
            continue
        # the children in their parents' order, each with the parent's map and the weight w - log npp
        assert np.all(np.abs(gw - r.lw) <= 3 * R.EPS32 * np.maximum(np.abs(r.lw), 1.0)), what
        sizes = np.diff(c.offs)[r.parent]
        assert np.array_equal(np.diff(go), sizes)
        want = np.concatenate([c.maps[c.offs[p]:c.offs[p + 1]] for p in r.parent]) if m else c.maps[:0]
        assert gm.tobytes() == want.tobytes()
    if len(c.offsets) > 1:  # the offset moves the poses: it cannot be ignored
        a, b = runs[-2][2][0], runs[-1][2][0]
        assert not np.array_equal(a["px"], b["px"]) and not np.array_equal(a["ptheta"], b["ptheta"])


@pytest.mark.parametrize("name", C.EP_CASES)
def test_expected_pose_matches_reference(gpu, name):
    import phdslam
    from phdslam.types import GAUSSIAN2D
    poses, lw, ties = C.ep_inputs(name)
    ref, mi = C.ep_reference(name)
    n = len(lw)
    cfg = phdslam.config_scenario(2, n=1, G=1, M=1)[0]
    maps = np.zeros(n, GAUSSIAN2D)
    maps["weight"] = 0.5
    maps["cov"] = (1, 0, 0, 1)
    f = _filter(cfg, n)
    f.load(poses, lw, maps, np.arange(n + 1, dtype=np.int32))
    got, gmi = f.expected_pose()
    f.close()
    assert gmi == mi == ties[0]  # the first of the equal maxima: no arithmetic, no tolerance
    _check(f"state ref64 expected pose {name}", name, C.pose_deviations(ref, got, scale=1e-3), C.EP_CLASSES, particles=n)


def _card_check(what, f):
    cn = f.cardinalities()
    gm, go = f.export()[2:]
    ref = R.cardinalities(gm, go)
    assert cn.dtype == np.float32 and len(cn) == len(ref)
    assert np.all(cn[ref == 0] == 0), what  # an empty slab: exactly 0
    worst = float(np.max(np.abs(cn - ref) / np.maximum(ref, 1e-300), initial=0.0, where=ref > 0))
    print(f"state ref64 cardinalities {what}: {worst:.3g}")
    _record_elementwise(dict(label=f"state ref64 cardinalities {what}", reference="state_ref64", particles=len(cn),
                             ref64_card=worst))
    assert worst <= C.CARD_RTOL, what
    return gm, go


def test_cardinalities_match_reference(gpu):
    """Right after load, after an update (the other slab set) and after a
    resample (slab references other than the identity); the last two against the
    exported maps."""
    cfg, poses, lw, maps, offs, z = C.card_inputs()
    n = len(poses)
    f = _filter(cfg.copy(), n, map_capacity=C.CARD_CAP, max_measurements=16)
    f.load(poses, lw, maps, offs)
    gm, go = _card_check("after load", f)
    assert gm.tobytes() == maps.tobytes() and np.array_equal(go, offs)
    assert sorted(set(np.diff(go))) == sorted(C.CARD_SIZES)
    f.update(z)
    f.check_errors()
    gm2, _ = _card_check("after update", f)
    assert gm2.tobytes() != gm.tobytes()
    f.normalize()
    idx = f.resample(step=3)
    assert not np.array_equal(idx, np.arange(n))
    _card_check("after resample", f)
    f.close()


@pytest.mark.parametrize("name", C.EAP_CASES)
def test_expected_map_matches_reference(gpu, name):
    c = C.eap_inputs(name)
    ref, near, _ = C.eap_reference(name)
    assert near == 0
    n = len(c.lw)
    f = _filter(c.cfg.copy(), n, map_capacity=c.cap, max_measurements=16, candidate_capacity=256, survivor_capacity=128)
    if name == "duplicates":  # the state after a resample: children share their parent's slab
        b = c.extra
        f.load(c.poses, b["lw"], b["maps"], b["offs"])
        idx = f.resample(uniforms=b["u"])
        assert np.array_equal(idx, b["parents"])
        _, gw, gm, go = f.export()
        assert gm.tobytes() == c.maps.tobytes() and np.array_equal(go, c.offs) and np.array_equal(gw, c.lw)
    else:
        f.load(c.poses, c.lw, c.maps, c.offs)
    eap = f.expected_map()
    rounds = f.expected_map_groups()
    f.close()
    worst = C.field_deviations(ref, eap)
    assert worst is not None, (f"{name}: {len(eap)} components, the reference has {len(ref)}"
                               " (or a NaN where the reference has a number)")
    _check(f"state ref64 eap {name}", name, worst, C.FIELD_CLASSES, components=len(ref), rounds=rounds)
    if name == "chains":
        assert rounds > 3, rounds
    if name == "fallback":
        assert rounds == 1, rounds  # the one-workgroup greedy
