"""The estimate trace of the mixed static + dynamic feature model
(phd_trace_enable_mixed / phd_trace_read_dynamic / phd_trace_shape_dynamic).

CPU: the dyn record's layout and the exported symbols.  GPU: every record of a
free-running phd_step chain on a feature_model 2 context — the static half as
tests/test_trace.py holds it, the dynamic half (phd_trace_dyn_record and the
Gaussian4D snapshot) against the synchronous exports of a twin context with
the same seed, which runs the same scans through phd_predict_update ->
phd_normalize -> (estimates, exports) -> phd_resample with the same step
number.  Tiny shapes (mixed_config / mixed_scenario as tests/test_gpu_mixed.py).
"""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW_SYMBOLS = ("phd_trace_enable_mixed", "phd_trace_read_dynamic", "phd_trace_shape_dynamic")


# ------------------------------------------------------------------ CPU

def test_dyn_record_layout_and_symbols(built):
    from phdslam import types as T
    from phdslam._lib import SIGNATURES
    assert ctypes.sizeof(T.TraceDynRecord) == T.TRACE_DYN_RECORD.itemsize == 32
    assert T.TraceDynRecord.map_size.offset == 8 == T.TRACE_DYN_RECORD.fields["map_size"][1]
    assert T.TraceDynRecord.card_map.offset == 4 and T.TraceDynRecord.reserved.offset == 12
    txt = open(os.path.join(REPO, "include", "phd_types.h")).read()
    body = re.search(r"typedef struct phd_trace_dyn_record \{(.*?)\} phd_trace_dyn_record;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"\b(\w+)(?:\[\d+\])?\s*;", body) == [f for f, _ in T.TraceDynRecord._fields_]
    assert int(re.search(r"sizeof\(phd_trace_dyn_record\) == (\d+)", txt).group(1)) == 32
    assert ctypes.sizeof(T.TraceRecord) == 96  # the static record is unchanged
    so = os.path.join(REPO, "cuda-phdslam_amd", "phdslam", "libphdslam.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    names = set(line.split()[-1] for line in out.splitlines() if line.strip())
    for sym in NEW_SYMBOLS:
        assert sym in names, sym
    assert set(NEW_SYMBOLS) <= set(SIGNATURES)


# ------------------------------------------------------------------ GPU

def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _config(thresh=1.0):
    from phdslam.scenario import mixed_config
    c = mixed_config()
    c.motionType = 0  # CV
    c.resampleThresh = thresh
    return c


def _filter(cfg, n, cap=128, dcap=64, M=32, K=4096):
    import phdslam
    f = phdslam.PHDFilter(n, cfg, map_capacity=cap, max_measurements=M, candidate_capacity=K, survivor_capacity=256)
    f.set_seed(77)
    f.enable_dynamic(dcap)
    f.set_check_each_update(False)
    return f


def _load(f, state, lw=None):
    poses, sm, sof, dm, dof = state
    n = len(poses)
    f.load(poses, np.full(n, -np.log(n), np.float32) if lw is None else lw, sm, sof)
    f.load_dynamic(dm, dof)


def _twin_scan(t, c, zk, k, do_predict):
    """One scan through the synchronous entry points (tests/test_trace.py's twin)."""
    t.set_measurements(zk)
    t.predict_update(None, k, do_predict=do_predict)
    t.normalize()
    pose, mi = t.expected_pose()
    s = dict(pose=pose.copy(), mi=mi, neff=t.neff(), cn=t.cardinalities(), M=len(zk))
    s["poses"], s["w"], s["maps"], s["offs"] = t.export()
    s["dmaps"], s["doffs"] = t.export_dynamic()
    s["resampled"] = bool(len(zk) > 0 and s["neff"] <= c.resampleThresh)
    s["parents"] = t.resample(step=k) if s["resampled"] else None
    return s


def _dyn_of(s, p):
    return s["dmaps"][s["doffs"][p]:s["doffs"][p + 1]]


def _dyn_sums64(s):
    """Σ_j w_nj of every particle's exported dynamic map, in float64."""
    return np.array([_dyn_of(s, p)["weight"].astype(np.float64).sum() for p in range(len(s["w"]))])


def _ulp(x):
    return float(np.spacing(np.abs(np.float32(x))))


def _check_dynamic(k, r, d, snap, s, dsnap, twin_rule=False):
    """The dynamic half of scan k (dyn record d, snapshot entry snap) against the
    twin's exports s; r is the scan's static record (map_particle)."""
    mi = s["mi"]
    assert r["map_particle"] == mi, k
    want = _dyn_of(s, mi)
    assert d["map_size"] == len(want), (k, d["map_size"], len(want))
    assert not d["reserved"].any(), k
    if dsnap:
        rows = min(len(want), dsnap)
        for fld in ("weight", "mean", "cov"):
            assert _bits(snap[:rows][fld]) == _bits(want[:rows][fld]), (k, fld)
        assert not np.any(snap[rows:].view(np.uint8)), "rows past map_size are zero"
    # a double sum of at most dyn_capacity floats is exact far below a float ulp:
    # only the final rounding to float can differ
    cm = np.float32(want["weight"].astype(np.float64).sum())
    gap = abs(float(d["card_map"]) - float(cm))
    print(f"scan {k}: dyn card_map gap {gap:.3g} (1 ulp {_ulp(cm):.3g})")
    assert gap <= _ulp(cm), (k, d["card_map"], cm)
    # card_expected against the float64 value Σ_n exp(w_n) Σ_j w_nj of the twin's store
    w64 = s["w"].astype(np.float64)
    sums = _dyn_sums64(s)
    ce64 = float(np.sum(np.exp(w64) * sums))
    gap = abs(float(d["card_expected"]) - ce64)
    if twin_rule:
        # the tolerance of the static field in tests/test_trace.py: twice the
        # distance between the float statement of the sum (Σ_n exp(w_n) cn_n in
        # particle order, all float) and its float64 value
        ce32 = float(np.cumsum(np.exp(s["w"]).astype(np.float32) * sums.astype(np.float32), dtype=np.float32)[-1])
        tol = 2.0 * abs(ce32 - ce64)
    else:
        # what the device's form allows at any shape: every term exp(w_n) cn_n is
        # >= 0 and carries the relative error of a float exp (at most 1 ulp, 2^-23),
        # cn_n is exact to a float rounding the twin's sum shares, the double sum
        # adds nothing visible, and the result is rounded to float once (2^-24)
        tol = (2.0 ** -23 + 2.0 ** -24) * ce64
    print(f"scan {k}: dyn card_expected {float(d['card_expected'])!r} gap to fp64 {gap:.3g} "
          f"= {gap / max(_ulp(ce64), 1e-300):.2f} ulp (tolerance {tol:.3g})")
    assert gap <= tol, (k, d["card_expected"], ce64)


def _check_static(k, r, s, n, sums=True):
    """tests/test_trace.py::test_records_equal_twin's comparisons of one record
    (sums=False: the fields it holds bit for bit only)."""
    w64 = s["w"].astype(np.float64)
    mi = s["mi"]
    assert int(r["step"]) == k and r["n_live"] == n and r["n_measure"] == s["M"]
    assert bool(r["resampled"]) == s["resampled"], k
    assert r["map_particle"] == mi, k
    assert _bits(r["expected_pose"]) == _bits(s["pose"]), k
    assert _bits(r["map_pose"]) == _bits(s["poses"][mi]), k
    assert r["map_size"] == s["offs"][mi + 1] - s["offs"][mi], k
    if not sums:
        return
    neff64 = 1.0 / np.sum(np.exp(2.0 * w64)) / n
    tol = 2.0 * abs(float(s["neff"]) - neff64)
    gap = abs(float(r["neff"]) - float(s["neff"]))
    print(f"scan {k}: nEff gap {gap:.3g} (tolerance {tol:.3g})")
    assert gap <= tol, (k, r["neff"], s["neff"])
    cmap64 = float(np.sum(s["maps"][s["offs"][mi]:s["offs"][mi + 1]]["weight"].astype(np.float64)))
    tol = 2.0 * abs(float(s["cn"][mi]) - cmap64)
    gap = abs(float(r["card_map"]) - float(s["cn"][mi]))
    print(f"scan {k}: card_map gap {gap:.3g} (tolerance {tol:.3g})")
    assert gap <= tol, (k, r["card_map"], s["cn"][mi])
    ce32 = float(np.cumsum(np.exp(s["w"]).astype(np.float32) * s["cn"], dtype=np.float32)[-1])
    cn64 = np.add.reduceat(s["maps"]["weight"].astype(np.float64), s["offs"][:-1].astype(np.int64)) \
        if len(s["maps"]) else np.zeros(n)
    cn64 = np.where(np.diff(s["offs"]) > 0, cn64, 0.0)
    ce64 = float(np.sum(np.exp(w64) * cn64))
    tol = 2.0 * abs(ce32 - ce64)
    gap = abs(float(r["card_expected"]) - ce32)
    print(f"scan {k}: card_expected gap {gap:.3g} (tolerance {tol:.3g}); distance to fp64 "
          f"{abs(float(r['card_expected']) - ce64):.3g}")
    assert gap <= tol, (k, r["card_expected"], ce32, ce64)


# two groups of the cardinality stage, the second partly filled; the scenario
# as tests/test_gpu_mixed.py generates it (its default pose spread)
TWIN_N, TWIN_JITTER = 40, 0.3


@functools.lru_cache(maxsize=None)
def _twin_case(n=TWIN_N, jitter=TWIN_JITTER):
    """Five scans (measurements, measurements, none, measurements, measurements)
    at resample threshold 1: nEff <= 1 resamples on every scan with measurements,
    the empty scan never does.  Computed once and shared, never modified."""
    from phdslam.scenario import mixed_scenario
    from phdslam.types import MEASUREMENT
    c = _config(1.0)
    poses, sm, sof, dm, dof, z = mixed_scenario(c, n, 12, 6, 10, seed=31, pose_jitter=jitter)
    state = (poses, sm, sof, dm, dof)
    sets = [z, z, np.zeros(0, MEASUREMENT), z, z]
    t = _filter(c, n)
    _load(t, state)
    scans = [_twin_scan(t, c, zk, k, k > 0) for k, zk in enumerate(sets)]
    final = t.export() + t.export_dynamic()
    t.close()
    return c, state, sets, scans, final


def _run_steps(f, sets, first=0):
    for k, zk in enumerate(sets, start=first):
        f.set_measurements(zk)
        assert f.step(None, do_predict=k > 0, step=k, readback=False) is None


@pytest.mark.gpu
def test_twin_run(gpu):
    """Traced chain A = untraced chain B bit for bit; every record of A equals the
    synchronous outputs of chain C (static half: tests/test_trace.py's
    comparisons; dynamic half: _check_dynamic).
    Measured on the MI355X (this case, scans 0..4), distance to the float64 value
    in float ulps of the result: dynamic card_expected 0.10 0.35 0.70 0.44 0.42
    (the float statement whose doubled distance is the tolerance: 0.90 0.35 1.30
    0.44 0.58), static card_expected 0.25 0.10 0.00 0.50 0.04."""
    c, state, sets, scans, final = _twin_case()
    dsnap = 16
    finals = []
    for traced in (True, False):
        f = _filter(c, TWIN_N)
        _load(f, state)
        if traced:
            f.enable_trace_mixed(len(sets), 8, dsnap)
        _run_steps(f, sets)
        if traced:
            assert f.trace_count() == len(sets)
            rec, smaps, _ = f.read_trace()
            drec, dmaps = f.read_trace_dynamic()
        finals.append(f.export() + f.export_dynamic())
        f.close()
    for a, b in zip(finals[0], finals[1]):
        assert _bits(a) == _bits(b), "the trace perturbed the chain"
    # (and the step chain is the synchronous chain, as tests/test_trace.py holds it)
    assert _bits(finals[0][0]) == _bits(final[0]) and _bits(finals[0][1]) == _bits(final[1])
    np.testing.assert_array_equal(finals[0][3], final[3])
    np.testing.assert_array_equal(finals[0][5], final[5])
    decisions = [s["resampled"] for s in scans]
    print("twin nEff", [round(float(s["neff"]), 4) for s in scans], "resampled", decisions)
    assert sum(decisions) >= 2 and not all(decisions)
    assert dmaps.shape == (len(sets), dsnap)
    for k, s in enumerate(scans):
        _check_static(k, rec[k], s, TWIN_N)
        mi = s["mi"]
        want = s["maps"][s["offs"][mi]:s["offs"][mi + 1]]
        rows = min(len(want), 8)
        assert _bits(smaps[k][:rows]) == _bits(want[:rows]) and not np.any(smaps[k][rows:].view(np.uint8)), k
        _check_dynamic(k, rec[k], drec[k], dmaps[k], s, dsnap, twin_rule=True)
    assert all(d["map_size"] > 0 for d in drec)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 33, 1025])
def test_particle_count_edges(gpu, n):
    """One particle, one past the 32-particle group of the cardinality stage, one
    past the 1024-entry weight chunk (maps of at most 4 components): 2 scans."""
    from phdslam.scenario import mixed_scenario
    c = _config(1.0)
    poses, sm, sof, dm, dof, z = mixed_scenario(c, n, 4, 3, 4, seed=7 + n)
    state = (poses, sm, sof, dm, dof)
    lw = np.random.default_rng(n).normal(-8, 2, n).astype(np.float32)
    kw = dict(cap=32, dcap=32, M=8, K=256)
    t = _filter(c, n, **kw)
    _load(t, state, lw)
    scans = [_twin_scan(t, c, z, k, k > 0) for k in range(2)]
    t.close()
    f = _filter(c, n, **kw)
    _load(f, state, lw)
    f.enable_trace_mixed(2, 0, 8)
    _run_steps(f, [z, z])
    rec = f.read_trace()
    drec, dmaps = f.read_trace_dynamic()
    f.close()
    for k, s in enumerate(scans):
        _check_static(k, rec[k], s, n, sums=False)
        _check_dynamic(k, rec[k], drec[k], dmaps[k], s, 8)


@pytest.mark.gpu
@pytest.mark.parametrize("size", [0, 64, 65, 192])
def test_dynamic_map_size_edges(gpu, size):
    """dyn_capacity 192; the arg-max particle's dynamic map holds 0, 64, 65 (one
    strip of the transpose and one component) or 192 components; snapshot
    capacities of 1, below, equal to and above the size.  No predict and an empty
    scan: the loaded map is the recorded one, on both scans."""
    from phdslam.scenario import mixed_scenario
    from phdslam.types import MEASUREMENT
    c = _config(1.0)
    n, sizes = 4, [0, 64, 65, 192]
    poses, sm, sof, dm, _, _ = mixed_scenario(c, n, 3, 192, 4, seed=19)
    dm = np.concatenate([dm[p * 192:p * 192 + sizes[p]] for p in range(n)])
    dof = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    best = sizes.index(size)
    lw = np.full(n, -9.0, np.float32)
    lw[best] = -0.5
    none = np.zeros(0, MEASUREMENT)
    kw = dict(cap=32, dcap=192, M=8, K=256)
    t = _filter(c, n, **kw)
    _load(t, (poses, sm, sof, dm, dof), lw)
    t.normalize()
    s = dict(mi=t.expected_pose()[1], w=t.export(with_maps=False)[1])
    s["dmaps"], s["doffs"] = t.export_dynamic()
    t.close()
    assert s["mi"] == best
    f = _filter(c, n, **kw)
    _load(f, (poses, sm, sof, dm, dof), lw)
    want = dm[dof[best]:dof[best + 1]]
    for dsnap in sorted({1, max(size - 1, 1), max(size, 1), size + 3}):
        f.enable_trace_mixed(2, 0, dsnap)
        for k in range(2):
            f.set_measurements(none)
            f.step(None, do_predict=False, step=k, readback=False)
        rec = f.read_trace()
        drec, dmaps = f.read_trace_dynamic()
        assert dmaps.shape == (2, dsnap)
        for k in range(2):
            assert rec[k]["n_measure"] == 0 and rec[k]["resampled"] == 0
            assert drec[k]["map_size"] == size == len(want)
            _check_dynamic(k, rec[k], drec[k], dmaps[k], s, dsnap)
    gd, gdo = f.export_dynamic()
    f.close()
    assert _bits(gd) == _bits(dm) and np.array_equal(gdo, dof)  # (the store is as loaded)


@pytest.mark.gpu
def test_shared_slabs(gpu):
    """After a resample that draws every child from one parent, a later child is
    made the arg-max (phd_set_log_weights): its dynamic map is read through the
    slab reference it shares — on an empty scan (predict only: the references
    stay shared) and after the next scan's update."""
    import torch
    from phdslam.scenario import mixed_scenario
    from phdslam.types import MEASUREMENT
    c = _config(1.0)
    n, parent, child = 8, 2, 5
    poses, sm, sof, dm, dof, z = mixed_scenario(c, n, 10, 6, 8, seed=23)
    lw0 = np.full(n, -400.0, np.float32)
    lw0[parent] = 0.0
    lw1 = np.full(n, -300.0, np.float32)
    lw1[child] = 0.0
    dev_lw1 = torch.tensor(lw1, device="cuda")
    torch.cuda.synchronize()
    sets = [z, np.zeros(0, MEASUREMENT), z]
    t = _filter(c, n)
    _load(t, (poses, sm, sof, dm, dof), lw0)
    scans = []
    for k, zk in enumerate(sets):
        if k > 0:
            t.set_log_weights_from(dev_lw1.data_ptr())
        scans.append(_twin_scan(t, c, zk, k, k > 0))
    t.close()
    parents = scans[0]["parents"]
    assert (parents == parent).sum() >= 3 and parents[child] == parent != child
    f = _filter(c, n)
    _load(f, (poses, sm, sof, dm, dof), lw0)
    f.enable_trace_mixed(3, 0, 64)
    for k, zk in enumerate(sets):
        if k > 0:
            f.set_log_weights_from(dev_lw1.data_ptr())
        f.set_measurements(zk)
        f.step(None, do_predict=k > 0, step=k, readback=False)
    rec = f.read_trace()
    drec, dmaps = f.read_trace_dynamic()
    f.close()
    for k, s in enumerate(scans):
        _check_dynamic(k, rec[k], drec[k], dmaps[k], s, 64)
    assert rec[1]["map_particle"] == child and rec[2]["map_particle"] == child
    assert drec[1]["map_size"] > 0 and drec[2]["map_size"] > 0
    # the empty scan recorded the shared slab after its predict, not the slab of the child's own index
    assert _bits(dmaps[1][:drec[1]["map_size"]]) == _bits(_dyn_of(scans[1], parent))


@pytest.mark.gpu
def test_empty_scan_records_predicted_store(gpu):
    """M = 0 with the predict on: a record is appended from the predicted dynamic
    maps (every weight times p_jmm ps: the cardinality differs from the scan before)."""
    c, state, sets, scans, _ = _twin_case()
    f = _filter(c, TWIN_N)
    _load(f, state)
    f.enable_trace_mixed(4, 0, 16)
    _run_steps(f, sets[:3])
    assert f.trace_count() == 3
    rec = f.read_trace()
    drec, dmaps = f.read_trace_dynamic()
    f.close()
    assert rec[2]["n_measure"] == 0 and rec[2]["resampled"] == 0 and rec[1]["n_measure"] == len(sets[1])
    _check_dynamic(2, rec[2], drec[2], dmaps[2], scans[2], 16)
    # the arg-max particle's map of the scan before (its parent's posterior), predicted once
    s1, s2 = scans[1], scans[2]
    before = _dyn_of(s1, s1["parents"][s2["mi"]])
    after = _dyn_of(s2, s2["mi"])
    assert len(before) == len(after) == drec[2]["map_size"] > 0
    assert (after["weight"] < before["weight"]).all()
    assert drec[2]["card_map"] < np.float32(before["weight"].astype(np.float64).sum())


@pytest.mark.gpu
def test_ring_wraps(gpu):
    import phdslam
    c, state, sets, scans, _ = _twin_case()
    f = _filter(c, TWIN_N)
    _load(f, state)
    f.enable_trace_mixed(8, 0, 4)
    _run_steps(f, sets)
    want_s, (want_d, want_m) = f.read_trace(0, 5), f.read_trace_dynamic(0, 5)
    f.close()
    f = _filter(c, TWIN_N)
    _load(f, state)
    f.enable_trace_mixed(3, 0, 4)
    with pytest.raises(phdslam.PHDError) as e:  # nothing written yet
        f.read_trace_dynamic(0, 1)
    assert e.value.code == phdslam._lib.PHD_E_ARG
    _run_steps(f, sets)
    assert f.trace_count() == 5
    got_d, got_m = f.read_trace_dynamic(2, 3)
    assert _bits(got_d) == _bits(want_d[2:5]) and _bits(got_m) == _bits(want_m[2:5])
    with pytest.raises(phdslam.PHDError) as e:  # scans 0 and 1 are overwritten
        f.read_trace_dynamic(0, 1)
    assert e.value.code == phdslam._lib.PHD_E_ARG and "overwritten" in str(e.value)
    with pytest.raises(phdslam.PHDError) as e:  # scan 5 is not written yet
        f.read_trace_dynamic(3, 3)
    assert e.value.code == phdslam._lib.PHD_E_ARG
    # both rings hold the same scans: defaults read what is left, and the static ring refuses the same range
    got_s = f.read_trace()
    assert [int(r["step"]) for r in got_s] == [2, 3, 4] and _bits(got_s) == _bits(want_s[2:5])
    assert _bits(f.read_trace_dynamic()[0]) == _bits(want_d[2:5])
    with pytest.raises(phdslam.PHDError):
        f.read_trace(0, 1)
    assert f.read_trace_dynamic(4, 1)[0][0]["map_size"] == len(_dyn_of(scans[4], scans[4]["mi"]))
    # dmaps may be NULL
    from phdslam.types import TRACE_DYN_RECORD
    one = np.zeros(1, TRACE_DYN_RECORD)
    phdslam._lib.check(phdslam._lib.lib().phd_trace_read_dynamic(f.handle, 4, 1, ctypes.c_void_p(one.ctypes.data), None),
                       "phd_trace_read_dynamic")
    assert _bits(one) == _bits(want_d[4:5])
    f.close()


def _refused(code, text, call, *a, **kw):
    import phdslam
    with pytest.raises(phdslam.PHDError) as e:
        call(*a, **kw)
    assert e.value.code == code, str(e.value)
    assert text in str(e.value), str(e.value)


@pytest.mark.gpu
def test_refusals(gpu):
    import phdslam
    import torch
    from phdslam._lib import PHD_E_ARG, PHD_E_UNSUPPORTED
    from phdslam.scenario import mixed_scenario
    from phdslam.types import TRACE_CARD_DIST
    L = phdslam._lib.lib()
    c = _config(1.0)
    n = 4
    poses, sm, sof, dm, dof, z = mixed_scenario(c, n, 6, 4, 5, seed=2)
    kw = dict(map_capacity=128, max_measurements=32, candidate_capacity=4096, survivor_capacity=256)
    # phd_trace_enable on a mixed context: refused as before
    f = _filter(c, n)
    _refused(PHD_E_UNSUPPORTED, "static feature model only", f.enable_trace, 4)
    assert f.trace_count() == 0
    # PHD_TRACE_CARD_DIST: the mixed model has no CPHD
    with pytest.raises(phdslam.PHDError) as e:
        phdslam._lib.check(L.phd_trace_enable_mixed(f.handle, 4, 0, 0, TRACE_CARD_DIST), "phd_trace_enable_mixed")
    assert e.value.code == PHD_E_UNSUPPORTED and "CPHD" in str(e.value)
    # the sharded trace entry points on a mixed trace
    f.enable_trace_mixed(4, 0, 4)
    buf = torch.zeros(4096, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    _refused(PHD_E_UNSUPPORTED, "feature_model 2", f.trace_shard_pack, buf.data_ptr(), 1, 0, 0, buf.data_ptr())
    _refused(PHD_E_UNSUPPORTED, "feature_model 2", f.trace_shard_append, buf.data_ptr(), buf.data_ptr(), 1, 0)
    # a traced step re-checks: another dynamic capacity, another feature model
    _load(f, (poses, sm, sof, dm, dof))
    f.set_measurements(z)
    f.step(None, do_predict=False, step=0, readback=False)
    assert f.trace_count() == 1
    f.enable_dynamic(96)
    _refused(PHD_E_UNSUPPORTED, "enable the trace again", f.step, None, do_predict=False, step=1, readback=False)
    assert f.trace_count() == 1
    f.enable_dynamic(64)
    c0 = c.copy()
    c0.featureModel = 0
    f.set_config(c0)
    _refused(PHD_E_UNSUPPORTED, "enable the trace again", f.step, None, do_predict=False, step=1, readback=False)
    assert f.trace_count() == 1
    # capacity 0 through either entry point frees both rings
    f.set_config(c)
    f.enable_trace_mixed(2, 2, 2)
    f.enable_trace(0)
    assert f.trace_shape() == (0, 0, 0) and f.trace_count() == 0
    _refused(PHD_E_ARG, "is off", f.read_trace_dynamic, 0, 0)
    f.enable_trace_mixed(2, 2, 2)
    f.enable_trace_mixed(0)
    assert f.trace_shape() == (0, 0, 0)
    f.close()
    # no phd_enable_dynamic
    f = phdslam.PHDFilter(n, c, **kw)
    _refused(PHD_E_ARG, "phd_enable_dynamic", f.enable_trace_mixed, 4)
    f.close()
    # no phd_set_config
    f = phdslam.PHDFilter(n, None, **kw)
    _refused(PHD_E_ARG, "phd_set_config", f.enable_trace_mixed, 4)
    f.close()
    # feature_model other than 2
    c0 = phdslam.config_scenario(2, n=1, G=2, M=4)[0]
    f = phdslam.PHDFilter(n, c0, **kw)
    _refused(PHD_E_UNSUPPORTED, "feature_model 2", f.enable_trace_mixed, 4)
    f.close()
    # n_predict_particles > 1
    c2 = _config(1.0)
    c2.nPredictParticles = 2
    f = phdslam.PHDFilter(n, c2, max_particles=64, **kw)
    f.enable_dynamic(64)
    _refused(PHD_E_UNSUPPORTED, "n_predict_particles", f.enable_trace_mixed, 4)
    assert f.trace_count() == 0
    f.close()


@pytest.mark.gpu
def test_static_trace_unchanged(gpu):
    """A feature_model 0 context with the existing trace: the call sequence of
    tests/test_trace.py::test_reductions_equal_synchronous_calls at its smallest
    case (n = 1), the same equalities, and the map fields against phd_cardinalities."""
    import phdslam
    n = 1
    c, poses, lw, maps, offs, z = phdslam.config_scenario(2, n=n, G=2, M=4)
    c.resampleThresh = 0.5
    lw = np.random.default_rng(n).normal(-8, 3, n).astype(np.float32)
    run = []
    for _ in range(2):
        f = phdslam.PHDFilter(n, c, map_capacity=8, max_measurements=8, candidate_capacity=128, survivor_capacity=64)
        f.set_seed(4242)
        f.set_check_each_update(False)
        f.load(poses, lw, maps, offs)
        f.set_measurements(z)
        run.append(f)
    t, f = run
    t.predict_update((2.0, 0.05), 0, do_predict=False)
    t.normalize()
    neff = np.float32(t.neff())
    pose, mi = t.expected_pose()
    cn = t.cardinalities()
    tp, wn, tm, to = t.export()
    f.enable_trace(1, 4)
    assert f.step((2.0, 0.05), do_predict=False, step=0, readback=False) is None
    rec, snap, card = f.read_trace()
    r = rec[0]
    with pytest.raises(phdslam.PHDError):  # no dyn ring beside a static trace
        f.read_trace_dynamic(0, 1)
    t.close()
    f.close()
    assert card is None
    assert _bits(np.float32(r["neff"])) == _bits(neff)
    assert bool(r["resampled"]) == bool(neff <= c.resampleThresh)
    assert r["map_particle"] == mi == 0
    assert _bits(r["expected_pose"]) == _bits(pose)
    assert _bits(r["map_pose"]) == _bits(tp[mi])
    assert r["map_size"] == to[1]
    cmap64 = float(np.sum(tm["weight"].astype(np.float64)))
    assert abs(float(r["card_map"]) - float(cn[0])) <= 2.0 * abs(float(cn[0]) - cmap64)
    rows = min(int(to[1]), 4)
    assert _bits(snap[0][:rows]) == _bits(tm[:rows])
