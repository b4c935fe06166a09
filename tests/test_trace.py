"""The per-scan estimate trace (phd_trace_enable / phd_trace_count / phd_trace_read).

CPU: the record's layout (ctypes against include/phd_types.h) and the exported
symbols.  GPU: every record of a free-running phd_step chain equals what the
library's synchronous entry points return on a twin context with the same
seed, which runs the same scans through phd_predict_update -> phd_normalize ->
(estimates, exports) -> phd_resample.  Small synthetic scenarios (G = 8 prior
components, M = 4 measurements, map capacity 64).
"""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

G, M, CAP, SCANS = 8, 4, 64, 6
# resample thresholds (nEff is 1 / Σ exp(2w) / N in (0, 1]): between the nEff the
# twin shows one scan after a resample (PHD ~0.6, CPHD ~0.92) and two scans after
# (PHD ~0.25, CPHD ~0.85), so a chain of six scans both resamples and does not
# (asserted from the twin in every case)
THRESH = {2: 0.5, 3: 0.9}


# ------------------------------------------------------------------ CPU

def _header_record():
    txt = open(os.path.join(REPO, "include", "phd_types.h")).read()
    body = re.search(r"typedef struct phd_trace_record \{(.*?)\} phd_trace_record;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"\b(\w+)\s*;", body)
    size = int(re.search(r"sizeof\(phd_trace_record\) == (\d+)", txt).group(1))
    offs = {m.group(1): int(m.group(2))
            for m in re.finditer(r"offsetof\(phd_trace_record, (\w+)\) == (\d+)", txt)}
    return fields, size, offs


def test_trace_record_layout_matches_header():
    from phdslam import types as T
    fields, size, offs = _header_record()
    assert [f for f, _ in T.TraceRecord._fields_] == fields
    assert list(T.TRACE_RECORD.names) == fields
    assert ctypes.sizeof(T.TraceRecord) == size == T.TRACE_RECORD.itemsize == 96
    assert len(offs) >= 8
    for name, off in offs.items():
        assert getattr(T.TraceRecord, name).offset == off, name
        assert T.TRACE_RECORD.fields[name][1] == off, name
    assert ctypes.sizeof(T.Pose) == T.POSE.itemsize == 24


def test_trace_symbols_exported(built):
    so = os.path.join(REPO, "cuda-phdslam_amd", "phdslam", "libphdslam.so")
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    names = set(line.split()[-1] for line in out.splitlines() if line.strip())
    for sym in ("phd_trace_enable", "phd_trace_count", "phd_trace_read"):
        assert sym in names, sym
    from phdslam._lib import SIGNATURES
    assert {"phd_trace_enable", "phd_trace_count", "phd_trace_read"} <= set(SIGNATURES)


# ------------------------------------------------------------------ GPU

def _scenario(cid, n, G=G, M=M):
    import phdslam
    c, poses, lw, maps, offs, z = phdslam.config_scenario(cid, n=n, G=G, M=M)
    c.resampleThresh = THRESH[cid]
    return c, poses, lw, maps, offs, z


def _control(c):
    return (2.0, 0.05) if c.motionType == 1 else None


def _filter(c, n, state, split=False, **kw):
    import phdslam
    kw.setdefault("survivor_capacity", 64)
    f = phdslam.PHDFilter(n, c, map_capacity=CAP, max_measurements=8, candidate_capacity=128, **kw)
    f.set_seed(4242)
    if split:
        f.set_update_form(2)
    f.load(*state)
    return f


def _split(cid, n):
    # the PHD step arms the overlapped resample in its split form only
    return cid == 2 and n > 2048


def _twin_scan(t, c, zk, k, cphd, take_errors=False):
    """One scan of the reference's loop through the synchronous entry points."""
    t.set_measurements(zk)
    t.predict_update(_control(c), k, do_predict=k > 0)
    t.normalize()
    pose, mi = t.expected_pose()
    s = dict(pose=pose.copy(), mi=mi, neff=t.neff(), cn=t.cardinalities())
    s["cd"] = t.cardinality_distribution() if cphd else None
    s["poses"], s["w"], s["maps"], s["offs"] = t.export()
    s["errors"] = t.status_errors() if take_errors else None
    s["resampled"] = bool(len(zk) > 0 and s["neff"] <= c.resampleThresh)
    if s["resampled"]:
        t.resample(step=k, return_indices=False)
    return s


@functools.lru_cache(maxsize=None)
def _twin_run(cid, n, map_estimate=0):
    """The checker, computed once per case and shared (never modified)."""
    c, poses, lw, maps, offs, z = _scenario(cid, n)
    c.mapEstimate = map_estimate
    t = _filter(c, n, (poses, lw, maps, offs), split=_split(cid, n))
    scans = [_twin_scan(t, c, z, k, c.filterType == 1) for k in range(SCANS)]
    final = t.export()
    t.close()
    return scans, final


def _traced_run(cid, n, capacity, snap=0, card=False, map_estimate=0, scans=SCANS):
    c, poses, lw, maps, offs, z = _scenario(cid, n)
    c.mapEstimate = map_estimate
    f = _filter(c, n, (poses, lw, maps, offs), split=_split(cid, n))
    f.set_check_each_update(False)
    f.enable_trace(capacity, snap, card)
    for k in range(scans):
        f.set_measurements(z)
        assert f.step(_control(c), do_predict=k > 0, step=k, readback=False) is None
    return f, c


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("cid,n,map_estimate", [(2, 300, 0), (2, 2304, 0), (3, 300, 0), (3, 2304, 2)])
def test_records_equal_twin(gpu, cid, n, map_estimate):
    """Six free-running scans, PHD (config 2's model) and CPHD (config 3's): 300
    particles (several waves, no multiple of 64 or 256) and 2304 (above 2 x 1024:
    the chunked resample, which the untraced split / CPHD step overlaps)."""
    scans, final = _twin_run(cid, n, map_estimate)
    cphd = cid == 3
    f, c = _traced_run(cid, n, SCANS, card=cphd, map_estimate=map_estimate)
    assert f.trace_count() == SCANS
    out = f.read_trace()
    rec, card = (out[0], out[2]) if cphd else (out, None)
    got_final = f.export()
    f.close()
    decisions = [s["resampled"] for s in scans]
    print("twin nEff", [round(float(s["neff"]), 4) for s in scans], "resampled", decisions)
    for k, (r, s) in enumerate(zip(rec, scans)):
        w64 = s["w"].astype(np.float64)
        mi = s["mi"]
        assert int(r["step"]) == k and r["n_live"] == n and r["n_measure"] == M
        assert bool(r["resampled"]) == s["resampled"], k
        assert r["map_particle"] == mi, k
        assert _bits(r["expected_pose"]) == _bits(s["pose"]), k
        assert _bits(r["map_pose"]) == _bits(s["poses"][mi]), k
        assert r["map_size"] == s["offs"][mi + 1] - s["offs"][mi], k
        # tolerances: twice the distance between the twin's own fp32 value and an
        # fp64 sum of the twin's exported data (the reference path's rounding)
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
        # the twin's fp32 statement: Σ_n exp(w_n) cn_n summed in particle order in float
        ce32 = float(np.cumsum(np.exp(s["w"]).astype(np.float32) * s["cn"], dtype=np.float32)[-1])
        cn64 = np.add.reduceat(s["maps"]["weight"].astype(np.float64), s["offs"][:-1].astype(np.int64)) \
            if len(s["maps"]) else np.zeros(n)
        cn64 = np.where(np.diff(s["offs"]) > 0, cn64, 0.0)
        ce64 = float(np.sum(np.exp(w64) * cn64))
        tol = 2.0 * abs(ce32 - ce64)
        gap = abs(float(r["card_expected"]) - ce32)
        print(f"scan {k}: card_expected gap {gap:.3g} (tolerance {tol:.3g})")
        assert gap <= tol, (k, r["card_expected"], ce32, ce64)
        if cphd and not (map_estimate & 2):
            assert _bits(card[k]) == _bits(s["cd"][mi]), k
        elif cphd:  # Σ exp(w_n) cn_n[k] in particle order in float, as recoverSlamState combines it
            ew = np.exp(s["w"]).astype(np.float32)
            cd32 = np.cumsum(ew[:, None] * s["cd"], axis=0, dtype=np.float32)[-1]
            cd64 = np.sum(np.exp(w64)[:, None] * s["cd"].astype(np.float64), axis=0)
            # two float sums of the same n terms in the same order round differently
            # once a term differs in its last place (the device's expf, numpy's exp):
            # beside the reference's own distance to the fp64 sum, the expected
            # rounding of one such sum, sqrt(n) 2^-24 Σ|term| (Higham's rule of thumb)
            mag = np.sum(np.abs(np.exp(w64)[:, None] * s["cd"].astype(np.float64)), axis=0)
            tol = 2.0 * np.abs(cd32 - cd64) + np.sqrt(n) * 2.0 ** -24 * mag
            gap = np.abs(card[k].astype(np.float64) - cd32)
            print(f"scan {k}: cardinality rows worst gap {gap.max():.3g} (tolerance there "
                  f"{tol[np.argmax(gap)]:.3g})")
            assert (gap <= tol).all(), (k, card[k], cd32)
    assert sum(decisions) >= 2 and not all(decisions), "threshold: the chain must both resample and not"
    # the trace did not disturb the chain
    assert _bits(got_final[0]) == _bits(final[0]) and _bits(got_final[1]) == _bits(final[1])
    np.testing.assert_array_equal(got_final[3], final[3])


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 65, 1023, 1025, 2049])
def test_reductions_equal_synchronous_calls(gpu, n):
    """The block reductions the trace shares with the synchronous kernels, at one
    lane, a wave edge, a chunk edge (1024) and a third chunk: one scan (map
    capacity 8, 4 measurements) from spread log-weights; the record's nEff,
    decision, expected pose and arg-max equal phd_normalize / phd_neff /
    phd_expected_pose bit for bit.  phd_lse_parts' (max, Σ exp) give the same
    log-sum-exp: phd_normalize's is not returned, so the weights normalised by
    log(Σ) + max are held against phd_normalize's at the tolerance
    test_normalize_neff_resample_bit_exact uses for that comparison."""
    import parity
    import phdslam
    c, poses, lw, maps, offs, z = _scenario(2, n, G=2, M=M)
    lw = np.random.default_rng(n).normal(-8, 3, n).astype(np.float32)
    run = []
    for traced in (False, True):
        f = phdslam.PHDFilter(n, c, map_capacity=8, max_measurements=8, candidate_capacity=128, survivor_capacity=64)
        f.set_seed(4242)
        if _split(2, n):
            f.set_update_form(2)
        f.set_check_each_update(False)
        f.load(poses, lw, maps, offs)
        f.set_measurements(z)
        run.append(f)
    t, f = run
    t.predict_update(_control(c), 0, do_predict=False)
    w_un = t.export(with_maps=False)[1]
    mx, sm = t.lse_parts()
    t.normalize()
    neff = np.float32(t.neff())
    pose, mi = t.expected_pose()
    tp, wn = t.export(with_maps=False)[:2]
    f.enable_trace(1)
    assert f.step(_control(c), do_predict=False, step=0, readback=False) is None
    r = f.read_trace()[0]
    t.close()
    f.close()
    assert _bits(np.float32(r["neff"])) == _bits(neff)
    assert bool(r["resampled"]) == bool(neff <= c.resampleThresh)
    assert r["map_particle"] == mi
    assert _bits(r["expected_pose"]) == _bits(pose)
    assert _bits(r["map_pose"]) == _bits(tp[mi])
    lse = np.float32(np.log(np.float32(sm))) + np.float32(mx)
    assert parity.close(wn, w_un - lse, 1e-5, floor=1e-5).all()


@pytest.mark.gpu
@pytest.mark.parametrize("snap", [64, 4])
def test_map_snapshot(gpu, snap):
    scans, _ = _twin_run(2, 300, 0)
    f, _ = _traced_run(2, 300, SCANS, snap=snap)
    rec, maps, card = f.read_trace()
    f.close()
    assert card is None and maps.shape == (SCANS, snap)
    for k, s in enumerate(scans):
        mi = s["mi"]
        want = s["maps"][s["offs"][mi]:s["offs"][mi + 1]]
        assert rec[k]["map_size"] == len(want)
        rows = min(len(want), snap)
        assert _bits(maps[k][:rows]) == _bits(want[:rows]), k
        assert not np.any(maps[k][rows:].view(np.uint8)), "rows beyond the map are zero"
    if snap == 4:
        assert any(r["map_size"] > 4 for r in rec), "the snapshot is shorter than some map"


@pytest.mark.gpu
def test_ring_wraps(gpu):
    import phdslam
    full, _ = _traced_run(2, 300, 8)
    want = full.read_trace(0, SCANS)
    full.close()
    f, c = _traced_run(2, 300, 4, scans=0)
    with pytest.raises(phdslam.PHDError) as e:  # nothing written yet
        f.read_trace(0, 1)
    assert e.value.code == phdslam._lib.PHD_E_ARG
    z = _scenario(2, 300)[5]
    for k in range(SCANS):
        f.set_measurements(z)
        f.step(_control(c), do_predict=k > 0, step=k, readback=False)
    assert f.trace_count() == SCANS
    got = f.read_trace(2, 4)
    assert _bits(got) == _bits(want[2:6])
    assert _bits(f.read_trace()) == _bits(want[2:6])  # the default: what the ring still holds
    with pytest.raises(phdslam.PHDError) as e:  # records 0 and 1 are overwritten
        f.read_trace(0, 4)
    assert e.value.code == phdslam._lib.PHD_E_ARG
    with pytest.raises(phdslam.PHDError) as e:  # record 6 is not written yet
        f.read_trace(3, 4)
    assert e.value.code == phdslam._lib.PHD_E_ARG
    f.close()


@pytest.mark.gpu
def test_scan_without_measurements(gpu):
    from phdslam.types import MEASUREMENT
    n = 300
    c, poses, lw, maps, offs, z = _scenario(2, n)
    sets = [z, np.zeros(0, MEASUREMENT), z]
    t = _filter(c, n, (poses, lw, maps, offs))
    scans = [_twin_scan(t, c, zk, k, False) for k, zk in enumerate(sets)]
    t.close()
    f = _filter(c, n, (poses, lw, maps, offs))
    f.set_check_each_update(False)
    f.enable_trace(4)
    for k, zk in enumerate(sets):
        f.set_measurements(zk)
        f.step(_control(c), do_predict=k > 0, step=k, readback=False)
    assert f.trace_count() == 3
    rec = f.read_trace()
    f.close()
    assert rec[1]["n_measure"] == 0 and rec[1]["resampled"] == 0 and rec[0]["n_measure"] == M
    for k in range(3):
        assert _bits(rec[k]["expected_pose"]) == _bits(scans[k]["pose"]), k
        assert rec[k]["map_particle"] == scans[k]["mi"], k


@pytest.mark.gpu
def test_off_means_off(gpu):
    """Never enabled, and enabled then switched off: the chain of a context that
    never touched the trace API, bit for bit (2304 CPHD particles: the step with
    the overlapped resample)."""
    n = 2304
    c, poses, lw, maps, offs, z = _scenario(3, n)

    def run(touch):
        f = _filter(c, n, (poses, lw, maps, offs))
        f.set_check_each_update(False)
        if touch == "count":
            assert f.trace_count() == 0
        elif touch == "on-off":
            f.enable_trace(8, 16, True)
            f.enable_trace(0)
        for k in range(3):
            f.set_measurements(z)
            f.step(_control(c), do_predict=k > 0, step=k, readback=False)
        if touch:
            assert f.trace_count() == 0
        out = f.export()
        f.close()
        return out

    base = run(None)
    for touch in ("count", "on-off"):
        got = run(touch)
        for a, b in zip(got, base):
            assert _bits(a) == _bits(b), touch


@pytest.mark.gpu
def test_unsupported_configurations(gpu):
    import phdslam
    from phdslam.scenario import mixed_config
    f = phdslam.PHDFilter(8, mixed_config(), map_capacity=CAP, max_measurements=8)
    with pytest.raises(phdslam.PHDError) as e:
        f.enable_trace(4)
    assert e.value.code == phdslam._lib.PHD_E_UNSUPPORTED
    f.close()
    c = _scenario(2, 8)[0]
    c.nPredictParticles = 2
    f = phdslam.PHDFilter(8, c, map_capacity=CAP, max_measurements=8, max_particles=64)
    with pytest.raises(phdslam.PHDError) as e:
        f.enable_trace(4)
    assert e.value.code == phdslam._lib.PHD_E_UNSUPPORTED
    assert f.trace_count() == 0
    f.close()
    c = _scenario(2, 8)[0]  # the cardinality distribution is a CPHD output
    f = phdslam.PHDFilter(8, c, map_capacity=CAP, max_measurements=8)
    with pytest.raises(phdslam.PHDError) as e:
        f.enable_trace(4, card_dist=True)
    assert e.value.code == phdslam._lib.PHD_E_UNSUPPORTED
    f.close()


@pytest.mark.gpu
def test_status_errors_recorded(gpu):
    """survivor_capacity 1 (held as one group of 4 keys): the update of a particle
    with more listed detection terms overflows its survivor list — a reported
    capacity error, the terms beyond it dropped.  G = 16, M = 8: six of the
    measurements are detections, so the lists are longer than 4."""
    n = 300
    c, poses, lw, maps, offs, z = _scenario(2, n, G=16, M=8)
    t = _filter(c, n, (poses, lw, maps, offs), survivor_capacity=1)
    want = _twin_scan(t, c, z, 0, False, take_errors=True)["errors"]
    t.close()
    f = _filter(c, n, (poses, lw, maps, offs), survivor_capacity=1)
    f.set_check_each_update(False)
    f.enable_trace(2)
    for k in range(2):
        f.set_measurements(z)
        f.step(_control(c), do_predict=False, step=0, readback=False)
        if k == 0:
            f.load(poses, lw, maps, offs)  # the same scan again: the count is per step, not cumulative
    rec = f.read_trace()
    f.close()
    assert want > 0
    assert rec[0]["status_errors"] == want and rec[1]["status_errors"] == want
