"""The sharded resample and its migration plan on the device — phd_global_resample,
phd_shard_resample and phd_shard_resample_async in the one-launch form
(k_shard_plan) and the chain form (k_rs_* + k_shard_tail), phd_shard_poll —
against two references that share no code with them: the float64 weighting
reference (tests/weighting_ref.py) for the global part, the plain-integer plan
(tests/shard_plan_ref.py) for everything after the parent list.  The shared
cases are tests/shard_plan_cases.py; neither the oracle nor phdslam.dist is
called.

Global part: the normalised gathered weights and nEff within D_oracle(case) +
1e-5 of the reference (weighting_cases.D_ORACLE, as tests/test_gpu_weighting.py),
the decision equal unless the reference marks it near, the parents under
weighting_cases.hold_parents on the device's own normalised weights.  The
forms agree byte for byte: phd_global_resample, the one-launch plan and the
chain plan, on every checked rank.  Plan: demand, send and receive records,
keep_src, send_src, recv_rec, the pending count and the capacity errors equal
the reference's on the device's parent list.  Remap: the kept slots hold their
parents' poses and the new log-weight; without a resample nothing changes but
the log-weights, which are the rank's slice of the normalised vector.

Ranks checked: every rank up to world 16; above, rank 0, the last, the first
with a surplus, the first with a deficit, one with demand 0, the rank of the
first maximum and eight spread evenly (shard_plan_cases.checked_ranks).
"""
import numpy as np
import pytest

import shard_plan_cases as SC
import shard_plan_ref as S
import weighting_cases as C
import weighting_ref as R
from test_gpu_parity import _filter, _record_elementwise

pytestmark = pytest.mark.gpu

SHAPE_IDS = [SC.key(s) for s in SC.SHAPES]
_PLANS = {}  # shape -> (parent list bytes, its plan): the two tests of a shape share it


def _bits(t):
    import torch
    return t.view(torch.int32)


class Rig:
    """One context of n particles and the device buffers of a shape."""

    def __init__(self, shape, resample=True, measurements=True):
        import torch
        self.shape = shape
        self.world, self.n, self.dist = shape
        self.N = self.world * self.n
        self.wcase = SC.wcase(shape)
        self.dev = torch.device("cuda", 0)
        cfg, self.poses, self.empty, self.offs0, self.z = C.scenario("phd", self.n)
        cfg = cfg.copy()
        cfg.resampleThresh = C.thresh(self.dist, self.N) if resample else 0.0
        self.f = _filter(cfg, self.n, **C.CAPS)
        self.lw = np.full(self.n, -1.0, np.float32)
        self.reload()
        if measurements:
            self.f.set_measurements(self.z)
        self.base = C.weights(self.dist, self.N)
        self.seed, self.step = SC.seed_step(shape)
        self.new_logw = np.float32(-np.log(np.float64(self.N)))
        self.rec_bytes = self.f.record_bytes()
        i32 = dict(dtype=torch.int32, device=self.dev)
        self.w = torch.empty(self.N, dtype=torch.float32, device=self.dev)
        self.parents = torch.empty(self.N, **i32)
        self.keep = torch.empty(self.n, **i32)
        # (the plan writes every record's parent whatever the capacity of the record buffers)
        self.send = torch.empty(self.n * max(self.world - 1, 1), **i32)
        self.recv = torch.empty(self.n, **i32)
        self._bytes = {}

    def reload(self):
        self.f.load(self.poses, self.lw, self.empty, self.offs0)

    def upload(self):
        import torch
        self.w.copy_(torch.from_numpy(self.base))
        self.parents.fill_(-1)
        self.keep.fill_(-1)
        self.send.fill_(-1)
        self.recv.fill_(-1)
        torch.cuda.synchronize()

    def room(self, tag, records):
        """A device buffer of `records` records (0: a NULL pointer)."""
        import torch
        nbytes = records * self.rec_bytes
        if nbytes == 0:
            return 0
        if tag not in self._bytes or self._bytes[tag].numel() < nbytes:
            self._bytes[tag] = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        return self._bytes[tag].data_ptr()

    def ptrs(self):
        return (self.parents.data_ptr(), self.keep.data_ptr(), self.send.data_ptr(), self.recv.data_ptr())

    def close(self):
        self.f.close()


def _global(rig, rec):
    """phd_global_resample of the gathered weights, held to the weighting
    reference; returns (normalised weights on the device, their host copy, nEff,
    decision, parent list on the device, its host copy, the reference's Parents)."""
    import torch
    label = f"shard plan {SC.key(rig.shape)}"
    rig.upload()
    neff, rs = rig.f.global_resample(rig.w.data_ptr(), rig.N, 0, rig.seed, rig.step, rig.parents.data_ptr())
    torch.cuda.synchronize()
    gw_dev, par_dev = rig.w.clone(), rig.parents.clone()
    gw, par = gw_dev.cpu().numpy(), par_dev.cpu().numpy().astype(np.int64)
    wn, dec = C.reference(rig.wcase)
    tab = C.D_ORACLE[C.key(rig.wcase)]
    d_w, d_n = C.lognorm_deviation(gw, wn), C.neff_deviation(neff, dec.neff)
    rec.update(lognorm=d_w, d_oracle_lognorm=tab["lognorm"], neff=d_n, d_oracle_neff=tab["neff"])
    print(f"{label}: lognorm {d_w:.3g} (tolerance {tab['lognorm'] + C.CONTRACT:.3g}), nEff {neff:.9g}, "
          f"reference {dec.neff:.9g}: {d_n:.3g} (tolerance {tab['neff'] + C.CONTRACT:.3g})")
    assert d_w <= tab["lognorm"] + C.CONTRACT, f"{label}: normalised log-weights deviate {d_w:.3g}"
    assert d_n <= tab["neff"] + C.CONTRACT, f"{label}: nEff deviates {d_n:.3g}"
    assert dec.near or rs == dec.resample, f"{label}: decision {rs}, reference {dec}"
    assert rs, f"{label}: the case asks for a resample"
    assert par.min() >= 0 and par.max() < rig.N
    near, strata, ref = C.hold_parents(par, gw, SC.uniforms(rig.shape), label)
    rec.update(near=near, strata=strata, beyond=int(ref.beyond.size))
    print(f"{label}: {near} of {strata} strata near, {ref.beyond.size} past the CDF's end")
    return gw_dev, gw, neff, rs, par_dev, par, ref


def _plan_of(rig, par, ref):
    """The reference plan on the device's parent list, and the ranks to check."""
    hit = _PLANS.get(rig.shape)
    if hit is None or hit[0] != par.tobytes():
        hit = _PLANS[rig.shape] = (par.tobytes(), S.plan(par, rig.n, rig.world, rig.n))
    P = hit[1]
    if rig.dist == "tie":
        assert ref.beyond.size >= 1, "the committed (seed, step) overruns the CDF of the device's weights"
        assert np.any(np.diff(par) < 0) and par[-1] == ref.amax == rig.N // 3, "the parent list drops at its end"
        assert P.beyond >= 1 and P.ins is not None and P.ins < rig.N - P.beyond, "the suffix moves to the middle"
    return P, SC.checked_ranks(P, ref.amax)


def _hold_plan(rig, P, r, demand, snd, rcv, label):
    """Counts and index lists of rank r against the plan P (after a synchronise)."""
    n = rig.n
    assert demand == P.demand, f"{label}: demand"
    assert snd == P.send_records(r), f"{label}: send records"
    assert rcv == P.recv_records(r), f"{label}: receive records"
    kd = min(P.demand[r], n)
    np.testing.assert_array_equal(rig.keep.cpu().numpy()[:kd], P.keep(r), err_msg=f"{label}: keep_src")
    np.testing.assert_array_equal(rig.send.cpu().numpy()[:sum(snd)], P.send_src(r), err_msg=f"{label}: send_src")
    np.testing.assert_array_equal(rig.recv.cpu().numpy()[:n - kd], P.recv_rec(r), err_msg=f"{label}: recv_rec")
    return kd


def _hold_remap(rig, P, r, kd, label):
    gp, gw, _, _ = rig.f.export()
    assert gp[:kd].tobytes() == np.ascontiguousarray(rig.poses[P.keep(r)]).tobytes(), f"{label}: kept poses"
    np.testing.assert_array_equal(gw[:kd], rig.new_logw, err_msg=f"{label}: kept log-weights")


def _hold_global_bits(rig, gw_dev, par_dev, neff, neff_g, rs, label):
    import torch
    assert torch.equal(_bits(rig.w), _bits(gw_dev)), f"{label}: normalised weights differ from phd_global_resample's"
    assert torch.equal(rig.parents, par_dev), f"{label}: parents differ from phd_global_resample's"
    assert np.float32(neff).tobytes() == np.float32(neff_g).tobytes() and rs, f"{label}: nEff / decision"


def _skip_unless_chain_fallback(shape):
    import torch
    if shape[:2] == SC.CHAIN_FALLBACK:
        cu = torch.cuda.get_device_properties(0).multi_processor_count
        if cu > SC.MAX_RESIDENT_CU:
            pytest.skip(f"{cu} compute units hold the 257 workgroups of the one-launch plan resident: "
                        "the synchronous call does not fall back to the chain here")


def _hold_identity(rig, r, gw, out, label):
    """Flag 0: every count zero, identity keep, poses unchanged, the rank's slice as log-weights."""
    neff, rs, demand, snd, rcv = out[:5]
    n, world = rig.n, rig.world
    assert not rs and demand == [n] * world and snd == [0] * world and rcv == [0] * world, label
    np.testing.assert_array_equal(rig.keep.cpu().numpy(), np.arange(n), err_msg=label)
    gp, lw, _, _ = rig.f.export()
    assert gp.tobytes() == np.ascontiguousarray(rig.poses).tobytes(), f"{label}: poses"
    assert lw.tobytes() == gw[r * n:(r + 1) * n].tobytes(), f"{label}: log-weights are the normalised slice"


# ------------------------------------------------------------- synchronous form

@pytest.mark.parametrize("shape", SC.SHAPES, ids=SHAPE_IDS)
def test_global_and_synchronous_plan(gpu, shape):
    """phd_global_resample against the weighting reference; phd_shard_resample on
    every checked rank against it bit for bit and against the reference plan.
    (1024, 257): 257 chunks, the k_rs_* chain + k_shard_tail on a device of at
    most 256 compute units; every other shape the one-launch k_shard_plan."""
    import torch
    from phdslam import _lib
    _skip_unless_chain_fallback(shape)
    rig = Rig(shape)
    label = f"shard plan {SC.key(shape)}"
    rec = dict(label=label + " synchronous", reference="weighting_ref + shard_plan_ref", form="shard",
               particles=rig.N, world=rig.world)
    gw_dev, gw, neff_g, rs_g, par_dev, par, ref = _global(rig, rec)
    P, ranks = _plan_of(rig, par, ref)
    rec.update(ranks=ranks, moved=len(P.moves), records=sum(P._pair.values()))
    surplus_rank = next((r for r in ranks if len(P.send_src(r))), None)
    for r in ranks:
        sent = len(P.send_src(r))
        rig.reload()
        rig.upload()
        out = rig.f.shard_resample(rig.w.data_ptr(), rig.world, r, rig.seed, rig.step, *rig.ptrs(),
                                   rig.room("records", sent), sent, rig.new_logw)
        torch.cuda.synchronize()
        lab = f"{label} rank {r}"
        _hold_global_bits(rig, gw_dev, par_dev, out[0], neff_g, out[1], lab)
        kd = _hold_plan(rig, P, r, out[2], out[3], out[4], lab)
        _hold_remap(rig, P, r, kd, lab)
    if surplus_rank is not None:  # a record buffer one short: PHD_E_CAPACITY, the counts still the plan's
        r, sent = surplus_rank, len(P.send_src(surplus_rank))
        rig.reload()
        rig.upload()
        with pytest.raises(_lib.PHDError) as err:
            rig.f.shard_resample(rig.w.data_ptr(), rig.world, r, rig.seed, rig.step, *rig.ptrs(),
                                 rig.room("records", sent - 1), sent - 1, rig.new_logw)
        assert err.value.code == _lib.PHD_E_CAPACITY
        torch.cuda.synchronize()
        _, _, _, demand, snd, rcv = rig.f._shard_bufs
        _hold_plan(rig, P, r, list(demand), list(snd), list(rcv), f"{label} rank {r} one record short")
    rig.close()
    # flag 0: resampleThresh below nEff, and no measurement set
    for tag, kw in (("threshold 0", dict(resample=False)), ("no measurements", dict(measurements=False))):
        rig0 = Rig(shape, **kw)
        for r in sorted({ranks[0], ranks[-1]} if tag == "threshold 0" else {ranks[len(ranks) // 2]}):
            rig0.reload()
            rig0.upload()
            out = rig0.f.shard_resample(rig0.w.data_ptr(), rig0.world, r, rig0.seed, rig0.step, *rig0.ptrs(),
                                        0, 0, rig0.new_logw)
            torch.cuda.synchronize()
            assert torch.equal(_bits(rig0.w), _bits(gw_dev)), f"{label} {tag}: normalised weights"
            assert np.float32(out[0]).tobytes() == np.float32(neff_g).tobytes()
            _hold_identity(rig0, r, gw, out, f"{label} rank {r} {tag}")
        rig0.close()
    _record_elementwise(rec)


# ------------------------------------------------------------------- async form

def _async(rig, r, K, ovf_capacity):
    """phd_shard_resample_async + phd_shard_poll of rank r with blocks of K records."""
    import torch
    rig.reload()
    rig.upload()
    rig.f.shard_resample_async(rig.w.data_ptr(), rig.world, r, rig.seed, rig.step, *rig.ptrs(),
                               rig.room("blocks", rig.world * K) if rig.world > 1 else 0, K,
                               rig.room("overflow", ovf_capacity), ovf_capacity, rig.new_logw)
    try:
        return rig.f.shard_poll(rig.world)  # (before anything else)
    finally:
        torch.cuda.synchronize()


@pytest.mark.parametrize("shape", SC.SHAPES, ids=SHAPE_IDS)
def test_async_plan_one_launch_and_chain(gpu, shape):
    """phd_shard_resample_async + phd_shard_poll with blocks of K = 0, 1 and n
    records, as one launch and — with a plan stream set — as the k_rs_* chain +
    k_shard_tail: the same bits as phd_global_resample, the reference's plan and
    pending count, PHD_E_CAPACITY exactly when the overflow buffer is short."""
    import torch
    from phdslam import _lib
    rig = Rig(shape)
    label = f"shard plan {SC.key(shape)}"
    rec = dict(label=label + " async", reference="weighting_ref + shard_plan_ref", form="shard-async",
               particles=rig.N, world=rig.world)
    gw_dev, gw, neff_g, rs_g, par_dev, par, ref = _global(rig, rec)
    P, ranks = _plan_of(rig, par, ref)
    aux = torch.cuda.Stream(device=rig.dev)
    pend_total = 0
    for chain in (False, True):
        rig.f.set_plan_stream(aux.cuda_stream if chain else None)
        for r in ranks:
            for K in SC.KS(rig.n):
                lab = f"{label} rank {r} K {K} {'chain' if chain else 'one launch'}"
                neff, rs, demand, snd, rcv, pend = _async(rig, r, K, P.overflow_send(r, K))
                _hold_global_bits(rig, gw_dev, par_dev, neff, neff_g, rs, lab)
                kd = _hold_plan(rig, P, r, demand, snd, rcv, lab)
                assert pend == len(P.pending(r, K)), f"{lab}: pending {pend}, reference {len(P.pending(r, K))}"
                pend_total += pend
                _hold_remap(rig, P, r, kd, lab)
        # the overflow buffer one record short of the records beyond the blocks
        for K in (0, 1):
            r = next((r for r in ranks if P.overflow_send(r, K) > 0), None)
            if r is None:
                continue
            with pytest.raises(_lib.PHDError) as err:
                _async(rig, r, K, P.overflow_send(r, K) - 1)
            assert err.value.code == _lib.PHD_E_CAPACITY
            _, _, _, _, demand, snd, rcv = rig.f._poll_bufs
            assert list(demand) == P.demand and list(snd) == P.send_records(r) and list(rcv) == P.recv_records(r)
    rig.f.set_plan_stream(None)
    rig.close()
    # flag 0 on both forms: threshold 0, and no measurement set
    for tag, kw in (("threshold 0", dict(resample=False)), ("no measurements", dict(measurements=False))):
        rig0 = Rig(shape, **kw)
        r = ranks[0] if tag == "threshold 0" else ranks[-1]
        for chain in (False, True):
            rig0.f.set_plan_stream(aux.cuda_stream if chain else None)
            out = _async(rig0, r, 1, 0)
            assert torch.equal(_bits(rig0.w), _bits(gw_dev)), f"{label} {tag}: normalised weights"
            assert np.float32(out[0]).tobytes() == np.float32(neff_g).tobytes() and out[5] == 0
            _hold_identity(rig0, r, gw, out, f"{label} rank {r} {tag} {'chain' if chain else 'one launch'}")
        rig0.f.set_plan_stream(None)
        rig0.close()
    rec.update(ranks=ranks, pending=pend_total)
    _record_elementwise(rec)


# --------------------------------------------------------------------- refusals

def test_refusals_leave_the_store_unchanged(gpu):
    """world = 1025, rank = world and world n > 2^20 are refused by both forms
    with PHD_E_ARG before anything is enqueued."""
    from phdslam import _lib
    rig = Rig((4, 1025, "normal"))
    rig.upload()
    before = rig.f.export()
    for world, r in ((1025, 0), (4, 4), (1024, 0)):  # (1024 x 1025 = 2^20 + 1024 entries)
        for form in ("synchronous", "async"):
            with pytest.raises(_lib.PHDError) as err:
                if form == "async":
                    rig.f.shard_resample_async(rig.w.data_ptr(), world, r, rig.seed, rig.step, *rig.ptrs(),
                                               rig.room("blocks", 4), 0, 0, 0, rig.new_logw)
                else:
                    # (the wrapper sizes the host outputs by `world`)
                    rig.f.shard_resample(rig.w.data_ptr(), world, r, rig.seed, rig.step, *rig.ptrs(), 0, 0,
                                         rig.new_logw)
            assert err.value.code == _lib.PHD_E_ARG, (world, r, form)
            with pytest.raises(_lib.PHDError):  # no plan was opened
                rig.f.shard_poll(4)
            after = rig.f.export()
            for a, b in zip(before, after):
                assert a.tobytes() == b.tobytes(), (world, r, form)
    rig.close()


def test_second_async_call_without_a_poll_is_refused(gpu):
    """The refused call changes nothing: the poll and the store are those of the first call alone."""
    import torch
    from phdslam import _lib
    rig = Rig((3, 5, "normal"))
    runs = []
    for twice in (False, True):
        rig.reload()
        rig.upload()
        args = (rig.w.data_ptr(), 3, 1, rig.seed, rig.step, *rig.ptrs(), rig.room("blocks", 3), 1,
                rig.room("overflow", 10), 10, rig.new_logw)
        rig.f.shard_resample_async(*args)
        if twice:
            with pytest.raises(_lib.PHDError) as err:
                rig.f.shard_resample_async(*args)
            assert err.value.code == _lib.PHD_E_ARG
        out = rig.f.shard_poll(3)
        torch.cuda.synchronize()
        runs.append((out, rig.f.export(), rig.w.cpu().numpy(), rig.parents.cpu().numpy()))
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1], runs[1][1]):
        assert a.tobytes() == b.tobytes()
    assert runs[0][2].tobytes() == runs[1][2].tobytes() and runs[0][3].tobytes() == runs[1][3].tobytes()
    rig.close()
