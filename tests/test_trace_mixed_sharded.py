"""The estimate trace of the mixed static + dynamic model (feature_model 2) on
the sharded step (phd_trace_shard_pack_mixed / _append_mixed,
ShardedFilter.enable_trace_mixed, GroupRank.enable_trace_mixed).

The contract: on every rank the scan's phd_trace_record, its
phd_trace_dyn_record, the static snapshot and the dynamic snapshot equal, byte
for byte, what a single mixed context of N = world * n particles (the ranks'
settled particles in rank order, same seed) writes for that scan in a traced
phd_step; and tracing leaves the particles as an untraced run leaves them.
tests/test_trace_mixed.py holds the single context's records to the
synchronous entry points.

Emulated ranks on one device, the collectives as device copies
(phdslam.dist.LocalWorld).  Three runs
per case share a scenario: a settled run (every step's plan settled and the
shards exported: the state the single context is loaded from before each
scan), the free-running untraced run and the free-running traced run.  Every
comparison is byte equality.

References into the sets X at the time of a pack.  Every update — the full one
and the re-update of pending slots — writes particle p's posterior to slab p of
the current sets and resets its reference to the identity, so a pack that
follows an update finds no reference into X whatever K is.  References into X
are live at a pack exactly on a scan without measurements (no update) that
follows a step whose plan moved particles: the slots that received a record
name X, whose dynamic slabs the predict advanced in place.  The main cases
therefore carry such a scan, and _x_slots derives which slots name X there
from the plan's own counts (phd_shard_poll).  After a resample every
log-weight is equal, and without an update they stay equal, so the arg-max of
such a scan is global particle 0: a case of its own
(test_argmax_slab_in_set_x) sets the log-weights before the scan to put the
arg-max on a received slot.
"""
import ctypes
import functools

import numpy as np
import pytest

from sharded_helpers import gathered_mixed, slice_mixed
from test_gpu_mixed_sharded import _load
from test_trace_sharded import _exported

CAP, DCAP, MCAP, KCAP = 128, 64, 32, 4096
SMALL = dict(cap=32, dcap=32, M=8, cand=256)  # the particle-count edges: maps of at most 4 components
S = 0x5eed  # the contexts' seed and the plan's: the single context's resample draws the shards' uniforms
SNAP, DSNAP = 8, 16
NEW_SYMBOLS = ("phd_trace_shard_block_bytes_mixed", "phd_trace_shard_pack_mixed", "phd_trace_shard_append_mixed")
# (world, n, K): (scenario seed, resample threshold).  With these the chain of
# five scans both resamples and does not, the scan before the empty one
# resamples and moves particles, and the arg-max particle sits on a rank other
# than 0 in some scan — all asserted below from the runs themselves.
MAIN = {(2, 24, 4): (None, 0.6), (3, 16, 1): (None, 0.6), (3, 16, 0): (None, 0.6)}
MAIN_EMPTY = 2  # scan 2 of 5 carries no measurements


# ------------------------------------------------------------------ CPU

def test_symbols_exported(built):
    from phdslam._lib import SIGNATURES
    names = _exported("libphdslam.so")
    for sym in NEW_SYMBOLS:
        assert sym in names, sym
        assert sym in SIGNATURES, sym
    assert "phd_group_trace_enable_mixed" in _exported("libphdslam_group.so")


@pytest.mark.parametrize("n,snap,dsnap", [(24, 0, 0), (16, 4, 5), (530, 64, 192)])
def test_block_bytes_follow_the_documented_layout(built, n, snap, dsnap):
    """header 64 B | n poses (24 B) | n cardinalities (4 B) | snap Gaussian2D
    (28 B) | n dynamic cardinalities (4 B) | dsnap Gaussian4D (84 B), rounded up
    to 16 (include/phd_capi.h)."""
    import phdslam
    got = ctypes.c_size_t()
    assert phdslam.lib().phd_trace_shard_block_bytes_mixed(n, snap, dsnap, ctypes.byref(got)) == 0
    want = 64 + 28 * n + 28 * snap + 4 * n + 84 * dsnap
    want = (want + 15) // 16 * 16
    assert got.value == want and got.value % 16 == 0
    E_ARG = phdslam._lib.PHD_E_ARG
    assert phdslam.lib().phd_trace_shard_block_bytes_mixed(0, snap, dsnap, ctypes.byref(got)) == E_ARG
    assert phdslam.lib().phd_trace_shard_block_bytes_mixed(n, -1, dsnap, ctypes.byref(got)) == E_ARG
    assert phdslam.lib().phd_trace_shard_block_bytes_mixed(n, snap, -1, ctypes.byref(got)) == E_ARG


# ------------------------------------------------------------------ GPU helpers

def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _config(thresh=1.0, ackerman=False, subdivide=1, **kw):
    from phdslam.scenario import mixed_config
    cfg = mixed_config(motionType=1 if ackerman else 0, resampleThresh=thresh, subdividePredict=subdivide, **kw)
    if ackerman:  # (the defaults leave the vehicle's geometry and its control noise zero)
        cfg.l, cfg.h, cfg.a, cfg.b, cfg.stdEncoder, cfg.stdAlpha = 1.415, 0.38, 1.89, 0.5, 1.0, 0.034907
    return cfg


def _control(cfg):
    return (2.0, 0.05) if cfg.motionType == 1 else None


def _filter(cfg, n, cap=CAP, dcap=DCAP, M=MCAP, cand=KCAP):
    import phdslam
    f = phdslam.PHDFilter(n, cfg, map_capacity=cap, max_measurements=M, candidate_capacity=cand, survivor_capacity=256)
    f.set_seed(S)
    f.enable_dynamic(dcap)
    f.set_check_each_update(False)
    return f


def _scenario(cfg, N, Gs=30, Gd=10, M=10, seed=None, lw=None):
    from phdslam.scenario import mixed_scenario
    kw = {} if seed is None else {"seed": seed}
    poses, sm, sof, dm, dof, z = mixed_scenario(cfg, N, Gs, Gd, M, **kw)
    if lw is None:
        lw = np.full(N, -np.log(N), np.float32)
    return (poses, lw, sm, sof, dm, dof), z


def _spy_polls(sf):
    """Keep what the rank's phd_shard_poll returned last (sf.polled)."""
    poll = sf.f.shard_poll
    sf.polled = None

    def spy(world):
        sf.polled = poll(world)
        return sf.polled

    sf.f.shard_poll = spy


def _step(ranks, ctrl, k):
    """LocalWorld.step.  Returns the gathered trace blocks as int32 rows (None
    untraced), read from rank 0's buffer after the step; every rank's sf.polled
    holds what its poll of the previous step's plan returned (None: no plan was
    open)."""
    import torch
    shards = ranks.shards
    for sf in shards:
        sf.polled = None
    ranks.step(ctrl, k)
    if shards[0].trace_block is None:
        return None
    return shards[0].trace_blocks.view(torch.int32).view(len(shards), -1)


def _sharded_run(cfg, state, zsets, world, n, K, trace=None, settled=False, toggle=False, weights=None, **cap):
    """`world` emulated ranks through len(zsets) scans (steps 1, 2, ...).
    settled: every step's plan is settled right after it and the shards
    exported (the list of gathered states); else the chain runs free and only
    the last plan is flushed.  trace: (capacity, snap, dsnap) for
    enable_trace_mixed.  weights: {k: f(received) -> N log-weights}: before scan
    k the open plan is settled on every kind of run and the ranks' log-weights
    are set (the settled run exports them with the state of step k - 1).
    Returns a dict: final (per-shard store), states, rec / smaps / drec / dmaps
    (per rank), headers (per scan: the blocks' 16 header words per rank),
    received (per scan, per rank: the slots that received a record of the
    previous step's plan — the last received[r] slots of rank r name the sets X
    until the next update), decisions, pending."""
    import torch
    from phdslam.dist import LocalWorld, ShardedFilter
    dev = torch.device("cuda", 0)
    ctrl = _control(cfg)
    weights = weights or {}
    shards = []
    for r in range(world):
        f = _filter(cfg, n, **cap)
        f.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        _load(f, *slice_mixed(*state, r * n, (r + 1) * n))
        sf = ShardedFilter(f, None, dev, world=world, rank=r, seed=S, block_records=K)
        _spy_polls(sf)
        if toggle:
            sf.enable_trace_mixed(8, SNAP, DSNAP)
            sf.enable_trace_mixed(0)
            assert sf.trace_block is None and f.trace_shape() == (0, 0, 0)
        if trace:
            sf.enable_trace_mixed(*trace)
        shards.append(sf)
    ranks = LocalWorld(shards)
    out = dict(states=[], decisions=[], headers=[], received=[])
    keep = []  # (the device tensors the ranks' log-weights were set from)

    def polled():
        """Per rank, the slots that received a record of the plan just polled
        (None: no plan was polled); notes that plan's decision."""
        if all(sf.polled is None for sf in shards):
            return None
        assert len(set(sf.last[1] for sf in shards)) == 1
        out["decisions"].append(int(shards[0].last[1]))
        return [int(sum(sf.polled[4])) if sf.polled[1] else 0 for sf in shards]

    def settle_now():
        for sf in shards:
            sf.polled = None
        ranks.flush()
        torch.cuda.synchronize()
        return polled()

    early = None  # the previous step's plan, where it was settled before this step
    for k, zk in enumerate(zsets, start=1):
        for sf in shards:
            sf.f.set_measurements(zk)
        blocks = _step(ranks, ctrl, k)
        got = polled()
        out["received"].append(early if early is not None else got if got is not None else [0] * world)
        early = None
        if blocks is not None:
            out["headers"].append(blocks[:, :16].cpu().numpy().copy())
        if settled or k + 1 in weights:
            early = settle_now()
        if k + 1 in weights:
            lw = np.asarray(weights[k + 1](early), np.float32)
            for r, sf in enumerate(shards):
                keep.append(torch.tensor(lw[r * n:(r + 1) * n], device=dev))
                torch.cuda.synchronize()
                sf.f.set_log_weights_from(keep[-1].data_ptr())
            torch.cuda.synchronize()
        if settled:
            out["states"].append(gathered_mixed([sf.f for sf in shards]))
    if early is None:
        settle_now()
    torch.cuda.synchronize()
    out["pending"] = sum(sf.stats["pending_slots"] for sf in shards)
    out["final"] = [(*sf.f.export(), *sf.f.export_dynamic()) for sf in shards]
    if trace:
        assert all(sf.f.trace_count() == len(zsets) for sf in shards)
        reads = [sf.f.read_trace() for sf in shards]
        dreads = [sf.f.read_trace_dynamic() for sf in shards]
        out["rec"] = [r[0] for r in reads]
        out["smaps"] = [r[1] for r in reads]
        out["drec"] = [d[0] for d in dreads]
        out["dmaps"] = [d[1] for d in dreads]
    else:
        assert all(sf.f.trace_count() == 0 for sf in shards)
    for sf in shards:
        sf.f.close()
    return out


def _single_run(cfg, N, state, states, zsets, trace, **cap):
    """The single mixed context of N particles: before scan k it is loaded with
    the gathered shards of step k - 1 (static maps, dynamic maps, log-weights),
    then runs a traced phd_step(step=k).  Returns (rec, smaps, drec, dmaps)."""
    f = _filter(cfg, N, **cap)
    f.enable_trace_mixed(*trace)
    for k, zk in enumerate(zsets, start=1):
        _load(f, *(state if k == 1 else states[k - 2]))
        f.set_measurements(zk)
        assert f.step(_control(cfg), do_predict=True, step=k, readback=False) is None
    rec, smaps, _ = f.read_trace()
    drec, dmaps = f.read_trace_dynamic()
    f.close()
    return rec, smaps, drec, dmaps


def _runs(cfg, state, zsets, world, n, K, trace=None, weights=None, **cap):
    """The settled run, the single context, the free untraced and the free
    traced run of one case."""
    trace = trace or (len(zsets), SNAP, DSNAP)
    settled = _sharded_run(cfg, state, zsets, world, n, K, settled=True, weights=weights, **cap)
    single = _single_run(cfg, world * n, state, settled["states"], zsets, (len(zsets),) + tuple(trace[1:]), **cap)
    free = _sharded_run(cfg, state, zsets, world, n, K, weights=weights, **cap)
    traced = _sharded_run(cfg, state, zsets, world, n, K, trace=trace, weights=weights, **cap)
    return single, free, traced


def _assert_equal_single(single, free, traced, world, n, scans, first=0):
    """Both rings of every rank against the single context's (scans first ..),
    one owner per scan with its header words, and the traced run's particles
    against the untraced run's."""
    rec, smaps, drec, dmaps = single
    for r in range(world):
        for k in range(first, scans):
            j = k - first
            assert _bits(traced["rec"][r][j]) == _bits(rec[k]), (k, r, traced["rec"][r][j], rec[k])
            assert _bits(traced["drec"][r][j]) == _bits(drec[k]), (k, r, traced["drec"][r][j], drec[k])
            assert _bits(traced["smaps"][r][j]) == _bits(smaps[k]), (k, r, "static snapshot")
            assert _bits(traced["dmaps"][r][j]) == _bits(dmaps[k]), (k, r, "dynamic snapshot")
    for k in range(scans):
        hdr = traced["headers"][k]
        own = int(rec[k]["map_particle"]) // n
        assert hdr[:, 1].sum() == 1 and hdr[own, 1] == 1, (k, hdr[:, 1])
        assert hdr[own, 4] == drec[k]["map_size"] and hdr[own, 2] == rec[k]["map_size"], (k, hdr[own])
        assert hdr[own, 5:6].view(np.float32)[0].tobytes() == _bits(drec[k]["card_map"]), k
        for r in range(world):
            if r != own:
                assert not hdr[r, 1:].any(), (k, r, hdr[r])  # (word 0: the rank's own error count)
    assert traced["decisions"] == free["decisions"]
    for a, b in zip(traced["final"], free["final"]):
        for x, y in zip(a, b):
            assert _bits(x) == _bits(y), "the trace perturbed the chain"


def _x_slots(traced, zsets, k, n):
    """Per rank, the local slots whose slab references name the sets X at the
    pack of scan k (1-based): the slots that received a record of the previous
    step's plan, on a scan with no update to reset them."""
    if len(zsets[k - 1]) > 0:
        return [range(0)] * len(traced["received"][k - 1])
    return [range(n - c, n) for c in traced["received"][k - 1]]


@functools.lru_cache(maxsize=None)
def _main_case(world, n, K):
    """Five scans, the second without measurements.  Computed once and shared,
    never modified."""
    seed, thresh = MAIN[(world, n, K)]
    cfg = _config(thresh)
    state, z = _scenario(cfg, world * n, seed=seed)
    zsets = [z[:0] if k == MAIN_EMPTY else z for k in range(1, 6)]
    return zsets, _runs(cfg, state, zsets, world, n, K)


# ------------------------------------------------------------------ 3. free-running chains

@pytest.mark.gpu
@pytest.mark.parametrize("world,n,K", list(MAIN))
def test_chain_conditions(gpu, world, n, K):
    """What the main case needs from its scenario, asserted so that it cannot
    pass vacuously: the chain both resamples and does not on scans with
    measurements, the arg-max particle sits on a rank other than 0 in some
    scan, and at the pack of the empty scan some rank holds references into the
    sets X (the plan before it moved particles).  N = 48: the second
    32-particle partial of card_expected straddles a rank boundary."""
    zsets, ((rec, _, drec, _), _, traced) = _main_case(world, n, K)
    with_z = [k for k in range(5) if len(zsets[k])]
    print("single nEff", [round(float(x), 4) for x in rec["neff"]], "resampled", rec["resampled"].tolist(),
          "map_particle", rec["map_particle"].tolist(), "received", traced["received"], "dyn sizes",
          drec["map_size"].tolist())
    assert rec["resampled"][with_z].any() and not rec["resampled"][with_z].all()
    assert (rec["map_particle"] >= n).any(), "the owner is never a rank other than 0: pick another seed"
    assert rec["resampled"][MAIN_EMPTY - 2] == 1, "the scan before the empty one does not resample"
    x = _x_slots(traced, zsets, MAIN_EMPTY, n)
    assert any(len(s) for s in x), "no rank holds a reference into set X at the empty scan's pack"
    assert (drec["map_size"] > 0).any() and (rec["map_size"] > SNAP).any()
    if K == 0:
        assert traced["pending"] > 0, "no pending slot was re-updated before a pack"


@pytest.mark.gpu
@pytest.mark.parametrize("world,n,K", list(MAIN))
def test_rings_equal_single_context(gpu, world, n, K):
    """Five free-running scans with snapshots (8, 16): both rings on every rank
    equal the single context's, one rank's block carries the owner flag, and
    the particles after the traced run equal the untraced run's."""
    zsets, (single, free, traced) = _main_case(world, n, K)
    rec = single[0]
    _assert_equal_single(single, free, traced, world, n, 5)
    for k in range(5):
        assert int(rec[k]["step"]) == k + 1 and rec[k]["n_live"] == world * n and rec[k]["n_measure"] == len(zsets[k])
        assert int(rec[k]["resampled"]) == traced["decisions"][k], k
    e = MAIN_EMPTY - 1
    assert rec[e]["resampled"] == 0 and rec[e]["n_measure"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("world,n,K", [(3, 16, 0), (2, 24, 4)])
def test_argmax_slab_in_set_x(gpu, world, n, K):
    """The arg-max particle's slabs in the sets X: scan 1 resamples (threshold
    1) and moves particles; the plan is settled and the log-weights are set so
    that the last slot of the highest rank that received a record — a slot that
    names X — is the arg-max; scan 2 has no measurements, so no update resets
    the references: its record, dyn record and both snapshots come out of X,
    the dynamic slab predicted in place."""
    N = world * n
    cfg = _config(1.0)
    state, z = _scenario(cfg, N)
    picked = {}

    def lw(received):
        r = max(i for i, c in enumerate(received) if c > 0)  # (no rank received: the case is void, max() raises)
        picked["rank"], picked["received"] = r, received
        w = np.full(N, -9.0, np.float32)
        w[r * n + n - 1] = -0.5
        return w

    zsets = [z, z[:0]]
    single, free, traced = _runs(cfg, state, zsets, world, n, K, weights={2: lw})
    rec, _, drec, dmaps = single
    _assert_equal_single(single, free, traced, world, n, 2)
    best = int(rec[1]["map_particle"])
    assert rec[0]["resampled"] == 1 and best == picked["rank"] * n + n - 1
    assert best % n in _x_slots(traced, zsets, 2, n)[best // n], (best, traced["received"])
    assert traced["received"][1] == picked["received"]
    print("arg-max", best, "received", traced["received"][1], "dyn map_size", int(drec[1]["map_size"]))
    assert drec[1]["map_size"] > 0 and np.any(dmaps[1][:1].view(np.uint8))
    assert rec[1]["n_measure"] == 0 and rec[1]["resampled"] == 0


# ------------------------------------------------------------------ 4. Ackerman, subdivided predict

@pytest.mark.gpu
@pytest.mark.parametrize("ackerman,subdivide", [(True, 1), (False, 2)])
def test_motion_and_subdivided_predict(gpu, ackerman, subdivide):
    """(3, 16, 0) with Ackerman motion, and with two predicts per step (late
    records predicted twice before their re-update): 4 scans, a resample each."""
    world, n, K = 3, 16, 0
    cfg = _config(1.0, ackerman=ackerman, subdivide=subdivide)
    state, z = _scenario(cfg, world * n)
    single, free, traced = _runs(cfg, state, [z] * 4, world, n, K)
    _assert_equal_single(single, free, traced, world, n, 4)
    assert single[0]["resampled"].all() and traced["pending"] > 0


# ------------------------------------------------------------------ 5. an empty scan

@pytest.mark.gpu
@pytest.mark.parametrize("K", [0, 2])
def test_scan_without_measurements(gpu, K):
    """Four scans, the second empty (M = 0, predict on): its record comes from
    the predicted store — the ranks' slots that received a record of step 1
    read the sets X, predicted in place — with resampled 0 and n_measure 0."""
    world, n = 3, 16
    cfg = _config(1.0)
    state, z = _scenario(cfg, world * n)
    zsets = [z, z[:0], z, z]
    single, free, traced = _runs(cfg, state, zsets, world, n, K)
    rec, _, drec, _ = single
    _assert_equal_single(single, free, traced, world, n, 4)
    assert rec[1]["n_measure"] == 0 and rec[1]["resampled"] == 0 and rec[0]["n_measure"] == len(z)
    assert traced["decisions"] == [1, 0, 1, 1]
    assert any(len(s) for s in _x_slots(traced, zsets, 2, n)), traced["received"]
    # the dynamic maps were predicted: every weight times p_s, so the expected cardinality fell
    assert 0 < drec[1]["card_expected"] and drec[1]["map_size"] > 0
    if K == 0:
        assert traced["pending"] > 0


# ------------------------------------------------------------------ 6. particle-count edges

@pytest.mark.gpu
@pytest.mark.parametrize("world,n", [(2, 40), (2, 530)])
def test_particle_count_edges(gpu, world, n):
    """N = 80 with n no multiple of 32 (partials and waves straddle the rank
    edge), and N = 1060, which crosses the 1024-entry weight chunk; maps of at
    most 4 components, 2 scans, uneven initial log-weights."""
    N = world * n
    cfg = _config(1.0)
    lw = np.random.default_rng(N).normal(-8, 2, N).astype(np.float32)
    state, z = _scenario(cfg, N, Gs=4, Gd=3, M=4, seed=7 + N, lw=lw)
    single, free, traced = _runs(cfg, state, [z, z], world, n, 2, trace=(2, 4, 8), **SMALL)
    _assert_equal_single(single, free, traced, world, n, 2)
    assert single[0]["n_live"].tolist() == [N, N] and single[0]["resampled"].all()


# ------------------------------------------------------------------ 7. dynamic-size edges, no step

@pytest.mark.gpu
@pytest.mark.parametrize("size", [0, 64, 65, 192])
def test_dynamic_map_size_edges(gpu, size):
    """dyn_capacity 192, world 2, n = 4, hand-built stores; the arg-max
    particle, on rank 1, holds 0, 64, 65 (one strip of the transpose and one
    component) or 192 dynamic components; snapshot capacities of 1, below,
    equal to and above the size.  The reference is the single context's
    empty-scan step without a predict (tests/test_trace_mixed.py::
    test_dynamic_map_size_edges); the ranks call the pack, the gather and the
    append directly, w_all being the loaded log-weights."""
    import torch
    from phdslam.scenario import mixed_scenario
    from phdslam.types import MEASUREMENT
    world, n = 2, 4
    N = world * n
    cfg = _config(1.0)
    sizes = [3, 0, 192, 7, 0, 64, 65, 192]
    poses, sm, sof, dm, _, _ = mixed_scenario(cfg, N, 3, 192, 4, seed=19)
    dm = np.concatenate([dm[p * 192:p * 192 + sizes[p]] for p in range(N)])
    dof = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    best = n + sizes[n:].index(size)
    lw = np.full(N, -9.0, np.float32)
    lw[best] = -0.5
    state = (poses, lw, sm, sof, dm, dof)
    none = np.zeros(0, MEASUREMENT)
    kw = dict(cap=32, dcap=192, M=8, cand=256)
    dev = torch.device("cuda", 0)
    w_all = torch.tensor(lw, device=dev)
    single = _filter(cfg, N, **kw)
    _load(single, *state)
    ranks = []
    for r in range(world):
        f = _filter(cfg, n, **kw)
        f.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        _load(f, *slice_mixed(*state, r * n, (r + 1) * n))
        f.set_measurements(none)
        ranks.append(f)
    torch.cuda.synchronize()
    nbytes = ctypes.c_size_t()
    import phdslam
    for dsnap in sorted({1, max(size - 1, 1), max(size, 1), size + 3}):
        single.enable_trace_mixed(2, 0, dsnap)
        for k in range(2):
            single.set_measurements(none)
            single.step(None, do_predict=False, step=k, readback=False)
        rec = single.read_trace()
        drec, dmaps = single.read_trace_dynamic()
        assert (rec["map_particle"] == best).all() and (drec["map_size"] == size).all()
        assert phdslam.lib().phd_trace_shard_block_bytes_mixed(n, 0, dsnap, ctypes.byref(nbytes)) == 0
        blocks = torch.zeros(world * nbytes.value, dtype=torch.uint8, device=dev)
        for f in ranks:
            f.enable_trace_mixed(2, 0, dsnap)
        for k in range(2):
            blocks.fill_(0xA5)
            for r, f in enumerate(ranks):
                f.trace_shard_pack_mixed(w_all.data_ptr(), world, r, k, blocks[r * nbytes.value:].data_ptr())
            for r, f in enumerate(ranks):
                f.trace_shard_append_mixed(w_all.data_ptr(), blocks.data_ptr(), world, r)
            torch.cuda.synchronize()
            hdr = blocks.view(torch.int32).view(world, -1)[:, :16].cpu().numpy()
            assert hdr[:, 1].tolist() == [0, 1] and hdr[1, 4] == size and not hdr[0, 1:].any(), hdr
        for f in ranks:
            assert f.trace_count() == 2
            got = f.read_trace()
            gd, gm = f.read_trace_dynamic()
            assert _bits(got) == _bits(rec), (dsnap, got, rec)
            assert _bits(gd) == _bits(drec), (dsnap, gd, drec)
            assert gm.shape == (2, dsnap) and _bits(gm) == _bits(dmaps), dsnap
            assert (got["n_measure"] == 0).all() and (got["resampled"] == 0).all()
        rows = min(size, dsnap)
        want = dm[dof[best]:dof[best + 1]]
        assert _bits(dmaps[0][:rows]) == _bits(want[:rows]) and not np.any(dmaps[0][rows:].view(np.uint8))
    for r, f in enumerate(ranks):  # the stores are exported as loaded
        want = slice_mixed(*state, r * n, (r + 1) * n)
        for x, y in zip((*f.export(), *f.export_dynamic()), want):
            assert _bits(x) == _bits(y)
        f.close()
    single.close()


# ------------------------------------------------------------------ 8. the ring wraps; off means off

@pytest.mark.gpu
def test_ring_wraps(gpu):
    """Capacity 3 over the main case's 5 scans: the rings hold scans 3..5 (the
    slots of scans 1 and 2 written a second time)."""
    import phdslam
    world, n, K = 2, 24, 4
    zsets, (single, free, _) = _main_case(world, n, K)
    seed, thresh = MAIN[(world, n, K)]
    cfg = _config(thresh)
    state, _ = _scenario(cfg, world * n, seed=seed)
    traced = _sharded_run(cfg, state, zsets, world, n, K, trace=(3, SNAP, DSNAP))
    for r in range(world):
        assert [int(x["step"]) for x in traced["rec"][r]] == [3, 4, 5]
        assert traced["dmaps"][r].shape == (3, DSNAP)
    _assert_equal_single(single, free, traced, world, n, 5, first=2)


@pytest.mark.gpu
def test_off_means_off(gpu):
    """enable_trace_mixed(8) then enable_trace_mixed(0): the state of a run that never touched it."""
    world, n, K = 3, 16, 1
    cfg = _config(1.0)
    state, z = _scenario(cfg, world * n)
    base = _sharded_run(cfg, state, [z] * 3, world, n, K)
    got = _sharded_run(cfg, state, [z] * 3, world, n, K, toggle=True)
    assert got["decisions"] == base["decisions"]
    for a, b in zip(got["final"], base["final"]):
        for x, y in zip(a, b):
            assert _bits(x) == _bits(y)


# ------------------------------------------------------------------ 9. the C++ host

@pytest.mark.gpu
def test_group_rank_trace_matches_sharded_filter(gpu):
    """GroupRank.enable_trace_mixed (phd_group_trace_enable_mixed: the mixed
    pack, ncclAllGather of the blocks, the mixed append inside phd_group_step)
    through RCCL at world 1 against a world-1 ShardedFilter and the single
    context's traced phd_step chain: one step sequence each."""
    import torch
    from phdslam.dist import GroupRank, LocalWorld, ShardedFilter
    n, steps = 32, 4
    cfg = _config(1.0)
    state, z = _scenario(cfg, n)
    dev = torch.device("cuda", 0)
    got = {}
    for kind in ("single", "torch", "cxx"):
        f = _filter(cfg, n)
        _load(f, *state)
        f.set_measurements(z)
        if kind == "single":
            f.enable_trace_mixed(steps, SNAP, DSNAP)
            for k in range(1, steps + 1):
                f.step(None, do_predict=True, step=k, readback=False)
        else:
            if kind == "torch":
                sf = ShardedFilter(f, None, dev, world=1, rank=0, seed=S, block_records=4)
            else:
                sf = GroupRank(f, None, dev, world=1, rank=0, seed=S, block_records=4)
            sf.enable_trace_mixed(steps, SNAP, DSNAP)
            run = LocalWorld([sf]) if kind == "torch" else sf
            for k in range(1, steps + 1):
                run.step(None, k)
            run.flush()
            torch.cuda.synchronize()
        assert f.trace_count() == steps
        got[kind] = (*f.read_trace()[:2], *f.read_trace_dynamic())
        if kind == "cxx":
            sf.enable_trace_mixed(0)
            assert f.trace_shape() == (0, 0, 0)
            sf.close()
        f.close()
    assert got["single"][0]["resampled"].any()
    for a, b, c in zip(got["cxx"], got["torch"], got["single"]):
        assert _bits(a) == _bits(b)
        assert _bits(a) == _bits(c)


# ------------------------------------------------------------------ 10. refusals

def _refused(code, text, call, *a):
    import phdslam
    with pytest.raises(phdslam.PHDError) as e:
        call(*a)
    assert e.value.code == code, str(e.value)
    assert text in str(e.value), str(e.value)


@pytest.mark.gpu
def test_refusals(gpu):
    """Every refused call leaves the trace count and the store as they were."""
    import torch
    import phdslam
    from phdslam._lib import PHD_E_ARG, PHD_E_UNSUPPORTED
    n = 8
    cfg = _config(1.0)
    state, z = _scenario(cfg, n, Gs=12, Gd=4, M=6)
    dev = torch.device("cuda", 0)
    w = torch.tensor(state[1], device=dev)
    buf = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    f = _filter(cfg, n)
    _load(f, *state)
    f.set_measurements(z)
    before = (*f.export(), *f.export_dynamic())

    def untouched(count):
        assert f.trace_count() == count
        for x, y in zip((*f.export(), *f.export_dynamic()), before):
            assert _bits(x) == _bits(y)

    pack = lambda: f.trace_shard_pack_mixed(w.data_ptr(), 1, 0, 1, buf.data_ptr())
    append = lambda: f.trace_shard_append_mixed(w.data_ptr(), buf.data_ptr(), 1, 0)
    # no trace at all
    _refused(PHD_E_ARG, "is off", pack)
    _refused(PHD_E_ARG, "is off", append)
    untouched(0)
    # append without pack, pack twice
    f.enable_trace_mixed(4, SNAP, DSNAP)
    _refused(PHD_E_ARG, "without phd_trace_shard_pack_mixed", append)
    untouched(0)
    pack()
    _refused(PHD_E_ARG, "previous block first", pack)
    append()
    untouched(1)
    # the static calls on a mixed trace keep refusing
    _refused(PHD_E_UNSUPPORTED, "feature_model 2", f.trace_shard_pack, w.data_ptr(), 1, 0, 1, buf.data_ptr())
    _refused(PHD_E_UNSUPPORTED, "feature_model 2", f.trace_shard_append, w.data_ptr(), buf.data_ptr(), 1, 0)
    _refused(PHD_E_UNSUPPORTED, "static feature model only", f.enable_trace, 4)
    # (the refused phd_trace_enable freed the rings, as every phd_trace_enable call does first)
    untouched(0)
    # the dynamic capacity changed after enable
    f.enable_trace_mixed(4, SNAP, DSNAP)
    f.enable_dynamic(96)
    _refused(PHD_E_UNSUPPORTED, "enable the trace again", pack)
    assert f.trace_count() == 0
    f.close()
    # n_predict_particles = 2: refused at the pack (the trace was enabled under 1)
    f = _filter(cfg, n)
    _load(f, *state)
    before = (*f.export(), *f.export_dynamic())
    f.enable_trace_mixed(4, SNAP, DSNAP)
    c2 = cfg.copy()
    c2.nPredictParticles = 2
    f.set_config(c2)
    _refused(PHD_E_UNSUPPORTED, "n_predict_particles", pack)
    untouched(0)
    f.close()
    # the mixed calls on a static trace
    c0 = phdslam.config_scenario(2, n=n, G=4, M=4)
    s = phdslam.PHDFilter(n, c0[0], map_capacity=64, max_measurements=8, candidate_capacity=128, survivor_capacity=64)
    s.load(*c0[1:5])
    s.enable_trace(4)
    with pytest.raises(phdslam.PHDError) as e:
        s.trace_shard_pack_mixed(w.data_ptr(), 1, 0, 1, buf.data_ptr())
    assert e.value.code in (PHD_E_ARG, PHD_E_UNSUPPORTED) and "phd_trace_enable_mixed" in str(e.value)
    with pytest.raises(phdslam.PHDError) as e:
        s.trace_shard_append_mixed(w.data_ptr(), buf.data_ptr(), 1, 0)
    assert e.value.code in (PHD_E_ARG, PHD_E_UNSUPPORTED) and "phd_trace_enable_mixed" in str(e.value)
    assert s.trace_count() == 0
    s.trace_shard_pack(w.data_ptr(), 1, 0, 1, buf.data_ptr())  # (its own pair still serves it)
    s.trace_shard_append(w.data_ptr(), buf.data_ptr(), 1, 0)
    assert s.trace_count() == 1
    s.close()
