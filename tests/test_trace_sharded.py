"""The estimate trace on the sharded step (phd_trace_shard_pack / _append,
ShardedFilter.enable_trace, GroupRank.enable_trace).

The contract: every rank's record of a scan equals, bit for bit in every field,
the record a single context of N = world * n particles (the shards' particles
in rank order) writes for that scan in a traced phd_step.  tests/test_trace.py
holds the single context's record to the synchronous entry points.

Emulated ranks on one device, the collectives as device copies
(phdslam.dist.LocalWorld).  Three runs per case share a
scenario: a settled run (every step's plan settled and the shards exported: the
state the single context is loaded from before each scan), the free-running
untraced run and the free-running traced run.  Small synthetic scenarios as
tests/test_trace.py: G = 8 prior components, M = 4 measurements, map capacity 64.
"""
import ctypes
import functools
import os
import subprocess

import numpy as np
import pytest

from sharded_helpers import gathered_store, slice_store

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

G, M, CAP, SCANS = 8, 4, 64, 5
# resample thresholds as tests/test_trace.py: between the nEff one scan after a
# resample and two scans after, so the chain both resamples and does not
THRESH = {2: 0.5, 3: 0.9}
# scenario seeds: with these the arg-max particle sits on rank 0 in some scan and
# on another rank in some other (asserted from the single context's records)
SEED = {(2, 3, 48): 14, (3, 3, 48): 12, (2, 3, 700): 12}  # (cid, world, n): seed; others the preset's
FILTER_SEED = 4242  # the contexts' and the plan's: the single context's resample draws the shards' uniforms


# ------------------------------------------------------------------ CPU

def _exported(lib):
    so = os.path.join(REPO, "cuda-phdslam_amd", "phdslam", lib)
    out = subprocess.run(["nm", "-D", "--defined-only", so], capture_output=True, text=True, check=True).stdout
    return set(line.split()[-1] for line in out.splitlines() if line.strip())


def test_sharded_trace_symbols_exported(built):
    from phdslam._lib import SIGNATURES
    names = _exported("libphdslam.so")
    for sym in ("phd_trace_shard_block_bytes", "phd_trace_shard_pack", "phd_trace_shard_append"):
        assert sym in names, sym
        assert sym in SIGNATURES, sym
    assert "phd_group_trace_enable" in _exported("libphdslam_group.so")


@pytest.mark.parametrize("n,snap,K", [(48, 0, 0), (700, 4, 0), (48, 64, 33)])
def test_block_bytes_follow_the_documented_layout(built, n, snap, K):
    """header 64 B | n poses (24 B) | n cardinalities (4 B) | snap Gaussian2D
    (28 B) | K floats, rounded up to 16 (include/phd_capi.h)."""
    import phdslam
    got = ctypes.c_size_t()
    assert phdslam.lib().phd_trace_shard_block_bytes(n, snap, K, ctypes.byref(got)) == 0
    want = 64 + 28 * n + 28 * snap + 4 * K
    want = (want + 15) // 16 * 16
    assert got.value == want and got.value % 16 == 0
    assert phdslam.lib().phd_trace_shard_block_bytes(0, snap, K, ctypes.byref(got)) == phdslam._lib.PHD_E_ARG


# ------------------------------------------------------------------ GPU

def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _scenario(cid, N, seed=None, G=G, M=M, map_estimate=0):
    import phdslam
    c, poses, lw, maps, offs, z = phdslam.config_scenario(cid, n=N, G=G, M=M, seed=seed)
    c.resampleThresh = THRESH[cid]
    c.mapEstimate = map_estimate
    return c, (poses, lw, maps, offs), z


def _control(c):
    return (2.0, 0.05) if c.motionType == 1 else None


def _filter(c, n, **kw):
    import phdslam
    kw.setdefault("survivor_capacity", 64)
    f = phdslam.PHDFilter(n, c, map_capacity=CAP, max_measurements=8, candidate_capacity=128, **kw)
    f.set_seed(FILTER_SEED)
    f.set_step_births(0)
    f.set_check_each_update(False)
    return f


def _owners(shards):
    """Per rank, the owner flag of its trace block (None untraced), read from
    rank 0's gathered blocks after the step."""
    import torch
    if shards[0].trace_block is None:
        return None
    return shards[0].trace_blocks.view(torch.int32).view(len(shards), -1)[:, 1]  # TRACE_BH_OWNER


def _sharded_run(c, state, zsets, world, n, K, trace=None, settled=False, toggle=False, errors=False, **cap):
    """`world` emulated ranks through len(zsets) scans (steps 1, 2, ...).
    settled: every step's plan is settled right after it and the shards exported
    (the list of gathered states); else the chain runs free and only the last
    plan is flushed.  trace: (capacity, snap, card_dist) for enable_trace.
    Returns a dict: final (per-shard exports), states, records / maps / card
    (per rank), decisions (the plans', from sf.last), owners (per scan),
    errors (per scan, the ranks' status_errors() summed, with errors=True),
    pending (slots re-updated after their record arrived, over the run)."""
    import torch
    from phdslam.dist import LocalWorld, ShardedFilter
    dev = torch.device("cuda", 0)
    ctrl = _control(c)
    shards = []
    for r in range(world):
        f = _filter(c, n, **cap)
        f.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        f.load(*slice_store(state, r * n, (r + 1) * n))
        sf = ShardedFilter(f, None, dev, world=world, rank=r, seed=FILTER_SEED, block_records=K)
        if toggle:
            sf.enable_trace(8)
            sf.enable_trace(0)
        if trace:
            sf.enable_trace(*trace)
        shards.append(sf)
    ranks = LocalWorld(shards)
    out = dict(states=[], decisions=[], owners=[], errors=[])
    for k, zk in enumerate(zsets, start=1):
        for sf in shards:
            sf.f.set_measurements(zk)
        ranks.step(ctrl, k)
        owners = _owners(shards)
        if owners is not None:
            out["owners"].append(owners.cpu().numpy().copy())
        if settled:
            ranks.flush()
            torch.cuda.synchronize()
            out["states"].append(gathered_store([sf.f for sf in shards]))
        if errors:
            out["errors"].append(sum(sf.f.status_errors() for sf in shards))
        if k > 1 or settled:  # the plan of step k-1 was polled inside step k (settled: step k's, just now)
            assert len(set(sf.last[1] for sf in shards)) == 1
            out["decisions"].append(int(shards[0].last[1]))
    if not settled:
        ranks.flush()
        out["decisions"].append(int(shards[0].last[1]))
    torch.cuda.synchronize()
    out["pending"] = sum(sf.stats["pending_slots"] for sf in shards)
    out["final"] = [sf.f.export() for sf in shards]
    if trace:
        assert all(sf.f.trace_count() == len(zsets) for sf in shards)
        reads = [sf.f.read_trace() for sf in shards]
        tup = isinstance(reads[0], tuple)
        out["records"] = [r[0] if tup else r for r in reads]
        out["maps"] = [r[1] if tup else None for r in reads]
        out["card"] = [r[2] if tup else None for r in reads]
    else:
        assert all(sf.f.trace_count() == 0 for sf in shards)
    for sf in shards:
        sf.f.close()
    return out


def _single_run(c, N, state, states, zsets, trace, **cap):
    """The single context of N particles: before scan k it is loaded with the
    gathered shards of step k-1, then runs a traced phd_step(step=k)."""
    f = _filter(c, N, **cap)
    f.enable_trace(*trace)
    for k, zk in enumerate(zsets, start=1):
        f.load(*(state if k == 1 else states[k - 2]))
        f.set_measurements(zk)
        assert f.step(_control(c), do_predict=True, step=k, readback=False) is None
    got = f.read_trace()
    f.close()
    return got if isinstance(got, tuple) else (got, None, None)


@functools.lru_cache(maxsize=None)
def _case(cid, world, n, K, snap=0, card=False, empty=(), scans=SCANS):
    """The three sharded runs and the single context of one case, computed once
    and shared (never modified)."""
    from phdslam.types import MEASUREMENT
    N = world * n
    c, state, z = _scenario(cid, N, SEED.get((cid, world, n)))
    zsets = [np.zeros(0, MEASUREMENT) if k in empty else z for k in range(1, scans + 1)]
    trace = (scans, snap, card)
    settled = _sharded_run(c, state, zsets, world, n, K, settled=True)
    single = _single_run(c, N, state, settled["states"], zsets, trace)
    free = _sharded_run(c, state, zsets, world, n, K)
    traced = _sharded_run(c, state, zsets, world, n, K, trace=trace)
    return single, free, traced


MAIN = [(2, 2, 48, 4), (2, 3, 48, 0), (3, 3, 48, 1), (2, 3, 700, 2), (3, 2, 1024, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("cid,world,n,K", MAIN)
def test_single_context_chain_moves_the_owner_and_the_decision(gpu, cid, world, n, K):
    """What the main case needs from its scenario, from the single context's
    records alone: the chain both resamples and does not, and the arg-max
    particle is on rank 0 in some scan and on another rank in some other."""
    (rec, _, _), _, _ = _case(cid, world, n, K)
    print("single nEff", [round(float(x), 4) for x in rec["neff"]], "resampled", rec["resampled"].tolist(),
          "map_particle", rec["map_particle"].tolist())
    assert rec["resampled"].any() and not rec["resampled"].all()
    assert (rec["map_particle"] >= n).any(), "the owner is never a rank other than 0: pick another seed"
    assert (rec["map_particle"] < n).any(), "the owner is never rank 0: pick another seed"


@pytest.mark.gpu
@pytest.mark.parametrize("cid,world,n,K", MAIN)
def test_records_equal_single_context(gpu, cid, world, n, K):
    """Five free-running sharded scans.  48 is no multiple of 32 or 64 (the
    cardinality partials and the waves straddle rank edges); 3 x 700 = 2100 is
    three chunks of 1024, the last one partial; 2 x 1024 puts a chunk edge on a
    rank edge; K = 0 sends every record through the overflow path, so pending
    slots are re-updated before the pack."""
    (rec, _, _), free, traced = _case(cid, world, n, K)
    N = world * n
    for k in range(SCANS):
        for r in range(world):
            assert _bits(traced["records"][r][k]) == _bits(rec[k]), (k, r, traced["records"][r][k], rec[k])
        assert int(rec[k]["step"]) == k + 1 and rec[k]["n_live"] == N and rec[k]["n_measure"] == M
        assert int(rec[k]["resampled"]) == traced["decisions"][k], k
        own = traced["owners"][k]
        assert own.sum() == 1 and own[rec[k]["map_particle"] // n] == 1, (k, own)
    assert traced["decisions"] == free["decisions"]
    if K == 0:
        assert traced["pending"] > 0, "no pending slot was re-updated before a pack"
    # the trace did not disturb the chain
    for a, b in zip(traced["final"], free["final"]):
        for x, y in zip(a, b):
            assert _bits(x) == _bits(y)


@pytest.mark.gpu
@pytest.mark.parametrize("cid,world,n,K,snap,card", [(2, 3, 48, 2, 64, False), (2, 3, 48, 2, 4, False),
                                                     (3, 2, 48, 2, 0, True)])
def test_snapshot_and_cardinality_row(gpu, cid, world, n, K, snap, card):
    (rec, maps, rows), _, traced = _case(cid, world, n, K, snap=snap, card=card)
    for r in range(world):
        assert _bits(traced["records"][r]) == _bits(rec)
        if snap:
            assert traced["maps"][r].shape == (SCANS, snap)
            assert _bits(traced["maps"][r]) == _bits(maps)
        if card:
            assert traced["card"][r].shape == rows.shape and rows.shape[0] == SCANS
            assert _bits(traced["card"][r]) == _bits(rows)
    if snap:
        for k in range(SCANS):
            got = min(int(rec[k]["map_size"]), snap)
            assert got > 0 and np.any(maps[k][:got].view(np.uint8))
            assert not np.any(maps[k][got:].view(np.uint8)), "rows beyond the map are zero"
    if snap == 4:
        assert (rec["map_size"] > 4).any(), "the snapshot is shorter than some map"
    if card:
        assert np.any(rows[-1]), "a CPHD update has written the arg-max particle's row"


@pytest.mark.gpu
def test_scan_without_measurements(gpu):
    (rec, _, _), _, traced = _case(2, 3, 64, 0, empty=(2,), scans=4)
    for r in range(3):
        got = traced["records"][r]
        assert got[1]["n_measure"] == 0 and got[1]["resampled"] == 0 and got[0]["n_measure"] == M
        for name in ("expected_pose", "map_pose", "map_particle"):
            assert _bits(got[name]) == _bits(rec[name]), name
        assert _bits(got) == _bits(rec)
    assert traced["decisions"][1] == 0


@pytest.mark.gpu
def test_card_dist_with_expected_map_estimate_is_refused(gpu):
    import torch
    import phdslam
    from phdslam.dist import ShardedFilter
    c, state, z = _scenario(3, 16, map_estimate=2)
    f = _filter(c, 8)
    f.load(*slice_store(state, 0, 8))
    sf = ShardedFilter(f, None, torch.device("cuda", 0), world=2, rank=0, block_records=2)
    with pytest.raises(phdslam.PHDError) as e:
        sf.enable_trace(4, card_dist=True)
    assert e.value.code == phdslam._lib.PHD_E_UNSUPPORTED
    assert f.trace_count() == 0 and sf.trace_block is None
    # the library refuses it too, at the pack
    f.enable_trace(4, card_dist=True)
    block = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    with pytest.raises(phdslam.PHDError) as e:
        f.trace_shard_pack(sf.w_all.data_ptr(), 2, 0, 1, block.data_ptr())
    assert e.value.code == phdslam._lib.PHD_E_UNSUPPORTED and "map_estimate" in str(e.value)
    f.close()


@pytest.mark.gpu
def test_status_errors_summed_over_the_ranks(gpu):
    """survivor_capacity 1 (tests/test_trace.py::test_status_errors_recorded):
    the record's count is the sum of the ranks' status_errors() of the same
    step, taken on an untraced twin run (free-running as the traced one: a
    step's count includes the re-updates of its pending slots in both)."""
    world, n = 2, 48
    c, state, z = _scenario(2, world * n, G=16, M=8)
    twin = _sharded_run(c, state, [z, z], world, n, 4, errors=True, survivor_capacity=1)
    traced = _sharded_run(c, state, [z, z], world, n, 4, trace=(2, 0, False), survivor_capacity=1)
    for k in range(2):
        assert twin["errors"][k] > 0
        for r in range(world):
            assert traced["records"][r][k]["status_errors"] == twin["errors"][k], (k, r)


@pytest.mark.gpu
def test_off_means_off(gpu):
    """enable_trace(8) then enable_trace(0): the state of a run that never touched it."""
    c, state, z = _scenario(3, 3 * 48)
    base = _sharded_run(c, state, [z] * 3, 3, 48, 2)
    got = _sharded_run(c, state, [z] * 3, 3, 48, 2, toggle=True)
    assert got["decisions"] == base["decisions"]
    for a, b in zip(got["final"], base["final"]):
        for x, y in zip(a, b):
            assert _bits(x) == _bits(y)


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [2, 3])
def test_group_rank_trace_matches_sharded_filter(gpu, cid):
    """GroupRank.enable_trace (phd_group_trace_enable: pack, ncclAllGather of
    the blocks, append inside phd_group_step) through RCCL at world 1 against a
    world-1 ShardedFilter and the single context's traced phd_step chain."""
    import torch
    from phdslam.dist import GroupRank, LocalWorld, ShardedFilter
    n, steps = 300, 4
    c, state, z = _scenario(cid, n)
    dev = torch.device("cuda", 0)
    ctrl = _control(c)
    recs = {}
    for kind in ("single", "torch", "cxx"):
        f = _filter(c, n)
        f.load(*state)
        f.set_measurements(z)
        if kind == "single":
            f.enable_trace(steps)
            for k in range(1, steps + 1):
                f.step(ctrl, do_predict=True, step=k, readback=False)
        else:
            if kind == "torch":
                sf = ShardedFilter(f, None, dev, world=1, rank=0, seed=FILTER_SEED, block_records=4)
            else:
                sf = GroupRank(f, None, dev, world=1, rank=0, seed=FILTER_SEED, block_records=4)
            sf.enable_trace(steps)
            run = LocalWorld([sf]) if kind == "torch" else sf
            for k in range(1, steps + 1):
                run.step(ctrl, k)
            run.flush()
            torch.cuda.synchronize()
        assert f.trace_count() == steps
        recs[kind] = f.read_trace()
        if kind == "cxx":
            sf.close()
        f.close()
    assert recs["single"]["resampled"].any()
    assert _bits(recs["cxx"]) == _bits(recs["torch"])
    assert _bits(recs["cxx"]) == _bits(recs["single"])
