"""The mixed static + dynamic feature model (feature_model 2, PHD) on the
sharded multi-GPU step.

The contract is the static model's (tests/test_gpu_parity.py::
test_sharded_step_matches_single_context): after every step the particles
held across the ranks equal, bit for bit and up to order, those of a single
context of world * n particles — poses, log-weights, every static map and
every dynamic map.  The update is per particle and deterministic and the
plan's sums are canonical, so every comparison below is byte equality; no
tolerance is involved.

Every rank is emulated on one device: ShardedFilter(f, None, dev, world=…,
rank=…) under phdslam.dist.LocalWorld, which serves the collectives as device
copies between the ranks' buffers.  Capacities as
tests/test_gpu_mixed.py: cap 128, dcap 64, M 32, K 4096; resampleThresh 1.0
(a resample every step with measurements).

What the cases probe (the three hazards of the dynamic predict):
(a) a slab several particles share — copy on write after a resample, several
slots of one record — is predicted once per predict sub-step (every run
resamples every step, so shared slabs are the rule); (b) subdividePredict = 2
predicts twice per step, late records too; (c) an empty scan still predicts,
the pending slots' records included.
"""
import ctypes

import numpy as np
import pytest

from phdslam.scenario import mixed_config, mixed_scenario
from sharded_helpers import gathered_mixed, slice_mixed

CAP, DCAP, MCAP, KCAP = 128, 64, 32, 4096
S = 0x5eed


def _filter(cfg, n, dcap=DCAP, seed=S):
    import phdslam
    f = phdslam.PHDFilter(n, cfg, map_capacity=CAP, max_measurements=MCAP, candidate_capacity=KCAP,
                          survivor_capacity=256)
    f.set_seed(seed)
    if dcap:
        f.enable_dynamic(dcap)
    return f


# ------------------------------------------------------------------ CPU

@pytest.mark.parametrize("cap,cn,dcap", [(128, 0, 64), (128, 0, 0), (16, 9, 0), (5, 0, 3), (6, 0, 64), (128, 0, 1),
                                         (7, 3, 5)])
def test_record_bytes_follow_the_documented_layout(built, cap, cn, dcap):
    """The record-size arithmetic (record_words_mixed, phd_records.h, through
    phd_record_layout_bytes; no device): the static / CPHD record is
    4 * (8 + 7 cap + 2 cn) bytes as it always was; with a dynamic capacity that
    is padded to 16 bytes, then [dsize | 3 reserved | 21 * dcap floats], padded
    to 16 bytes again (include/phd_capi.h)."""
    import phdslam
    from phdslam._lib import SIGNATURES
    assert "phd_record_layout_bytes" in SIGNATURES
    got = ctypes.c_size_t()
    assert phdslam.lib().phd_record_layout_bytes(cap, cn, dcap, ctypes.byref(got)) == 0
    static = 4 * (8 + 7 * cap + 2 * cn)
    if dcap == 0:
        assert got.value == static
    else:
        dyn_at = (static + 15) // 16 * 16
        want = (dyn_at + 16 + 4 * 21 * dcap + 15) // 16 * 16
        assert got.value == want and got.value % 16 == 0 and got.value >= static + 4 + 84 * dcap
    assert phdslam.lib().phd_record_layout_bytes(-1, 0, 0, ctypes.byref(got)) == phdslam._lib.PHD_E_ARG


# ------------------------------------------------------------------ GPU helpers

def _load(f, poses, lw, sm, sof, dm, dof):
    f.load(poses, lw, sm, sof)
    f.load_dynamic(dm, dof)


def _assert_same_particles(a, b, label):
    """Two stores equal up to the order of the particles: poses matched by
    sort, then log-weights and both maps of matched particles, bytes."""
    ap, aw, asm, aso, adm, ado = a
    bp, bw, bsm, bso, bdm, bdo = b
    assert len(ap) == len(bp)
    key = lambda P: np.lexsort((P["ptheta"], P["py"], P["px"]))
    ka, kb = key(ap), key(bp)
    assert ap[ka].tobytes() == bp[kb].tobytes(), f"{label}: particle poses differ"
    assert aw[ka].tobytes() == bw[kb].tobytes(), f"{label}: log-weights differ"
    for i, j in zip(ka, kb):
        assert asm[aso[i]:aso[i + 1]].tobytes() == bsm[bso[j]:bso[j + 1]].tobytes(), \
            f"{label}: static map of particle {i} differs"
        assert ado[i + 1] - ado[i] == bdo[j + 1] - bdo[j], \
            f"{label}: dynamic map of particle {i}: {ado[i + 1] - ado[i]} vs {bdo[j + 1] - bdo[j]} components"
        assert adm[ado[i]:ado[i + 1]].tobytes() == bdm[bdo[j]:bdo[j + 1]].tobytes(), \
            f"{label}: dynamic map of particle {i} differs"


def _sharded_vs_single(world, n, K, steps=3, ackerman=False, empty_steps=(), subdivide=1, seed=None, after=None):
    """`world` emulated ranks of n particles against a single context of
    world * n stepped from the gathered shards of the previous step (predict_*,
    update, normalize, resample), about 30 static and 10 dynamic components per
    particle and 10 measurements; equal after every step.  after(shards): called
    on the settled shards after the last step.  Returns (pending, moved)."""
    import torch
    from phdslam.dist import LocalWorld, ShardedFilter
    N = world * n
    cfg = mixed_config(motionType=1 if ackerman else 0, resampleThresh=1.0, subdividePredict=subdivide)
    if ackerman:  # (the defaults leave the vehicle's geometry and its control noise zero)
        cfg.l, cfg.h, cfg.a, cfg.b, cfg.stdEncoder, cfg.stdAlpha = 1.415, 0.38, 1.89, 0.5, 1.0, 0.034907
    kw = {} if seed is None else {"seed": seed}
    poses, sm, sof, dm, dof, z = mixed_scenario(cfg, N, 30, 10, 10, **kw)
    lw = np.full(N, -np.log(N), np.float32)
    ctrl = (2.0, 0.05) if ackerman else None
    dev = torch.device("cuda", 0)
    single = _filter(cfg, N)
    _load(single, poses, lw, sm, sof, dm, dof)
    shards = []
    for r in range(world):
        f = _filter(cfg, n)
        f.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        _load(f, *slice_mixed(poses, lw, sm, sof, dm, dof, r * n, (r + 1) * n))
        shards.append(ShardedFilter(f, None, dev, world=world, rank=r, seed=S, block_records=K))
    ranks = LocalWorld(shards)
    z_empty = z[:0]
    prev = None
    for k in range(1, steps + 1):
        zk = z_empty if k in empty_steps else z
        if prev is not None:  # predict noise is keyed by the global particle index: the gathered order
            _load(single, *prev)
        for j in range(subdivide):  # (main.cpp:1248-1254: subdividePredict calls of phdPredict)
            if ackerman:
                single.predict_ackerman(*ctrl, noise=None, step=k * subdivide + j)
            else:
                single.predict_cv(noise=None, step=k * subdivide + j)
        single.set_measurements(zk)
        single.update()
        single.normalize()
        if len(zk):
            single.resample(uniforms=None, step=k)
        for sf in shards:
            sf.f.set_measurements(zk)
        ranks.step(ctrl, k)
        ranks.flush()  # the store is final
        torch.cuda.synchronize()
        if k in empty_steps:  # (no update: no resample)
            assert not any(sf.last[1] for sf in shards)
        else:
            assert all(sf.last[1] for sf in shards)
        prev = gathered_mixed([sf.f for sf in shards])
        _assert_same_particles((*single.export(), *single.export_dynamic()), prev, f"step {k}")
    pending = sum(sf.stats["pending_slots"] for sf in shards)
    moved = sum(sf.stats["migrated"] for sf in shards)
    if after is not None:
        after(cfg, shards)
    single.close()
    for sf in shards:
        sf.f.close()
    return pending, moved


# ------------------------------------------------------------------ 1. records

def _round_trip_input(cfg, n):
    """8 particles, about 6 dynamic components each; particle 2's dynamic map
    is empty, particle 5's holds exactly DCAP components."""
    poses, sm, sof, dm, dof, z = mixed_scenario(cfg, n, 30, 6, 10, seed=4242)
    full = mixed_scenario(cfg, n, 30, DCAP, 10, seed=4243)[3][5 * DCAP:6 * DCAP]
    parts = [dm[dof[p]:dof[p + 1]] for p in range(n)]
    parts[2] = dm[:0]
    parts[5] = full
    dof = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int32)
    return poses, sm, sof, np.concatenate(parts), dof, z


@pytest.mark.gpu
def test_record_round_trip(gpu):
    """phd_pack_particles of a mixed context -> phd_unpack_particles into a
    second one: poses, log-weights, static and dynamic maps arrive bit for bit
    (an empty dynamic map, a full one, two particles sharing a slab after a
    resample with given parents); one update with the same scan on both is
    equal again — the second context reads its priors from the sets X.  The
    record of a static context of the same capacities is 4 * (8 + 7 cap) bytes
    as before, the mixed one larger by the dynamic part phd_capi.h documents."""
    import torch
    n = 8
    cfg = mixed_config()
    poses, sm, sof, dm, dof, z = _round_trip_input(cfg, n)
    lw = np.random.default_rng(3).normal(-8, 3, n).astype(np.float32)
    dev = torch.device("cuda", 0)
    a, b = _filter(cfg, n), _filter(cfg, n)
    _load(a, poses, lw, sm, sof, dm, dof)
    # (other poses, weights and dynamic maps: everything must be overwritten)
    _load(b, poses[::-1].copy(), lw[::-1].copy(), sm, sof, dm[:0], np.zeros(n + 1, np.int32))
    parents = torch.tensor([0, 1, 2, 3, 3, 5, 6, 7], dtype=torch.int32, device=dev)
    a.apply_resample(parents.data_ptr(), -2.5)
    a.synchronize()
    static = _filter(mixed_config(featureModel=0), n, dcap=0)
    assert static.record_bytes() == 4 * (8 + 7 * CAP)
    static.close()
    rb = a.record_bytes()
    dyn_at = (4 * (8 + 7 * CAP) + 15) // 16 * 16
    assert rb == (dyn_at + 16 + 4 * 21 * DCAP + 15) // 16 * 16 and rb == b.record_bytes()
    rec = torch.zeros(n * rb, dtype=torch.uint8, device=dev)
    idx = torch.arange(n, dtype=torch.int32, device=dev)
    a.pack(idx.data_ptr(), n, rec.data_ptr())
    torch.cuda.synchronize()  # (the two contexts run on their own streams)
    b.unpack(rec.data_ptr(), idx.data_ptr(), n)

    def state(f):
        return (*f.export(), *f.export_dynamic())

    def same(x, y, label):
        for u, v, name in zip(x, y, ("poses", "log-weights", "static maps", "static offsets", "dynamic maps",
                                     "dynamic offsets")):
            assert u.tobytes() == v.tobytes(), f"{label}: {name} differ"

    sa = state(a)
    np.testing.assert_array_equal(np.diff(sa[5]), [6, 6, 0, 6, 6, DCAP, 6, 6])
    assert sa[4][sa[5][3]:sa[5][4]].tobytes() == sa[4][sa[5][4]:sa[5][5]].tobytes()  # 3 and 4 share a slab
    same(sa, state(b), "after unpack")
    a.update(z)
    b.update(z)
    same(state(a), state(b), "after one update")
    a.close()
    b.close()


# ------------------------------------------------------------------ 2-5. the sharded step

def _check_readers(cfg, shards):
    """Each rank's dynamic_sizes() and expected_map_dynamic(), read through
    the slab references into the sets X, against a fresh context of n particles
    loaded with that rank's exported store."""
    for sf in shards:
        f = sf.f
        st = (*f.export(), *f.export_dynamic())
        fresh = _filter(cfg, f.n)
        _load(fresh, *st)
        assert f.dynamic_sizes().tobytes() == fresh.dynamic_sizes().tobytes() == np.diff(st[5]).astype(np.int32).tobytes()
        eap, ref = f.expected_map_dynamic(), fresh.expected_map_dynamic()
        assert len(eap) > 0 and eap.tobytes() == ref.tobytes()
        fresh.close()


@pytest.mark.gpu
@pytest.mark.parametrize("world,n,K,ackerman", [(2, 24, 4, False), (3, 16, 1, False), (3, 16, 0, False),
                                                (3, 16, 0, True)])
def test_sharded_step_matches_single_context(gpu, world, n, K, ackerman):
    """Three steps, CV motion with device noise (and K = 0 once more with
    Ackerman): records in the fixed blocks, beyond them (K = 1), and all of
    them late (K = 0: every record's dynamic slab of X is predicted on its own
    and its slots re-updated)."""
    pending, moved = _sharded_vs_single(world, n, K, ackerman=ackerman)
    assert moved > 0  # (conditions on the input: another seed if one fails)
    if K == 0:
        assert pending > 0


@pytest.mark.gpu
@pytest.mark.parametrize("K", [0, 2])
def test_sharded_step_with_empty_scan(gpu, K):
    """Four steps, the second with an empty scan: no update and no resample
    that step, but the dynamic maps are predicted — the records that arrive
    late for that step (K = 0) included."""
    pending, moved = _sharded_vs_single(3, 16, K, steps=4, empty_steps=(2,))
    assert moved > 0
    if K == 0:
        assert pending > 0


@pytest.mark.gpu
def test_sharded_step_subdivided_predict(gpu):
    """subdividePredict = 2: two dynamic predicts per step, each slab once per
    sub-step, late records predicted twice before their re-update."""
    pending, moved = _sharded_vs_single(3, 16, 0, subdivide=2)
    assert moved > 0 and pending > 0


@pytest.mark.gpu
def test_readers_after_migration(gpu):
    """dynamic_sizes and expected_map_dynamic on ranks that hold migrated slabs
    (after the last step's receive every record's particles refer to the sets X)."""
    pending, moved = _sharded_vs_single(2, 24, 4, after=_check_readers)
    assert moved > 0


# ------------------------------------------------------------------ 6. the C++ host

@pytest.mark.gpu
def test_group_rank_matches_sharded_filter(gpu):
    """GroupRank (the C++ host's per-process rank, one C call per step) at world
    1 on a mixed context against ShardedFilter at world 1, three steps: the same
    store, bytes.  At world 1 the exchange is skipped, so this checks that the
    C++ host accepts the model and the record size, no more."""
    import torch
    from phdslam.dist import GroupRank, LocalWorld, ShardedFilter
    n, steps = 32, 3
    cfg = mixed_config(motionType=0, resampleThresh=1.0)
    poses, sm, sof, dm, dof, z = mixed_scenario(cfg, n, 30, 10, 10)
    lw = np.full(n, -np.log(n), np.float32)
    dev = torch.device("cuda", 0)
    out = []
    for kind in ("torch", "cxx"):
        f = _filter(cfg, n)
        _load(f, poses, lw, sm, sof, dm, dof)
        f.set_measurements(z)
        if kind == "torch":
            sf = ShardedFilter(f, None, dev, world=1, rank=0, block_records=4)
        else:
            sf = GroupRank(f, None, dev, world=1, rank=0, block_records=4)
        run = LocalWorld([sf]) if kind == "torch" else sf
        for k in range(1, steps + 1):
            run.step(None, k)
        run.flush()
        torch.cuda.synchronize()
        f.check_errors()
        out.append(((*f.export(), *f.export_dynamic()), dict(sf.stats)))
        if kind == "cxx":
            sf.close()
        f.close()
    (a, sa), (b, sb) = out
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert sa["resamples"] == sb["resamples"] == steps


# ------------------------------------------------------------------ 7. refusals

def _plan_raises(cfg, code, dcap_after=None):
    """A world-2 ShardedFilter's plan on a context of `cfg` raises `code`; the
    send buffers keep the pattern they were filled with."""
    import torch
    import phdslam
    n = 8
    poses, sm, sof, dm, dof, z = mixed_scenario(mixed_config(), n, 12, 4, 6)
    dev = torch.device("cuda", 0)
    f = _filter(cfg, n)
    f.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    _load(f, poses, np.full(n, -np.log(2 * n), np.float32), sm, sof, dm, dof)
    f.set_measurements(z)
    from phdslam.dist import ShardedFilter
    sf = ShardedFilter(f, None, dev, world=2, rank=0, seed=S, block_records=2)
    if dcap_after:
        f.enable_dynamic(dcap_after)
    sf.send_blocks.fill_(0xA5)
    sf.ovf_send.fill_(0xA5)
    sf.w_all.fill_(float(-np.log(2 * n)))
    with pytest.raises(phdslam.PHDError) as e:
        sf.plan(1)
    torch.cuda.synchronize()
    assert e.value.code == code, str(e.value)
    assert bool((sf.send_blocks == 0xA5).all()) and bool((sf.ovf_send == 0xA5).all())
    f.close()
    return str(e.value)


@pytest.mark.gpu
def test_refusals_kept(gpu):
    """Mixed + CPHD and mixed + n_predict_particles 2 still refuse the sharded
    plan (PHD_E_UNSUPPORTED); a dynamic capacity changed after the ShardedFilter
    sized its buffers is PHD_E_ARG, with nothing written."""
    from phdslam._lib import PHD_E_ARG, PHD_E_UNSUPPORTED
    _plan_raises(mixed_config(filterType=1), PHD_E_UNSUPPORTED)
    assert "n_predict_particles" in _plan_raises(mixed_config(nPredictParticles=2), PHD_E_UNSUPPORTED)
    assert "phd_record_bytes" in _plan_raises(mixed_config(), PHD_E_ARG, dcap_after=96)
