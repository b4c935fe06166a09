"""The EAP expected maps of the mixed static + dynamic model (feature_model 2)
on the sharded filter: phd_eap_dyn_shard_count / _block_bytes / _pack,
phd_expected_map_dynamic_blocks, ShardedFilter.expected_map_dynamic,
GroupRank.expected_map_dynamic, and the static map's blocks form
(ShardedFilter.expected_map, GroupRank.expected_map) on a mixed context.

The contract: every rank returns, byte for byte and in the same emission
order, what PHDFilter.expected_map_dynamic (the static map: expected_map)
returns on a single mixed context of world * n particles loaded with the
ranks' settled stores in rank order.  The dynamic reduce is a stable sort and
one workgroup (k_eap4_merge), so its result depends on the concatenated
component array alone: every comparison below is byte equality of the
returned arrays; no tolerance is involved.

Emulated ranks on one device (phdslam.dist.LocalWorld), with the helpers of
tests/test_gpu_mixed_sharded.py (the mixed filters, stores and the stepped
chain).  The hand-built cases drive the phases (eap_dyn_count, eap_dyn_pack,
eap_dyn_finish) with the all-gather as torch.cat; the chains run
ShardedFilter's own expected-map phases (LocalWorld.expected_map_dynamic).
"""
import ctypes

import numpy as np
import pytest

import test_eap_sharded as tes
import test_gpu_mixed_sharded as tms

from phdslam.scenario import mixed_config, mixed_scenario
from sharded_helpers import gathered_mixed, slice_mixed

DCAP = 16  # dynamic capacity of the hand-built stores
N = 8      # their particles per rank
EAP1, EAP4 = 0x31504145, 0x34504145


# ------------------------------------------------------------------ CPU

DYN_SYMBOLS = ("phd_eap_dyn_shard_count", "phd_eap_dyn_shard_block_bytes", "phd_eap_dyn_shard_pack",
               "phd_expected_map_dynamic_blocks")


def test_dynamic_eap_symbols_exported(built):
    from phdslam._lib import SIGNATURES
    names = tes.tts._exported("libphdslam.so")
    for sym in DYN_SYMBOLS:
        assert sym in names, sym
        assert sym in SIGNATURES, sym
    assert "phd_group_expected_map_dynamic" in tes.tts._exported("libphdslam_group.so")


@pytest.mark.parametrize("k_max", [0, 1, 7, 1000, (1 << 33) + 5])
def test_dyn_block_bytes_follow_the_documented_layout(built, k_max):
    """header 64 B | 21 float fields of stride K_max, rounded up to 16
    (include/phd_capi.h); pure arithmetic, no device."""
    import phdslam
    got = ctypes.c_size_t()
    assert phdslam.lib().phd_eap_dyn_shard_block_bytes(k_max, ctypes.byref(got)) == 0
    assert got.value == (64 + 84 * k_max + 15) // 16 * 16 and got.value % 16 == 0


def test_dyn_block_bytes_rejects_a_negative_stride(built):
    import phdslam
    got = ctypes.c_size_t(12345)
    assert phdslam.lib().phd_eap_dyn_shard_block_bytes(-1, ctypes.byref(got)) == phdslam._lib.PHD_E_ARG
    assert phdslam.lib().phd_last_error()
    assert got.value == 12345


# ------------------------------------------------------------------ GPU helpers

def _bits(a):
    return np.ascontiguousarray(a).tobytes()


_same = tes._same


def _dyn_components(rng, K, lo=-18.0, hi=18.0):
    """K Gaussian4D components drawn as phdslam.scenario.mixed_scenario draws
    them, positions uniform in [lo, hi]^2 (far apart: few merges)."""
    from phdslam.types import GAUSSIAN4D
    d = np.zeros(K, GAUSSIAN4D)
    d["mean"] = np.concatenate([rng.uniform(lo, hi, (K, 2)), rng.normal(0, 1.5, (K, 2))], 1).astype(np.float32)
    cov = np.zeros((K, 4, 4))
    cov[:, 0, 0] = rng.uniform(0.05, 0.3, K)
    cov[:, 1, 1] = rng.uniform(0.05, 0.3, K)
    cov[:, 2, 2] = rng.uniform(0.2, 1.0, K)
    cov[:, 3, 3] = rng.uniform(0.2, 1.0, K)
    cov[:, 0, 2] = cov[:, 2, 0] = rng.uniform(-0.02, 0.02, K)
    cov[:, 1, 3] = cov[:, 3, 1] = rng.uniform(-0.02, 0.02, K)
    d["cov"] = cov.transpose(0, 2, 1).reshape(K, 16)
    d["weight"] = rng.uniform(0.2, 1.0, K)
    return d


def _store(cfg, lw, dm, dsizes, seed=77):
    """A rank's store (poses, lw, sm, sof, dm, dof): three static components
    per particle beside the given dynamic maps."""
    n = len(dsizes)
    poses, sm, sof, _, _, _ = mixed_scenario(cfg, n, 3, 1, 4, seed=seed)
    dof = np.concatenate([[0], np.cumsum(dsizes)]).astype(np.int32)
    assert dof[-1] == len(dm) and len(lw) == n and max(dsizes) <= DCAP
    return poses, np.asarray(lw, np.float32), sm, sof, dm, dof


def _concat(stores):
    def offs(i):
        o = [0]
        for s in stores:
            o.extend((np.asarray(s[i][1:]) + o[-1]).tolist())
        return np.asarray(o, np.int32)

    return (np.concatenate([s[0] for s in stores]), np.concatenate([s[1] for s in stores]),
            np.concatenate([s[2] for s in stores]), offs(3), np.concatenate([s[4] for s in stores]), offs(5))


def _shards(cfg, stores, dcap=DCAP):
    import torch
    from phdslam.dist import ShardedFilter
    dev = torch.device("cuda", 0)
    shards = []
    for r, s in enumerate(stores):
        f = tms._filter(cfg, len(s[0]), dcap=dcap)
        f.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        tms._load(f, *s)
        shards.append(ShardedFilter(f, None, dev, world=len(stores), rank=r, seed=tms.S, block_records=1))
    return shards


def _phases(shards, k_max=None):
    """count, pack, all-gather (torch.cat), finish on every emulated rank."""
    import torch
    counts = [sf.eap_dyn_count() for sf in shards]
    k_max = max(counts) if k_max is None else k_max
    for sf in shards:
        sf.eap_dyn_pack(k_max)
    blocks = torch.cat([sf.eap_dyn_block for sf in shards])
    eaps = []
    for sf in shards:
        sf.eap_dyn_blocks.copy_(blocks)
        eaps.append(sf.eap_dyn_finish(k_max, sum(counts)))
    return eaps, counts, k_max, blocks


def _close(shards):
    for sf in shards:
        sf.f.close()


def _single(cfg, state, dcap=DCAP):
    """(expected_map_dynamic, expected_map) of one mixed context holding `state`."""
    f = tms._filter(cfg, len(state[0]), dcap=dcap)
    tms._load(f, *state)
    out = f.expected_map_dynamic().copy(), f.expected_map().copy()
    f.close()
    return out


def _held(cfg, stores, k_max=None):
    """The sharded dynamic map of `stores` on every rank, held to the single
    context's.  Returns (rank 0's map, counts, the single context's map)."""
    shards = _shards(cfg, stores)
    eaps, counts, k_max, _ = _phases(shards, k_max)
    _close(shards)
    assert counts == [int(s[5][-1]) for s in stores]
    single, _ = _single(cfg, _concat(stores))
    for r in range(len(stores)):
        _same(eaps[r], single, f"rank {r} vs single context")
    return eaps[0], counts, single


def _uneven_stores(cfg):
    """World 3, n 8: rank 1 holds no dynamic component at all; rank 0 a
    particle with exactly DCAP components and one with none."""
    rng = np.random.default_rng(21)
    sizes = [np.array([DCAP, 0, 3, 5, 1, 2, 4, 6]), np.zeros(N, np.int64), np.array([2, 3, 1, 0, 4, 5, 7, 8])]
    landmarks = _dyn_components(rng, 12)
    stores = []
    for r, s in enumerate(sizes):
        lw = rng.normal(-np.log(3 * N), 0.4, N)
        # every component a jittered copy of one of 12 landmarks: merges cross the ranks
        k = int(s.sum())
        dm = landmarks[rng.integers(0, len(landmarks), k)].copy()
        dm["mean"] += rng.normal(0, 0.1, (k, 4)).astype(np.float32)
        dm["weight"] = rng.uniform(0.2, 1.0, k)
        stores.append(_store(cfg, lw, dm, s, seed=77 + r))
    return stores


# ------------------------------------------------------------------ 1. uneven stores

@pytest.mark.gpu
def test_uneven_ranks(gpu):
    """Hand-built uneven stores, the phases driven by hand.  The counts are
    chosen so that both paths of the concatenation run: with K_max 37 and 67
    components in all, field f of rank 0 (offset 0) leaves its block at float
    residue f mod 4 and lands at 3 f mod 4 — equal for the even fields (16
    bytes per lane), different for the odd ones (4 bytes per lane) — and rank
    2's offset 37 is 1 mod 4."""
    cfg = mixed_config()
    stores = _uneven_stores(cfg)
    lws = np.concatenate([s[1] for s in stores])
    assert len(set(lws.tolist())) == len(lws), "distinct log-weights"
    counts = [int(s[5][-1]) for s in stores]
    assert counts == [37, 0, 30]
    k_max, K = max(counts), sum(counts)
    offs = np.concatenate([[0], np.cumsum(counts)])
    assert offs[0] % 4 != offs[2] % 4
    paths = set()
    for r in (0, 2):
        for f in range(21):
            same = (f * k_max) % 4 == (f * K + offs[r]) % 4
            lead = (4 - (f * k_max) % 4) % 4
            paths.add((same, same and counts[r] - lead >= 4))
    assert (True, True) in paths and (False, False) in paths  # whole quads moved, and the 4-byte path
    eap, got, single = _held(cfg, stores)
    assert got == counts
    assert 0 < len(eap) < K, "some components merged, not all"


# ------------------------------------------------------------------ 2. the global greedy

@pytest.mark.gpu
def test_global_greedy_is_needed(gpu):
    """Two ranks hold components of the same landmarks (mixed_scenario jitters
    every particle's copy of six landmarks by 0.2, well inside minSeparation):
    the sharded map equals the single context's, and the ranks' own
    expected_map_dynamic outputs, concatenated, do not."""
    cfg = mixed_config()
    poses, sm, sof, dm, dof, _ = mixed_scenario(cfg, 2 * N, 3, 6, 4, seed=4711)
    lw = np.random.default_rng(5).normal(-np.log(2 * N), 0.4, 2 * N).astype(np.float32)
    stores = [slice_mixed(poses, lw, sm, sof, dm, dof, r * N, (r + 1) * N) for r in range(2)]
    shards = _shards(cfg, stores, dcap=DCAP)
    per_rank = np.concatenate([sf.f.expected_map_dynamic() for sf in shards])
    eaps, counts, _, _ = _phases(shards)
    _close(shards)
    single, _ = _single(cfg, _concat(stores))
    assert counts == [6 * N, 6 * N] and 0 < len(single) < sum(counts)
    for r in range(2):
        _same(eaps[r], single, f"rank {r} vs single context")
    assert len(per_rank) > len(single) and _bits(per_rank) != _bits(single), "the input does not discriminate"


# ------------------------------------------------------------------ 3. ties

@pytest.mark.gpu
def test_ties_across_ranks(gpu):
    """Equal log-weights everywhere, and equal-weight neighbours X (rank 0), Y
    (rank 1), Z (rank 0) 0.5 apart in a row (d(X, Y) = d(Y, Z) = 2.5 < 4 =
    minSeparation < 10 = d(X, Z)): in rank order X is the seed and absorbs Y
    alone; with the shards swapped Y comes first and absorbs both.  The
    concatenation index decides, on the ranks as on the single context."""
    cfg = mixed_config()
    rng = np.random.default_rng(3)
    per = 4
    stores = []
    for r in range(2):
        dm = _dyn_components(rng, N * per, lo=-19.0, hi=-5.0)
        stores.append(_store(cfg, np.full(N, -np.log(2 * N)), dm, np.full(N, per), seed=90 + r))
    for store, slot, x in ((0, 5, 10.0), (1, 9, 10.5), (0, 22, 11.0)):
        g = stores[store][4][slot]
        g["weight"] = 0.7
        g["mean"] = (x, 3.0, 0.5, -0.5)
        g["cov"] = np.diag([0.1, 0.1, 0.5, 0.5]).astype(np.float32).reshape(16)
        stores[store][4][slot] = g
    # the tie: equal component weight and equal log-weight on different ranks
    assert stores[0][4][5]["weight"] == stores[1][4][9]["weight"] and stores[0][1][5 // per] == stores[1][1][9 // per]
    a, _, single_a = _held(cfg, stores)
    b, _, single_b = _held(cfg, stores[::-1])
    assert len(a) == len(b) + 1 and _bits(a) != _bits(b), "swapping the shards changes the map"
    near = a[(np.abs(a["mean"][:, 1] - 3.0) < 1e-3)]
    assert len(near) == 2, "X with Y, and Z on its own"


# ------------------------------------------------------------------ 4. the stride

@pytest.mark.gpu
def test_stride_independence(gpu):
    """K_max the largest count, one more and five more: the stride is K_max,
    never K_r, the padding is never read, the output bytes are the same."""
    cfg = mixed_config()
    stores = _uneven_stores(cfg)
    k = max(int(s[5][-1]) for s in stores)
    a, _, _ = _held(cfg, stores, k_max=k)
    for pad in (k + 1, k + 5):
        b, _, _ = _held(cfg, stores, k_max=pad)
        _same(a, b, f"K_max {k} vs {pad}")


# ------------------------------------------------------------------ 5. nothing to reduce

@pytest.mark.gpu
def test_all_ranks_empty(gpu):
    import torch
    import phdslam
    from phdslam.types import GAUSSIAN4D
    cfg = mixed_config()
    stores = [_store(cfg, np.full(N, -np.log(2 * N)), np.zeros(0, GAUSSIAN4D), np.zeros(N, np.int64)) for _ in range(2)]
    shards = _shards(cfg, stores)
    eaps, counts, k_max, blocks = _phases(shards)
    assert counts == [0, 0] and k_max == 0 and blocks.numel() == 2 * 64
    assert all(len(e) == 0 for e in eaps)
    # the C call itself: PHD_OK, n_out 0, out untouched
    out = np.frombuffer(bytes([0xA5]) * (4 * GAUSSIAN4D.itemsize), np.uint8).copy()
    nout = ctypes.c_long(-1)
    sf = shards[0]
    sf.eap_dyn_blocks.copy_(blocks)
    rc = phdslam.lib().phd_expected_map_dynamic_blocks(sf.f.handle, ctypes.c_void_p(sf.eap_dyn_blocks.data_ptr()), 2, 0,
                                                       out.ctypes.data_as(ctypes.c_void_p), 4, ctypes.byref(nout))
    torch.cuda.synchronize()
    assert rc == phdslam._lib.PHD_OK and nout.value == 0 and bool((out == 0xA5).all())
    _close(shards)
    single, _ = _single(cfg, _concat(stores))
    assert len(single) == 0


# ------------------------------------------------------------------ 6. after migration

@pytest.mark.gpu
@pytest.mark.parametrize("world,n,K", [(2, 24, 4), (3, 16, 0)])
def test_after_migration(gpu, monkeypatch, world, n, K):
    """Three sharded steps of the mixed model (a resample every step; K = 0:
    every record late, its slabs in the sets X), then both expected maps of
    the filter from ShardedFilter on every rank (LocalWorld), against a fresh
    single mixed context loaded with the gathered stores."""
    from phdslam.dist import LocalWorld
    sent_before = []
    steps = []
    step = LocalWorld.step

    def counting_step(ranks, ctrl, k):
        sent_before[:] = [sf.stats["records"] for sf in ranks.shards]  # the steps before this one (each is polled in turn)
        steps.append(k)
        return step(ranks, ctrl, k)

    monkeypatch.setattr(LocalWorld, "step", counting_step)
    seen = {}

    def after(cfg, shards):
        gathered = gathered_mixed([sf.f for sf in shards])
        single = tms._filter(cfg, world * n)
        tms._load(single, *gathered)
        want_dyn, want_static = single.expected_map_dynamic().copy(), single.expected_map().copy()
        single.close()
        ranks = LocalWorld(shards)
        got = list(zip(ranks.expected_map_dynamic(), ranks.expected_map()))
        assert 0 < len(want_dyn) < int(gathered[5][-1]) and 0 < len(want_static) < int(gathered[3][-1])
        for r in range(world):
            _same(got[r][0], want_dyn, f"rank {r}: dynamic map vs single context")
            _same(got[r][1], want_static, f"rank {r}: static map vs single context")
        # the last step's plan moved records: after its receive (no update since) the
        # slots they fed hold slab references into the sets X
        seen["last_sent"] = [sf.stats["records"] - b for sf, b in zip(shards, sent_before)]

    pending, moved = tms._sharded_vs_single(world, n, K, after=after)
    assert steps == [1, 2, 3]
    assert moved > 0
    if K == 0:
        assert pending > 0
    assert sum(seen["last_sent"]) > 0, "no rank holds a slab reference into set X: pick another seed"


# ------------------------------------------------------------------ 7. the C++ host

@pytest.mark.gpu
def test_group_rank_expected_maps_match_filter(gpu):
    """GroupRank.expected_map_dynamic (phd_group_expected_map_dynamic: the
    settle, ncclAllGather of the counts and of the blocks, the reduce) and
    GroupRank.expected_map through RCCL at world 1, on a mixed context after
    three steps, equal PHDFilter's maps of the same store."""
    import torch
    from phdslam.dist import GroupRank
    n, steps = 32, 3
    cfg = mixed_config(motionType=0, resampleThresh=1.0)
    poses, sm, sof, dm, dof, z = mixed_scenario(cfg, n, 30, 10, 10)
    f = tms._filter(cfg, n)
    tms._load(f, poses, np.full(n, -np.log(n), np.float32), sm, sof, dm, dof)
    f.set_measurements(z)
    g = GroupRank(f, None, torch.device("cuda", 0), world=1, rank=0, block_records=4)
    for k in range(1, steps + 1):
        g.step(None, k)
    got_dyn = g.expected_map_dynamic()  # settles the open plan
    got_static = g.expected_map()
    want_dyn, want_static = f.expected_map_dynamic().copy(), f.expected_map().copy()
    again = g.expected_map_dynamic()
    g.close()
    f.close()
    assert len(want_dyn) > 0 and len(want_static) > 0
    _same(got_dyn, want_dyn, "group vs filter, dynamic map")
    _same(got_static, want_static, "group vs filter, static map")
    _same(again, want_dyn, "second call")


# ------------------------------------------------------------------ 8. refusals

def _state(f):
    return (*f.export(), *f.export_dynamic())


@pytest.mark.gpu
def test_refusals_leave_the_blocks_and_the_stores_unchanged(gpu):
    import torch
    import phdslam
    E_ARG = phdslam._lib.PHD_E_ARG
    refused = tes._assert_refused
    cfg = mixed_config()
    stores = _uneven_stores(cfg)[::2]
    shards = _shards(cfg, stores)
    before = [_state(sf.f) for sf in shards]
    eaps, counts, k_max, blocks = _phases(shards)
    total = sum(counts)
    sf = shards[0]
    words = sf.eap_dyn_block.numel() // 4
    held = sf.eap_dyn_block.clone()

    def header(word, value):
        bad = blocks.clone()
        bad.view(torch.int32)[word] = value
        sf.eap_dyn_blocks.copy_(bad)

    # a store larger than the stride is refused by the pack, the block untouched
    refused(lambda: sf.f.eap_dyn_shard_pack(counts[0] - 1, sf.eap_dyn_block.data_ptr()), E_ARG, "K_max")
    # headers: a count above K_max, another n, the static map's layout word
    header(words + 1, k_max + 1)
    refused(lambda: sf.eap_dyn_finish(k_max, total), E_ARG, "rank 1 is refused: its component count exceeds K_max")
    header(4, N + 1)
    refused(lambda: sf.eap_dyn_finish(k_max, total), E_ARG, "rank 0 is refused: its particle count")
    header(0, EAP1)
    refused(lambda: sf.eap_dyn_finish(k_max, total), E_ARG, "rank 0 is refused: its layout word")
    assert int(blocks.view(torch.int32)[0]) == EAP4
    # a world that disagrees with the buffer: refused by the binding that owns the
    # buffer and by the library (the third block carries no header)
    sf.eap_dyn_blocks.copy_(blocks)
    refused(lambda: sf.eap_dyn_finish(k_max, total, world=3), E_ARG, "3 blocks")
    three = torch.zeros(3 * sf.eap_dyn_block.numel(), dtype=torch.uint8, device="cuda")
    three[:blocks.numel()] = blocks
    refused(lambda: sf.f.expected_map_dynamic_blocks(three.data_ptr(), 3, k_max, total), E_ARG, "rank 2 is refused")
    refused(lambda: sf.f.expected_map_dynamic_blocks(blocks.data_ptr(), 0, k_max, total), E_ARG, "world")
    # misaligned pointers
    refused(lambda: sf.f.expected_map_dynamic_blocks(blocks.data_ptr() + 4, 2, k_max, total), E_ARG, "aligned")
    refused(lambda: sf.f.eap_dyn_shard_pack(k_max, sf.eap_dyn_block.data_ptr() + 4), E_ARG, "aligned")
    # a context without phd_enable_dynamic
    plain = tms._filter(cfg, N, dcap=0)
    plain.load(*stores[0][:4])
    spare = torch.zeros(sf.eap_dyn_block.numel(), dtype=torch.uint8, device="cuda")
    refused(plain.eap_dyn_shard_count, E_ARG, "phd_enable_dynamic")
    refused(lambda: plain.eap_dyn_shard_pack(k_max, spare.data_ptr()), E_ARG, "phd_enable_dynamic")
    refused(lambda: plain.expected_map_dynamic_blocks(blocks.data_ptr(), 2, k_max, total), E_ARG, "phd_enable_dynamic")
    torch.cuda.synchronize()
    assert not spare.any()
    plain.close()
    # the block, the gathered blocks and the stores are what they were, and still reduce
    assert _bits(sf.eap_dyn_block.cpu().numpy()) == _bits(held.cpu().numpy())
    assert _bits(sf.eap_dyn_blocks.cpu().numpy()) == _bits(blocks.cpu().numpy())
    good = sf.eap_dyn_finish(k_max, total)
    single, _ = _single(cfg, _concat(stores))
    _same(good, single, "after the refusals")
    _same(eaps[1], single, "before the refusals")
    for a, b in zip(before, [_state(s.f) for s in shards]):
        for x, y in zip(a, b):
            assert _bits(x) == _bits(y)
    _close(shards)
