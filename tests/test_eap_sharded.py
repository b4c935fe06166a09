"""The EAP expected map of the sharded filter (phd_eap_shard_count / _pack,
phd_expected_map_blocks, ShardedFilter.expected_map, GroupRank.expected_map).

The contract: every rank returns, bit for bit and in the same emission order,
what PHDFilter.expected_map returns on a single context of world * n particles
loaded with the ranks' settled stores in rank order, which is the oracle's
orc_expected_map of the gathered export.  Every comparison
below is byte equality of the returned arrays.

The decision rounds (expected_map_groups) are not compared for equality: a
round's read of a neighbouring workgroup's state sees that round's decisions
or not with the scheduling ("a same-round read only decides earlier",
phd_eap.hip), so the count varies between runs of the same input on the same
context form — on the chains case below three ranks reducing identical blocks
reported 7, 6 and 6 rounds and the single context 5, with identical maps.
What is fixed is asserted: 1 for the exhaustive greedy (non-finite input),
more than 3 on the chains layout, at least 1 otherwise.

Emulated ranks on one device (phdslam.dist.LocalWorld, the scenarios of
tests/test_trace_sharded.py).  The chain test runs ShardedFilter's own
expected-map phases on every rank in lockstep (LocalWorld.expected_map); the
hand-built cases drive the phases (eap_count, eap_pack, eap_finish) with the
all-gathers as torch.cat.
"""
import ctypes
import functools

import numpy as np
import pytest

import test_trace_sharded as tts
from sharded_helpers import gathered_store, slice_store

CAP = tts.CAP
T_SEP = 10.0  # minSeparation of the hand-built cases (tests/test_gpu_parity.py::test_expected_map_edge_cases)


# ------------------------------------------------------------------ CPU

EAP_SYMBOLS = ("phd_eap_shard_count", "phd_eap_shard_block_bytes", "phd_eap_shard_pack", "phd_expected_map_blocks")


def test_sharded_eap_symbols_exported(built):
    from phdslam._lib import SIGNATURES
    names = tts._exported("libphdslam.so")
    for sym in EAP_SYMBOLS:
        assert sym in names, sym
        assert sym in SIGNATURES, sym
    assert "phd_group_expected_map" in tts._exported("libphdslam_group.so")


@pytest.mark.parametrize("k_max", [0, 1, 7, 1000, (1 << 33) + 5])
def test_eap_block_bytes_follow_the_documented_layout(built, k_max):
    """header 64 B | seven float fields of stride K_max, rounded up to 16
    (include/phd_capi.h); pure arithmetic, no device."""
    import phdslam
    got = ctypes.c_size_t()
    assert phdslam.lib().phd_eap_shard_block_bytes(k_max, ctypes.byref(got)) == 0
    want = (64 + 28 * k_max + 15) // 16 * 16
    assert got.value == want and got.value % 16 == 0


def test_eap_block_bytes_rejects_a_negative_stride(built):
    import phdslam
    got = ctypes.c_size_t(12345)
    assert phdslam.lib().phd_eap_shard_block_bytes(-1, ctypes.byref(got)) == phdslam._lib.PHD_E_ARG
    assert phdslam.lib().phd_last_error()
    assert got.value == 12345


# ------------------------------------------------------------------ GPU

def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _same(a, b, what):
    assert len(a) == len(b), f"{what}: {len(a)} vs {len(b)} components"
    if _bits(a) != _bits(b):
        bad = [k for k in range(len(a)) if _bits(a[k]) != _bits(b[k])]
        raise AssertionError(f"{what}: {len(bad)} of {len(a)} components differ, first at {bad[0]}: "
                             f"{a[bad[0]]} vs {b[bad[0]]}")


def _single(c, state, **cap):
    """PHDFilter.expected_map of one context holding `state`, and its rounds."""
    f = tts._filter(c, len(state[0]), **cap)
    f.load(*state)
    eap = f.expected_map()
    rounds = f.expected_map_groups()
    f.close()
    return eap, rounds


@functools.lru_cache(maxsize=None)
def _chain(cid, world, K):
    """Five free-running sharded scans (the scenario, thresholds and seeds of
    tests/test_trace_sharded.py), then expected_map() on every rank with the
    last plan still open.  Computed once per case, never modified."""
    import torch
    import pyoracle
    from phdslam.dist import LocalWorld, ShardedFilter
    n = 48
    N = world * n
    # the seeds of test_trace_sharded.py: with every one of these the chain
    # resamples and at least one particle migrates (asserted by the test)
    c, state, z = tts._scenario(cid, N, tts.SEED.get((cid, world, n)))
    dev = torch.device("cuda", 0)
    shards = []
    for r in range(world):
        f = tts._filter(c, n)
        f.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        f.load(*slice_store(state, r * n, (r + 1) * n))
        shards.append(ShardedFilter(f, None, dev, world=world, rank=r, seed=tts.FILTER_SEED, block_records=K))
    ranks = LocalWorld(shards)
    ctrl = tts._control(c)
    for k in range(1, tts.SCANS + 1):
        for sf in shards:
            sf.f.set_measurements(z)
        ranks.step(ctrl, k)
    assert all(sf._open for sf in shards), "the last plan is open: expected_map() settles it"
    eaps = ranks.expected_map()
    rounds = [sf.expected_map_groups() for sf in shards]
    torch.cuda.synchronize()
    assert not any(sf._open for sf in shards)
    stats = {k: sum(sf.stats[k] for sf in shards) for k in shards[0].stats}
    stats["resamples"] = shards[0].stats["resamples"]
    gathered = gathered_store([sf.f for sf in shards])
    for sf in shards:
        sf.f.close()
    single, rounds1 = _single(c, gathered)
    ref = pyoracle.expected_map(c, gathered[1], gathered[2], gathered[3])
    return eaps, rounds, single, rounds1, ref, stats, int(gathered[3][-1])


@pytest.mark.gpu
@pytest.mark.parametrize("K", [0, 4])
@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("cid", [2, 3])
def test_after_a_free_running_chain(gpu, cid, world, K):
    """block_records 0 sends every record through the overflow path (pending
    slots re-updated by the settle inside expected_map); 4 through the blocks.
    The store holds migrated slabs (set X), read through the slab references."""
    eaps, rounds, single, rounds1, ref, stats, total = _chain(cid, world, K)
    print("components", total, "->", len(single), "rounds", rounds1, "stats", stats)
    assert stats["resamples"] > 0, "the chain never resampled: pick another seed"
    assert stats["migrated"] > 0, "no particle migrated: pick another seed"
    if K == 0:
        assert stats["overflow_records"] > 0
    assert 0 < len(single) < total
    _same(single, ref, "single context vs oracle")
    for r in range(world):
        _same(eaps[r], single, f"rank {r} vs single context")
        _same(eaps[r], ref, f"rank {r} vs oracle")
    assert rounds1 > 1 and min(rounds) > 1, (rounds, rounds1)  # the decision rounds, not the one-workgroup greedy


# ---- hand-built stores, loaded directly into the shards

def _config():
    import phdslam
    c = phdslam.default_config()
    c.minSeparation = T_SEP
    return c


def _components(rng, K, lo=-30.0, hi=30.0):
    """K components as test_expected_map_edge_cases draws them."""
    from phdslam.types import GAUSSIAN2D
    maps = np.zeros(K, GAUSSIAN2D)
    maps["mean"] = rng.uniform(lo, hi, (K, 2)).astype(np.float32)
    maps["weight"] = rng.uniform(0.2, 1.0, K).astype(np.float32)
    a = rng.uniform(0.05, 0.15, K).astype(np.float32)
    b = (0.2 * a * rng.uniform(-1, 1, K)).astype(np.float32)
    maps["cov"][:, 0] = a
    maps["cov"][:, 3] = a
    maps["cov"][:, 1] = b
    maps["cov"][:, 2] = b
    return maps


def _store(lw, maps, sizes):
    from phdslam.types import POSE
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    assert offs[-1] == len(maps) and len(lw) == len(sizes)
    return np.zeros(len(sizes), POSE), np.asarray(lw, np.float32), maps, offs


def _concat(stores):
    offs = [0]
    for s in stores:
        offs.extend((np.asarray(s[3][1:]) + offs[-1]).tolist())
    return (np.concatenate([s[0] for s in stores]), np.concatenate([s[1] for s in stores]),
            np.concatenate([s[2] for s in stores]), np.asarray(offs, np.int32))


def _shards(c, stores):
    import torch
    from phdslam.dist import ShardedFilter
    dev = torch.device("cuda", 0)
    shards = []
    for r, s in enumerate(stores):
        f = tts._filter(c, len(s[0]))
        f.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        f.load(*s)
        shards.append(ShardedFilter(f, None, dev, world=len(stores), rank=r, seed=tts.FILTER_SEED, block_records=1))
    return shards


def _phases(shards, k_max=None):
    """count, pack, all-gather (torch.cat), finish on every emulated rank.
    Returns the ranks' maps, their rounds and (counts, k_max)."""
    import torch
    counts = [sf.eap_count() for sf in shards]
    k_max = max(counts) if k_max is None else k_max
    for sf in shards:
        sf.eap_pack(k_max)
    blocks = torch.cat([sf.eap_block for sf in shards])
    eaps, rounds = [], []
    for sf in shards:
        sf.eap_blocks.copy_(blocks)
        eaps.append(sf.eap_finish(k_max, sum(counts)))
        rounds.append(sf.expected_map_groups())
    return eaps, rounds, counts, k_max


def _close(shards):
    for sf in shards:
        sf.f.close()


def _held(c, stores, k_max=None):
    """The sharded map of `stores` held to the single context and the oracle."""
    import pyoracle
    shards = _shards(c, stores)
    eaps, rounds, counts, k_max = _phases(shards, k_max)
    _close(shards)
    whole = _concat(stores)
    assert counts == [int(s[3][-1]) for s in stores]
    single, rounds1 = _single(c, whole)
    ref = pyoracle.expected_map(c, whole[1], whole[2], whole[3])
    _same(single, ref, "single context vs oracle")
    for r in range(len(stores)):
        _same(eaps[r], single, f"rank {r} vs single context")
        _same(eaps[r], ref, f"rank {r} vs oracle")
    print("rounds", rounds, "single", rounds1)
    assert min(rounds + [rounds1]) >= 1
    return eaps[0], rounds + [rounds1], ref


def _uneven_stores(rng):
    n = 16
    sizes = [rng.integers(0, 41, n), np.zeros(n, np.int64), rng.integers(1, 26, n)]
    sizes[0][[2, 3, 11]] = 0  # particles with empty maps among full ones
    sizes[0][5] = 40
    return [_store(rng.normal(-np.log(3 * n), 0.3, n), _components(rng, int(s.sum())), s) for s in sizes]


def _chain_components(K, lines=8):
    """The `chains` layout of test_expected_map_edge_cases: minSeparation 10
    with covariance ~0.1 I merges within ~1; neighbours 0.9 apart along lines."""
    rng = np.random.default_rng(7)
    maps = _components(rng, K)
    t = np.arange(K) % (K // lines)
    line = np.arange(K) // (K // lines)
    maps["mean"][:, 0] = (0.9 * t - 100).astype(np.float32)
    maps["mean"][:, 1] = (5.0 * line).astype(np.float32)
    return maps, rng


def _split(maps, lw, world, n, per):
    return [_store(lw[r * n:(r + 1) * n], maps[r * n * per:(r + 1) * n * per].copy(), np.full(n, per)) for r in
            range(world)]


@pytest.mark.gpu
def test_uneven_ranks(gpu):
    """Ranks with different component counts, particles with empty maps, one
    rank with no component at all (its block is a header)."""
    stores = _uneven_stores(np.random.default_rng(11))
    counts = [int(s[3][-1]) for s in stores]
    assert counts[1] == 0 and len(set(counts)) == 3 and counts[0] % 4 != counts[2] % 4
    eap, _, _ = _held(_config(), stores)
    assert 0 < len(eap) <= sum(counts)


@pytest.mark.gpu
def test_all_empty(gpu):
    from phdslam.types import GAUSSIAN2D
    n = 16
    stores = [_store(np.full(n, -np.log(2 * n)), np.zeros(0, GAUSSIAN2D), np.zeros(n, np.int64)) for _ in range(2)]
    shards = _shards(_config(), stores)
    eaps, rounds, counts, k_max = _phases(shards)
    _close(shards)
    assert counts == [0, 0] and k_max == 0
    assert all(len(e) == 0 for e in eaps)
    single, rounds1 = _single(_config(), _concat(stores))
    assert len(single) == 0 and rounds == [rounds1, rounds1]


@pytest.mark.gpu
def test_kmax_padding(gpu):
    """The same store packed with K_max the largest count and with K_max
    several times it (odd: the fields then start off the 16-byte grid): the
    stride is K_max, never K_r, and the padding is never read."""
    stores = _uneven_stores(np.random.default_rng(11))
    k = max(int(s[3][-1]) for s in stores)
    a, _, _ = _held(_config(), stores, k_max=k)
    for pad in (k + 1, 5 * k + 3, 8 * k):
        b, _, _ = _held(_config(), stores, k_max=pad)
        _same(a, b, f"K_max {k} vs {pad}")


@pytest.mark.gpu
def test_nonfinite_last_rank(gpu):
    """A NaN mean on the last rank only: every rank takes the exhaustive
    greedy (one round), as the single context does — on the chains layout, where
    the decision rounds of a rank that missed the flag would need several."""
    world, n, per = 2, 16, 40
    maps, rng = _chain_components(world * n * per)
    lw = rng.normal(-np.log(world * n), 0.3, world * n).astype(np.float32)
    stores = _split(maps, lw, world, n, per)
    clean, rounds_clean, _ = _held(_config(), stores)
    assert min(rounds_clean) > 3, rounds_clean
    stores[-1][2]["mean"][n * per // 3, 0] = np.nan
    eap, rounds, _ = _held(_config(), stores)
    assert rounds == [1, 1, 1], rounds  # both ranks and the single context
    assert np.isnan(eap["mean"]).any()


@pytest.mark.gpu
def test_wide_last_rank(gpu):
    """Rank 0's covariances are ~0.01; the last rank holds pairs of covariance
    ~25 that merge at a spacing many lattice cells of rank 0's own Λ wide: the
    lattice must come from the maximum Λ over the ranks."""
    rng = np.random.default_rng(5)
    n, T = 16, T_SEP
    m0 = _components(rng, n * 8)
    for j in (0, 3):
        m0["cov"][:, j] = rng.uniform(0.008, 0.012, len(m0)).astype(np.float32)
    m0["cov"][:, 1] = m0["cov"][:, 2] = 0.0
    m1 = _components(rng, n * 2)
    for j in (0, 3):
        m1["cov"][:, j] = rng.uniform(24.0, 26.0, len(m1)).astype(np.float32)
    m1["cov"][:, 1] = m1["cov"][:, 2] = 0.0
    sep = 8.0
    for p in range(n):  # one pair per particle, the pairs 100 apart
        m1["mean"][2 * p] = (200.0 + 100.0 * p, 0.0)
        m1["mean"][2 * p + 1] = (200.0 + 100.0 * p + sep, 0.0)
    # from the inputs alone: the pairs merge (d < T) and lie further apart than
    # two cells of the lattice rank 0's own Λ gives (not even neighbours there)
    lam0 = float(np.max(m0["cov"][:, [0, 3]]))
    cell0 = np.sqrt(1.05 * T * lam0) * 1.0001
    d_pair = sep * sep / float(np.min(m1["cov"][:, [0, 3]]))
    assert d_pair < 0.5 * T and sep > 2.0 * cell0, (d_pair, cell0)
    lw = np.full(n, -np.log(2 * n))
    stores = [_store(lw, m0, np.full(n, 8)), _store(lw, m1, np.full(n, 2))]
    eap, _, ref = _held(_config(), stores)
    merged = ref[ref["mean"][:, 0] > 150.0]
    assert len(merged) == n, "every wide pair merged in the oracle"


@pytest.mark.gpu
def test_ties_across_ranks(gpu):
    """Identical components with identical weights on different ranks, and
    equal-weight neighbours X (rank 0), Y (rank 1), Z (rank 0) 0.9 apart in a
    row: in rank order X is the seed and absorbs Y alone; with the shards
    swapped Y comes first and absorbs both.  The concatenation index decides."""
    import pyoracle
    rng = np.random.default_rng(3)
    n, per = 16, 6
    stores = []
    for r in range(2):
        m = _components(rng, n * per, lo=-90.0, hi=-40.0)
        stores.append(_store(np.full(n, -np.log(2 * n)), m, np.full(n, per)))
    same = stores[0][2][7].copy()
    same["mean"] = (40.0, 40.0)
    stores[0][2][7] = same
    stores[1][2][7] = same  # identical component, identical weight, both ranks
    for store, slot, x in ((0, 13, 10.0), (1, 20, 10.9), (0, 31, 11.8)):
        g = stores[store][2][slot]
        g["weight"], g["mean"] = 0.7, (x, 0.0)
        g["cov"] = (0.1, 0.0, 0.0, 0.1)
        stores[store][2][slot] = g
    c = _config()
    a, b = _concat(stores), _concat(stores[::-1])
    ra, rb = pyoracle.expected_map(c, a[1], a[2], a[3]), pyoracle.expected_map(c, b[1], b[2], b[3])
    assert _bits(ra) != _bits(rb) and len(ra) == len(rb) + 1, "swapping the shards changes the oracle's map"
    _held(c, stores)
    _held(c, stores[::-1])


@pytest.mark.gpu
def test_zero_weight_rank(gpu):
    rng = np.random.default_rng(9)
    n, per = 16, 10
    stores = []
    for r in range(3):
        lw = rng.normal(-np.log(3 * n), 0.3, n)
        if r == 1:
            lw[:] = -np.inf
        stores.append(_store(lw, _components(rng, n * per, lo=-6.0, hi=6.0), np.full(n, per)))
    eap, _, _ = _held(_config(), stores)
    assert (eap["weight"] > 0).any()


@pytest.mark.gpu
def test_chains_split_across_ranks(gpu):
    """8 lines of 240 components over 3 ranks of 640: both rank edges fall
    inside a line, so chains of waiting decisions cross the ranks."""
    world, n, per = 3, 16, 40
    maps, rng = _chain_components(world * n * per)
    assert (n * per) % (world * n * per // 8) != 0
    lw = rng.normal(-np.log(world * n), 0.3, world * n).astype(np.float32)
    _, rounds, _ = _held(_config(), _split(maps, lw, world, n, per))
    assert min(rounds) > 3, rounds  # every rank and the single context


# ---- refusals: argument checks made before any kernel reads a block

def _assert_refused(fn, code, text):
    import phdslam
    with pytest.raises(phdslam.PHDError) as e:
        fn()
    assert e.value.code == code, e.value
    assert text in str(e.value), e.value


@pytest.mark.gpu
def test_refusals_leave_the_store_unchanged(gpu):
    import torch
    import phdslam
    E_ARG, E_UNSUP = phdslam._lib.PHD_E_ARG, phdslam._lib.PHD_E_UNSUPPORTED
    stores = _uneven_stores(np.random.default_rng(11))[::2]
    shards = _shards(_config(), stores)
    before = [sf.f.export() for sf in shards]
    counts = [sf.eap_count() for sf in shards]
    k_max, total = max(counts), sum(counts)
    for sf in shards:
        sf.eap_pack(k_max)
    blocks = torch.cat([sf.eap_block for sf in shards])
    sf = shards[0]
    words = sf.eap_block.numel() // 4
    # a store larger than the stride is refused by the pack
    _assert_refused(lambda: sf.f.eap_shard_pack(counts[0] - 1, sf.eap_block.data_ptr()), E_ARG, "K_max")
    # a header whose count exceeds K_max
    bad = blocks.clone()
    bad.view(torch.int32)[words + 1] = k_max + 1
    sf.eap_blocks.copy_(bad)
    _assert_refused(lambda: sf.eap_finish(k_max, total), E_ARG, "rank 1 is refused: its component count exceeds K_max")
    # a header of another particle count
    bad = blocks.clone()
    bad.view(torch.int32)[4] += 1
    sf.eap_blocks.copy_(bad)
    _assert_refused(lambda: sf.eap_finish(k_max, total), E_ARG, "rank 0 is refused: its particle count")
    # a world that disagrees with the buffer: refused by the binding that owns the
    # buffer, and by the library (the third block lies outside the allocation or
    # carries no header)
    sf.eap_blocks.copy_(blocks)
    _assert_refused(lambda: sf.eap_finish(k_max, total, world=3), E_ARG, "3 blocks")
    three = torch.zeros(3 * sf.eap_block.numel(), dtype=torch.uint8, device="cuda")
    three[:blocks.numel()] = blocks
    _assert_refused(lambda: sf.f.expected_map_blocks(three.data_ptr(), 3, k_max, total), E_ARG, "rank 2 is refused")
    _assert_refused(lambda: sf.f.expected_map_blocks(blocks.data_ptr(), 0, k_max, total), E_ARG, "world")
    # the untouched blocks still reduce, and the stores are what they were
    good = sf.eap_finish(k_max, total)
    single, _ = _single(_config(), _concat(stores))
    _same(good, single, "after the refusals")
    after = [s.f.export() for s in shards]
    for a, b in zip(before, after):
        for x, y in zip(a, b):
            assert _bits(x) == _bits(y)
    _close(shards)
    # feature_model 2: refused as the sharded step refuses it
    c = _config()
    c.featureModel = 2
    f = tts._filter(c, 16)
    f.load(*stores[0])
    before = f.export()
    block = torch.zeros(sf.eap_block.numel(), dtype=torch.uint8, device="cuda")
    _assert_refused(f.eap_shard_count, E_UNSUP, "feature_model")
    _assert_refused(lambda: f.eap_shard_pack(k_max, block.data_ptr()), E_UNSUP, "feature_model")
    _assert_refused(lambda: f.expected_map_blocks(blocks.data_ptr(), 2, k_max, total), E_UNSUP, "feature_model")
    assert not block.any()
    for x, y in zip(before, f.export()):
        assert _bits(x) == _bits(y)
    f.close()


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [2, 3])
def test_group_rank_expected_map_matches_filter(gpu, cid):
    """GroupRank.expected_map (phd_group_expected_map: the settle, ncclAllGather
    of the counts and of the blocks, the reduce) through RCCL at world 1 equals
    PHDFilter.expected_map of the same store."""
    import torch
    from phdslam.dist import GroupRank
    n, steps = 300, 3
    c, state, z = tts._scenario(cid, n)
    f = tts._filter(c, n)
    f.load(*state)
    f.set_measurements(z)
    g = GroupRank(f, None, torch.device("cuda", 0), world=1, rank=0, seed=tts.FILTER_SEED, block_records=4)
    for k in range(1, steps + 1):
        g.step(tts._control(c), k)
    got = g.expected_map()  # settles the open plan
    rounds = g.expected_map_groups()
    want = f.expected_map()
    assert rounds >= 1 and f.expected_map_groups() >= 1
    again = g.expected_map()
    g.close()
    f.close()
    assert len(want) > 0
    _same(got, want, "group vs filter")
    _same(again, want, "second call")
