"""The decision rounds of the dynamic expected map on the sharded filter: the
blocks form (phd_expected_map_dynamic_blocks, ShardedFilter.expected_map_dynamic)
reaches the single context's bytes through the same reduce, in both modes, and
computes Λ, so the cells, from the concatenated SoA alone — the "EAP4" header
carries no bound and its words other than 0, 1, 4 and 5 stay zero.

Emulated ranks on one device (phdslam.dist.LocalWorld) with the helpers of
tests/test_eap_dynamic_sharded.py; the stores are the chain, tie and fallback
cases of tests/eap_dynamic_cases.py split over world 2 and 3, one rank of
world 3 holding no dynamic component at all, and the stride K_max padded.
"""
import numpy as np
import pytest

import eap_dynamic_cases as edc
import test_eap_dynamic_sharded as teds
import test_gpu_mixed_sharded as tms
from phdslam.scenario import mixed_config

pytestmark = pytest.mark.gpu

N_RANK = 4
NAMES = ("chain_x", "chain_diagonal", "chain_velocity", "ties_XYZ", "ties_YXZ", "fallback_nan_mean",
         "fallback_zero_trace", "fallback_T_zero")


def split(cfg, cs, world, empty_rank):
    """The case's particles dealt in order to the ranks that hold any (every
    rank padded with empty particles to N_RANK: the headers' n must agree)."""
    holders = [r for r in range(world) if r != empty_rank]
    P = len(cs["sizes"])
    per = -(-P // len(holders))
    assert per <= N_RANK
    off = edc.offsets(cs)
    stores, p = [], 0
    for r in range(world):
        take = min(per, P - p) if r in holders else 0
        sizes = np.concatenate([cs["sizes"][p:p + take], np.zeros(N_RANK - take, np.int64)])
        lw = np.full(N_RANK, cs["lw"][0], np.float32)
        stores.append(teds._store(cfg, lw, cs["comps"][off[p]:off[p + take]], sizes, seed=77 + r))
        p += take
    assert p == P
    return stores


def header_words(blocks, world):
    import torch
    w = blocks.view(torch.int32).cpu().numpy().reshape(world, -1)[:, :16]
    return w


@pytest.mark.parametrize("world,empty_rank,pad", [(2, None, 0), (3, 1, 3)])
@pytest.mark.parametrize("name", NAMES)
def test_sharded_rounds_equal_the_single_context(gpu, name, world, empty_rank, pad):
    from phdslam.dist import LocalWorld
    cs = edc.CASES[name]()
    cfg = mixed_config(minSeparation=cs["T"])
    stores = split(cfg, cs, world, empty_rank)
    if empty_rank is not None:
        assert int(stores[empty_rank][5][-1]) == 0
    # the single context of all the particles, both modes
    whole = teds._concat(stores)
    single = tms._filter(cfg, world * N_RANK, dcap=teds.DCAP)
    tms._load(single, *whole)
    want = {}
    for mode in (0, 1):
        single.set_expected_map_dynamic_mode(mode)
        want[mode] = (single.expected_map_dynamic().copy(), single.expected_map_dynamic_groups())
    single.close()
    teds._same(want[0][0], want[1][0], "single context: rounds vs one workgroup")
    assert want[1][1] == (1, 0)
    assert (want[0][1][1] == 0) == cs["fallback"]
    if cs["n_out"] is not None:
        assert len(want[0][0]) == cs["n_out"]
    shards = teds._shards(cfg, stores)
    k_max = max(int(s[5][-1]) for s in stores) + pad
    for mode in (0, 1):
        for sf in shards:
            sf.set_expected_map_dynamic_mode(mode)
        eaps, counts, _, blocks = teds._phases(shards, k_max)
        served = LocalWorld(shards).expected_map_dynamic()  # ShardedFilter's own phases (K_max the largest count)
        for r, sf in enumerate(shards):
            teds._same(eaps[r], want[mode][0], f"mode {mode}, rank {r}: blocks vs single context")
            teds._same(served[r], want[mode][0], f"mode {mode}, rank {r}: expected_map_dynamic vs single context")
            rounds, cells = sf.expected_map_dynamic_groups()
            assert cells == want[mode][1][1], f"mode {mode}, rank {r}: cells are a function of the SoA"
            assert rounds >= 1
        h = header_words(blocks, world)
        assert (h[:, 0] == teds.EAP4).all() and h[:, 1].tolist() == counts
        assert (h[:, 4] == N_RANK).all() and (h[:, 5] == k_max).all()
        assert not h[:, [2, 3] + list(range(6, 16))].any(), "the header carries no bound and no flag"
    teds._close(shards)
