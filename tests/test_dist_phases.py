"""The order of the sharded step's phases, on CPU.

phdslam.dist.ShardedFilter states the order once, in its phase generators;
step / flush / expected_map serve the collectives through the rank's transport
and LocalWorld through copies between the ranks of one process.  Here a
recording stub stands in for the local PHDFilter (every call ShardedFilter makes
on it is logged with its key arguments and answered with canned values) and a
recording transport for `comm`:

  * the log of step(), flush() and both expected maps equals a list written
    down here from the step as it stood before the generators existed;
  * each rank's filter calls under LocalWorld equal that rank's under its own
    step() at world 2 and 3;
  * LocalWorld's collectives on CPU tensors, and its three refusals.
"""
import contextlib
import types

import numpy as np
import pytest
import torch

from phdslam import dist
from phdslam.dist import AllGather, AllToAll, Exchange, LocalWorld, ShardedFilter, overflow_slices

RB = 16  # record bytes of the stub
N = 6    # particles per rank
CTX_STREAM, PLAN_STREAM = 7, 1000  # handles of the fake streams (the plan stream of rank r: PLAN_STREAM + r)


class _Filter:
    """Every method ShardedFilter calls on its local filter: logs (name, key
    arguments) and returns canned values.  polls: what shard_poll returns, in
    turn."""

    def __init__(self, log, form=0, polls=(), count=3):
        self.n = N
        self.log, self.form, self.polls, self.count = log, form, list(polls), count

    def record_bytes(self):
        return RB

    def update_form(self):
        return self.form

    def set_stream(self, s):
        assert s == CTX_STREAM

    def set_index_offset(self, o):
        self.offset = o

    def set_plan_stream(self, s):
        self.plan_stream = s

    def predict_update(self, control, k, logw):
        self.log.append(("predict_update", control, k))

    def shard_poll(self, world):
        self.log.append(("shard_poll", world))
        return self.polls.pop(0)

    def shard_receive_overflow(self, buf, K, slots):
        self.log.append(("shard_receive_overflow", K))

    def update_pending(self, control, k, logw):
        self.log.append(("update_pending", control, k))

    def wait_logw(self, stream):
        self.log.append(("wait_logw", stream))

    def shard_resample_async(self, w_all, world, rank, seed, k, *rest):
        self.log.append(("shard_resample_async", world, rank, k, rest[5]))  # rest[5]: block_records

    def trace_shard_pack(self, w_all, world, rank, k, block):
        self.log.append(("trace_shard_pack", world, rank, k))

    def trace_shard_append(self, w_all, blocks, world, rank):
        self.log.append(("trace_shard_append", world, rank))

    def trace_shard_pack_mixed(self, w_all, world, rank, k, block):
        self.log.append(("trace_shard_pack_mixed", world, rank, k))

    def trace_shard_append_mixed(self, w_all, blocks, world, rank):
        self.log.append(("trace_shard_append_mixed", world, rank))

    def shard_receive_blocks(self, blocks, K, slots):
        self.log.append(("shard_receive_blocks", K))

    def eap_shard_count(self):
        self.log.append(("eap_shard_count",))
        return self.count

    def eap_shard_pack(self, k_max, block):
        self.log.append(("eap_shard_pack", k_max))

    def expected_map_blocks(self, blocks, world, k_max, out_cap):
        self.log.append(("expected_map_blocks", world, k_max, out_cap))
        return "static map"

    def eap_dyn_shard_count(self):
        self.log.append(("eap_dyn_shard_count",))
        return self.count

    def eap_dyn_shard_pack(self, k_max, block):
        self.log.append(("eap_dyn_shard_pack", k_max))

    def expected_map_dynamic_blocks(self, blocks, world, k_max, out_cap):
        self.log.append(("expected_map_dynamic_blocks", world, k_max, out_cap))
        return "dynamic map"


class _Comm:
    """The comm interface, recording: sizes, peers and the stream torch was
    switched to.  An all-gather fills every rank's slot with this rank's."""

    def __init__(self, log, world, cuda):
        self.log, self.world, self.cuda = log, world, cuda

    def all_gather(self, out, inp):
        self.log.append(("all_gather", out.numel(), inp.numel(), self.cuda.current))
        out.view(self.world, -1).copy_(inp.view(1, -1).expand(self.world, -1))

    def all_to_all_equal(self, out, inp):
        self.log.append(("all_to_all_equal", out.numel(), inp.numel()))

    def exchange(self, sends, recvs):
        self.log.append(("exchange", [(p, t.numel()) for p, t in sends], [(p, t.numel()) for p, t in recvs]))


@pytest.fixture
def cuda(monkeypatch):
    """torch.cuda's streams as plain handles: ShardedFilter's constructor and its
    all-gather on the plan stream run without a device."""
    state = types.SimpleNamespace(current=None, made=0)

    class Stream:
        def __init__(self, device=None, priority=0):
            self.cuda_stream = PLAN_STREAM + state.made
            state.made += 1

    @contextlib.contextmanager
    def stream(s):
        state.current, before = s.cuda_stream, state.current
        yield
        state.current = before

    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=CTX_STREAM))
    monkeypatch.setattr(torch.cuda, "Stream", Stream)
    monkeypatch.setattr(torch.cuda, "stream", stream)
    return state


def _poll(snd, rcv, rs=1, pend=0):
    """(neff, resampled, demand, send records, receive records, pending slots)."""
    return (3.5, rs, [N] * len(snd), list(snd), list(rcv), pend)


def _rank(cuda, world=2, rank=0, form=0, polls=(), K=1, trace=None, count=3, comm=True):
    log = []
    f = _Filter(log, form, polls, count)
    sf = ShardedFilter(f, None, torch.device("cpu"), world=world, rank=rank, block_records=K,
                       comm=_Comm(log, world, cuda) if comm else None)
    if trace:  # (enable_trace sizes these from the library; any size will do here)
        sf.trace_block = torch.zeros(32, dtype=torch.uint8)
        sf.trace_blocks = torch.zeros(world * 32, dtype=torch.uint8)
        sf.trace_mixed = trace == "mixed"
    return sf, log


# ------------------------------------------------------------------ 1. the order, per rank

@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("overflow", [False, True])
@pytest.mark.parametrize("trace", [None, "static", "mixed"])
def test_step_order(cuda, trace, overflow, form):
    """Rank 0 of world 2, block_records 1, step 5 with control (2.0, 0.05) on
    an open plan.  overflow: the poll reports 3 records for rank 1 and 5 from
    it, so 2 and 4 records travel point to point and the slots are re-updated."""
    u = (2.0, 0.05)
    sf, log = _rank(cuda, form=form, trace=trace, polls=[_poll([0, 3], [0, 5]) if overflow else _poll([0, 1], [0, 0])])
    assert sf.step(u, 4) == (None, None)
    del log[:]
    want = [("predict_update", u, 5), ("shard_poll", 2)]
    if overflow:
        want += [("exchange", [(1, 2 * RB)], [(1, 4 * RB)]), ("shard_receive_overflow", 1), ("update_pending", u, 5)]
    if form:
        want += [("wait_logw", PLAN_STREAM), ("all_gather", 2 * N, N, PLAN_STREAM)]
    else:
        want += [("all_gather", 2 * N, N, None)]
    if trace == "static":
        want += [("trace_shard_pack", 2, 0, 5), ("all_gather", 64, 32, None), ("trace_shard_append", 2, 0)]
    if trace == "mixed":
        want += [("trace_shard_pack_mixed", 2, 0, 5), ("all_gather", 64, 32, None), ("trace_shard_append_mixed", 2, 0)]
    want += [("shard_resample_async", 2, 0, 5, 1), ("all_to_all_equal", 2 * RB, 2 * RB), ("shard_receive_blocks", 1)]
    assert sf.step(u, 5) == (3.5, 1)
    assert log == want
    assert sf._open and sf._ovf == ([], [])
    assert sf.stats["overflow_records"] == (2 if overflow else 0)


@pytest.mark.parametrize("trace", [None, "static"])
def test_first_step_polls_nothing(cuda, trace):
    sf, log = _rank(cuda, trace=trace)
    assert sf.step(None, 1) == (None, None)
    want = [("predict_update", None, 1), ("all_gather", 2 * N, N, None)]
    if trace:
        want += [("trace_shard_pack", 2, 0, 1), ("all_gather", 64, 32, None), ("trace_shard_append", 2, 0)]
    want += [("shard_resample_async", 2, 0, 1, 1), ("all_to_all_equal", 2 * RB, 2 * RB), ("shard_receive_blocks", 1)]
    assert log == want


def test_flush_order(cuda):
    sf, log = _rank(cuda, polls=[_poll([0, 3], [0, 5]), _poll([0, 1], [0, 1])])
    assert sf.flush() == (None, None) and log == []  # no plan is open
    sf.step(None, 1)
    del log[:]
    assert sf.flush() == (3.5, 1)
    # (no update ran on the late records' slots: nothing to re-update)
    assert log == [("shard_poll", 2), ("exchange", [(1, 2 * RB)], [(1, 4 * RB)]), ("shard_receive_overflow", 1)]
    sf.step(None, 2)
    del log[:]
    assert sf.settle() == (3.5, 1)
    assert log == [("shard_poll", 2)]
    assert not sf._open


@pytest.mark.parametrize("dynamic", [False, True])
def test_expected_map_order(built, cuda, dynamic):
    """The plan of step 1 is open: the map settles it first.  Every rank holds 3
    components under the recording transport: k_max 3, 6 in all; the blocks
    are 64 + 28 k_max (dynamic: 84 k_max) bytes, rounded up to 16."""
    sf, log = _rank(cuda, polls=[_poll([0, 1], [0, 1])])
    sf.step(None, 1)
    del log[:]
    if dynamic:
        assert sf.expected_map_dynamic() == "dynamic map"
        assert log == [("shard_poll", 2), ("eap_dyn_shard_count",), ("all_gather", 2, 1, None), ("eap_dyn_shard_pack", 3),
                       ("all_gather", 2 * 320, 320, None), ("expected_map_dynamic_blocks", 2, 3, 6)]
    else:
        assert sf.expected_map() == "static map"
        assert log == [("shard_poll", 2), ("eap_shard_count",), ("all_gather", 2, 1, None), ("eap_shard_pack", 3),
                       ("all_gather", 2 * 160, 160, None), ("expected_map_blocks", 2, 3, 6)]
    assert not sf._open


# ------------------------------------------------------------------ 2. LocalWorld against the ranks' own step

def _polls(world, K, steps, seed):
    """Per rank, the polls of `steps` plans from random record counts
    (counts[s, d]: records s -> d, some beyond the K of a block)."""
    rng = np.random.default_rng(seed)
    polls = [[] for _ in range(world)]
    for _ in range(steps):
        counts = rng.integers(0, K + 4, (world, world))
        np.fill_diagonal(counts, 0)
        for r in range(world):
            polls[r].append(_poll(counts[r], counts[:, r]))
    return polls


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("trace", [None, "static", "mixed"])
@pytest.mark.parametrize("world", [2, 3])
def test_local_world_runs_each_ranks_own_step(built, cuda, world, trace, form):
    """Three steps, the flush and both expected maps.  The all-gather on the
    plan stream is the one difference: in one process rank r's stream has to
    wait for every rank's log-weights, so each filter is asked once per rank;
    the rank's own wait is the one its own step() makes."""
    u = (2.0, 0.05)
    polls = _polls(world, 1, 3, seed=world)

    def ranks(comm):
        cuda.made = 0
        return [_rank(cuda, world, r, form, polls[r], trace=trace, count=2 + r, comm=comm) for r in range(world)]

    alone = ranks(True)
    for sf, log in alone:
        for k in (1, 2, 3):
            sf.step(u, k)
        sf.flush()
        sf.expected_map()
        sf.expected_map_dynamic()
    together = ranks(False)
    lw = LocalWorld([sf for sf, _ in together])
    assert [lw.step(u, k) for k in (1, 2, 3)] == [[(None, None)] * world] + [[(3.5, 1)] * world] * 2
    assert lw.flush() == [(3.5, 1)] * world
    assert lw.expected_map() == ["static map"] * world and lw.expected_map_dynamic() == ["dynamic map"] * world
    comm_calls = ("all_gather", "all_to_all_equal", "exchange")
    for r in range(world):
        own = [e for e in alone[r][1] if e[0] not in comm_calls]
        got = [e for e in together[r][1] if e[0] != "wait_logw" or e[1] == PLAN_STREAM + r]
        # every rank gathered its own count under the recording transport, all of them under LocalWorld
        cmax, csum = max(2 + q for q in range(world)), sum(2 + q for q in range(world))
        own = [(e[0], cmax) if e[0].endswith("_pack") and e[0].startswith("eap") else
               (e[0], world, cmax, csum) if e[0].startswith("expected_map") else e for e in own]
        assert got == own, r
        if form:
            waits = [e[1] for e in together[r][1] if e[0] == "wait_logw"]
            assert waits == [PLAN_STREAM + q for q in range(world)] * 3


# ------------------------------------------------------------------ 3. the in-process collectives

@pytest.mark.parametrize("world", [1, 2, 3])
def test_local_all_gather(world):
    inps = [torch.arange(4, dtype=torch.float32) + 10 * r for r in range(world)]
    calls = [AllGather(torch.zeros(4 * world), inps[r], None, None) for r in range(world)]
    dist.local_all_gather(calls)
    for c in calls:
        assert torch.equal(c.out, torch.cat(inps))


@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("records", [0, 1])
def test_local_all_to_all(world, records):
    blk = records * RB
    inps = [torch.arange(world * blk, dtype=torch.int32).to(torch.uint8) + 100 * r for r in range(world)]
    calls = [AllToAll(torch.full((world * blk,), 255, dtype=torch.uint8), inps[r]) for r in range(world)]
    dist.local_all_to_all(calls)
    for d, c in enumerate(calls):
        assert c.out.numel() == world * blk
        for s in range(world):
            assert torch.equal(c.out[s * blk:(s + 1) * blk], inps[s][d * blk:(d + 1) * blk])


def _exchange_calls(counts, K, rb):
    world = len(counts)
    calls, bufs = [], []
    for r in range(world):
        sends, recvs = overflow_slices(counts[r], counts[:, r], K, rb)
        out = torch.arange(max(int(np.maximum(counts[r] - K, 0).sum()), 1) * rb, dtype=torch.int32) + 100000 * r
        inn = torch.full((max(int(np.maximum(counts[:, r] - K, 0).sum()), 1) * rb,), -1, dtype=torch.int32)
        bufs.append((out, inn))
        calls.append(Exchange([(d, out[lo:hi]) for d, lo, hi in sends], [(s, inn[lo:hi]) for s, lo, hi in recvs]))
    return calls, bufs


def test_local_exchange_pairs_up():
    """Random record counts as test_dist.py::test_overflow_slices_pair_up: every
    receive slice holds the sender's slice for that rank."""
    rng = np.random.default_rng(3)
    world, K, rb = 5, 2, 24
    counts = rng.integers(0, 7, (world, world))
    np.fill_diagonal(counts, 0)
    calls, bufs = _exchange_calls(counts, K, rb)
    dist.local_exchange(calls)
    moved = 0
    for r in range(world):
        for s, buf in calls[r].recvs:
            (src,) = [t for d, t in calls[s].sends if d == r]
            assert buf.numel() == (counts[s, r] - K) * rb and torch.equal(buf, src) and int(buf[0]) // 100000 == s
            moved += 1
    assert moved == int((counts > K).sum()) > 0


def test_local_exchange_refusals():
    counts = np.array([[0, 5], [0, 0]])
    calls, _ = _exchange_calls(counts, 2, 8)
    with pytest.raises(RuntimeError, match="rank 1 receives from rank 0, which has 0 sends"):
        dist.local_exchange([Exchange([], []), calls[1]])
    with pytest.raises(RuntimeError, match="rank 0 sends 24 elements to rank 1, which expects 16"):
        dist.local_exchange([calls[0], Exchange([], [(0, calls[1].recvs[0][1][:16])])])
    with pytest.raises(RuntimeError, match="1 sends for 0 receives"):
        dist.local_exchange([calls[0], Exchange([], [])])


class _Phases:
    """A rank whose step yields the given collectives."""

    def __init__(self, world, rank, *calls):
        self.world, self.rank, self.calls = world, rank, calls

    def step_phases(self, control, k):
        for c in self.calls:
            yield c
        return self.rank


def test_local_world_refuses_diverging_ranks():
    g = AllGather(torch.zeros(2), torch.zeros(1), None, None)
    a = AllToAll(torch.zeros(0), torch.zeros(0))
    assert LocalWorld([_Phases(2, 0, g, a), _Phases(2, 1, g, a)]).step(None, 1) == [0, 1]
    with pytest.raises(RuntimeError, match="rank 0 at AllGather, rank 1 at AllToAll"):
        LocalWorld([_Phases(2, 0, g, g), _Phases(2, 1, g, a)]).step(None, 1)
    with pytest.raises(RuntimeError, match="rank 0 at AllToAll, rank 1 returned"):
        LocalWorld([_Phases(2, 0, g, a), _Phases(2, 1, g)]).step(None, 1)
    with pytest.raises(ValueError, match="shard 1 of 2 is rank 0 of world 2"):
        LocalWorld([_Phases(2, 0), _Phases(2, 0)])
