"""Multi-GPU particle sharding: one process per GPU, RCCL over xGMI.

Rank r owns a contiguous shard of n particles (global ids r*n .. r*n+n-1).
Predict and update are per-particle independent and run locally with no
communication.  The cross-particle steps (phdfilter.cu:3748-3755 normalise,
main.cpp:1281-1297 nEff + resample) need every log-weight:

  1. all_gather of the n unnormalised log-weights per rank (RCCL);
  2. every rank runs the same deterministic kernels on the identical gathered
     vector: global logSumExp, nEff, resample decision and the parent index of
     every one of the N = world*n strata (fixed-point CDF, phd_detmath.h), so
     no broadcast is needed and all ranks agree bit for bit;
  3. migration plan (k_shard_tail on the device; plan_migration is its host
     statement, migration_counts the per-rank record counts every rank derives
     from the per-rank demand): children of a local parent stay local; only the
     imbalance moves.  Surplus children are packed as particle records into
     fixed blocks per peer and exchanged with one equal-split all_to_all_single
     per step — no host read-back sits on the step (ShardedFilter below).

The particle order after a resample is a permutation of the single-GPU order;
the resampled multiset of particles is the same.

The order of a sharded step's phases is stated once, in ShardedFilter's
generators (step_phases, settle_phases, expected_map_phases): they run the
rank-local phases and yield an AllGather, AllToAll or Exchange wherever a
collective has to happen.  Two drivers serve what they yield: ShardedFilter's
own step / flush / expected_map through the rank's transport (TorchComm), and
LocalWorld, which advances the ranks of one process in lockstep and serves the
collectives with device copies.
"""
from collections import namedtuple

import numpy as np

# What a phase generator yields: the collective every rank takes part in next.
# AllGather: `stream` None, or the stream the gather runs on once
# ready(stream.cuda_stream) has made it wait for `inp`.  AllToAll: equal split,
# block d of `inp` goes to rank d.  Exchange: point-to-point [(peer, tensor)];
# yielded with empty lists too, so that the ranks stay aligned.
AllGather = namedtuple("AllGather", "out inp stream ready")
AllToAll = namedtuple("AllToAll", "out inp")
Exchange = namedtuple("Exchange", "sends recvs")


def plan_migration(parents, n_local, world):
    """Deterministic migration plan from the global parent list.

    parents: int array (world*n_local,), parent global id of every stratum.
    Returns per-rank dicts with
      keep:  local parent indices of the children that stay (new slots 0..len-1)
      send:  {dst_rank: local parent indices to send}, in stratum order
      recv:  {src_rank: count}, received into slots len(keep).. in src-rank order
    """
    parents = np.asarray(parents, np.int64)
    owner = parents // n_local
    plans = []
    surplus = []  # per rank: parent global ids beyond the local quota
    deficit = np.zeros(world, np.int64)
    for r in range(world):
        mine = parents[owner == r]  # stratum order
        keep = mine[:n_local] - r * n_local
        surplus.append(mine[n_local:])
        deficit[r] = n_local - len(keep)
        plans.append({"keep": keep.astype(np.int32), "send": {}, "recv": {}})
    # match surplus (rank order) to deficits (rank order)
    d = 0
    for s in range(world):
        todo = surplus[s]
        pos = 0
        while pos < len(todo):
            while deficit[d] == 0:
                d += 1
            take = int(min(deficit[d], len(todo) - pos))
            chunk = todo[pos:pos + take] - s * n_local
            plans[s]["send"].setdefault(d, []).extend(chunk.tolist())
            plans[d]["recv"][s] = plans[d]["recv"].get(s, 0) + take
            deficit[d] -= take
            pos += take
    for p in plans:
        p["send"] = {k: np.array(v, np.int32) for k, v in p["send"].items()}
    assert int(deficit.sum()) == 0
    return plans


def migration_counts(demand, n_local, world, rank):
    """All-to-all counts of plan_migration from the per-rank demand alone.

    demand[s] = number of children of rank s's particles (phd_shard_resample
    returns it; identical on every rank).  Surplus children beyond n_local, in rank
    order, fill the deficits, in rank order.  Returns (keep, send_counts,
    recv_counts) for `rank`, the same as plan_migration's keep/send/recv sizes.
    """
    demand = [int(d) for d in demand]
    s0, f0 = [0], [0]  # surplus / deficit ranges of rank s: [s0[s], s0[s+1])
    for d in demand:
        s0.append(s0[-1] + max(d - n_local, 0))
        f0.append(f0[-1] + max(n_local - d, 0))
    assert s0[-1] == f0[-1], "demand does not sum to world * n_local"

    def overlap(a0, a1, b0, b1):
        return max(0, min(a1, b1) - max(a0, b0))

    send = [overlap(s0[rank], s0[rank + 1], f0[d], f0[d + 1]) for d in range(world)]
    recv = [overlap(s0[s], s0[s + 1], f0[rank], f0[rank + 1]) for s in range(world)]
    return min(demand[rank], n_local), send, recv


def overflow_slices(send_records, recv_records, block_records, record_bytes):
    """Byte ranges of the records beyond the fixed blocks of a sharded step.

    The sender's overflow buffer holds, per destination d in rank order, its
    records block_records .. send_records[d]-1; the receiver's holds, per source
    s in rank order, records block_records .. recv_records[s]-1 (record_slot of
    csrc/phd_records.hip, which the block pack and unpack share).  Returns ([(d, lo, hi)], [(s, lo, hi)]) in
    bytes; both sides derive the same pairs from the same global plan.
    """
    K = block_records
    sends, recvs = [], []
    o = 0
    for d, c in enumerate(send_records):
        x = max(int(c) - K, 0)
        if x:
            sends.append((d, o * record_bytes, (o + x) * record_bytes))
        o += x
    o = 0
    for s_, c in enumerate(recv_records):
        x = max(int(c) - K, 0)
        if x:
            recvs.append((s_, o * record_bytes, (o + x) * record_bytes))
        o += x
    return sends, recvs


class TorchComm:
    """The step's transport over torch.distributed (RCCL over xGMI for "nccl").

    gloo moves CPU tensors only for some collectives: with CUDA buffers under
    gloo (a functional rehearsal of N ranks on one GPU) every transfer is staged
    through host memory."""

    def __init__(self, dist, device):
        self.dist = dist
        self.stage = str(dist.get_backend()) == "gloo" and getattr(device, "type", "cpu") == "cuda"

    def _host(self, t):
        return t.cpu() if self.stage else t

    def all_gather(self, out, inp):
        if self.stage:
            o = out.cpu()
            self.dist.all_gather_into_tensor(o, inp.cpu())
            out.copy_(o)
        else:
            self.dist.all_gather_into_tensor(out, inp)

    def all_to_all_equal(self, out, inp):
        if out.numel() == 0:
            return
        if self.stage:
            o = out.cpu()
            self.dist.all_to_all_single(o, inp.cpu())
            out.copy_(o)
        else:
            self.dist.all_to_all_single(out, inp)

    def exchange(self, sends, recvs):
        """Point-to-point transfers of [(peer, tensor)] (only the ranks a pair
        involves take part; both sides know the pair from the global plan)."""
        if not sends and not recvs:
            return
        dist = self.dist
        sb = [(p, self._host(t)) for p, t in sends]
        rb = [(p, torch_empty_like_host(t) if self.stage else t) for p, t in recvs]
        ops = [dist.P2POp(dist.isend, t, p) for p, t in sb] + [dist.P2POp(dist.irecv, t, p) for p, t in rb]
        for r in dist.batch_isend_irecv(ops):
            r.wait()
        if self.stage:
            for (p, t), (_, h) in zip(recvs, rb):
                t.copy_(h)


def torch_empty_like_host(t):
    import torch
    return torch.empty(t.shape, dtype=t.dtype, device="cpu")


class ShardedFilter:
    """Sync-free sharded filter step over a local PHDFilter (one per GPU).

    Per step k, all on torch's current stream (collectives and kernels are
    ordered without host waits):
      1. predict + update of the local shard, log-weights into w_local;
      2. settle step k-1's plan: its counts were read back asynchronously and are
         long complete (the update of step k is running); only when a peer had
         more than `block_records` records for this rank are the rest exchanged
         point to point and their slots re-updated — else nothing happens;
      3. all_gather of the log-weights; the plan (global normalise, nEff,
         decision, parents, migration, remap; one record per distinct parent and
         destination) packs FIXED blocks of `block_records` records per peer;
      4. one equal-split all_to_all of the blocks (every step: the host never
         learns the decision before it), and the receive into the deficit slots.
    With enable_trace (the mixed model: enable_trace_mixed), between 3's
    all_gather and its plan: every rank packs its trace block, one all_gather of
    the blocks, and the scan's record (the one a single context of all world * n
    particles writes) joins every rank's ring.
    flush() settles the last plan (before reading the store on the host).
    step_phases states this order, the one statement of it in Python; step()
    serves its collectives through `comm`, LocalWorld through device copies.
    Fix the local filter's update form (set_update_form / set_update_threads)
    before constructing: the plan stream beside part C is set up only for the
    split form found here (a later change stays correct — the all-gather waits
    on phd_wait_logw, which every form records — without the overlap).
    The record buffers are sized here, from f.record_bytes(): with the mixed
    model (feature_model 2) call f.enable_dynamic first — its records carry the
    dynamic map — and construct again after another dynamic capacity (the plan
    refuses records of a size the buffers were not made for).
    """

    def __init__(self, f, dist, device, world=None, rank=None, seed=0x9e3779b97f4a7c15, block_records=4, comm=None,
                 overlap=True):
        import torch
        self.f = f
        self.dist = dist
        self.device = device
        self.world = dist.get_world_size() if world is None else world
        self.rank = dist.get_rank() if rank is None else rank
        self.n = f.n
        self.N = self.n * self.world
        self.K = int(block_records)
        self.w_local = torch.empty(self.n, dtype=torch.float32, device=device)
        self.w_all = torch.empty(self.N, dtype=torch.float32, device=device)
        self.parents = torch.empty(self.N, dtype=torch.int32, device=device)
        self.keep_src = torch.empty(self.n, dtype=torch.int32, device=device)
        self.send_src = torch.empty(self.n * max(self.world - 1, 1), dtype=torch.int32, device=device)
        self.recv_rec = torch.empty(self.n, dtype=torch.int32, device=device)
        self.record_bytes = f.record_bytes()
        blk = self.world * self.K * self.record_bytes  # may be 0: every record then goes by overflow
        self.send_blocks = torch.empty(blk, dtype=torch.uint8, device=device)
        self.recv_blocks = torch.empty(blk, dtype=torch.uint8, device=device)
        # beyond the blocks: a rank sends at most n (world - 1) records, receives at most n
        self.ovf_capacity = self.n * max(self.world - 1, 1)
        self.ovf_send = torch.empty(self.ovf_capacity * self.record_bytes, dtype=torch.uint8, device=device)
        self.ovf_recv = torch.empty(self.n * self.record_bytes, dtype=torch.uint8, device=device)
        self.stats = {"resamples": 0, "migrated": 0, "records": 0, "overflow_records": 0, "pending_slots": 0}
        self.seed = seed  # shared by all ranks: identical resample uniforms
        self.new_logw = float(np.float32(-np.log(self.N)))
        self.comm = comm if comm is not None else (TorchComm(dist, device) if dist is not None else None)
        self._open = False
        self._ovf = ([], [])
        self.last = (None, None)
        f.set_stream(torch.cuda.current_stream(device).cuda_stream)
        f.set_index_offset(self.rank * self.n)
        # the all-gather and the plan on a second, high-priority stream beside the
        # update's part C (its log-weights are final after the CPHD terms / the
        # split PHD part A: phd_wait_logw); the pack waits for the plan
        self.trace_block = self.trace_blocks = None  # enable_trace / enable_trace_mixed
        self.trace_mixed = False
        self.eap_block = self.eap_blocks = None  # eap_pack
        self.eap_dyn_block = self.eap_dyn_blocks = None  # eap_dyn_pack
        self.aux = None
        if overlap and f.update_form():
            self.aux = torch.cuda.Stream(device=device, priority=-1)
            f.set_plan_stream(self.aux.cuda_stream)

    # The rank-local phases are separate methods; the generators below put them
    # in order, so the same code runs under torch.distributed (step) and as
    # several ranks of one process (LocalWorld).
    def local_update(self, control, k):
        """predict + update of the local shard (the predict fused into the update
        launch when it pays, as phd_step); log-weights into w_local (device)."""
        self.f.predict_update(control, k, self.w_local.data_ptr())

    def poll(self):
        """Counts of the open plan (waits only for that plan's read-back).
        Returns (neff, resampled); sets the overflow transfers of settle()."""
        if not self._open:
            return self.last
        # the C side closes the plan whichever way the poll ends (a capacity error
        # included): close it here first, so both sides agree and a later settle
        # does not poll again and mask the real error
        self._open = False
        neff, rs, demand, snd, rcv, pend = self.f.shard_poll(self.world)
        if rs:
            self.stats["resamples"] += 1
            self.stats["migrated"] += max(demand[self.rank] - self.n, 0)
            self.stats["records"] += sum(snd)
        self.stats["overflow_records"] += sum(max(c - self.K, 0) for c in snd)
        self.stats["pending_slots"] += pend
        sends, recvs = overflow_slices(snd, rcv, self.K, self.record_bytes)
        self._ovf = ([(d, self.ovf_send[lo:hi]) for d, lo, hi in sends],
                     [(s_, self.ovf_recv[lo:hi]) for s_, lo, hi in recvs])
        self.last = (neff, rs)
        return self.last

    def settle_finish(self, control=None, k=None):
        """After the overflow transfers: place those records, re-update their
        slots when an update (step k) already ran on them."""
        if self._ovf[1]:
            self.f.shard_receive_overflow(self.ovf_recv.data_ptr(), self.K, self.recv_rec.data_ptr())
            if k is not None:
                self.f.update_pending(control, k, self.w_local.data_ptr())
        self._ovf = ([], [])

    def gather(self):
        """The all-gather of the log-weights (beside part C on the plan stream)."""
        if self.aux is None:
            return AllGather(self.w_all, self.w_local, None, None)
        return AllGather(self.w_all, self.w_local, self.aux, self.f.wait_logw)

    def plan(self, k):
        """After the all-gather into w_all: the global plan, the fixed send blocks,
        the local remap — enqueued, nothing read back."""
        self.f.shard_resample_async(
            self.w_all.data_ptr(), self.world, self.rank, self.seed, k, self.parents.data_ptr(),
            self.keep_src.data_ptr(), self.send_src.data_ptr(), self.recv_rec.data_ptr(), self.send_blocks.data_ptr(),
            self.K, self.ovf_send.data_ptr(), self.ovf_capacity, self.new_logw)
        self._open = True

    def enable_trace(self, capacity, map_snapshot_cap=0, card_dist=False):
        """The per-scan estimate trace (PHDFilter.enable_trace) on the sharded
        step: every step() then appends the scan's record to the local filter's
        ring (read it with f.read_trace / f.trace_count).  capacity 0: off.  Same
        arguments on every rank."""
        import ctypes
        import torch
        from . import _lib
        self.trace_block = self.trace_blocks = None
        self.trace_mixed = False
        if capacity and card_dist and self.f.config.mapEstimate & 2:
            self.f.enable_trace(0)
            raise _lib.PHDError(_lib.PHD_E_UNSUPPORTED, "ShardedFilter.enable_trace",
                                "card_dist with map_estimate & 2: the expected rows are a sequential sum over "
                                "every rank's particles")
        self.f.enable_trace(capacity, map_snapshot_cap, card_dist)
        if not capacity:
            return
        nbytes = ctypes.c_size_t()
        _lib.check(_lib.lib().phd_trace_shard_block_bytes(self.n, int(map_snapshot_cap), self.f.trace_shape()[2],
                                                          ctypes.byref(nbytes)), "phd_trace_shard_block_bytes")
        self.trace_block = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
        self.trace_blocks = torch.empty(self.world * nbytes.value, dtype=torch.uint8, device=self.device)

    def enable_trace_mixed(self, capacity, map_snapshot_cap=0, dyn_snapshot_cap=0):
        """The estimate trace of the mixed model (PHDFilter.enable_trace_mixed,
        feature_model 2) on the sharded step: every step() then appends the
        scan's record and dyn record to the local filter's rings (f.read_trace /
        f.read_trace_dynamic / f.trace_count) — what a single mixed context of
        all world * n particles writes.  capacity 0: off, as enable_trace(0).
        Same arguments on every rank."""
        import ctypes
        import torch
        from . import _lib
        self.trace_block = self.trace_blocks = None
        self.trace_mixed = False
        self.f.enable_trace_mixed(capacity, map_snapshot_cap, dyn_snapshot_cap)
        if not capacity:
            return
        nbytes = ctypes.c_size_t()
        _lib.check(_lib.lib().phd_trace_shard_block_bytes_mixed(self.n, int(map_snapshot_cap), int(dyn_snapshot_cap),
                                                                ctypes.byref(nbytes)),
                   "phd_trace_shard_block_bytes_mixed")
        self.trace_block = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
        self.trace_blocks = torch.empty(self.world * nbytes.value, dtype=torch.uint8, device=self.device)
        self.trace_mixed = True

    def trace_pack(self, k):
        """After gather() and the settle, before plan(): this rank's trace block
        (the poses, cardinalities and arg-max rows of the store the plan remaps;
        with enable_trace_mixed the dynamic cardinalities and rows too)."""
        pack = self.f.trace_shard_pack_mixed if self.trace_mixed else self.f.trace_shard_pack
        pack(self.w_all.data_ptr(), self.world, self.rank, k, self.trace_block.data_ptr())

    def trace_append(self):
        """After the all-gather of the trace blocks into trace_blocks, before plan()
        (which normalises w_all in place)."""
        append = self.f.trace_shard_append_mixed if self.trace_mixed else self.f.trace_shard_append
        append(self.w_all.data_ptr(), self.trace_blocks.data_ptr(), self.world, self.rank)

    # -- the EAP expected map of the whole filter (phd_capi.h) -------------
    def eap_count(self):
        """This rank's component count (the store settled: after flush())."""
        return self.f.eap_shard_count()

    def eap_pack(self, k_max):
        """This rank's block for the stride k_max (the largest count over the
        ranks) into eap_block; eap_blocks takes the all-gather of the blocks."""
        import ctypes
        import torch
        from . import _lib
        nbytes = ctypes.c_size_t()
        _lib.check(_lib.lib().phd_eap_shard_block_bytes(int(k_max), ctypes.byref(nbytes)), "phd_eap_shard_block_bytes")
        if self.eap_block is None or self.eap_block.numel() != nbytes.value:
            self.eap_block = torch.empty(nbytes.value, dtype=torch.uint8, device=self.device)
            self.eap_blocks = torch.empty(self.world * nbytes.value, dtype=torch.uint8, device=self.device)
        self.f.eap_shard_pack(k_max, self.eap_block.data_ptr())

    def eap_finish(self, k_max, out_cap, blocks=None, world=None):
        """After the all-gather of the blocks (rank order) into eap_blocks: the
        expected map, reduced on this rank.  out_cap: the sum of the counts."""
        import ctypes
        from . import _lib
        blocks = self.eap_blocks if blocks is None else blocks
        world = self.world if world is None else int(world)
        nbytes = ctypes.c_size_t()
        _lib.check(_lib.lib().phd_eap_shard_block_bytes(int(k_max), ctypes.byref(nbytes)), "phd_eap_shard_block_bytes")
        if blocks is None or blocks.numel() != world * nbytes.value:
            raise _lib.PHDError(_lib.PHD_E_ARG, "ShardedFilter.eap_finish",
                                f"{world} blocks of k_max {k_max} are {world * nbytes.value} bytes, the buffer holds "
                                f"{0 if blocks is None else blocks.numel()}")
        return self.f.expected_map_blocks(blocks.data_ptr(), world, k_max, out_cap)

    def expected_map(self):
        """The EAP expected map of all world * n particles, on every rank: what
        PHDFilter.expected_map returns on a single context holding the ranks'
        settled stores in rank order, bit for bit (expected_map_phases)."""
        return self._serve(self.expected_map_phases(False))

    def expected_map_groups(self):
        """Decision rounds of the last expected_map (the single context's)."""
        return self.f.expected_map_groups()

    # -- the EAP map of the dynamic maps of the whole filter (feature_model 2) --
    def _eap_dyn_bytes(self, k_max):
        import ctypes
        from . import _lib
        nbytes = ctypes.c_size_t()
        _lib.check(_lib.lib().phd_eap_dyn_shard_block_bytes(int(k_max), ctypes.byref(nbytes)),
                   "phd_eap_dyn_shard_block_bytes")
        return nbytes.value

    def eap_dyn_count(self):
        """This rank's dynamic component count (the store settled: after flush())."""
        return self.f.eap_dyn_shard_count()

    def eap_dyn_pack(self, k_max):
        """This rank's "EAP4" block for the stride k_max (the largest count over
        the ranks) into eap_dyn_block; eap_dyn_blocks takes the all-gather."""
        import torch
        nbytes = self._eap_dyn_bytes(k_max)
        if self.eap_dyn_block is None or self.eap_dyn_block.numel() != nbytes:
            self.eap_dyn_block = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self.eap_dyn_blocks = torch.empty(self.world * nbytes, dtype=torch.uint8, device=self.device)
        self.f.eap_dyn_shard_pack(k_max, self.eap_dyn_block.data_ptr())

    def eap_dyn_finish(self, k_max, out_cap, blocks=None, world=None):
        """After the all-gather of the blocks (rank order) into eap_dyn_blocks:
        the dynamic expected map, reduced on this rank.  out_cap: the sum of the
        counts."""
        from . import _lib
        blocks = self.eap_dyn_blocks if blocks is None else blocks
        world = self.world if world is None else int(world)
        nbytes = self._eap_dyn_bytes(k_max)
        if blocks is None or blocks.numel() != world * nbytes:
            raise _lib.PHDError(_lib.PHD_E_ARG, "ShardedFilter.eap_dyn_finish",
                                f"{world} blocks of k_max {k_max} are {world * nbytes} bytes, the buffer holds "
                                f"{0 if blocks is None else blocks.numel()}")
        return self.f.expected_map_dynamic_blocks(blocks.data_ptr(), world, k_max, out_cap)

    def expected_map_dynamic(self):
        """The EAP map of the dynamic maps of all world * n particles, on every
        rank: what PHDFilter.expected_map_dynamic returns on a single mixed
        context holding the ranks' settled stores in rank order, bit for bit
        (expected_map_phases, on buffers of its own)."""
        return self._serve(self.expected_map_phases(True))

    def expected_map_dynamic_groups(self):
        """(rounds, cells) of the last expected_map_dynamic (the single context's cells)."""
        return self.f.expected_map_dynamic_groups()

    def set_expected_map_dynamic_mode(self, mode):
        self.f.set_expected_map_dynamic_mode(mode)

    def receive(self):
        """After the all-to-all of the blocks into recv_blocks."""
        self.f.shard_receive_blocks(self.recv_blocks.data_ptr(), self.K, self.recv_rec.data_ptr())

    # -- the order of the phases, and the collectives between them ----------
    def settle_phases(self, control=None, k=None):
        """Settle the open plan: poll, the overflow transfers, settle_finish."""
        out = self.poll()
        yield Exchange(*self._ovf)
        self.settle_finish(control, k)
        return out

    def step_phases(self, control, k):
        """One sharded step; returns what step() returns."""
        self.local_update(control, k)
        prev = yield from self.settle_phases(control, k)
        yield self.gather()
        if self.trace_block is not None:
            self.trace_pack(k)
            yield AllGather(self.trace_blocks, self.trace_block, None, None)
            self.trace_append()
        self.plan(k)
        yield AllToAll(self.recv_blocks, self.send_blocks)
        self.receive()
        return prev

    def expected_map_phases(self, dynamic):
        """The static (dynamic: the dynamic) expected map: settle the open plan,
        all-gather the component counts, pack this rank's block at the largest,
        all-gather the blocks, reduce them locally."""
        import torch
        count, pack, finish = ((self.eap_dyn_count, self.eap_dyn_pack, self.eap_dyn_finish) if dynamic else
                               (self.eap_count, self.eap_pack, self.eap_finish))
        yield from self.settle_phases(None, None)
        mine = torch.tensor([count()], dtype=torch.int64, device=self.device)
        counts = torch.empty(self.world, dtype=torch.int64, device=self.device)
        yield AllGather(counts, mine, None, None)
        counts = [int(c) for c in counts.tolist()]
        pack(max(counts))
        if dynamic:
            yield AllGather(self.eap_dyn_blocks, self.eap_dyn_block, None, None)
        else:
            yield AllGather(self.eap_blocks, self.eap_block, None, None)
        return finish(max(counts), sum(counts))

    def _serve(self, phases):
        """Run a phase generator on this rank, its collectives through comm."""
        comm = self.comm
        try:
            while True:
                c = next(phases)
                if type(c) is Exchange:
                    if c.sends or c.recvs:
                        comm.exchange(c.sends, c.recvs)
                elif type(c) is AllToAll:
                    comm.all_to_all_equal(c.out, c.inp)
                elif c.stream is None:
                    comm.all_gather(c.out, c.inp)
                else:
                    import torch
                    c.ready(c.stream.cuda_stream)
                    with torch.cuda.stream(c.stream):
                        comm.all_gather(c.out, c.inp)
        except StopIteration as done:
            return done.value

    def step(self, control, k):
        """One sharded filter step.  Returns (neff, resampled) of the PREVIOUS
        step's plan — its decision is only known once that plan is polled here
        (the current step's plan is polled by the next step, or by flush()); the
        first step returns (None, None).  The device store is final only after
        flush()."""
        return self._serve(self.step_phases(control, k))

    def settle(self, control=None, k=None):
        return self._serve(self.settle_phases(control, k))

    def flush(self):
        """Settle the last plan (no update follows): the store is then final."""
        return self._serve(self.settle_phases(None, None))


class LocalWorld:
    """The `world` ranks of a sharded filter in one process on one device:
    ShardedFilter(f, None, device, world=..., rank=r) for r = 0 .. world - 1,
    without a transport of their own.  Every call advances each rank's phase
    generator to its next collective, requires all ranks to have arrived at the
    same kind, and serves it with device copies between the ranks' buffers.
    Each returns the ranks' results in rank order."""

    def __init__(self, shards):
        self.shards = list(shards)
        for r, sf in enumerate(self.shards):
            if sf.rank != r or sf.world != len(self.shards):
                raise ValueError(f"shard {r} of {len(self.shards)} is rank {sf.rank} of world {sf.world}")

    def step(self, control, k):
        return self._serve([sf.step_phases(control, k) for sf in self.shards])

    def flush(self):
        return self._serve([sf.settle_phases(None, None) for sf in self.shards])

    def expected_map(self):
        return self._serve([sf.expected_map_phases(False) for sf in self.shards])

    def expected_map_dynamic(self):
        return self._serve([sf.expected_map_phases(True) for sf in self.shards])

    def _serve(self, phases):
        results = [None] * len(phases)
        while True:
            calls = []
            for r, g in enumerate(phases):
                try:
                    calls.append(next(g))
                except StopIteration as done:
                    results[r] = done.value
                    calls.append(None)
            kinds = set(type(c) for c in calls)
            if len(kinds) != 1:
                raise RuntimeError("the ranks diverged: " + ", ".join(
                    f"rank {r} {'returned' if c is None else 'at ' + type(c).__name__}" for r, c in enumerate(calls)))
            if calls[0] is None:
                return results
            _LOCAL[kinds.pop()](calls)


def local_all_gather(calls):
    """The ranks' inputs, in rank order, into every rank's output.  On a rank's
    stream: after every rank's input is ready for that stream."""
    import torch
    for c in calls:
        if c.stream is None:
            c.out.copy_(torch.cat([o.inp for o in calls]))
            continue
        for o in calls:
            o.ready(c.stream.cuda_stream)
        with torch.cuda.stream(c.stream):
            c.out.copy_(torch.cat([o.inp for o in calls]))


def local_all_to_all(calls):
    """Block d of every rank to rank d, in source-rank order."""
    import torch
    blk = calls[0].inp.numel() // len(calls)
    if blk == 0:
        return
    for d, c in enumerate(calls):
        c.out.copy_(torch.cat([s.inp[d * blk:(d + 1) * blk] for s in calls]))


def local_exchange(calls):
    """Every receive buffer of rank r from source s takes the one send of s
    addressed to r; every send is taken."""
    taken = 0
    for r, c in enumerate(calls):
        for s, buf in c.recvs:
            src = [t for d, t in calls[s].sends if d == r]
            if len(src) != 1:
                raise RuntimeError(f"rank {r} receives from rank {s}, which has {len(src)} sends for it")
            if src[0].numel() != buf.numel():
                raise RuntimeError(f"rank {s} sends {src[0].numel()} elements to rank {r}, which expects {buf.numel()}")
            buf.copy_(src[0])
            taken += 1
    if taken != sum(len(c.sends) for c in calls):
        raise RuntimeError(f"{sum(len(c.sends) for c in calls)} sends for {taken} receives")


_LOCAL = {AllGather: local_all_gather, AllToAll: local_all_to_all, Exchange: local_exchange}


class GroupRank:
    """The sharded step of ShardedFilter as ONE C call per step: this process's
    rank of an RCCL group driven by the C++ host (libphdslam_group.so,
    include/phd_group.h: phd_group_create_rank + phd_group_step).  The
    communicator is RCCL's own (ncclCommInitRank); its unique id is made on rank
    0 and broadcast over the torch.distributed group `dist`.  Same step, same
    plans, same results bit for bit as ShardedFilter (tests/test_gpu_parity.py::
    test_group_rank_matches_sharded_filter); the Python dispatch of the step's
    phases (poll, all-gather on the plan stream, plan, all-to-all, unpack) is
    gone from the step.  The local filter's update form is fixed before
    construction (phd_group.h)."""

    def __init__(self, f, dist, device, world=None, rank=None, seed=0x9e3779b97f4a7c15, block_records=4,
                 unique_id=None):
        import ctypes
        from . import _lib
        self.f = f
        self.world = dist.get_world_size() if world is None else world
        self.rank = dist.get_rank() if rank is None else rank
        self.n = f.n
        self.K = int(block_records)
        self.L = group_lib()
        if unique_id is None:
            uid = bytearray(128)
            if self.rank == 0:
                buf = (ctypes.c_char * 128).from_buffer(uid)
                _group_check(self.L, self.L.phd_group_unique_id(buf, 128), "phd_group_unique_id")
            if self.world > 1:
                obj = [bytes(uid)]
                dist.broadcast_object_list(obj, src=0)
                uid = bytearray(obj[0])
            unique_id = bytes(uid)
        self._uid = ctypes.create_string_buffer(bytes(unique_id), 128)
        f.set_stream(__import__("torch").cuda.current_stream(device).cuda_stream)
        h = ctypes.c_void_p()
        _group_check(self.L, self.L.phd_group_create_rank(ctypes.byref(h), f.handle, int(device.index or 0),
                                                         self.world, self.rank, self._uid, self.K,
                                                         ctypes.c_uint64(seed)), "phd_group_create_rank")
        self._g = h
        self.last = (None, None)
        _lib.lib()  # (the product library is loaded first: the group library resolves against it)

    def step(self, control, k):
        """One sharded step; returns the PREVIOUS step's (neff, resampled)."""
        import ctypes
        from .types import AckermanControl
        u = ctypes.byref(AckermanControl(float(control[1]), float(control[0]))) if control is not None else None
        ne, rs = ctypes.c_float(), ctypes.c_int()
        _group_check(self.L, self.L.phd_group_step(self._g, u, ctypes.c_uint64(int(k)), ctypes.byref(ne),
                                                   ctypes.byref(rs)), "phd_group_step")
        self.last = (ne.value, rs.value) if rs.value >= 0 else (None, None)
        return self.last

    def enable_trace(self, capacity, map_snapshot_cap=0, card_dist=False):
        """phd_group_trace_enable: as ShardedFilter.enable_trace (records through
        the local filter's read_trace / trace_count)."""
        from .types import TRACE_CARD_DIST
        _group_check(self.L, self.L.phd_group_trace_enable(self._g, int(capacity), int(map_snapshot_cap),
                                                           TRACE_CARD_DIST if card_dist else 0),
                     "phd_group_trace_enable")

    def enable_trace_mixed(self, capacity, map_snapshot_cap=0, dyn_snapshot_cap=0):
        """phd_group_trace_enable_mixed: as ShardedFilter.enable_trace_mixed
        (records through the local filter's read_trace / read_trace_dynamic)."""
        _group_check(self.L, self.L.phd_group_trace_enable_mixed(self._g, int(capacity), int(map_snapshot_cap),
                                                                 int(dyn_snapshot_cap), 0),
                     "phd_group_trace_enable_mixed")

    def flush(self):
        _group_check(self.L, self.L.phd_group_flush(self._g), "phd_group_flush")

    def expected_map(self):
        """phd_group_expected_map: as ShardedFilter.expected_map (settles the
        open plan first; every rank calls it and receives the same map)."""
        import ctypes
        import numpy as np
        from .types import GAUSSIAN2D
        cap = self.world * self.n * int(self.f.capacity.map_capacity)
        out = np.zeros(max(cap, 1), GAUSSIAN2D)
        nout = ctypes.c_long()
        _group_check(self.L, self.L.phd_group_expected_map(self._g, out.ctypes.data_as(ctypes.c_void_p), cap,
                                                           ctypes.byref(nout)), "phd_group_expected_map")
        return out[:nout.value].copy()

    def expected_map_groups(self):
        return self.f.expected_map_groups()

    def expected_map_dynamic(self):
        """phd_group_expected_map_dynamic: as ShardedFilter.expected_map_dynamic
        (a mixed filter; settles the open plan first; the same map on every rank)."""
        import ctypes
        import numpy as np
        from .types import GAUSSIAN4D
        cap = self.world * self.n * int(self.f.dyn_capacity)
        out = np.zeros(max(cap, 1), GAUSSIAN4D)
        nout = ctypes.c_long()
        _group_check(self.L, self.L.phd_group_expected_map_dynamic(self._g, out.ctypes.data_as(ctypes.c_void_p), cap,
                                                                   ctypes.byref(nout)),
                     "phd_group_expected_map_dynamic")
        return out[:nout.value].copy()

    def expected_map_dynamic_groups(self):
        return self.f.expected_map_dynamic_groups()

    def set_expected_map_dynamic_mode(self, mode):
        self.f.set_expected_map_dynamic_mode(mode)

    @property
    def stats(self):
        import ctypes
        out = (ctypes.c_longlong * 5)()
        _group_check(self.L, self.L.phd_group_stats(self._g, out), "phd_group_stats")
        return {"resamples": out[0], "migrated": out[1], "records": out[2], "overflow_records": out[3],
                "pending_slots": out[4]}

    def close(self):
        if self._g:
            self.L.phd_group_destroy(self._g)
            self._g = None


_GROUP = None


def group_lib():
    """libphdslam_group.so (built in-tree by build.py next to libphdslam.so)."""
    global _GROUP
    if _GROUP is None:
        import ctypes
        import os
        from . import _lib
        _lib.lib()
        path = os.path.join(os.path.dirname(os.path.abspath(_lib.LIB_PATH)), "libphdslam_group.so")
        if not os.path.exists(path):
            raise OSError(f"{path} not found: build it with `python cuda-phdslam_amd/build.py`")
        L = ctypes.CDLL(path)
        vp = ctypes.c_void_p
        L.phd_group_unique_id.argtypes = [vp, ctypes.c_size_t]
        L.phd_group_create_rank.argtypes = [ctypes.POINTER(vp), vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, vp,
                                            ctypes.c_int, ctypes.c_uint64]
        L.phd_group_step.argtypes = [vp, vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_float),
                                     ctypes.POINTER(ctypes.c_int)]
        L.phd_group_flush.argtypes = [vp]
        L.phd_group_expected_map.argtypes = [vp, vp, ctypes.c_long, ctypes.POINTER(ctypes.c_long)]
        L.phd_group_expected_map_dynamic.argtypes = [vp, vp, ctypes.c_long, ctypes.POINTER(ctypes.c_long)]
        L.phd_group_trace_enable.argtypes =[vp, ctypes.c_int, ctypes.c_int, ctypes.c_uint]
        L.phd_group_trace_enable_mixed.argtypes = [vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint]
        L.phd_group_stats.argtypes = [vp, vp]
        L.phd_group_destroy.argtypes = [vp]
        L.phd_group_last_error.restype = ctypes.c_char_p
        _GROUP = L
    return _GROUP


def _group_check(L, rc, where):
    if rc != 0:
        from ._lib import PHDError
        raise PHDError(rc, where, (L.phd_group_last_error() or b"").decode())
