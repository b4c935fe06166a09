"""The migration plan of a sharded resample in plain Python integers, written
from the rule as include/phd_capi.h (phd_shard_resample,
phd_shard_resample_async, phd_shard_poll) and the comment above
migration_plan_block (csrc/phd_kernels.hip) state it.

TEST INFRASTRUCTURE ONLY.  It imports neither phdslam.dist nor the oracle, and
it does not restate the kernel's arithmetic (rank boundaries by search, prefix
ranges of surplus and deficit): it walks the children one by one.

The rule.  Rank s of `world` owns the parents [s n, (s + 1) n).  The parent
list (one parent per stratum, N = world n strata, identical on every rank) is
nondecreasing, except that strata past the CDF's end take the first maximum pm
and so may form a trailing run that drops below the stratum before it.  Such a
run is read as children of pm's rank, placed after that rank's other children.
Grouped so, rank s has demand[s] children in stratum order.  Its first
min(demand, n) children stay (keep: their local parents, new slots 0 ..); the
rest are its part of the job-wide surplus sequence (ranks in order, each rank's
children beyond n in stratum order).  The deficit slots — slot demand[s] + i of
every rank short of n children, ranks in order — take the surplus sequence one
by one.  Children of one parent are identical, so a sender ships one record
per run of surplus children with the same (source, parent, destination), and
every slot fed by that run points at the one record.  (A parent whose children
form two runs — the moved trailing run behind other parents of its rank — gets
a record per run, also towards the same destination; sender and receiver count
alike.)  A rank numbers the records it sends by destination ascending, the
records it receives by source ascending; with fixed blocks of K records per
peer, a record whose index among the records of its (source, destination) pair
is >= K travels by overflow, and the slots it feeds are pending.

Without a resample (flag 0) nothing moves: demand n everywhere, identity keep,
every count zero.
"""
import numpy as np


class Plan:
    """The plan of every rank.  Per-rank accessors return plain lists / arrays."""

    def __init__(self, n, world, K, resampled):
        self.n, self.world, self.K, self.resampled = n, world, K, bool(resampled)
        self.view = []        # the rank-grouped parent list
        self.ins = None       # view position of the moved run (None: nothing moved)
        self.beyond = 0       # length of the trailing run that dropped
        self.demand = [n] * world
        self._keep = {}       # rank -> local parents of the kept children
        self._send_src = {}   # source -> local parent of each record, in sending order
        self._send_dst = {}   # source -> destination of each record
        self._pair = {}       # (source, destination) -> records
        self._recv_rec = {}   # destination -> record index of each deficit slot
        self._within = {}     # destination -> (deficit slot, its record's index among its source's records)
        self.moves = []       # (source, parent, destination, slot) of every surplus child

    def keep(self, s):
        return np.asarray(self._keep.get(s, range(self.n) if not self.resampled else []), np.int32)

    def send_src(self, s):
        return np.asarray(self._send_src.get(s, []), np.int32)

    def send_dst(self, s):
        return list(self._send_dst.get(s, []))

    def send_records(self, s):
        return [self._pair.get((s, d), 0) for d in range(self.world)]

    def recv_records(self, d):
        return [self._pair.get((s, d), 0) for s in range(self.world)]

    def recv_rec(self, d):
        return np.asarray(self._recv_rec.get(d, []), np.int32)

    def pending(self, d, K=None):
        """The deficit slots of rank d whose record lies beyond a block of K records."""
        K = self.K if K is None else K
        return [q for q, within in self._within.get(d, []) if within >= K]

    def settled(self, d, K=None):
        K = self.K if K is None else K
        return [q for q, within in self._within.get(d, []) if within < K]

    def overflow_send(self, s, K=None):
        K = self.K if K is None else K
        return sum(max(c - K, 0) for c in self.send_records(s))

    def overflow_recv(self, d, K=None):
        K = self.K if K is None else K
        return sum(max(c - K, 0) for c in self.recv_records(d))


def trailing_run(parents):
    """Length of the trailing run that drops below the stratum before it (0: the
    list is nondecreasing)."""
    parents = [int(p) for p in parents]
    drop = None
    for j in range(1, len(parents)):
        if parents[j] < parents[j - 1]:
            assert drop is None, f"the parent list drops twice (strata {drop} and {j})"
            drop = j
    if drop is None:
        return 0
    assert all(p == parents[-1] for p in parents[drop:]), "the trailing run has one parent"
    return len(parents) - drop


def plan(parents, n, world, K, resampled=True):
    parents = [int(p) for p in parents]
    N = n * world
    assert len(parents) == N
    P = Plan(n, world, K, resampled)
    if not resampled:
        return P
    # the rank-grouped view
    P.beyond = trailing_run(parents)
    children = [[] for _ in range(world)]
    for p in parents[:N - P.beyond]:
        assert 0 <= p < N
        children[p // n].append(p)
    if P.beyond:
        pm = parents[-1]
        later = sum(len(c) for c in children[pm // n + 1:])
        if later:
            P.ins = N - P.beyond - later
        children[pm // n].extend([pm] * P.beyond)
    for s in range(world):
        P.view.extend(children[s])
        P.demand[s] = len(children[s])
        P._keep[s] = [p - s * n for p in children[s][:n]]
    # the surplus sequence onto the deficit slots
    surplus = [(s, p) for s in range(world) for p in children[s][n:]]
    slots = [(d, q) for d in range(world) for q in range(P.demand[d], n)]
    assert len(surplus) == len(slots)
    last = None          # (source, parent, destination) of the child before
    index = {}           # (source, parent, destination) -> its open record, as received
    arrived = {}         # destination -> records so far
    for (s, p), (d, q) in zip(surplus, slots):
        key = (s, p, d)
        if key != last:  # a new run: a new record
            index[key] = (arrived.get(d, 0), P._pair.get((s, d), 0))
            arrived[d] = arrived.get(d, 0) + 1
            P._pair[(s, d)] = P._pair.get((s, d), 0) + 1
            P._send_src.setdefault(s, []).append(p - s * n)
            P._send_dst.setdefault(s, []).append(d)
            last = key
        rec, within = index[key]
        P._recv_rec.setdefault(d, []).append(rec)
        P._within.setdefault(d, []).append((q, within))
        P.moves.append((s, p, d, q))
    for s, dst in P._send_dst.items():
        assert dst == sorted(dst), "a rank's records go out by destination ascending"
    return P
