"""The plain-integer reference of the sharded migration plan
(tests/shard_plan_ref.py) on the CPU, on the parents weighting_ref.parents gives
for every shared case (tests/shard_plan_cases.py):

1. the input condition of every case from the reference alone (no near
   decision, at most 1 % near strata: weighting_cases.hold_parents' cap);
2. the product's host statements of the plan — phdslam.dist.plan_migration
   (with the device's record fold), migration_counts, overflow_slices — held
   to the reference;
3. properties of the reference itself: the kept and received children are the
   parent list as a multiset, no child of a local parent moves while its rank
   has a deficit, sends equal receives pair by pair, pending and settled slots
   make up the deficit slots.

`python tests/test_shard_plan_ref.py --tie` prints the (seed, step) pairs of the
overrun cases from the current oracle.
"""
import collections
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import shard_plan_cases as SC  # noqa: E402
import shard_plan_ref as S  # noqa: E402
import weighting_cases as C  # noqa: E402
import weighting_ref as R  # noqa: E402

SHAPE_IDS = [SC.key(s) for s in SC.SHAPES]
RECORD_BYTES = 1824  # (any positive size: the slices scale with it)


def _fold(local_parents):
    """One record per run of equal parents (as test_gpu_parity._plan_reference)."""
    out, prev = [], None
    for q in local_parents:
        if q != prev:
            out.append(q)
        prev = q
    return out


def _hold_host_statements(parents, n, world, P):
    """phdslam.dist's plan_migration / migration_counts / overflow_slices against the plan P."""
    from phdslam.dist import migration_counts, overflow_slices, plan_migration
    plans = plan_migration(parents, n, world)
    moved = {}
    for s, p, d, _ in P.moves:
        moved.setdefault((s, d), []).append(p - s * n)
    for r in (range(world) if world <= 64 else SC.checked_ranks(P, 0)):
        h = plans[r]
        np.testing.assert_array_equal(h["keep"], P.keep(r))
        assert sorted(h["send"]) == sorted(d for (s, d) in moved if s == r)
        recs = []
        for d in sorted(h["send"]):
            assert h["send"][d].tolist() == moved[(r, d)], (r, d)
            folded = _fold(h["send"][d].tolist())
            assert len(folded) == P.send_records(r)[d], (r, d)
            recs += folded
        np.testing.assert_array_equal(recs, P.send_src(r))
        assert {s: c for s, c in h["recv"].items()} == {s: len(v) for (s, d), v in moved.items() if d == r}
        keep, send, recv = migration_counts(P.demand, n, world, r)
        assert keep == len(P.keep(r)) == min(P.demand[r], n)
        assert send == [len(moved.get((r, d), [])) for d in range(world)]
        assert recv == [len(moved.get((s, r), [])) for s in range(world)]
        for K in SC.KS(n):
            snd, rcv = overflow_slices(P.send_records(r), P.recv_records(r), K, RECORD_BYTES)
            for got, counts, total in ((snd, P.send_records(r), P.overflow_send(r, K)),
                                       (rcv, P.recv_records(r), P.overflow_recv(r, K))):
                o, want = 0, []
                for peer, c in enumerate(counts):  # per peer in rank order, its records K .. c - 1
                    if c > K:
                        want.append((peer, o * RECORD_BYTES, (o + c - K) * RECORD_BYTES))
                        o += c - K
                assert got == want and o == total


def _hold_properties(parents, n, world, P):
    got = collections.Counter()
    for s in range(world):
        got.update((P.keep(s).astype(np.int64) + s * n).tolist())
    got.update(p for _, p, _, _ in P.moves)
    assert got == collections.Counter(int(p) for p in parents), "kept + received children are the parent list"
    for s, p, d, q in P.moves:
        assert p // n == s and s != d and P.demand[s] > n and P.demand[d] <= q < n
    pair = collections.Counter((s, d) for s, _, d, _ in P.moves)
    for s in range(world) if world <= 64 else (0, world // 2, world - 1):
        for d in range(world):
            assert (P.send_records(s)[d] > 0) == (pair[(s, d)] > 0)
            assert P.send_records(s)[d] == P.recv_records(d)[s] <= pair[(s, d)]
    assert sum(len(P.send_src(s)) for s in range(world)) == sum(P._pair.values())
    for d in range(world):
        slots = list(range(min(P.demand[d], n), n))
        assert len(P.keep(d)) + len(slots) == n
        for K in SC.KS(n):
            assert sorted(P.pending(d, K) + P.settled(d, K)) == slots
        assert P.pending(d, 0) == slots and P.pending(d, n) == []
        rec = P.recv_rec(d)
        assert len(rec) == len(slots)
        if len(rec):  # records are numbered in the order they arrive, every one used
            assert rec[0] == 0 and set(np.diff(rec).tolist()) <= {0, 1} and rec[-1] + 1 == sum(P.recv_records(d))


# ------------------------------------------------------------- hand-made lists

def test_hand_made_plan():
    """world 3, n 4: rank 0 has 7 children (parents 1 1 1 2 2 2 2), rank 1 has 1, rank 2 has 4."""
    parents = [1, 1, 1, 2, 2, 2, 2, 5, 8, 8, 9, 11]
    P = S.plan(parents, 4, 3, 1)
    assert P.demand == [7, 1, 4] and P.beyond == 0 and P.ins is None
    assert P.keep(0).tolist() == [1, 1, 1, 2] and P.keep(1).tolist() == [1] and P.keep(2).tolist() == [0, 0, 1, 3]
    assert P.send_src(0).tolist() == [2] and P.send_records(0) == [0, 1, 0] and P.recv_records(1) == [1, 0, 0]
    assert P.recv_rec(1).tolist() == [0, 0, 0] and P.pending(1, 1) == [] and P.pending(1, 0) == [1, 2, 3]
    assert P.overflow_send(0, 0) == 1 and P.overflow_recv(1, 0) == 1 and P.overflow_send(0, 1) == 0
    _hold_host_statements(np.array(parents), 4, 3, P)
    _hold_properties(parents, 4, 3, P)


def test_hand_made_two_sources_two_parents():
    """world 4, n 3: ranks 0 and 3 hold the surplus (4 and 2), ranks 1 and 2 the deficit (3 and 3)."""
    parents = [0, 0, 1, 1, 1, 2, 2, 9, 9, 10, 10, 11]
    P = S.plan(parents, 3, 4, 1)
    assert P.demand == [7, 0, 0, 5]
    assert [(s, p, d, q) for s, p, d, q in P.moves] == [(0, 1, 1, 0), (0, 1, 1, 1), (0, 2, 1, 2), (0, 2, 2, 0),
                                                        (3, 10, 2, 1), (3, 11, 2, 2)]
    assert P.send_src(0).tolist() == [1, 2, 2] and P.send_dst(0) == [1, 1, 2] and P.send_records(0) == [0, 2, 1, 0]
    assert P.send_src(3).tolist() == [1, 2] and P.recv_records(2) == [1, 0, 0, 2]
    assert P.recv_rec(1).tolist() == [0, 0, 1] and P.recv_rec(2).tolist() == [0, 1, 2]
    assert P.pending(1, 1) == [2] and P.pending(2, 1) == [2] and P.overflow_send(0, 1) == 1 == P.overflow_recv(2, 1)
    _hold_host_statements(np.array(parents), 3, 4, P)
    _hold_properties(parents, 3, 4, P)


def test_hand_made_moved_suffix():
    """The last two strata past the CDF's end take the first maximum 4 (rank 1
    of 3, n 4): read as rank 1's children after its other child (of 5), in front
    of rank 2's — the host statement is held on the moved list.  Parent 4's
    surplus children form two runs towards rank 0: a record each."""
    parents = [4, 4, 4, 4, 4, 5, 8, 9, 10, 11, 4, 4]
    P = S.plan(parents, 4, 3, 1)
    assert P.beyond == 2 and P.ins == 6 and P.view == [4, 4, 4, 4, 4, 5, 4, 4, 8, 9, 10, 11]
    assert P.demand == [0, 8, 4] and P.keep(1).tolist() == [0, 0, 0, 0] and P.keep(2).tolist() == [0, 1, 2, 3]
    # surplus 4 5 4 4 -> rank 0's slots 0 1 2 3
    assert P.send_src(1).tolist() == [0, 1, 0] and P.send_dst(1) == [0, 0, 0] and P.send_records(1) == [3, 0, 0]
    assert P.recv_rec(0).tolist() == [0, 1, 2, 2] and P.recv_records(0) == [0, 3, 0]
    assert P.pending(0, 1) == [1, 2, 3] and P.pending(0, 3) == [] and P.overflow_recv(0, 1) == 2
    _hold_host_statements(np.array(P.view), 4, 3, P)
    _hold_properties(parents, 4, 3, P)
    # a run that already sits at the end of its rank is not moved
    Q = S.plan([0, 1, 2, 3, 4, 5, 6, 7, 9, 10, 8, 8], 4, 3, 1)
    assert Q.beyond == 2 and Q.ins is None and Q.demand == [4, 4, 4]


def test_no_resample_is_the_identity():
    P = S.plan(list(range(12)), 4, 3, 1, resampled=False)
    assert P.demand == [4, 4, 4] and P.keep(2).tolist() == [0, 1, 2, 3] and P.moves == []
    assert P.send_records(1) == [0, 0, 0] == P.recv_records(1) and P.pending(1, 0) == [] and len(P.send_src(0)) == 0


# ------------------------------------------------------------------- the cases

def _oracle_for_tie(request, shape):
    if shape[2] == "tie":  # (its parents are taken on the oracle's normalised weights)
        request.getfixturevalue("built")


@pytest.mark.parametrize("wcase", SC.WCASES, ids=[C.key(c) for c in SC.WCASES])
def test_case_conditions_from_the_reference_alone(request, wcase):
    """No near decision (asked for, and at threshold 0), at most 1 % near strata."""
    wn, dec = C.reference(wcase)
    assert dec.resample and not dec.near, dec
    d0 = R.decision(C.weights(wcase[3], wcase[2]), 0.0)
    assert not d0.resample and not d0.near, d0
    shape = next(s for s in SC.SHAPES if SC.wcase(s) == wcase)
    _oracle_for_tie(request, shape)
    p = SC.reference_parents(shape)
    assert p.near.sum() <= 0.01 * len(p.parent), (int(p.near.sum()), len(p.parent))


@pytest.mark.parametrize("shape", SC.SHAPES, ids=SHAPE_IDS)
def test_branches_reached(request, shape):
    """Each distribution reaches what its shape is listed for."""
    _oracle_for_tie(request, shape)
    world, n, dist = shape
    P, p = SC.reference_plan(shape), SC.reference_parents(shape)
    N = world * n
    if dist == "flat":  # the identity, but for a stratum drawn within the float32 rounding of -log N of its edge
        assert np.abs(p.parent - np.arange(N)).max() <= 1 and (p.parent != np.arange(N)).sum() <= 0.002 * N + 1
        assert len(P.moves) <= 0.002 * N + 1
    if dist == "sparse":
        assert min(P.demand) < n < max(P.demand) and sum(d > 0 for d in P.demand) > world // 2
    if dist == "one":
        assert sorted(P.demand)[-1] == N and (world == 1 or sorted(P.demand)[-2] == 0)
        src = (3 * N // 4) // n
        assert P.send_records(src) == [0 if d == src else 1 for d in range(world)]
    if dist == "two_far" and world >= 3 and n >= 8:  # (entries 5 and N - 7 hold the mass)
        assert P.demand[0] > n and P.demand[-1] > n and all(d < n for d in P.demand[1:-1])
    if dist == "holes" and world >= 64:
        assert any(a == 0 and b == 0 for a, b in zip(P.demand, P.demand[1:])), "two ranks in a row with demand 0"
    if dist == "tie":
        assert p.beyond.size >= 1 and P.beyond == p.beyond.size and P.ins is not None and P.ins < N - P.beyond
        assert p.amax == N // 3 and p.amax // n not in (world - 1, int(p.parent[N - P.beyond - 1]) // n)
    if world == 1:
        assert P.moves == [] and P.demand == [n]


@pytest.mark.parametrize("shape", SC.SHAPES, ids=SHAPE_IDS)
def test_host_statements_against_reference(request, shape):
    _oracle_for_tie(request, shape)
    world, n, _ = shape
    P = SC.reference_plan(shape)
    # plan_migration takes the list grouped by rank (the device reads it through parent_view)
    _hold_host_statements(np.asarray(P.view), n, world, P)


@pytest.mark.parametrize("shape", SC.SHAPES, ids=SHAPE_IDS)
def test_reference_properties(request, shape):
    _oracle_for_tie(request, shape)
    world, n, _ = shape
    _hold_properties(SC.reference_parents(shape).parent, n, world, SC.reference_plan(shape))


@pytest.mark.parametrize("wcase", SC.WCASES, ids=[C.key(c) for c in SC.WCASES])
def test_oracle_against_reference(built, wcase):
    """weighting_cases.D_ORACLE of the gathered sizes is the oracle's measured
    deviation (as tests/test_weighting_ref.py holds the other keys)."""
    from test_weighting_ref import oracle_figures
    _, d_w, d_neff = oracle_figures(wcase)
    k = C.key(wcase)
    print(f"{k}: lognorm {d_w:.3g}, neff {d_neff:.3g}")
    for name, got in (("lognorm", d_w), ("neff", d_neff)):
        want = C.D_ORACLE[k][name]
        assert got <= want, (k, name, got, want)
        assert want <= 2 * got + 1e-12, (k, name, "table entry is stale", got)


@pytest.mark.parametrize("shape", [s for s in SC.SHAPES if s[2] == "tie"], ids=SC.key)
def test_tie_pairs_overrun(built, shape):
    """The committed (seed, step): a stratum past the CDF's end on the oracle's normalised weights."""
    from test_weighting_ref import oracle_normalised
    ref = R.parents(oracle_normalised(SC.wcase(shape)), SC.uniforms(shape))
    assert ref.beyond.size >= 1 and ref.amax == shape[0] * shape[1] // 3


def _find_tie_pairs():
    """The first step at which the last stratum's draw lies past the CDF's end of
    the oracle's float32 normalised weights, by half the gap to one or more."""
    from test_weighting_ref import oracle_normalised
    out = {}
    for world, n in SC.TIE_SHAPES:
        N = world * n
        wc = ("shard", "phd", N, "tie")
        totals = [np.cumsum(np.exp(w.astype(np.float64)))[-1]
                  for w in (oracle_normalised(wc), C.reference(wc)[0].astype(np.float32))]
        total = totals[0]  # (the reference's own rounding of these weights ends above one)
        steps = np.arange(1, 4000001, dtype=np.uint64)
        x0 = R.philox4x32_10([N - 1, steps, 0, R.STREAM_RESAMPLE], [C.SEED & 0xFFFFFFFF, C.SEED >> 32])[0]
        r = (N - 1 + x0.astype(np.float64) * 2.0 ** -32) / N
        hit = np.flatnonzero(r > total + 0.5 * (1.0 - total))
        out[N] = (C.SEED, int(steps[hit[0]])) if hit.size else None
        print(N, "totals", totals, "first steps", steps[hit[:5]])
    return out


if __name__ == "__main__":
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "oracle"))
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "cuda-phdslam_amd"))
    if "--tie" in sys.argv:
        print("TIE_SEED_STEP =", _find_tie_pairs())
