"""Shared cases of the sharded-plan tests (tests/test_shard_plan_ref.py on the
CPU, tests/test_gpu_shard_plan.py on the device).

A case is (world, n, dist, K): `world` ranks of n particles, the gathered
log-weights weighting_cases.weights(dist, world n) — N = world n plays the role
of the standalone n — and blocks of K records per peer (the async form; the
synchronous form has no blocks).  SHAPES lists (world, n, dist); KS(n) the
block sizes of each.
"""
import functools

import numpy as np

import shard_plan_ref as S
import weighting_cases as C
import weighting_ref as R

DISTS = ("normal", "flat", "one", "two_far", "holes", "wide")
ORDER = DISTS + ("sparse", "tie")

# (world, n): the smallest shape that reaches each branch
#   (1, 64)                            world 1: nothing can move, no send blocks
#   (2, 8), (3, 5), (8, 4)             tiny and odd shards, fewer entries than a wave
#   (3, 341), (4, 256), (5, 205)       N = 1023, 1024, 1025: the chunk edge
#   (4, 1024), (4, 1025)               the last fully staged CDF (4 chunks) and the first that is not
#   (64, 33), (65, 17)                 a wave of ranks, and one rank more
#   (1024, 2), (1024, 3)               MIG_MAX_WORLD: one thread per rank in the tail, T.pre[world]
#   (1024, 128), (1024, 129)           N = 131072: sample stride 64 with ns = 2048; N = 132096: stride 128
#   (1024, 257)                        257 chunks: the synchronous call's chain fallback (<= 256 compute units)
EVERY_DIST = [(3, 5), (5, 205), (4, 1025), (65, 17)]
SOME = {
    (1, 64): ("normal",),
    (2, 8): ("normal", "one", "two_far"),
    (8, 4): ("normal", "one", "two_far"),          # demand 0 on several ranks in a row
    (3, 341): ("normal", "two_far"),
    (4, 256): ("normal", "two_far"),
    (4, 1024): ("normal", "two_far", "holes"),
    (64, 33): ("normal", "one", "two_far", "holes"),
    (1024, 2): ("normal", "one", "two_far", "holes"),
    (1024, 3): ("normal", "one", "two_far", "holes"),
    # from N = 131072 on `normal` and `holes` leave more than 1 % of the strata near on the reference's own
    # weights (1.5 % and 1.4 %; 3.3 % at 263168: the band is fixed, the strata narrow as 1 / N), so
    # `sparse` — `normal` on every eighth entry, parents on every rank — stands in for them
    (1024, 128): ("sparse", "one", "two_far"),     # one: a record to each of 1023 ranks
    (1024, 129): ("sparse", "one", "two_far"),
    (1024, 257): ("sparse", "two_far"),
}
CHAIN_FALLBACK = (1024, 257)  # more chunks than a device of <= 256 compute units holds resident
MAX_RESIDENT_CU = 256

# The overrun cases: `tie` weights whose last strata fall past the CDF's end and
# take the first maximum, particle N // 3 — on a rank that is neither the last
# nor the owner of the last prefix stratum (>= 2 N // 3), so the moved run is
# inserted in the middle of the view.  (seed, step) found with weighting_ref's
# Philox on the oracle's normalised weights (python tests/test_shard_plan_ref.py --tie).
TIE_SHAPES = [(8, 125), (3, 683), (17, 241)]
TIE_SEED_STEP = {1000: (4242, 3305), 2049: (4242, 4010), 4097: (4242, 2528)}

SHAPES = ([(w, n, d) for w, n in EVERY_DIST for d in DISTS]
          + [(w, n, d) for (w, n), ds in SOME.items() for d in ds]
          + [(w, n, "tie") for w, n in TIE_SHAPES])
SHAPES.sort(key=lambda c: (c[0] * c[1], c[0], ORDER.index(c[2])))


def KS(n):
    return (0, 1, n)


CASES = [(w, n, d, K) for w, n, d in SHAPES for K in KS(n)]


def key(shape):
    return "-".join(str(x) for x in shape)


def wcase(shape):
    """The weighting case (weighting_cases' form) of a shape: its D_ORACLE key,
    reference() and thresh() go by N."""
    return ("shard", "phd", shape[0] * shape[1], shape[2])


WCASES = sorted(set(wcase(s) for s in SHAPES), key=lambda c: (c[2], c[3]))


def seed_step(shape):
    if shape[2] == "tie":
        return TIE_SEED_STEP[shape[0] * shape[1]]
    return C.SEED, C.STEP


def uniforms(shape):
    return R.resample_uniforms(shape[0] * shape[1], *seed_step(shape))


@functools.lru_cache(maxsize=None)
def reference_parents(shape):
    """weighting_ref.parents on the reference's own float32 normalised weights
    (`tie`: on the oracle's, whose rounding leaves the CDF's end below one — the
    reference's own ends a few 1e-8 above; needs the oracle built)."""
    if shape[2] == "tie":
        import pyoracle
        return R.parents(pyoracle.normalize(C.weights("tie", shape[0] * shape[1]))[0], uniforms(shape))
    wn, _ = C.reference(wcase(shape))
    return R.parents(wn.astype(np.float32), uniforms(shape))


@functools.lru_cache(maxsize=None)
def reference_plan(shape):
    world, n, _ = shape
    return S.plan(reference_parents(shape).parent, n, world, n)


def checked_ranks(P, amax):
    """Every rank up to world 16.  Above: rank 0 and the last, the first rank
    with a surplus and the first with a deficit, a rank with demand 0 where
    there is one, the rank of the first maximum, and eight more spread evenly."""
    world, n = P.world, P.n
    if world <= 16:
        return list(range(world))
    pick = {0, world - 1, amax // n}
    for want in (lambda d: d > n, lambda d: d < n, lambda d: d == 0):
        hit = [s for s in range(world) if want(P.demand[s])]
        if hit:
            pick.add(hit[0])
    pick.update(int(x) for x in np.linspace(0, world - 1, 10)[1:-1])
    return sorted(pick)
