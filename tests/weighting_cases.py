"""Shared cases of the weighting-stage tests (tests/test_weighting_ref.py on the
CPU, tests/test_gpu_weighting.py on the device): fixed seeds, float32 inputs,
M = 4 measurements and empty maps, so the update is the births and a weight
shift common to every particle and the normalised weights are those of the
input log-weights (weighting_ref.normalize).

A case is (path, config, n, dist):
  path    "standalone" (normalize / neff / resample) or "step" (phd_step)
  config  "phd" (config 2, fused update), "split" (config 2, part A + part C)
          or "cphd" (config 3)
  dist    the weight distribution (weights())
"""
import functools

import numpy as np

import weighting_ref as R

CHUNK = 1024   # RS_THREADS: one workgroup's chunk of the chunked forms
CONTRACT = 1e-5
SEED = 4242    # phd_set_seed of every case
STEP = 11      # ... and its step counter
CAPS = dict(map_capacity=64, max_measurements=8)  # (the smallest set the suite already runs)
# the benched config-3 capacities: a part C launch whose LDS holds the lead
# workgroup's tables (with CAPS it does not: the resample takes the second stream)
CAPS_ROOMY = dict(map_capacity=704, max_measurements=64, candidate_capacity=832, survivor_capacity=288)
M = 4
DISTS = ("normal", "flat", "one", "two_far", "holes", "wide", "shifted", "tie")

# (seed, step) of the phd_step `tie` cases: found with weighting_ref's Philox so
# that the reference reports a stratum past the CDF's end on the oracle's
# normalised weights (test_weighting_ref.test_tie_pairs_overrun repeats the search's check)
TIE_SEED_STEP = {1000: (4242, 3305), 2049: (4242, 2396), 4097: (4242, 216), 20000: (4242, 2332)}


# the two maxima of `tie`: of 1, 1.125 .. 5 a level at which the float32
# normalised weights leave the CDF's end below 1 (2 parts in 1e8 at 20000, 2 to 3
# in 1e7 at the other sizes) both as
# the oracle and as the device normalise them — the two differ by an ulp of the
# log-sum-exp on one level in five — so a last stratum drawn close enough to 1
# overruns the CDF on either
TIE_LEVEL = {1000: 3.5, 2049: 3.0, 4097: 2.75, 20000: 5.0}  # (each above every other entry)


def weights(dist, n, seed=3):
    """float32 log-weights (not normalised) of one distribution at n particles."""
    rng = np.random.default_rng(seed + 7919 * n)
    w = rng.normal(-8, 3, n).astype(np.float32)
    B = (n + CHUNK - 1) // CHUNK
    if dist == "normal":
        pass
    elif dist == "flat":
        w[:] = -3.0
    elif dist == "one":  # every fixed-point term but one is 0
        w[:] = -60.0
        w[(3 * n) // 4] = 0.0
    elif dist == "two_far":  # the mass in the first and the last chunk
        w[:] = -200.0
        w[min(5, n - 1)] = -1.0
        w[max(n - 7, 0)] = -0.5
    elif dist == "holes":  # a whole interior chunk, the whole last chunk, every fifth entry elsewhere
        w[::5] = -np.inf
        if B >= 3:
            w[(B // 2) * CHUNK:(B // 2 + 1) * CHUNK] = -np.inf
        if B >= 2:
            w[(B - 1) * CHUNK:] = -np.inf
        if not np.isfinite(w).any():
            w[0] = -8.0
    elif dist == "wide":
        w = rng.normal(0, 30, n).astype(np.float32)
    elif dist == "sparse":  # `normal` on every eighth entry: an eighth of the CDF's steps, so of the near strata
        w[np.arange(n) % 8 != 0] = -np.inf
    elif dist == "shifted":
        w = (w - np.float32(3e4)).astype(np.float32)
    elif dist == "tie":  # two exactly equal maxima, neither the last entry's neighbour
        w[n // 3] = w[(2 * n) // 3] = np.float32(TIE_LEVEL.get(n, 2.0))
    else:
        raise KeyError(dist)
    return w


def thresh(dist, n):
    """resampleThresh that asks for a resample: nEff = 1 (`flat`, or a single
    particle) against 1.0 is a near decision."""
    return 1.5 if dist == "flat" or n == 1 else 1.0


def chunks(n):
    return (n + CHUNK - 1) // CHUNK


def _with_far(sizes):
    """`normal` at every size, `two_far` and `holes` wherever more chunks than are staged (4)."""
    return [(n, d) for n in sizes for d in ("normal", "two_far", "holes") if d == "normal" or chunks(n) > 4]


EVERY = [(n, d) for n in (1000, 2049, 4097, 20000) for d in DISTS]

# standalone: one workgroup; CDF in LDS up to 8192 entries, in global memory above
STANDALONE = sorted(set(_with_far([1, 63, 1024, 1025, 8192, 8193]) + EVERY))
# phd_step by form: one block (n <= 2048), one launch of n/1024 workgroups
# (n <= 16384), four launches above
STEP_BLOCK = sorted(set(_with_far([1, 64, 1000, 1024, 1025, 2047, 2048]) + [e for e in EVERY if e[0] <= 2048]))
STEP_ONE_LAUNCH = sorted(set(_with_far([2049, 4096, 4097, 16384]) + [e for e in EVERY if 2048 < e[0] <= 16384]))
STEP_MULTI = sorted(set(_with_far([16385, 20000]) + [e for e in EVERY if e[0] > 16384]))
# the overlapped forms beside part C, CPHD and the split PHD update: the lead
# workgroup of the part C launch (roomy capacities), the second stream (small ones)
STEP_LEAD = [("cphd", 2049, "normal"), ("cphd", 4097, "normal"), ("cphd", 4097, "two_far"), ("cphd", 4097, "holes"),
             ("split", 4097, "normal"), ("split", 4097, "two_far")]
LIVE = (2500, 1000)  # n_live -> n_out of the standalone n_out < n case

CASES = ([("standalone", "phd", n, d) for n, d in STANDALONE]
         + [("step", "phd", n, d) for n, d in STEP_BLOCK + STEP_ONE_LAUNCH + STEP_MULTI]
         + [("step", c, n, d) for c, n, d in STEP_LEAD])


def key(case):
    return "-".join(str(x) for x in case)


def seed_step(case):
    path, _, n, dist = case
    if path == "step" and dist == "tie":
        return TIE_SEED_STEP[n]
    return SEED, STEP


@functools.lru_cache(maxsize=None)
def scenario(config, n):
    """(cfg, poses with px = particle index, empty maps, offsets, measurements), read-only."""
    import phdslam
    c, poses, _, maps, _, z = phdslam.config_scenario(3 if config == "cphd" else 2, n=n, G=8, M=M)
    poses["px"] = np.arange(n, dtype=np.float32)  # distinct poses identify parents
    empty, offs0 = np.zeros(0, maps.dtype), np.zeros(n + 1, np.int32)
    for a in (poses, empty, offs0, z):
        a.setflags(write=False)
    return c, poses, empty, offs0, z


def config(case, resample=True):
    c = scenario(case[1], case[2])[0].copy()
    c.resampleThresh = thresh(case[3], case[2]) if resample else 0.0
    return c


@functools.lru_cache(maxsize=None)
def reference(case):
    """(normalised float64 weights, Decision at the case's threshold) of the reference."""
    w = weights(case[3], case[2])
    wn, _ = R.normalize(w)
    wn.setflags(write=False)
    return wn, R.decision(w, thresh(case[3], case[2]))


def lognorm_deviation(a, b):
    """Worst |a - b| / max(|a|, |b|) of normalised log-weights beyond the 1e-5
    absolute floor; -inf entries must coincide."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert np.array_equal(np.isneginf(a), np.isneginf(b)), "-inf entries differ"
    fin = np.isfinite(a) & np.isfinite(b)
    assert np.array_equal(fin, ~np.isneginf(a)), "non-finite entries"
    a, b = a[fin], b[fin]
    d = np.abs(a - b)
    d = np.where(d <= 1e-5, 0.0, d - 1e-5)
    return float(np.max(d / np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300))) if d.size else 0.0


def neff_deviation(a, b):
    return abs(float(a) - float(b)) / max(abs(float(a)), abs(float(b)))


def hold_parents(got, w32, u, label):
    """Assert the reference's rule for a parent list (weighting_ref.check_parents)
    and that no -inf entry is a parent; returns (near strata, strata, the reference)."""
    ref = R.parents(np.ascontiguousarray(w32, np.float32), u)
    wrong, outside, near = R.check_parents(got, ref)
    got = np.asarray(got)
    assert wrong.size == 0, (f"{label}: {wrong.size} strata differ from the reference, first {wrong[:5]}: "
                             f"got {got[wrong[:5]]}, reference {ref.parent[wrong[:5]]}")
    assert outside.size == 0, (f"{label}: near strata {outside[:5]} outside [{ref.lo[outside[:5]]}, "
                               f"{ref.hi[outside[:5]]}]: got {got[outside[:5]]}")
    assert near <= 0.01 * len(got), f"{label}: {near} of {len(got)} strata near"
    assert not np.isneginf(np.asarray(w32)[got]).any(), f"{label}: a -inf entry is a parent"
    return near, len(got), ref


def round_up(x):
    """x rounded up to two significant figures."""
    if x <= 0:
        return 0.0
    e = int(np.floor(np.log10(x))) - 1
    return float(np.ceil(x / 10.0 ** e - 1e-9) * 10.0 ** e)


# The oracle's measured deviation from the reference per case (tests/
# test_weighting_ref.py regenerates it: python tests/test_weighting_ref.py):
# normalised log-weights in SURVEY §8(d)'s form, nEff relative.
D_ORACLE = {
    "standalone-phd-1-normal": dict(lognorm=0, neff=0),
    "standalone-phd-63-normal": dict(lognorm=0, neff=1.1e-07),
    "standalone-phd-1000-flat": dict(lognorm=0, neff=2.4e-07),
    "standalone-phd-1000-holes": dict(lognorm=0, neff=1.2e-08),
    "standalone-phd-1000-normal": dict(lognorm=0, neff=3.9e-08),
    "standalone-phd-1000-one": dict(lognorm=0, neff=4.8e-08),
    "standalone-phd-1000-shifted": dict(lognorm=0.00049, neff=0.0016),
    "standalone-phd-1000-tie": dict(lognorm=0, neff=3.9e-07),
    "standalone-phd-1000-two_far": dict(lognorm=0, neff=1.3e-08),
    "standalone-phd-1000-wide": dict(lognorm=7.3e-09, neff=6.7e-06),
    "standalone-phd-1024-normal": dict(lognorm=0, neff=7.6e-08),
    "standalone-phd-1025-normal": dict(lognorm=0, neff=1.6e-07),
    "standalone-phd-2049-flat": dict(lognorm=0, neff=3.6e-07),
    "standalone-phd-2049-holes": dict(lognorm=0, neff=7.6e-09),
    "standalone-phd-2049-normal": dict(lognorm=0, neff=8.6e-08),
    "standalone-phd-2049-one": dict(lognorm=0, neff=1.2e-10),
    "standalone-phd-2049-shifted": dict(lognorm=0.00033, neff=0.0014),
    "standalone-phd-2049-tie": dict(lognorm=0, neff=3e-07),
    "standalone-phd-2049-two_far": dict(lognorm=0, neff=2.2e-08),
    "standalone-phd-2049-wide": dict(lognorm=9.3e-09, neff=7.2e-06),
    "standalone-phd-4097-flat": dict(lognorm=0, neff=1.2e-07),
    "standalone-phd-4097-holes": dict(lognorm=0, neff=2.3e-07),
    "standalone-phd-4097-normal": dict(lognorm=0, neff=7.6e-08),
    "standalone-phd-4097-one": dict(lognorm=0, neff=1.5e-11),
    "standalone-phd-4097-shifted": dict(lognorm=0.00022, neff=0.0012),
    "standalone-phd-4097-tie": dict(lognorm=0, neff=5.7e-07),
    "standalone-phd-4097-two_far": dict(lognorm=0, neff=1.8e-08),
    "standalone-phd-4097-wide": dict(lognorm=0, neff=9.5e-07),
    "standalone-phd-8192-holes": dict(lognorm=0, neff=1.4e-07),
    "standalone-phd-8192-normal": dict(lognorm=0, neff=3.2e-07),
    "standalone-phd-8192-two_far": dict(lognorm=0, neff=9.8e-10),
    "standalone-phd-8193-holes": dict(lognorm=0, neff=2.7e-07),
    "standalone-phd-8193-normal": dict(lognorm=0, neff=2.7e-07),
    "standalone-phd-8193-two_far": dict(lognorm=0, neff=7.5e-09),
    "standalone-phd-20000-flat": dict(lognorm=0, neff=7.2e-07),
    "standalone-phd-20000-holes": dict(lognorm=0, neff=1.2e-07),
    "standalone-phd-20000-normal": dict(lognorm=0, neff=7e-08),
    "standalone-phd-20000-one": dict(lognorm=0, neff=2.6e-08),
    "standalone-phd-20000-shifted": dict(lognorm=3.2e-05, neff=0.00017),
    "standalone-phd-20000-tie": dict(lognorm=0, neff=4.5e-08),
    "standalone-phd-20000-two_far": dict(lognorm=0, neff=2.8e-08),
    "standalone-phd-20000-wide": dict(lognorm=0, neff=1.8e-06),
    "step-phd-1-normal": dict(lognorm=0, neff=0),
    "step-phd-64-normal": dict(lognorm=0, neff=3.7e-07),
    "step-phd-1000-flat": dict(lognorm=0, neff=2.4e-07),
    "step-phd-1000-holes": dict(lognorm=0, neff=3.7e-07),
    "step-phd-1000-normal": dict(lognorm=0, neff=1.3e-07),
    "step-phd-1000-one": dict(lognorm=0, neff=4.8e-08),
    "step-phd-1000-shifted": dict(lognorm=0.00049, neff=0.0016),
    "step-phd-1000-tie": dict(lognorm=0, neff=3.9e-07),
    "step-phd-1000-two_far": dict(lognorm=0, neff=4.5e-07),
    "step-phd-1000-wide": dict(lognorm=3.7e-08, neff=6.7e-06),
    "step-phd-1024-normal": dict(lognorm=0, neff=4.5e-07),
    "step-phd-1025-normal": dict(lognorm=0, neff=1.6e-07),
    "step-phd-2047-normal": dict(lognorm=0, neff=3.6e-07),
    "step-phd-2048-normal": dict(lognorm=0, neff=2.6e-07),
    "step-phd-2049-flat": dict(lognorm=0, neff=3.6e-07),
    "step-phd-2049-holes": dict(lognorm=0, neff=4.4e-07),
    "step-phd-2049-normal": dict(lognorm=0, neff=3.2e-07),
    "step-phd-2049-one": dict(lognorm=0, neff=1.2e-10),
    "step-phd-2049-shifted": dict(lognorm=0.00033, neff=0.0014),
    "step-phd-2049-tie": dict(lognorm=0, neff=4e-07),
    "step-phd-2049-two_far": dict(lognorm=0, neff=4.3e-07),
    "step-phd-2049-wide": dict(lognorm=3.9e-08, neff=7.2e-06),
    "step-phd-4096-normal": dict(lognorm=0, neff=8e-07),
    "step-phd-4097-flat": dict(lognorm=0, neff=1.2e-07),
    "step-phd-4097-holes": dict(lognorm=0, neff=5.3e-07),
    "step-phd-4097-normal": dict(lognorm=0, neff=2.6e-07),
    "step-phd-4097-one": dict(lognorm=0, neff=1.5e-11),
    "step-phd-4097-shifted": dict(lognorm=0.00022, neff=0.0012),
    "step-phd-4097-tie": dict(lognorm=0, neff=5.7e-07),
    "step-phd-4097-two_far": dict(lognorm=0, neff=4.6e-07),
    "step-phd-4097-wide": dict(lognorm=1.5e-08, neff=9.5e-07),
    "step-phd-16384-holes": dict(lognorm=0, neff=2e-07),
    "step-phd-16384-normal": dict(lognorm=0, neff=8.4e-07),
    "step-phd-16384-two_far": dict(lognorm=0, neff=4.5e-07),
    "step-phd-16385-holes": dict(lognorm=0, neff=5.1e-07),
    "step-phd-16385-normal": dict(lognorm=0, neff=8.7e-07),
    "step-phd-16385-two_far": dict(lognorm=0, neff=4.5e-07),
    "step-phd-20000-flat": dict(lognorm=0, neff=7.2e-07),
    "step-phd-20000-holes": dict(lognorm=0, neff=1.2e-07),
    "step-phd-20000-normal": dict(lognorm=0, neff=1.4e-07),
    "step-phd-20000-one": dict(lognorm=0, neff=2.6e-08),
    "step-phd-20000-shifted": dict(lognorm=3.2e-05, neff=0.00017),
    "step-phd-20000-tie": dict(lognorm=0, neff=4.5e-08),
    "step-phd-20000-two_far": dict(lognorm=0, neff=4.2e-07),
    "step-phd-20000-wide": dict(lognorm=1.9e-08, neff=1.8e-06),
    "step-cphd-2049-normal": dict(lognorm=0, neff=2.4e-07),
    "step-cphd-4097-normal": dict(lognorm=0, neff=7.6e-08),
    "step-cphd-4097-two_far": dict(lognorm=0, neff=4.6e-07),
    "step-cphd-4097-holes": dict(lognorm=0, neff=7.2e-07),
    "step-split-4097-normal": dict(lognorm=0, neff=2.6e-07),
    "step-split-4097-two_far": dict(lognorm=0, neff=4.6e-07),
    # the gathered sizes of the sharded plan (tests/shard_plan_cases.py)
    "shard-phd-15-flat": dict(lognorm=0, neff=1.2e-07),
    "shard-phd-15-holes": dict(lognorm=0, neff=5.2e-08),
    "shard-phd-15-normal": dict(lognorm=0, neff=6.6e-08),
    "shard-phd-15-one": dict(lognorm=0, neff=5.3e-08),
    "shard-phd-15-two_far": dict(lognorm=0, neff=2.5e-08),
    "shard-phd-15-wide": dict(lognorm=0, neff=2.6e-06),
    "shard-phd-16-normal": dict(lognorm=0, neff=1.9e-07),
    "shard-phd-16-one": dict(lognorm=0, neff=0),
    "shard-phd-16-two_far": dict(lognorm=0, neff=9.8e-10),
    "shard-phd-32-normal": dict(lognorm=0, neff=1.6e-07),
    "shard-phd-32-one": dict(lognorm=0, neff=0),
    "shard-phd-32-two_far": dict(lognorm=0, neff=9.8e-10),
    "shard-phd-64-normal": dict(lognorm=0, neff=1.5e-07),
    "shard-phd-1000-tie": dict(lognorm=0, neff=3.9e-07),
    "shard-phd-1023-normal": dict(lognorm=0, neff=2.5e-07),
    "shard-phd-1023-two_far": dict(lognorm=0, neff=5.5e-09),
    "shard-phd-1024-normal": dict(lognorm=0, neff=7.6e-08),
    "shard-phd-1024-two_far": dict(lognorm=0, neff=9.8e-10),
    "shard-phd-1025-flat": dict(lognorm=0, neff=4.5e-16),
    "shard-phd-1025-holes": dict(lognorm=0, neff=1.1e-07),
    "shard-phd-1025-normal": dict(lognorm=0, neff=1.6e-07),
    "shard-phd-1025-one": dict(lognorm=0, neff=9.4e-10),
    "shard-phd-1025-two_far": dict(lognorm=0, neff=1.6e-08),
    "shard-phd-1025-wide": dict(lognorm=8.1e-09, neff=6.8e-06),
    "shard-phd-1105-flat": dict(lognorm=0, neff=3.6e-07),
    "shard-phd-1105-holes": dict(lognorm=0, neff=2.2e-08),
    "shard-phd-1105-normal": dict(lognorm=0, neff=1.5e-07),
    "shard-phd-1105-one": dict(lognorm=0, neff=4.8e-09),
    "shard-phd-1105-two_far": dict(lognorm=0, neff=2e-08),
    "shard-phd-1105-wide": dict(lognorm=1.1e-08, neff=7.6e-06),
    "shard-phd-2048-holes": dict(lognorm=0, neff=3.4e-08),
    "shard-phd-2048-normal": dict(lognorm=0, neff=2.6e-07),
    "shard-phd-2048-one": dict(lognorm=0, neff=0),
    "shard-phd-2048-two_far": dict(lognorm=0, neff=9.8e-10),
    "shard-phd-2049-tie": dict(lognorm=0, neff=3e-07),
    "shard-phd-2112-holes": dict(lognorm=0, neff=3e-07),
    "shard-phd-2112-normal": dict(lognorm=0, neff=2.8e-07),
    "shard-phd-2112-one": dict(lognorm=0, neff=3e-08),
    "shard-phd-2112-two_far": dict(lognorm=0, neff=1.1e-08),
    "shard-phd-3072-holes": dict(lognorm=0, neff=8.5e-08),
    "shard-phd-3072-normal": dict(lognorm=0, neff=6e-07),
    "shard-phd-3072-one": dict(lognorm=0, neff=3e-08),
    "shard-phd-3072-two_far": dict(lognorm=0, neff=9.8e-10),
    "shard-phd-4096-holes": dict(lognorm=0, neff=5.2e-07),
    "shard-phd-4096-normal": dict(lognorm=0, neff=5.1e-07),
    "shard-phd-4096-two_far": dict(lognorm=0, neff=9.8e-10),
    "shard-phd-4097-tie": dict(lognorm=0, neff=5.7e-07),
    "shard-phd-4100-flat": dict(lognorm=0, neff=9e-07),
    "shard-phd-4100-holes": dict(lognorm=0, neff=2.5e-07),
    "shard-phd-4100-normal": dict(lognorm=0, neff=3.1e-07),
    "shard-phd-4100-one": dict(lognorm=0, neff=9.4e-10),
    "shard-phd-4100-two_far": dict(lognorm=0, neff=1.6e-08),
    "shard-phd-4100-wide": dict(lognorm=5.4e-09, neff=6.2e-06),
    "shard-phd-131072-one": dict(lognorm=0, neff=0),
    "shard-phd-131072-sparse": dict(lognorm=0, neff=9.7e-08),
    "shard-phd-131072-two_far": dict(lognorm=0, neff=9.8e-10),
    "shard-phd-132096-one": dict(lognorm=0, neff=3.8e-09),
    "shard-phd-132096-sparse": dict(lognorm=0, neff=4.6e-08),
    "shard-phd-132096-two_far": dict(lognorm=0, neff=9.8e-10),
    "shard-phd-263168-sparse": dict(lognorm=0, neff=9.3e-08),
    "shard-phd-263168-two_far": dict(lognorm=0, neff=1.8e-08),
}
