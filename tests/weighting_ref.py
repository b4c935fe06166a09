"""Float64 reference of the weighting stage — log-sum-exp normalisation, nEff,
the resample decision and the stratified resample (main.cpp
1281-1297 and 453-501) — in plain numpy, scipy and Python integers.

TEST INFRASTRUCTURE ONLY.  It imports neither the oracle nor any routine of
include/phd_detmath.h / include/phd_rng.h; it restates what those two headers
document in prose: Philox4x32-10 (Salmon et al., SC'11) with the 64-bit seed as
key and the counter (stratum j, step low word, step high word, 'RSMP'),
u_j = x0 2^-32; a CDF of float32-rounded exp(w) terms held in 2^-40 fixed point
(each term and each stratum position truncated), searched for the first entry
that reaches r_j = (j + u_j) / n_out; the first maximum for a stratum past the
CDF's end.

Exact statement here: normalised w = w64 - logsumexp(w64); nEff =
1 / sum(exp(2 w)) / n; decision = has_meas and nEff <= thresh; for float32
normalised weights w, c = cumsum(exp(float64(w))), parent_j = first k with
c[k] >= r_j, else the first arg-max of w.

Admissible parents (the band).  An implementation's CDF entry k may differ from
c[k] by

    band[k] = c[k] 2^-23 + (k + 2) 2^-40

— each addend is exp(w) rounded to float32 (relative 2^-24), so the prefix is
off by at most c[k] 2^-24, taken twice as margin (it also covers the 2^-53
rounding of r_j and of the float64 prefix sum); each of the k + 1 terms and the
stratum lose less than 2^-40 to truncation.  Stratum j's admissible parents are
[lo_j, hi_j]: lo_j the lower bound of r_j in c + band, hi_j in c - band (made
monotone by a running maximum: an implementation's CDF is nondecreasing, so it
lies above the largest lower limit so far).  A stratum is near when
lo_j != hi_j; with hi_j == n the first arg-max is admissible as well.

The decision's float32 bound (first order, eps = 2^-24; p = softmax(w64),
q = p^2 / sum(p^2)):

    log-sum-exp  E_lse = eps sum p |w - max|      the exponent w - max, rounded
                       + 2 eps                    expf, within an ulp
                       + eps                      the double sum cast to float
                       + 2 eps max(1, |log S|)    logf, within an ulp
                       + eps |lse|                log S + max, rounded
    normalised w       + eps sum q |w_norm|       w - lse rounded, weighted as nEff sees it
    nEff (relative)  2 (E_lse + eps sum q |w_norm|)   d nEff / nEff = -2 d w
                       + 2 eps                    expf(2 w), within an ulp
                       + 3 eps                    s2 cast to float, the quotient cast to float
    bound = nEff x that.

A decision is near when |nEff - thresh| <= max(1e-4 thresh, 2 bound).
"""
from collections import namedtuple

import numpy as np
from scipy.special import logsumexp

STREAM_RESAMPLE = 0x52534D50  # 'RSMP'
EPS32 = 2.0 ** -24

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(ctr, key):
    """Philox4x32 with 10 rounds.  ctr: four arrays (or scalars) of 32-bit words,
    key: two 32-bit words.  Returns the four output words as uint32 arrays."""
    c = [np.atleast_1d(np.asarray(x, np.uint64)) & _LO32 for x in ctr]
    shape = np.broadcast(*c).shape
    c = [np.broadcast_to(x, shape) for x in c]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for r in range(10):
        if r:
            k0 = (k0 + _W0) & 0xFFFFFFFF
            k1 = (k1 + _W1) & 0xFFFFFFFF
        p0, p1 = _M0 * c[0], _M1 * c[2]  # 32 x 32 -> 64 bits, exact in uint64
        c = [(p1 >> _S32) ^ c[1] ^ np.uint64(k0), p1 & _LO32, (p0 >> _S32) ^ c[3] ^ np.uint64(k1), p0 & _LO32]
    return [x.astype(np.uint32) for x in c]


def resample_uniforms(n_out, seed, step):
    """u_j, j < n_out: the first output word of the draw with counter
    (j, step_lo, step_hi, 'RSMP') and key seed, times 2^-32 (exact in float64)."""
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    x = philox4x32_10([np.arange(n_out, dtype=np.uint64), step & 0xFFFFFFFF, step >> 32, STREAM_RESAMPLE],
                      [seed & 0xFFFFFFFF, seed >> 32])
    return x[0].astype(np.float64) * 2.0 ** -32


def normalize(w):
    """(w64 - logsumexp(w64), logsumexp(w64)) of log-weights of any float type."""
    w = np.asarray(w, np.float64)
    lse = float(logsumexp(w))
    return w - lse, lse


def neff(wn):
    """1 / sum(exp(2 w)) / n of normalised log-weights."""
    wn = np.asarray(wn, np.float64)
    return 1.0 / float(np.sum(np.exp(2.0 * wn))) / len(wn)


Decision = namedtuple("Decision", "neff resample near bound")


def decision(w, thresh, has_meas=True):
    """nEff of the raw log-weights w, the resample decision, whether a float32
    implementation may decide otherwise (near), and the bound (module docstring)."""
    w = np.asarray(w, np.float64)
    wn, lse = normalize(w)
    ne = neff(wn)
    fin = np.isfinite(w)
    mx = float(np.max(w))
    p = np.exp(wn[fin])
    q = p * p / np.sum(p * p)
    log_s = lse - mx
    e_lse = EPS32 * (float(np.sum(p * np.abs(w[fin] - mx))) + 3.0 + 2.0 * max(1.0, abs(log_s)) + abs(lse))
    e_w = EPS32 * float(np.sum(q * np.abs(wn[fin])))
    bound = ne * (2.0 * (e_lse + e_w) + 5.0 * EPS32)
    near = abs(ne - thresh) <= max(1e-4 * thresh, 2.0 * bound)
    return Decision(ne, bool(has_meas and ne <= thresh), bool(has_meas and near), bound)


Parents = namedtuple("Parents", "parent lo hi near amax beyond n")


def parents(w32, u):
    """Stratified parents of float32 normalised log-weights w32 for the uniforms
    u (one per stratum; fewer strata than entries after a predict that spawned
    children).  parent[j]: the exact rule's parent; [lo[j], hi[j]]: the
    admissible parents (hi[j] == n: the CDF's end may lie below the stratum, so
    the first arg-max `amax` is admissible too); near[j] = lo[j] != hi[j];
    beyond: the strata the exact rule itself puts past the CDF's end; n: entries."""
    w32 = np.asarray(w32)
    assert w32.dtype == np.float32
    n = len(w32)
    u = np.asarray(u, np.float64)
    n_out = len(u)
    c = np.cumsum(np.exp(w32.astype(np.float64)))
    r = (np.arange(n_out, dtype=np.float64) + u) / n_out
    band = c * 2.0 ** -23 + (np.arange(n, dtype=np.float64) + 2.0) * 2.0 ** -40
    amax = int(np.argmax(w32))  # the first maximum
    k = np.searchsorted(c, r, side="left")  # first k with c[k] >= r
    lo = np.searchsorted(c + band, r, side="left")
    hi = np.searchsorted(np.maximum.accumulate(c - band), r, side="left")
    beyond = np.flatnonzero(k == n)
    parent = np.where(k == n, amax, k).astype(np.int64)
    return Parents(parent, lo.astype(np.int64), hi.astype(np.int64), lo != hi, amax, beyond, n)


def check_parents(got, ref):
    """Hold a parent list to the reference's rule.  Returns (strata that are not
    near and differ, near strata outside their admissible parents, near count)."""
    got = np.asarray(got, np.int64)
    assert got.shape == ref.parent.shape
    wrong = np.flatnonzero(~ref.near & (got != ref.parent))
    inside = ((got >= ref.lo) & (got <= ref.hi)) | ((ref.hi == ref.n) & (got == ref.amax))
    outside = np.flatnonzero(ref.near & ~inside)
    return wrong, outside, int(ref.near.sum())
