"""Input sets of the CPU / gfx950 bit contract (tests/test_contract_host.py,
tests/test_gpu_contract.py): deterministic (fixed LCG seeds, no files), each
set at most 2^20 elements, laid out as the records of tests/contract_probe.hip.

TEST INFRASTRUCTURE ONLY.
"""
import functools
import math

import numpy as np

F = np.float32
FLT_MAX = float(np.finfo(F).max)
FLT_MIN = float(np.finfo(F).tiny)
SUB_MIN = float(np.float32(1e-45))
PI = math.pi


def lcg(seed, n):
    """n 32-bit words: the high halves of x <- 6364136223846793005 x +
    1442695040888963407 (mod 2^64), x0 = seed (Knuth's MMIX constants); the
    sequence is laid out by doubling, so it is the sequential one."""
    with np.errstate(over="ignore"):
        A = np.array([6364136223846793005], np.uint64)
        C = np.array([1442695040888963407], np.uint64)
        am, cm = A[0], C[0]
        while len(A) < n:
            A, C = np.concatenate([A, am * A]), np.concatenate([C, am * C + cm])
            am, cm = am * am, am * cm + cm
        x = A[:n] * np.uint64(seed) + C[:n]
    return (x >> np.uint64(32)).astype(np.uint32)


def uniform(seed, n, lo=0.0, hi=1.0):
    """float64 uniforms on [lo, hi) from lcg(seed)."""
    return lo + (hi - lo) * (lcg(seed, n).astype(np.float64) * 2.0 ** -32)


def f32_from_bits(b):
    return np.ascontiguousarray(b, np.uint32).view(F)


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def near(centers, ulps=2):
    """The floats within +-ulps of the float nearest to each centre (ulps
    counted on the magnitude, so a centre at 0 gives 0 and the subnormals next
    to it on its side)."""
    c = np.asarray(centers, np.float64).astype(F)
    b = bits(c).astype(np.int64)
    sign, mag = b & 0x80000000, b & 0x7fffffff
    d = np.arange(-ulps, ulps + 1, dtype=np.int64)
    m = np.clip(mag[:, None] + d[None, :], 0, 0x7f800000)
    return f32_from_bits((m | sign[:, None]).ravel().astype(np.uint32))


@functools.lru_cache(None)
def sweep():
    """Every exponent field (256) x both signs x 2048 mantissas (0, 1, 2^22,
    2^23 - 1 and LCG values): +-0, every subnormal binade, +-inf, NaNs."""
    man = (lcg(101, 512 * 2048) & np.uint32(0x7fffff)).reshape(512, 2048)
    man[:, 0], man[:, 1], man[:, 2], man[:, 3] = 0, 1, 1 << 22, (1 << 23) - 1
    head = (np.arange(512, dtype=np.uint32) << np.uint32(23))[:, None]  # sign | exponent
    x = f32_from_bits((head | man).ravel())
    x.setflags(write=False)
    return x


def sweep_sample(k=4096):
    """k points of the sweep, spread over every exponent and mantissa column."""
    i = np.arange(k, dtype=np.int64)
    return sweep()[i * (len(sweep()) // k) + (i * 37) % (len(sweep()) // k)]


def expf_set():
    k = np.arange(-160, 131, dtype=np.float64)
    centers = np.concatenate([(k + 0.5) * math.log(2.0),
                              [-110.0, -103.28, math.log(2.0 ** -149), math.log(2.0 ** -150), -87.34,
                               math.log(2.0 ** -126), 88.7228, math.log(FLT_MAX), 89.0]])
    return near(centers)


def logf_set():
    e = np.arange(-149, 128, dtype=np.float64)
    r2 = math.sqrt(2.0) * 2.0 ** e
    centers = np.concatenate([2.0 ** e, r2[r2 < FLT_MAX], [1.0]])
    edge = np.array([0.0, -0.0, -SUB_MIN, -FLT_MIN, -1.0, -FLT_MAX, -np.inf, np.inf, np.nan], F)
    return np.concatenate([near(centers), edge])


def _signed_swapped(num, den):
    """(y, x) records of every (num, den): both swaps x four sign quadrants."""
    out = []
    for y, x in ((num, den), (den, num)):
        for sy in (1, -1):
            for sx in (1, -1):
                out.append(np.stack([F(sy) * y, F(sx) * x], 1))
    return np.concatenate(out)


def atan2f_set():
    """(y, x) records.  The choice of k: pairs whose float quotient times 8
    lies within ~2 ulp of k + 1/2 (numerators +-4 ulp of (k + 1/2) / 8 den, 64
    denominators over 40 binades per k); |y| = |x|; zeros; subnormal /
    subnormal; huge / tiny; inf and NaN combinations."""
    parts = []
    for k in range(8):
        w = lcg(200 + k, 128)
        den = f32_from_bits(((w[:64] % np.uint32(40) + np.uint32(107)) << np.uint32(23)) | (w[64:] & np.uint32(0x7fffff)))
        num0 = ((k + 0.5) / 8.0 * den.astype(np.float64))
        num = near(num0, 4)
        parts.append(_signed_swapped(num, np.repeat(den, 9)))
    eq = f32_from_bits(lcg(210, 256) & np.uint32(0x7fffffff))
    eq = eq[np.isfinite(eq)]
    parts.append(_signed_swapped(eq, eq))
    s = np.array([0.0, -0.0, SUB_MIN, -SUB_MIN, 3 * SUB_MIN, FLT_MIN - SUB_MIN, FLT_MIN, -FLT_MIN, 1e-30, 1.0, -1.0,
                  0.125, 3.0, 1e30, FLT_MAX, -FLT_MAX, np.inf, -np.inf, np.nan], F)
    yy, xx = np.meshgrid(s, s, indexing="ij")
    parts.append(np.stack([yy.ravel(), xx.ravel()], 1))
    sub = f32_from_bits(lcg(211, 512) & np.uint32(0x7fffff))  # subnormal / subnormal
    parts.append(_signed_swapped(sub[:256], sub[256:]))
    return np.ascontiguousarray(np.concatenate(parts), F)


def trig_set():
    """Floats within +-2 ulp of k pi/2 and (2k + 1) pi/4 for |k| <= 4096 and
    4096 LCG values of |k| < 2^20 (both signs), and of the +-1.5e6 boundary."""
    k = np.arange(-4096, 4097, dtype=np.float64)
    kr = (lcg(300, 4096) >> np.uint32(12)).astype(np.float64)
    kr = np.concatenate([kr, -kr])
    centers = np.concatenate([k * (PI / 2), (2 * k + 1) * (PI / 4), kr * (PI / 2), (2 * kr + 1) * (PI / 4),
                              [1.5e6, -1.5e6]])
    return near(centers)


def fix_term_set():
    t = np.array([0.0, SUB_MIN, FLT_MIN, 2.0 ** -41, 2.0 ** -40, 1.0, 2.0 ** 23 - 0.5], F)
    edge = np.concatenate([t, near([2.0 ** -40, 1.0], 1)])
    w = lcg(400, 3 << 16)
    lin = ((w[:1 << 16] >> np.uint32(8)).astype(np.float64) * 2.0 ** -24 * 2.0 ** 23).astype(F)
    lin = np.minimum(lin, F(2.0 ** 23 - 0.5))
    log = f32_from_bits(((w[1 << 16:2 << 16] % np.uint32(150)) << np.uint32(23)) | (w[2 << 16:] & np.uint32(0x7fffff)))
    return np.concatenate([edge, lin, log])


STRATUM = np.dtype([("u", np.float64), ("j", np.int32), ("n", np.int32)])


def fix_stratum_set():
    us = np.concatenate([[0.0, 2.0 ** -32, 0.5, 1 - 2.0 ** -32], lcg(500, 64).astype(np.float64) * 2.0 ** -32])
    rec = []
    for n in (1, 2, 3, 63, 64, 65, 1000, 4096, 9000, 65536, 1 << 20):
        for j in (0, 1, n // 2, n - 2, n - 1):
            j = min(max(j, 0), n - 1)
            rec += [(u, j, n) for u in us]
            # knots: u = q n / 2^32 - j (a phd_u01 value), so (j + u) / n = q / 2^32 exactly and the
            # scaled position is the integer 2^8 q: a quotient that is not correctly rounded (a
            # multiplication by 1 / n, an approximate division) and lands below it truncates to
            # 2^8 q - 1.  (Scaling before dividing, (j + u) (2^40 / n), cannot be told apart on
            # phd_u01's 2^-32 grid: the scaled position is at least 2^8 / n from any integer it does
            # not equal, its rounding error at most 2^-11.)
            q0, q1 = -(-(j << 32) // n), -(-((j + 1) << 32) // n)
            for w in lcg(501 + n + j, 64).tolist():
                q = q0 + (w * 2654435761) % (q1 - q0)
                rec.append(((q * n - (j << 32)) / 2.0 ** 32, j, n))
    return np.array(rec, STRATUM)


# Random123 kat_vectors, philox4x32 with 10 rounds (as tests/weighting_ref.py carries them)
PHILOX_KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
              ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
              ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
               (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def philox_set():
    """(ctr[4], k0, k1) records: the three known-answer vectors, then LCG words."""
    kat = np.array([c + k for c, k, _ in PHILOX_KAT], np.uint32)
    return np.concatenate([kat, lcg(600, 6 * 4096).reshape(-1, 6)])


DRAW = np.dtype([("seed", np.uint64), ("step", np.uint64), ("index", np.uint32), ("stream", np.uint32)])
STREAMS = (0x50524544, 0x52534d50, 0x53594e54)  # PHD_STREAM_PREDICT / RESAMPLE / SYNTH


def rng_draw_set():
    seeds = (0, 1, 1234, 0xffffffff00000000, 0x8000000000000001, 0xdeadbeefcafef00d, 2 ** 64 - 1)
    steps = (0, 1, 2 ** 32, 2 ** 32 + 5, 0x1ffffffff, 2 ** 63, 2 ** 64 - 1)
    idx = (0, 1, 2 ** 31, 2 ** 32 - 1)
    return np.array([(s, t, i, m) for s in seeds for t in steps for i in idx for m in STREAMS], DRAW)


def u01_set():
    return np.concatenate([np.array([0, 1, 2 ** 31, 2 ** 32 - 1], np.uint32), lcg(700, 1 << 16)])


BM_CROSSED = 16


@functools.lru_cache(None)
def box_muller_set():
    """(a, b) records: {0, 1, 2^31, 2^32 - 1}^2 (a = 2^32 - 1: u1 = 1, rad = -0),
    then 2^18 LCG pairs."""
    e = np.array([0, 1, 2 ** 31, 2 ** 32 - 1], np.uint32)
    aa, bb = np.meshgrid(e, e, indexing="ij")
    x = np.concatenate([np.stack([aa.ravel(), bb.ravel()], 1), lcg(800, 2 << 18).reshape(-1, 2)])
    x.setflags(write=False)
    return x


def _covs(seed, n):
    """n covariances (P0, P1, P2, P3), P1 = P2.  First half: eigenvalues l1 in
    [1e-4, 1], l1 / l2 up to 1e6, any rotation.  Second half: standard
    deviations within a factor 20 of each other, correlation over +-0.999."""
    h = n // 2
    l1 = 10.0 ** uniform(seed, h, -4, 0)
    l2 = l1 / 10.0 ** uniform(seed + 1, h, 0, 6)
    t = uniform(seed + 2, h, -PI, PI)
    c, s = np.cos(t), np.sin(t)
    e = np.stack([c * c * l1 + s * s * l2, c * s * (l1 - l2), s * s * l1 + c * c * l2], 1)
    sx = 10.0 ** uniform(seed + 3, n - h, -2, 0)
    sy = sx * 20.0 ** uniform(seed + 4, n - h, -1, 1)
    rho = 0.999 * np.sin(uniform(seed + 5, n - h, -PI / 2, PI / 2) * 1.0)
    rho[:8] = [0.999, -0.999, 0.0, 0.5, -0.5, 0.99, -0.99, 0.9]
    r = np.stack([sx * sx, rho * sx * sy, sy * sy], 1)
    p = np.concatenate([e, r])
    return np.stack([p[:, 0], p[:, 1], p[:, 1], p[:, 2]], 1).astype(F)


N_TYPICAL = 1 << 16


def ekf_set():
    """(px, py, pth, mx, my, P0..P3): 2^16 typical (range 0.5 .. 60 m, headings
    over (-pi, pi]), then the edges: the bearing at +-pi to the ulp (feature
    dead astern, dy = +-0 / +-tiny, and pth within +-2 ulp of heading -+ pi) and
    dx = dy = 0."""
    n = N_TYPICAL
    px, py = uniform(900, n, -50, 50).astype(F), uniform(901, n, -50, 50).astype(F)
    pth = (-uniform(902, n, -PI, PI)).astype(F)  # (-pi, pi]
    r, h = uniform(903, n, 0.5, 60), -uniform(904, n, -PI, PI)
    mx = (px + r * np.cos(h)).astype(F)
    my = (py + r * np.sin(h)).astype(F)
    typ = np.concatenate([np.stack([px, py, pth, mx, my], 1), _covs(910, n)], 1)
    # the bearing at +-pi
    m = 512
    ex, ey = uniform(920, m, -50, 50).astype(F), uniform(921, m, -50, 50).astype(F)
    er = uniform(922, m, 0.5, 60).astype(F)
    tiny = np.tile(np.array([0.0, -0.0, SUB_MIN, -SUB_MIN, 1e-30, -1e-30, 1e-6, -1e-6], F), m // 8)
    astern = np.stack([ex, ey, np.zeros(m, F), ex - er, ey], 1)  # dy = 0 at dx < 0
    astern2 = np.stack([np.zeros(m, F), np.zeros(m, F), np.zeros(m, F), -er, tiny], 1)  # dy = +-0, +-tiny at dx < 0
    eh = -uniform(923, m, -PI, PI)
    qx, qy = (er * np.cos(eh)).astype(F), (er * np.sin(eh)).astype(F)
    b = np.arctan2(qy.astype(np.float64), qx.astype(np.float64))
    rows = []
    for sgn in (-1.0, 1.0):
        c = near(b + sgn * PI, 2).reshape(m, 5)
        for k in range(5):
            rows.append(np.stack([np.zeros(m, F), np.zeros(m, F), c[:, k], qx, qy], 1))
    zero = np.stack([ex, ey, pth[:m], ex, ey], 1)  # dx = dy = 0
    edge5 = np.concatenate([astern, astern2] + rows + [zero])
    edge = np.concatenate([edge5, np.tile(_covs(930, 64), (len(edge5) // 64 + 1, 1))[:len(edge5)]], 1)
    return np.ascontiguousarray(np.concatenate([typ, edge]), F), n


def birth_set():
    """(px, py, pth, range, bearing): 2^16 typical, then range 0 / tiny / huge
    and pth + bearing at multiples of pi/2."""
    n = N_TYPICAL
    typ = np.stack([uniform(1000, n, -50, 50), uniform(1001, n, -50, 50), -uniform(1002, n, -PI, PI),
                    uniform(1003, n, 0.5, 60), -uniform(1004, n, -PI, PI)], 1).astype(F)
    e = []
    for zr in (0.0, SUB_MIN, FLT_MIN, 1e-20, 1e20, FLT_MAX, np.inf, 0.5, 60.0):
        for th, zb in ((0.0, 0.0), (PI / 2, 0.0), (PI, -PI), (PI, PI), (1.0, PI / 2 - 1.0), (-3.0, 3.0), (2.5, 2.5)):
            e.append((1.5, -2.5, th, zr, zb))
    return np.ascontiguousarray(np.concatenate([typ, np.array(e, F)]), F), n


def pair_set():
    """(ax, ay, a0..a3, bx, by, b0..b3) of d_mahal / d_hellinger: 2^16 typical
    pairs a few standard deviations apart, then the edges: the summed
    covariance's determinant cancelling to a few ulp (correlation 1 -+ ulps),
    determinants at or below FLT_MIN (the identity branch of the Hellinger
    form), zero and negative determinants, a negative p0 p3 - p2 p1."""
    n = N_TYPICAL
    ca, cb = _covs(1100, n), _covs(1110, n)
    am = np.stack([uniform(1120, n, -50, 50), uniform(1121, n, -50, 50)], 1)
    sc = np.sqrt(np.maximum(ca[:, 0], ca[:, 3]).astype(np.float64))[:, None]
    bm = am + sc * np.stack([uniform(1122, n, -4, 4), uniform(1123, n, -4, 4)], 1)
    typ = np.concatenate([am.astype(F), ca, bm.astype(F), cb], 1)
    m = 1024
    v0 = (10.0 ** uniform(1130, m, -3, 1)).astype(F)
    v3 = (10.0 ** uniform(1131, m, -3, 1)).astype(F)
    off = near(np.sqrt(v0.astype(np.float64) * v3.astype(np.float64)), 2).reshape(m, 5)[np.arange(m), np.arange(m) % 5]
    off = off * np.where(np.arange(m) % 2 == 0, F(1), F(-1))
    cancel = np.stack([v0, off, off, v3], 1)  # |P1| = sqrt(P0 P3) -+ 2 ulp: det of a few ulp, either sign
    dm = np.stack([uniform(1132, m, -1, 1), uniform(1133, m, -1, 1)], 1).astype(F)
    e1 = np.concatenate([np.zeros((m, 2), F), cancel, dm, cancel], 1)  # a = b: s = 2a, p = a a
    e2 = np.concatenate([np.zeros((m, 2), F), cancel, dm, np.roll(cancel, 1, 0)], 1)
    tiny = []
    for s in (1e-19, 1.1e-19, 7.7e-20, 1e-20, 1e-23, 0.0):  # det of the sum around / below FLT_MIN
        for rho in (0.0, 0.5, -0.9):
            tiny.append((0.0, 0.0, s, rho * s, rho * s, s, 0.25, -0.5, s, rho * s, rho * s, 1.5 * s))
    for d in (0.1, 1.0):  # negative determinants: |P1| > sqrt(P0 P3)
        tiny.append((0.0, 0.0, 1.0, 1.5, 1.5, 1.0, d, d, 1.0, 0.2, 0.2, 1.0))
        tiny.append((0.0, 0.0, 1.0, 1.5, 1.5, 1.0, d, d, 1.0, 1.5, 1.5, 1.0))
        tiny.append((0.0, 0.0, 1.0, 0.9, 0.9, 1.0, d, d, 1.0, -1.2, -1.2, 1.0))
        tiny.append((0.0, 0.0, 2.0, 0.0, 0.0, 2.0, d, d, 1.0, 3.0, 3.0, 1.0))
    return np.ascontiguousarray(np.concatenate([typ, e1, e2, np.array(tiny, F)]), F), n
