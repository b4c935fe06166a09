/*
 * contract_probe.hip — TEST ONLY: one function of the shared headers per entry
 * point, on the device and on the host, over arrays.
 *
 * DESIGN §2 rests the oracle's deviations D5, D6, D8, D14 and D16-D18 on "the
 * same bits on the CPU and on gfx950" for the helpers of include/phd_detmath.h
 * and include/phd_rng.h and for the float expressions of csrc/phd_device.h.
 * This unit evaluates each of them alone, so a difference is seen at the
 * function and the input where it arises (tests/test_gpu_contract.py,
 * tests/test_contract_host.py).  Built by build_contract_probe() of build.py
 * with the product's ARCH, FLAGS and include paths to
 * tests/libcontract_probe.so; never linked into libphdslam.so.
 *
 *   probe_dev_<f>(in, out, n)   one elementwise kernel (256 threads,
 *                               grid-stride) on host pointers: its own
 *                               hipMalloc and copies; returns the HIP status
 *   probe_host_<f>(in, out, n)  the same functor in a plain loop, compiled by
 *                               hipcc's host compiler in this unit
 *
 * in / out are arrays of records, one per element (layouts at each functor).
 * phd_device.h declares its helpers __device__ only; it is included unchanged
 * with __device__ widened to __host__ __device__ for the span of the include,
 * so the host loop runs the header's own expressions (the device code of a
 * __host__ __device__ function is that of the __device__ one).
 */
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "phd_detmath.h"
#include "phd_rng.h"
#include "phd_types.h"

#pragma push_macro("__device__")
#undef __device__
#define __device__ __attribute__((host)) __attribute__((device))
#include "phd_device.h"
#pragma pop_macro("__device__")

#define PROBE_HD __host__ __device__ __forceinline__

namespace {

template <class F>
__global__ __launch_bounds__(256) void k_probe(F f, const char* in, char* out, long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
        f(in + i * F::IN, out + i * F::OUT);
}

template <class F>
int run_dev(F f, const void* in, void* out, long n) {
    if (n <= 0) return 0;
    char *din = nullptr, *dout = nullptr;
    hipError_t e = hipMalloc((void**)&din, (size_t)n * F::IN);
    if (e != hipSuccess) return (int)e;
    e = hipMalloc((void**)&dout, (size_t)n * F::OUT);
    if (e == hipSuccess) e = hipMemcpy(din, in, (size_t)n * F::IN, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const long blocks = (n + 255) / 256;
        hipLaunchKernelGGL(k_probe<F>, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, 0, f, din, dout,
                           n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(out, dout, (size_t)n * F::OUT, hipMemcpyDeviceToHost);
    hipFree(din);
    hipFree(dout);
    return (int)e;
}

template <class F>
int run_host(F f, const void* in, void* out, long n) {
    for (long i = 0; i < n; i++) f((const char*)in + i * F::IN, (char*)out + i * F::OUT);
    return 0;
}

/* float -> float */
#define PROBE_F2F(NAME, EXPR)                                  \
    struct NAME {                                              \
        enum { IN = 4, OUT = 4 };                              \
        PROBE_HD void operator()(const char* i, char* o) const { \
            const float x = *(const float*)i;                  \
            *(float*)o = EXPR;                                 \
        }                                                      \
    };
PROBE_F2F(F_det_expf, phd_det_expf(x))
PROBE_F2F(F_det_logf, phd_det_logf(x))
PROBE_F2F(F_det_tanf, phd_det_tanf(x))
PROBE_F2F(F_wrap, d_wrap(x))
PROBE_F2F(F_det_safe_log, d_det_safe_log(x))

/* x -> (sin, cos) */
struct F_det_sincosf {
    enum { IN = 4, OUT = 8 };
    PROBE_HD void operator()(const char* i, char* o) const {
        float s, c;
        phd_det_sincosf(*(const float*)i, &s, &c);
        ((float*)o)[0] = s;
        ((float*)o)[1] = c;
    }
};

/* (y, x) -> atan2 */
struct F_atan2f {
    enum { IN = 8, OUT = 4 };
    PROBE_HD void operator()(const char* i, char* o) const {
        const float* v = (const float*)i;
        *(float*)o = phd_atan2f(v[0], v[1]);
    }
};

struct F_fix_term {
    enum { IN = 4, OUT = 8 };
    PROBE_HD void operator()(const char* i, char* o) const { *(uint64_t*)o = phd_fix_term(*(const float*)i); }
};

/* {double u; int32 j; int32 n} -> u64 */
struct F_fix_stratum {
    enum { IN = 16, OUT = 8 };
    PROBE_HD void operator()(const char* i, char* o) const {
        const double u = *(const double*)i;
        const int* jn = (const int*)(i + 8);
        *(uint64_t*)o = phd_fix_stratum(jn[0], u, jn[1]);
    }
};

/* {ctr[4], k0, k1} -> u32[4] */
struct F_philox4x32_10 {
    enum { IN = 24, OUT = 16 };
    PROBE_HD void operator()(const char* i, char* o) const {
        const uint32_t* v = (const uint32_t*)i;
        phd_u32x4 c = {{v[0], v[1], v[2], v[3]}};
        const phd_u32x4 r = phd_philox4x32_10(c, v[4], v[5]);
        for (int k = 0; k < 4; k++) ((uint32_t*)o)[k] = r.v[k];
    }
};

/* {u64 seed; u64 step; u32 index; u32 stream} -> u32[4] */
struct F_rng_draw {
    enum { IN = 24, OUT = 16 };
    PROBE_HD void operator()(const char* i, char* o) const {
        const uint64_t* s = (const uint64_t*)i;
        const uint32_t* w = (const uint32_t*)(i + 16);
        const phd_u32x4 r = phd_rng_draw(s[0], w[0], s[1], w[1]);
        for (int k = 0; k < 4; k++) ((uint32_t*)o)[k] = r.v[k];
    }
};

struct F_u01 {
    enum { IN = 4, OUT = 8 };
    PROBE_HD void operator()(const char* i, char* o) const { *(double*)o = phd_u01(*(const uint32_t*)i); }
};

/* (a, b) -> (n0, n1), double */
struct F_box_muller {
    enum { IN = 8, OUT = 16 };
    PROBE_HD void operator()(const char* i, char* o) const {
        const uint32_t* v = (const uint32_t*)i;
        double n0, n1;
        phd_box_muller(v[0], v[1], &n0, &n1);
        ((double*)o)[0] = n0;
        ((double*)o)[1] = n1;
    }
};

/* (px, py, pth, mx, my, P0..P3) -> the 16 floats of DevEkf in declaration order */
struct F_compute_ekf {
    enum { IN = 36, OUT = 64 };
    DevCfg c;
    PROBE_HD void operator()(const char* i, char* o) const {
        const float* v = (const float*)i;
        DevEkf e;
        d_compute_ekf(c, v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], e);
        float* r = (float*)o;
        r[0] = e.r, r[1] = e.bearing, r[2] = e.pd, r[3] = e.det;
        r[4] = e.S0, r[5] = e.S1, r[6] = e.S2, r[7] = e.S3;
        r[8] = e.K0, r[9] = e.K1, r[10] = e.K2, r[11] = e.K3;
        r[12] = e.cu0, r[13] = e.cu1, r[14] = e.cu2, r[15] = e.cu3;
    }
};

/* (px, py, pth, zr, zb) -> (mean[2], cov[4]) */
struct F_birth {
    enum { IN = 20, OUT = 24 };
    DevCfg c;
    PROBE_HD void operator()(const char* i, char* o) const {
        const float* v = (const float*)i;
        float mean[2], cov[4];
        d_birth(c, v[0], v[1], v[2], v[3], v[4], mean, cov);
        float* r = (float*)o;
        r[0] = mean[0], r[1] = mean[1];
        r[2] = cov[0], r[3] = cov[1], r[4] = cov[2], r[5] = cov[3];
    }
};

/* (ax, ay, a0..a3, bx, by, b0..b3) -> distance */
struct F_mahal {
    enum { IN = 48, OUT = 4 };
    PROBE_HD void operator()(const char* i, char* o) const {
        const float* v = (const float*)i;
        *(float*)o = d_mahal(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11]);
    }
};
struct F_hellinger {
    enum { IN = 48, OUT = 4 };
    PROBE_HD void operator()(const char* i, char* o) const {
        const float* v = (const float*)i;
        *(float*)o = d_hellinger(v[0], v[1], v[2], v[3], v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11]);
    }
};

/* Only the fields the helpers above read (as set_dev_cfg fills them). */
DevCfg cfg_of(const phd_slam_config* c) {
    DevCfg d = {};
    d.minRange = c->minRange;
    d.maxRange = c->maxRange;
    d.maxBearing = c->maxBearing;
    d.stdRange = c->stdRange;
    d.stdBearing = c->stdBearing;
    d.pd = c->pd;
    d.birthNoiseFactor = c->birthNoiseFactor;
    return d;
}

}  // namespace

#define PROBE_EXPORT(f)                                                                               \
    extern "C" int probe_dev_##f(const void* in, void* out, long n) { return run_dev(F_##f(), in, out, n); } \
    extern "C" int probe_host_##f(const void* in, void* out, long n) { return run_host(F_##f(), in, out, n); }
#define PROBE_EXPORT_CFG(f)                                                                   \
    extern "C" int probe_dev_##f(const phd_slam_config* c, const void* in, void* out, long n) { \
        F_##f fn;                                                                             \
        fn.c = cfg_of(c);                                                                     \
        return run_dev(fn, in, out, n);                                                       \
    }                                                                                         \
    extern "C" int probe_host_##f(const phd_slam_config* c, const void* in, void* out, long n) { \
        F_##f fn;                                                                             \
        fn.c = cfg_of(c);                                                                     \
        return run_host(fn, in, out, n);                                                      \
    }

PROBE_EXPORT(det_expf)
PROBE_EXPORT(det_logf)
PROBE_EXPORT(det_tanf)
PROBE_EXPORT(det_sincosf)
PROBE_EXPORT(atan2f)
PROBE_EXPORT(fix_term)
PROBE_EXPORT(fix_stratum)
PROBE_EXPORT(philox4x32_10)
PROBE_EXPORT(rng_draw)
PROBE_EXPORT(u01)
PROBE_EXPORT(box_muller)
PROBE_EXPORT(wrap)
PROBE_EXPORT(det_safe_log)
PROBE_EXPORT(mahal)
PROBE_EXPORT(hellinger)
PROBE_EXPORT_CFG(compute_ekf)
PROBE_EXPORT_CFG(birth)
