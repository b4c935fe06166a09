/*
 * phd_block.h — the 1024-thread block primitives that define the canonical
 * reduction orders: every path that must agree bit for bit on a block sum, max
 * or arg-max calls these.  The wave-level helpers are in phd_devutil.h.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "phd_devutil.h"
#include "phd_kernels.h"

namespace phd {

template <typename T>
__device__ __forceinline__ T block_reduce_1024(T v, T* s, bool is_max) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const T u = __shfl_xor(v, o, 64);
        v = is_max ? (u > v ? u : v) : v + u;
    }
    if (lane == 0) s[wid] = v;
    __syncthreads();
    T r = is_max ? (T)-INFINITY : (T)0;
    const int nw = (blockDim.x + 63) >> 6;
    for (int w = 0; w < nw; w++) r = is_max ? (s[w] > r ? s[w] : r) : r + s[w];
    __syncthreads();
    return r;
}

/* The max step of the log-sum-exp: m, the thread's own maximum, becomes the
 * block's (the wave maxima by wave_incl_max, lane 63's through LDS, the 16 in
 * wave order).  s_f: 16 floats; no trailing barrier (the caller's next one
 * frees s_f).  A macro: through a function (inlined or not, m by value or by
 * reference, lane and wid passed in or not) the register allocation of the
 * normalise and k_rs_* kernels changes. */
#define PHD_BLOCK_MAX_1024(m, s_f, lane, wid)                                          \
    {                                                                                  \
        (m) = wave_incl_max(m);                                                        \
        if ((lane) == 63) (s_f)[wid] = (m);                                            \
        __syncthreads();                                                               \
        (m) = -INFINITY;                                                               \
        _Pragma("unroll") for (int w_ = 0; w_ < RS_THREADS / 64; w_++)(m) = fmaxf((m), (s_f)[w_]); \
    }

/* The canonical order of the double sums of the normalisation (oracle D3: the
 * intended exact sum, up to one fixed reduction tree shared by every path).
 * The entries are cut into chunks of RS_THREADS; chunk c holds entries
 * c*1024 + t.  A chunk's sum is the wave_incl_scan_d total of each of its 16
 * waves, added in wave order; the chunk sums are added in chunk order.  The
 * single-block kernels (one thread per entry of every chunk) and the
 * multi-block sharded plan (one workgroup per chunk, k_rs_*) all evaluate
 * exactly this, so their weights agree bit for bit. */
template <class F>
__device__ double chunk_sum_block(int n, F&& f, double* s /* 32 doubles */) {
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    double total = 0.0;
    for (int c = 0; c * RS_THREADS < n; c++) {
        const int i = c * RS_THREADS + t;
        double x = i < n ? f(i) : 0.0;
        x = wave_incl_scan_d(x);
        double* sb = s + (c & 1) * 16;  // double-buffered: one barrier per chunk
        if (lane == 63) sb[wid] = x;
        __syncthreads();
        double cs = 0.0;
#pragma unroll
        for (int w = 0; w < RS_THREADS / 64; w++) cs += sb[w];
        total += cs;
    }
    return total;
}

/* First arg-max over the block (strict >, main.cpp:348-353: the lowest index
 * among equal maxima) of each thread's own first maximum (bw, bi): LDS tree.
 * Valid on thread 0. */
__device__ __forceinline__ int first_argmax_block(float bw, int bi) {
    __shared__ float sv[1024];
    __shared__ int si[1024];
    sv[threadIdx.x] = bw;
    si[threadIdx.x] = bi;
    __syncthreads();
    for (int o = blockDim.x / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            const float ov = sv[threadIdx.x + o];
            const int oi = si[threadIdx.x + o];
            if (ov > sv[threadIdx.x] || (ov == sv[threadIdx.x] && oi < si[threadIdx.x])) {
                sv[threadIdx.x] = ov;
                si[threadIdx.x] = oi;
            }
        }
        __syncthreads();
    }
    return si[0];
}

/* The expected pose Σ exp(w_i) pose_i (main.cpp:331-347; thread t accumulates
 * entries t, t + blockDim, ... in double, block_reduce_1024 per field) and the
 * first arg-max of w, where w_of(i) is entry i's normalised log-weight and
 * pose_of(i) points to its 6 pose floats (the sharded trace reads them from the
 * ranks' gathered blocks).  ep and the returned index are valid on thread 0.
 * s: 32 doubles. */
template <class W, class P>
__device__ __forceinline__ int expected_pose_block_at(int n, W&& w_of, P&& pose_of, float (&ep)[6], double* s) {
    double acc[6] = {0, 0, 0, 0, 0, 0};
    float bw = -FLT_MAX;
    int bi = INT_MAX;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const float w = w_of(i);
        const float ew = expf(w);
        const float* ps = pose_of(i);
        for (int k = 0; k < 6; k++) acc[k] += (double)(ew * ps[k]);
        if (w > bw) {
            bw = w;
            bi = i;
        }
    }
    for (int k = 0; k < 6; k++) ep[k] = (float)block_reduce_1024<double>(acc[k], s, false);
    return first_argmax_block(bw, bi);
}
template <class W>
__device__ __forceinline__ int expected_pose_block(int n, W&& w_of, const phd_pose* __restrict__ pose, float (&ep)[6],
                                                   double* s) {
    return expected_pose_block_at(n, w_of, [&](int i) { return (const float*)&pose[i]; }, ep, s);
}

/* nEff (main.cpp:1281-1284) from s2 = Σ exp(2 w) of the n normalised entries
 * and the resample decision (main.cpp:1286-1289; has_meas 2: forced, n > 5N). */
__device__ __forceinline__ float neff_of(double s2, int n) { return (float)(1.0 / (double)(float)s2 / (double)n); }
__device__ __forceinline__ int resample_decision(float neff, int has_meas, float resample_thresh) {
    return (has_meas == 2 || (has_meas && neff <= resample_thresh)) ? 1 : 0;
}

/* 64-bit DPP helpers for the single-block resample (1024 threads). */
template <int CTRL, int ROWMASK>
__device__ __forceinline__ unsigned long long dpp_or_zero_u64(unsigned long long v) {
    const unsigned int lo = (unsigned int)v, hi = (unsigned int)(v >> 32);
    const unsigned int lo2 = (unsigned int)dpp_or_zero<CTRL, ROWMASK>((int)lo);
    const unsigned int hi2 = (unsigned int)dpp_or_zero<CTRL, ROWMASK>((int)hi);
    return ((unsigned long long)hi2 << 32) | lo2;
}

__device__ __forceinline__ unsigned long long wave_incl_scan_u64(unsigned long long x) {
    x += dpp_or_zero_u64<0x111, 0xf>(x);
    x += dpp_or_zero_u64<0x112, 0xf>(x);
    x += dpp_or_zero_u64<0x114, 0xf>(x);
    x += dpp_or_zero_u64<0x118, 0xf>(x);
    x += dpp_or_zero_u64<0x142, 0xa>(x);
    x += dpp_or_zero_u64<0x143, 0xc>(x);
    return x;
}

__device__ __forceinline__ unsigned long long wave_incl_max_u64(unsigned long long x) {
    unsigned long long y;
    y = dpp_or_zero_u64<0x111, 0xf>(x); x = y > x ? y : x;
    y = dpp_or_zero_u64<0x112, 0xf>(x); x = y > x ? y : x;
    y = dpp_or_zero_u64<0x114, 0xf>(x); x = y > x ? y : x;
    y = dpp_or_zero_u64<0x118, 0xf>(x); x = y > x ? y : x;
    y = dpp_or_zero_u64<0x142, 0xa>(x); x = y > x ? y : x;
    y = dpp_or_zero_u64<0x143, 0xc>(x); x = y > x ? y : x;
    return x;
}

}  // namespace phd
