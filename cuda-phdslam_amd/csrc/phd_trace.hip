/*
 * phd_trace.hip — the per-scan estimate trace (phd_trace_enable, phd_capi.h):
 * the outputs of recoverSlamState (main.cpp:318-388) and the loop's nEff
 * decision (main.cpp:1281-1289) of one phd_step, written to a device ring by
 * kernels on the context's stream — no host read-back.
 *
 * Two stages, both enqueued after the update and before the step's resample
 * (which rewrites the poses, the log-weights and the slab references):
 *   stage 1  k_trace_weights   one 1024-thread workgroup: its own log-sum-exp
 *            of the un-normalised log-weights, nEff and the decision, the
 *            expected pose and the first arg-max, by k_normalize's and
 *            k_expected_pose's block functions; leaves the normalised weights and the
 *            arg-max particle's slab reference for stage 2
 *   stage 2  k_trace_card      one workgroup per TRACE_PB particles: Σ_j w_j of
 *            each map by one wave (k_cardinality's sum), weighted partials
 *            k_trace_finish    the fixed-order combine, the map snapshot and
 *            the expected cardinality rows
 * No float atomics anywhere: a run reproduces its records bit for bit.
 */
#include <hip/hip_runtime.h>

#include <cstdint>

#include "phd_block.h"
#include "phd_device.h"
#include "phd_devutil.h"
#include "phd_kernels.h"
#include "phd_slab.h"
#include "phd_trace.h"

namespace phd {

__global__ void __launch_bounds__(RS_THREADS) k_trace_weights(TraceArgs a) {
    __shared__ double s_d[64];
    __shared__ double s_r[32];
    __shared__ float s_f[32];
    const int t = threadIdx.x;
    const int n = a.n;
    // log-sum-exp, nEff and the decision: normalize_block's arithmetic (w_norm beside logw)
    float mx = -INFINITY;
    for (int i = t; i < n; i += RS_THREADS) mx = fmaxf(mx, a.logw[i]);
    PHD_BLOCK_MAX_1024(mx, s_f, t & 63, t >> 6);
    const double sum = chunk_sum_block(n, [&](int i) { return (double)expf(a.logw[i] - mx); }, s_d);
    const float lse = d_safe_log((float)sum) + mx;
    const double s2 = chunk_sum_block(
        n,
        [&](int i) {
            const float w = a.logw[i] - lse;
            a.w_norm[i] = w;
            return (double)expf(2 * w);
        },
        s_d + 32);
    const float neff = neff_of(s2, n);
    const int resample = resample_decision(neff, a.has_meas, a.resample_thresh);
    // expected pose and first arg-max: k_expected_pose's routine on the normalised weights
    float ep[6];
    const int amax = expected_pose_block(n, [&](int i) { return a.logw[i] - lse; }, a.pose, ep, s_r);
    if (t == 0) {
        // (every weight NaN or below -FLT_MAX: no arg-max; particle 0 stands in)
        const int best = amax >= 0 && amax < n ? amax : 0;
        phd_trace_record r;
        r.step = a.step;
        r.n_live = n;
        r.n_measure = a.M;
        r.resampled = resample;
        r.neff = neff;
        r.expected_pose = phd_pose{ep[0], ep[1], ep[2], ep[3], ep[4], ep[5]};
        r.map_particle = amax;
        r.map_pose = a.pose[best];
        r.card_expected = 0.f;  // stage 2
        r.card_map = 0.f;
        r.map_size = 0;
        const int e = a.err[3], prev = a.hand[TRACE_H_ERRPREV];
        r.status_errors = e >= prev ? e - prev : e;  // (the counter was taken and cleared in between)
        r.reserved = 0;
        *a.rec = r;
        a.hand[TRACE_H_ERRPREV] = e;
        a.hand[TRACE_H_PARTICLE] = best;
        a.hand[TRACE_H_SLAB] = a.src[best];
    }
}

/* Σ_j w_j of TRACE_PB maps per workgroup, one wave per map at a time (the
 * double sum of k_cardinality, rounded to float as phd_cardinalities returns
 * it), times exp(w_n); the workgroup's partial of card_expected is the sum of
 * its particles' terms in index order. */
__global__ void __launch_bounds__(256) k_trace_card(TraceArgs a) {
    __shared__ double s_term[TRACE_PB];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int base = blockIdx.x * TRACE_PB;
    const int best = a.hand[TRACE_H_PARTICLE];
    for (int q = wid; q < TRACE_PB; q += 4) {
        const int p = base + q;
        double term = 0.0;
        if (p < a.n) {
            const Slab m = slab_of(a.src[p], a.map_in, a.size_in, a.map_x, a.size_x, a.cap);
            const int sz = min(max(m.size, 0), a.cap);
            double s = 0.0;
            for (int k = lane; k < sz; k += 64) s += (double)m.map[k];
            s = wave_sum_d(s);
            const float cn = (float)s;
            term = (double)expf(a.w_norm[p]) * (double)cn;
            if (p == best && lane == 0) {
                a.rec->card_map = cn;
                a.rec->map_size = sz;
            }
        }
        if (lane == 0) s_term[q] = term;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int q = 0; q < TRACE_PB; q++) s += s_term[q];
        a.part[blockIdx.x] = s;
    }
}

/* Workgroup 0: the partials of card_expected in a fixed order (thread t takes
 * partials t, t + 256, ...; wave scans; the wave totals in order).
 * Workgroup 1: the arg-max particle's map into the snapshot entry — the entry
 * as a flat run of floats, so consecutive lanes store consecutive words.
 * Workgroup 2: the expected cardinality rows, Σ_n exp(w_n) cn_n[k] in particle
 * order (float, the sum recoverSlamState makes), one thread per k. */
__global__ void __launch_bounds__(256) k_trace_finish(TraceArgs a, int nparts) {
    const int t = threadIdx.x;
    if (blockIdx.x == 0) {
        __shared__ double s_w[4];
        double v = 0.0;
        for (int i = t; i < nparts; i += 256) v += a.part[i];
        v = wave_incl_scan_d(v);
        if ((t & 63) == 63) s_w[t >> 6] = v;
        __syncthreads();
        if (t == 0) a.rec->card_expected = (float)(((s_w[0] + s_w[1]) + s_w[2]) + s_w[3]);
    } else if (blockIdx.x == 1) {
        if (!a.snap) return;
        const Slab m = slab_of(a.hand[TRACE_H_SLAB], a.map_in, a.size_in, a.map_x, a.size_x, a.cap);
        const int sz = min(max(m.size, 0), a.cap);
        const int rows = min(sz, a.snap_cap);
        float* o = (float*)a.snap;
        // Gaussian2D words: cov[0..3] (rows 3..6), mean[0..1] (rows 1..2), weight (row 0)
        for (int e = t; e < a.snap_cap * PHD_NF; e += 256) {
            const int k = e / PHD_NF, j = e - k * PHD_NF;
            const int f = j < 4 ? 3 + j : j < 6 ? j - 3 : 0;
            o[e] = k < rows ? m.map[(size_t)f * a.cap + k] : 0.f;
        }
    } else {
        if (!a.card || !a.card_all) return;
        for (int k = t; k < a.K; k += 256) {
            float c = 0.f;
            for (int i = 0; i < a.n; i++) c += expf(a.w_norm[i]) * a.card_all[(size_t)i * a.K + k];
            a.card[k] = c;
        }
    }
}

void trace_launch_stage1(const TraceArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_trace_weights, dim3(1), dim3(RS_THREADS), 0, st, a);
}

void trace_launch_stage2(const TraceArgs& a, hipStream_t st) {
    const int nparts = (a.n + TRACE_PB - 1) / TRACE_PB;
    hipLaunchKernelGGL(k_trace_card, dim3(nparts), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_trace_finish, dim3(3), dim3(256), 0, st, a, nparts);
}

}  // namespace phd
