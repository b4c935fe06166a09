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
 * The mixed model's trace (phd_trace_enable_mixed, feature_model 2) rides in the
 * same launches: k_trace_card also sums every particle's dynamic slab (the
 * weights row of the 21-row SoA slab, through the same slab reference) into a
 * second set of partials, k_trace_finish gets one more workgroup for their
 * combine and one per 256 snapshot components for the Gaussian4D transpose.
 * Stage 1 is shared: one arg-max, one set of normalised weights per scan.
 * The sharded step's trace (phd_trace_shard_pack / _append, below): the same
 * record from all world * n particles — k_trace_shard_weights on the gathered
 * log-weights, k_trace_shard_pack into this rank's block, the caller's
 * all-gather of the blocks, k_trace_shard_finish.  Both come without and with
 * the dynamic half (phd_trace_shard_pack_mixed / _append_mixed): the static
 * form carries no dynamic code.
 * No float atomics anywhere: a run reproduces its records bit for bit.
 */
#include <hip/hip_runtime.h>

#include <cstdint>

#include "phd_block.h"
#include "phd_device.h"
#include "phd_devutil.h"
#include "phd_kernels.h"
#include "phd_mixed_k.h"
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

#if PHD_TRACE_DYN
/* Particle p's dynamic map: slab slab_index(src[p]) of the dynamic set, 21 SoA
 * rows of dcap floats (the mixed model holds no migrated slabs). */
__device__ __forceinline__ Slab dyn_slab_of(int sref, const float* dmap, const int* dsize, int dcap) {
    const int r = slab_index(sref);
    return Slab{dmap + (size_t)r * PHD_DYN_FIELDS * dcap, dsize[r]};
}
#endif

/* The fixed-order combine of nparts partials by one 256-thread workgroup
 * (thread t takes partials t, t + 256, ...; wave scans; the wave totals in
 * order): card_expected's rule, for the static and the dynamic maps. */
__device__ __forceinline__ float combine_partials(const double* part, int nparts, double* s_w) {
    const int t = threadIdx.x;
    double v = 0.0;
    for (int i = t; i < nparts; i += 256) v += part[i];
    v = wave_incl_scan_d(v);
    if ((t & 63) == 63) s_w[t >> 6] = v;
    __syncthreads();
    return (float)(((s_w[0] + s_w[1]) + s_w[2]) + s_w[3]);
}

/* Σ_j w_j of TRACE_PB maps per workgroup, one wave per map at a time (the
 * double sum of k_cardinality, rounded to float as phd_cardinalities returns
 * it), times exp(w_n); the workgroup's partial of card_expected is the sum of
 * its particles' terms in index order. */
__global__ void __launch_bounds__(256) k_trace_card(TraceArgs a) {
    __shared__ double s_term[TRACE_PB];
#if PHD_TRACE_DYN
    __shared__ double s_dterm[TRACE_PB];
#endif
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
#if PHD_TRACE_DYN
    // the same sum over the particles' dynamic slabs (row 0 of a slab: the weights)
    if (a.dmap)
        for (int q = wid; q < TRACE_PB; q += 4) {
            const int p = base + q;
            double term = 0.0;
            if (p < a.n) {
                const Slab m = dyn_slab_of(a.src[p], a.dmap, a.dsize, a.dcap);
                const int sz = min(max(m.size, 0), a.dcap);
                double s = 0.0;
                for (int k = lane; k < sz; k += 64) s += (double)m.map[k];
                s = wave_sum_d(s);
                const float cn = (float)s;
                term = (double)expf(a.w_norm[p]) * (double)cn;
                if (p == best && lane == 0) {
                    a.drec->card_map = cn;
                    a.drec->map_size = sz;
                    for (int i = 0; i < 5; i++) a.drec->reserved[i] = 0;
                }
            }
            if (lane == 0) s_dterm[q] = term;
        }
#endif
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int q = 0; q < TRACE_PB; q++) s += s_term[q];
        a.part[blockIdx.x] = s;
    }
#if PHD_TRACE_DYN
    if (threadIdx.x == 64 && a.dmap) {
        double s = 0.0;
        for (int q = 0; q < TRACE_PB; q++) s += s_dterm[q];
        a.dpart[blockIdx.x] = s;
    }
#endif
}

/* Workgroup 0: the partials of card_expected in a fixed order (thread t takes
 * partials t, t + 256, ...; wave scans; the wave totals in order).
 * Workgroup 1: the arg-max particle's map into the snapshot entry — the entry
 * as a flat run of floats, so consecutive lanes store consecutive words.
 * Workgroup 2: the expected cardinality rows, Σ_n exp(w_n) cn_n[k] in particle
 * order (float, the sum recoverSlamState makes), one thread per k.
 * A mixed-model scan adds workgroup 3: the dynamic card_expected from its
 * partials, workgroup 0's combine; and workgroups 4 onward: the arg-max
 * particle's dynamic map into the dyn snapshot entry, one wave per strip of 64
 * components — each field's 64 values in one coalesced load, then every lane
 * stores its component's whole phd_gaussian4d (zeros past the map's size). */
__global__ void __launch_bounds__(256) k_trace_finish(TraceArgs a, int nparts) {
    const int t = threadIdx.x;
    __shared__ double s_w[4];
#if PHD_TRACE_DYN
    if (blockIdx.x == 3) {
        const float ce = combine_partials(a.dpart, nparts, s_w);
        if (t == 0) a.drec->card_expected = ce;
        return;
    }
    if (blockIdx.x > 3) {
        const Slab m = dyn_slab_of(a.hand[TRACE_H_SLAB], a.dmap, a.dsize, a.dcap);
        const int rows = min(min(max(m.size, 0), a.dcap), a.dsnap_cap);
        const int k = (blockIdx.x - 4) * TRACE_DSNAP_PB + t;  // (a wave's 64 lanes: one strip)
        if (k >= a.dsnap_cap) return;
        phd_gaussian4d g;
        if (k < rows) {
            g.weight = m.map[k];
            for (int i = 0; i < 4; i++) g.mean[i] = m.map[(size_t)(1 + i) * a.dcap + k];
            for (int i = 0; i < 16; i++) g.cov[i] = m.map[(size_t)(5 + i) * a.dcap + k];
        } else {
            g.weight = 0.f;
            for (int i = 0; i < 4; i++) g.mean[i] = 0.f;
            for (int i = 0; i < 16; i++) g.cov[i] = 0.f;
        }
        a.dsnap[k] = g;
        return;
    }
#endif
    if (blockIdx.x == 0) {
        const float ce = combine_partials(a.part, nparts, s_w);
        if (t == 0) a.rec->card_expected = ce;
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
    int finish = 3;
#if PHD_TRACE_DYN
    if (a.dmap) finish = 4 + (a.dsnap ? (a.dsnap_cap + TRACE_DSNAP_PB - 1) / TRACE_DSNAP_PB : 0);
#endif
    hipLaunchKernelGGL(k_trace_finish, dim3(finish), dim3(256), 0, st, a, nparts);
}

/* ---- the trace of a sharded step: the record the single context of
 * N = world * n particles (global index = rank * n + local index) writes, bit
 * for bit.  The per-particle inputs travel (poses, cardinalities), never
 * partial sums: the block functions run over all N entries on every rank. ---- */

/* Σ_j w_j of one map by one wave (k_trace_card's sum); sz: its clamped size */
__device__ __forceinline__ float map_cardinality(const Slab& m, int cap, int lane, int& sz) {
    sz = min(max(m.size, 0), cap);
    double s = 0.0;
    for (int k = lane; k < sz; k += 64) s += (double)m.map[k];
    s = wave_sum_d(s);
    return (float)s;
}

/* Stage 1: k_trace_weights' log-sum-exp, nEff, decision and first arg-max (of
 * the normalised weights w_all[i] - lse, as expected_pose_block takes it) over
 * the gathered log-weights. */
__global__ void __launch_bounds__(RS_THREADS) k_trace_shard_weights(TraceShardArgs a) {
    __shared__ double s_d[64];
    __shared__ float s_f[32];
    const int t = threadIdx.x;
    const int N = a.world * a.n;
    float mx = -INFINITY;
    for (int i = t; i < N; i += RS_THREADS) mx = fmaxf(mx, a.w_all[i]);
    PHD_BLOCK_MAX_1024(mx, s_f, t & 63, t >> 6);
    const double sum = chunk_sum_block(N, [&](int i) { return (double)expf(a.w_all[i] - mx); }, s_d);
    const float lse = d_safe_log((float)sum) + mx;
    const double s2 = chunk_sum_block(N, [&](int i) { return (double)expf(2 * (a.w_all[i] - lse)); }, s_d + 32);
    const float neff = neff_of(s2, N);
    const int resample = resample_decision(neff, a.has_meas, a.resample_thresh);
    float bw = -FLT_MAX;
    int bi = INT_MAX;
    for (int i = t; i < N; i += RS_THREADS) {
        const float w = a.w_all[i] - lse;
        if (w > bw) {
            bw = w;
            bi = i;
        }
    }
    const int amax = first_argmax_block(bw, bi);
    if (t == 0) {
        const int best = amax >= 0 && amax < N ? amax : 0;
        phd_trace_record r;
        r.step = a.step;
        r.n_live = N;
        r.n_measure = a.M;
        r.resampled = resample;
        r.neff = neff;
        r.expected_pose = phd_pose{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};  // the finish stage
        r.map_particle = amax;
        r.map_pose = phd_pose{0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        r.card_expected = 0.f;
        r.card_map = 0.f;
        r.map_size = 0;
        r.status_errors = 0;
        r.reserved = 0;
        *a.rec = r;
        a.hand[TRACE_H_PARTICLE] = best;
        // (a rank that does not own the particle: any valid reference, its rows are not sent)
        a.hand[TRACE_H_SLAB] = a.src[best / a.n == a.rank ? best - a.rank * a.n : 0];
        a.hand[TRACE_H_LSE] = __float_as_int(lse);
    }
}

/* The dynamic map a slab reference names on a sharded rank: the slab of that
 * id in the current dynamic set or — bit 30, a migrated particle — in the
 * dynamic set X (phd_slab.h).  Set X exists from the first receive on, and no
 * reference names it before. */
__device__ __forceinline__ Slab dyn_slab_ref(int sref, const TraceShardArgs& a) {
    return Slab{dyn_slab_map(sref, a.dmap, a.dmap_x, a.dcap), slab_size(sref, a.dsize, a.dsize_x)};
}

/* Words of one strip of the dynamic snapshot: 64 components as phd_gaussian4d.
 * The row stride is odd, so a wave's 64 stores of one field — lane k to word
 * k * 21 + j — fall on distinct LDS banks. */
#define TRACE_STRIP_WORDS (64 * PHD_DYN_FIELDS)

/* Stage 2: this rank's block.  Workgroup b takes local particles b * TRACE_PB
 * onward, one wave per map at a time; every store runs over consecutive words.
 * Workgroup 0 also writes the header; the snapshot and the cardinality row are
 * dealt over the whole grid.
 * DYN (a mixed-model trace) adds the dynamic half: the same sum over row 0 of
 * each particle's dynamic slab, read through its slab reference (dyn_slab_ref),
 * the owner's dynamic size and cardinality into the header, and the owner's
 * dynamic snapshot — k_trace_finish's transpose, strips of 64 components dealt
 * over the grid's waves: each field's 64 values in one coalesced load (zero
 * past the map's size, and on the ranks that do not own the particle) into the
 * wave's LDS strip at its phd_gaussian4d word, then the strip's 1344 words to
 * the block with consecutive lanes on consecutive words. */
template <bool DYN>
__global__ void __launch_bounds__(256) k_trace_shard_pack(TraceShardArgs a) {
    __shared__ float s_cn[TRACE_PB];
    __shared__ int s_hdr[TRACE_BH_WORDS];
    const int t = threadIdx.x, lane = t & 63, wid = t >> 6;
    const int base = blockIdx.x * TRACE_PB;
    const int best = a.hand[TRACE_H_PARTICLE];
    const bool owner = best / a.n == a.rank;
    float* pose_o = a.block + TRACE_BH_WORDS;
    float* cn_o = pose_o + (size_t)6 * a.n;
    float* snap_o = cn_o + a.n;
    float* row_o = snap_o + (size_t)PHD_NF * a.snap_cap;
    for (int q = wid; q < TRACE_PB; q += 4) {
        const int p = base + q;
        if (p >= a.n) break;
        int sz;
        const float cn = map_cardinality(slab_of(a.src[p], a.map_in, a.size_in, a.map_x, a.size_x, a.cap), a.cap, lane, sz);
        if (lane == 0) s_cn[q] = cn;
    }
    if (blockIdx.x == 0) {
        if (t < TRACE_BH_WORDS) s_hdr[t] = 0;
        __syncthreads();
        if (wid == 0 && owner) {
            int sz;
            const float cn =
                map_cardinality(slab_of(a.hand[TRACE_H_SLAB], a.map_in, a.size_in, a.map_x, a.size_x, a.cap), a.cap, lane, sz);
            if (lane == 0) {
                s_hdr[TRACE_BH_OWNER] = 1;
                s_hdr[TRACE_BH_SIZE] = sz;
                s_hdr[TRACE_BH_CARD] = __float_as_int(cn);
            }
        }
        if (t == 64) {
            const int e = a.err[3], prev = a.hand[TRACE_H_ERRPREV];
            s_hdr[TRACE_BH_ERR] = e >= prev ? e - prev : e;  // (the counter was taken and cleared in between)
            a.hand[TRACE_H_ERRPREV] = e;
        }
        if constexpr (DYN) {
            if (wid == 2 && owner) {
                int sz;
                const float cn = map_cardinality(dyn_slab_ref(a.hand[TRACE_H_SLAB], a), a.dcap, lane, sz);
                if (lane == 0) {
                    s_hdr[TRACE_BH_DSIZE] = sz;
                    s_hdr[TRACE_BH_DCARD] = __float_as_int(cn);
                }
            }
        }
    }
    __syncthreads();
    if (blockIdx.x == 0 && t < TRACE_BH_WORDS) ((int*)a.block)[t] = s_hdr[t];
    const int np = min(TRACE_PB, a.n - base);
    if (t < np) cn_o[base + t] = s_cn[t];
    if (t < 6 * np) pose_o[(size_t)6 * base + t] = ((const float*)a.pose)[(size_t)6 * base + t];
    // the owner's snapshot (Gaussian2D words, as k_trace_finish) and cardinality row; zeros elsewhere
    const Slab m = slab_of(a.hand[TRACE_H_SLAB], a.map_in, a.size_in, a.map_x, a.size_x, a.cap);
    const int rows = owner ? min(min(max(m.size, 0), a.cap), a.snap_cap) : 0;
    const int stride = gridDim.x * 256, g = blockIdx.x * 256 + t;
    for (int e = g; e < a.snap_cap * PHD_NF; e += stride) {
        const int k = e / PHD_NF, j = e - k * PHD_NF;
        const int f = j < 4 ? 3 + j : j < 6 ? j - 3 : 0;
        snap_o[e] = k < rows ? m.map[(size_t)f * a.cap + k] : 0.f;
    }
    for (int k = g; k < a.K; k += stride) row_o[k] = owner && a.card_row ? a.card_row[k] : 0.f;
    int used = TRACE_BH_WORDS + 7 * a.n + PHD_NF * a.snap_cap + a.K;  // (the rounding words)
    if constexpr (DYN) {
        __shared__ float s_dcn[TRACE_PB];
        __shared__ float s_strip[4][TRACE_STRIP_WORDS];
        float* dcn_o = a.block + used;
        float* dsnap_o = dcn_o + a.n;
        used += a.n + PHD_DYN_FIELDS * a.dsnap_cap;
        for (int q = wid; q < TRACE_PB; q += 4) {
            const int p = base + q;
            if (p >= a.n) break;
            int sz;
            const float cn = map_cardinality(dyn_slab_ref(a.src[p], a), a.dcap, lane, sz);
            if (lane == 0) s_dcn[q] = cn;
        }
        __syncthreads();
        if (t < np) dcn_o[base + t] = s_dcn[t];
        const Slab dm = dyn_slab_ref(a.hand[TRACE_H_SLAB], a);
        const int drows = owner ? min(min(max(dm.size, 0), a.dcap), a.dsnap_cap) : 0;
        const int strips = (a.dsnap_cap + 63) >> 6;
        const size_t dwords = (size_t)a.dsnap_cap * PHD_DYN_FIELDS;
        for (int s0 = blockIdx.x * 4; s0 < strips; s0 += gridDim.x * 4) {  // (the same trips for the four waves)
            const int k = (s0 + wid) * 64 + lane;
            for (int f = 0; f < PHD_DYN_FIELDS; f++) {
                // Gaussian4D words: cov[0..15] (rows 5..20), mean[0..3] (rows 1..4), weight (row 0)
                const int j = f >= 5 ? f - 5 : f >= 1 ? 15 + f : 20;
                s_strip[wid][lane * PHD_DYN_FIELDS + j] = k < drows ? dm.map[(size_t)f * a.dcap + k] : 0.f;
            }
            __syncthreads();
            const size_t w0 = (size_t)(s0 + wid) * TRACE_STRIP_WORDS;
            for (int e = lane; e < TRACE_STRIP_WORDS; e += 64)
                if (w0 + e < dwords) dsnap_o[w0 + e] = s_strip[wid][e];
            __syncthreads();
        }
    }
    if (blockIdx.x == 0 && used + t < (int)a.block_words) a.block[used + t] = 0.f;
}

/* Stage 4.  Workgroup 0: the expected pose by expected_pose_block over the N
 * gathered poses, and the owner's header, the arg-max particle's pose and the
 * ranks' error counts into the record.  Workgroup 1: card_expected in
 * k_trace_card / k_trace_finish's order (partials of TRACE_PB consecutive
 * global indices, term by term; thread t < 256 adds partials t, t + 256, ...;
 * wave scans; the four wave totals in order), then the owner's snapshot and
 * cardinality row into this scan's ring entries.
 * DYN adds workgroup 2: the dynamic card_expected by the same rule over the
 * gathered dynamic cardinalities, the owner's dynamic card_map and map_size,
 * the zeroed reserved words, and its dynamic snapshot — already phd_gaussian4d
 * words in the block — into this scan's entries of the dyn ring. */

/* card_expected over the N = world * n gathered particles, cardinalities at
 * word cn_at of every rank's block: by threads 0..255 of the workgroup (every
 * thread calls it; the value is thread 0's). */
__device__ __forceinline__ float shard_card_expected(const TraceShardArgs& a, size_t cn_at, float lse, double* s_w) {
    const int t = threadIdx.x;
    const int n = a.n, N = a.world * n;
    const int nparts = (N + TRACE_PB - 1) / TRACE_PB;
    double v = 0.0;
    if (t < 256)
        for (int b = t; b < nparts; b += 256) {
            double s = 0.0;
            for (int q = 0; q < TRACE_PB; q++) {
                const int p = b * TRACE_PB + q;
                double term = 0.0;
                if (p < N) {
                    const int r = p / n;
                    const float cn = a.blocks[(size_t)r * a.block_words + cn_at + (p - r * n)];
                    term = (double)expf(a.w_all[p] - lse) * (double)cn;
                }
                s += term;
            }
            v += s;
        }
    v = wave_incl_scan_d(v);
    if (t < 256 && (t & 63) == 63) s_w[t >> 6] = v;
    __syncthreads();
    return (float)(((s_w[0] + s_w[1]) + s_w[2]) + s_w[3]);
}

template <bool DYN>
__global__ void __launch_bounds__(RS_THREADS) k_trace_shard_finish(TraceShardArgs a) {
    const int t = threadIdx.x;
    const int n = a.n, N = a.world * n;
    const float lse = __int_as_float(a.hand[TRACE_H_LSE]);
    const int best = a.hand[TRACE_H_PARTICLE];
    const float* own = a.blocks + (size_t)(best / n) * a.block_words;
    auto pose_of = [&](int i) {
        const int r = i / n;
        return a.blocks + (size_t)r * a.block_words + TRACE_BH_WORDS + (size_t)6 * (i - r * n);
    };
    __shared__ double s_w[4];
    if (blockIdx.x == 0) {
        __shared__ double s_r[32];
        float ep[6];
        expected_pose_block_at(N, [&](int i) { return a.w_all[i] - lse; }, pose_of, ep, s_r);
        if (t == 0) {
            const float* mp = pose_of(best);
            a.rec->expected_pose = phd_pose{ep[0], ep[1], ep[2], ep[3], ep[4], ep[5]};
            a.rec->map_pose = phd_pose{mp[0], mp[1], mp[2], mp[3], mp[4], mp[5]};
            a.rec->card_map = own[TRACE_BH_CARD];
            a.rec->map_size = ((const int*)own)[TRACE_BH_SIZE];
            int errs = 0;
            for (int r = 0; r < a.world; r++) errs += ((const int*)(a.blocks + (size_t)r * a.block_words))[TRACE_BH_ERR];
            a.rec->status_errors = errs;
        }
    } else if (!DYN || blockIdx.x == 1) {
        const float ce = shard_card_expected(a, TRACE_BH_WORDS + (size_t)6 * n, lse, s_w);
        if (t == 0) a.rec->card_expected = ce;
        const float* snap_i = own + TRACE_BH_WORDS + (size_t)7 * n;
        if (a.snap)
            for (int e = t; e < a.snap_cap * PHD_NF; e += RS_THREADS) ((float*)a.snap)[e] = snap_i[e];
        if (a.card)
            for (int k = t; k < a.K; k += RS_THREADS) a.card[k] = snap_i[(size_t)PHD_NF * a.snap_cap + k];
    } else {
        const size_t dyn_at = TRACE_BH_WORDS + (size_t)7 * n + (size_t)PHD_NF * a.snap_cap + a.K;
        const float ce = shard_card_expected(a, dyn_at, lse, s_w);
        if (t == 0) {
            phd_trace_dyn_record d;
            d.card_expected = ce;
            d.card_map = own[TRACE_BH_DCARD];
            d.map_size = ((const int*)own)[TRACE_BH_DSIZE];
            for (int i = 0; i < 5; i++) d.reserved[i] = 0;
            *a.drec = d;
        }
        const float* dsnap_i = own + dyn_at + n;
        if (a.dsnap)
            for (int e = t; e < a.dsnap_cap * PHD_DYN_FIELDS; e += RS_THREADS) ((float*)a.dsnap)[e] = dsnap_i[e];
    }
}

void trace_launch_shard_weights(const TraceShardArgs& a, hipStream_t st) {
    hipLaunchKernelGGL(k_trace_shard_weights, dim3(1), dim3(RS_THREADS), 0, st, a);
}

void trace_launch_shard_pack(const TraceShardArgs& a, hipStream_t st) {
    const dim3 grid((a.n + TRACE_PB - 1) / TRACE_PB);
#if PHD_TRACE_DYN
    if (a.dmap) {
        hipLaunchKernelGGL(k_trace_shard_pack<true>, grid, dim3(256), 0, st, a);
        return;
    }
#endif
    hipLaunchKernelGGL(k_trace_shard_pack<false>, grid, dim3(256), 0, st, a);
}

void trace_launch_shard_finish(const TraceShardArgs& a, hipStream_t st) {
#if PHD_TRACE_DYN
    if (a.dmap) {
        hipLaunchKernelGGL(k_trace_shard_finish<true>, dim3(3), dim3(RS_THREADS), 0, st, a);
        return;
    }
#endif
    hipLaunchKernelGGL(k_trace_shard_finish<false>, dim3(2), dim3(RS_THREADS), 0, st, a);
}

}  // namespace phd
