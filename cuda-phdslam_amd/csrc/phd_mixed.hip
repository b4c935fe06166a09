/*
 * phd_mixed.hip — the mixed static + dynamic feature model on gfx950
 * (feature_model = 2).
 *
 * k_predict_dynamic: predictMapMixed (phdfilter.cu:966-1035, kernel :910-963),
 *   one thread per dynamic component of every slab: constant-velocity
 *   prediction, weight x p_jmm x ps.  Static maps are not predicted (:1241).
 * k_update_mixed: phdUpdateSynth's MIXED_MODEL branch (:3412-3462,
 *   phdUpdateKernelMixed :2323-2635, mergeAndCopyMaps :3703-3726), one
 *   256-thread workgroup per particle:
 *     1. range classes of both maps (computeInRangeKernel :1327-1346),
 *        order-preserving ballot compaction (static: in / near / out; dynamic:
 *        in — the rest is dropped, :3715-3719);
 *     2. pre-update terms of every in-range component (computePreUpdate
 *        :302-521) into per-particle global scratch;
 *     3. one normaliser per measurement over BOTH maps' detection terms +
 *        clutter + birth weight(s) (:2463-2550), a thread per measurement
 *        summing in component order (double); Δ log w = Σ log η_m − Σ pd w
 *        (:2553);
 *     4. per map: candidates in the reference's update-array order
 *        [non-detect | detect (m-major) | births] (+ nearly in-range static
 *        components), pruned below minFeatureWeight (:2611-2633), compacted in
 *        order into global scratch;
 *     5. per map: the greedy merge of phdUpdateMergeKernel (:2739-2890): seed =
 *        heaviest unmerged (lowest index on ties, D1), members = unmerged with
 *        d(seed, i) < minSeparation (2-D / 4-D Mahalanobis), listed in index
 *        order; one lane sums them in that order in double, so the moments
 *        equal the oracle's bit for bit; static out-of-range components are
 *        appended.
 * k_predict_dynamic_x: the sharded step's share — the prediction of the
 *   dynamic migration set X in place (the migration records that carry the
 *   dynamic map: phd_records.hip).
 * The arithmetic is include/phd_mixed.h (the oracle restates it on its own in
 * oracle/mixed_ref.h; both are held to tests/mixed_ref64.py).  This is a
 * correctness-first form: no benchmark config of the reference uses the mixed
 * model, so it is not tuned like the static update.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>

#include <hipcub/hipcub.hpp>

#include <vector>

#include "phd_detmath.h"
#include "phd_kernels.h" /* the block header and the launches the blocks forms share (phd_eap.hip) */
#include "phd_mixed_k.h"

namespace phd {

#define MX_NT 256
#define MX_W (MX_NT / 64)
#define MX_EKF 32 /* floats of one phd_mx_ekf */

static_assert(sizeof(phd_mx_ekf) == MX_EKF * sizeof(float), "phd_mx_ekf layout");

/* rank of this thread among the block's threads with pred set (thread order) */
__device__ __forceinline__ int mx_rank(bool pred, int* s_w, int* total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const unsigned long long b = __ballot(pred);
    const int within = __popcll(b & ((1ull << lane) - 1ull));
    __syncthreads();  // s_w of a previous call has been read
    if (lane == 0) s_w[wid] = __popcll(b);
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < MX_W; w++) {
        const int c = s_w[w];
        off += (w < wid) ? c : 0;
        tot += c;
    }
    *total = tot;
    return off + within;
}

__device__ __forceinline__ bool mx_better(float aw, int ai, float bw, int bi) {
    return ai >= 0 && (bi < 0 || aw > bw || (aw == bw && ai < bi));
}

template <int D>
struct MxComp {
    static constexpr int F = 1 + D + D * D;  // w | mean | cov
};

/* prior component j of a slab (static SoA: w mx my P00 P10 P01 P11; dynamic:
 * w m0..m3 c0..c15) */
template <int D>
__device__ __forceinline__ void mx_read_prior(const float* slab, int scap, int j, float& w, float* m, float* c) {
    w = slab[j];
#pragma unroll
    for (int k = 0; k < D; k++) m[k] = slab[(1 + k) * scap + j];
#pragma unroll
    for (int k = 0; k < D * D; k++) c[k] = slab[(1 + D + k) * scap + j];
}

/* Candidates of one map in the reference's update-array order, pruned and
 * compacted into cand (AoS, F floats each).  Returns the count (> Kcap: overflow). */
template <int D>
__device__ int mx_candidates(const MixedArgs& a, const phd_pose& pose, const float* slab, int scap, const int* s_list,
                             int G, const phd_mx_ekf* ekf, const float* s_leta, const int* s_near, int Gnear,
                             int label, float* cand, int* s_w) {
    constexpr int F = MxComp<D>::F;
    const int M = a.M;
    const long R = (long)G + (long)M * G + M + Gnear;
    const float minw = a.c.minFeatureWeight;
    int K = 0;
    for (long base = 0; base < R; base += MX_NT) {
        const long r = base + threadIdx.x;
        float w = 0.f, m[D], c[D * D];
        bool keep = false;
        if (r < G) {  // non-detection
            const int j = s_list[r];
            float w0;
            mx_read_prior<D>(slab, scap, j, w0, m, c);
            w = w0 * (1 - ekf[r].pd);
            keep = !(w < minw);
        } else if (r < (long)G + (long)M * G) {  // detection of measurement mm by component t
            const long q = r - G;
            const int mm = (int)(q / G), t = (int)(q % G);
            const phd_mx_ekf& e = ekf[t];
            float w0;
            mx_read_prior<D>(slab, scap, s_list[t], w0, m, c);
            const int ok = a.zlab[mm] == label || !a.c.labeled;
            float i0, i1;
            const float lq = phd_mx_logq(e, w0, a.zr[mm], a.zb[mm], ok, &i0, &i1);
#pragma unroll
            for (int k = 0; k < D; k++) m[k] = m[k] + e.K[k] * i0 + e.K[(D == 2 ? 2 : 4) + k] * i1;
#pragma unroll
            for (int k = 0; k < D * D; k++) c[k] = e.cu[k];
            w = phd_det_expf(lq - s_leta[mm]);
            keep = !(w < minw);
        } else if (r < (long)G + (long)M * G + M) {  // birth of measurement mm
            const int mm = (int)(r - G - (long)M * G);
            const int ok = a.zlab[mm] == label || !a.c.labeled;
            const float lw = phd_mx_birth(a.c, pose, a.zr[mm], a.zb[mm], ok, D, m, c);
            w = phd_det_expf(lw - s_leta[mm]);
            keep = !(w < minw);
        } else if (r < R) {  // nearly in range (static): joins the merge unpruned
            mx_read_prior<D>(slab, scap, s_near[r - G - (long)M * G - M], w, m, c);
            keep = true;
        }
        int tot;
        const int slot = K + mx_rank(keep, s_w, &tot);
        if (keep && slot < a.Kcap) {
            float* o = cand + (size_t)slot * F;
            o[0] = w;
#pragma unroll
            for (int k = 0; k < D; k++) o[1 + k] = m[k];
#pragma unroll
            for (int k = 0; k < D * D; k++) o[1 + D + k] = c[k];
        }
        K += tot;
    }
    __syncthreads();  // candidates visible to the block
    return K;
}

/* Greedy merge (phdUpdateMergeKernel) of K candidates into dst (SoA slab,
 * capacity scap).  Returns the number of merged components (may exceed scap:
 * overflow, only the first scap written). */
template <int D>
__device__ int mx_merge(const MixedArgs& a, const float* cand, int K, float* dst, int scap, unsigned char* s_merged,
                        int* s_list, int* s_w, float* s_wf, int* s_wi, int* s_misc) {
    constexpr int F = MxComp<D>::F;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const float T = a.c.minSeparation;
    for (int i = tid; i < K; i += MX_NT) s_merged[i] = 0;
    __syncthreads();
    int nout = 0;
    while (true) {
        // seed: heaviest unmerged candidate, lowest index on ties (D1)
        float bw = 0.f;
        int bi = -1;
        for (int i = tid; i < K; i += MX_NT) {
            if (s_merged[i]) continue;
            const float w = cand[(size_t)i * F];
            if (mx_better(w, i, bw, bi)) {
                bw = w;
                bi = i;
            }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ow = __shfl_xor(bw, off);
            const int oi = __shfl_xor(bi, off);
            if (mx_better(ow, oi, bw, bi)) {
                bw = ow;
                bi = oi;
            }
        }
        if (lane == 0) {
            s_wf[wid] = bw;
            s_wi[wid] = bi;
        }
        __syncthreads();
        if (tid == 0) {
            float w0 = s_wf[0];
            int i0 = s_wi[0];
            for (int w = 1; w < MX_W; w++)
                if (mx_better(s_wf[w], s_wi[w], w0, i0)) {
                    w0 = s_wf[w];
                    i0 = s_wi[w];
                }
            s_misc[0] = i0;
        }
        __syncthreads();
        const int seed = s_misc[0];
        if (seed < 0) break;
        const float* sd = cand + (size_t)seed * F;
        float sm[D], sc[D * D];
#pragma unroll
        for (int k = 0; k < D; k++) sm[k] = sd[1 + k];
#pragma unroll
        for (int k = 0; k < D * D; k++) sc[k] = sd[1 + D + k];
        // members in index order
        int cnt = 0;
        for (int base = 0; base < K; base += MX_NT) {
            const int i = base + tid;
            bool mem = false;
            if (i < K && !s_merged[i]) {
                const float* ci = cand + (size_t)i * F;
                const float d = D == 2 ? phd_mahal2(sc, sm, ci + 1 + D, ci + 1) : phd_mahal4(sc, sm, ci + 1 + D, ci + 1);
                mem = d < T;
            }
            int tot;
            const int r = mx_rank(mem, s_w, &tot);
            if (mem) s_list[cnt + r] = i;
            cnt += tot;
        }
        __syncthreads();
        if (tid == 0) {
            double W = 0.0, md[D];
#pragma unroll
            for (int k = 0; k < D; k++) md[k] = 0.0;
            for (int q = 0; q < cnt; q++) {
                const float* ci = cand + (size_t)s_list[q] * F;
                W += (double)ci[0];
#pragma unroll
                for (int k = 0; k < D; k++) md[k] += (double)(ci[0] * ci[1 + k]);
            }
            const float Wf = (float)W;
            int stop = 0;
            if (Wf == 0.f) {
                stop = 1;
            } else {
                float g[D], gc[D * D];
                double cd[D * D];
#pragma unroll
                for (int k = 0; k < D; k++) g[k] = (float)md[k] / Wf;
#pragma unroll
                for (int k = 0; k < D * D; k++) cd[k] = 0.0;
                for (int q = 0; q < cnt; q++) {
                    const float* ci = cand + (size_t)s_list[q] * F;
                    float dm[D];
#pragma unroll
                    for (int k = 0; k < D; k++) dm[k] = g[k] - ci[1 + k];
                    const float w = ci[0];
#pragma unroll
                    for (int j = 0; j < D; j++)
#pragma unroll
                        for (int k = 0; k < D; k++)
                            cd[j * D + k] += (double)(w * (ci[1 + D + j * D + k] + dm[j] * dm[k]));
                    s_merged[s_list[q]] = 1;
                }
#pragma unroll
                for (int k = 0; k < D * D; k++) gc[k] = (float)cd[k] / Wf;
                phd_mx_symmetrize(gc, D);
                if (nout < scap) {
                    dst[nout] = Wf;
#pragma unroll
                    for (int k = 0; k < D; k++) dst[(1 + k) * scap + nout] = g[k];
#pragma unroll
                    for (int k = 0; k < D * D; k++) dst[(1 + D + k) * scap + nout] = gc[k];
                }
            }
            s_misc[1] = stop;
        }
        __syncthreads();
        if (s_misc[1]) break;
        nout++;
    }
    return nout;
}

__global__ void __launch_bounds__(MX_NT) k_update_mixed(MixedArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mx_smem[];
    // block b does particle b, or (a sharded step's overflow recovery) slots[b]:
    // either way it writes the particle's own slab of the output sets and
    // resets its reference itself
    const int n = a.slots ? a.slots[blockIdx.x] : blockIdx.x, tid = threadIdx.x;
    const int cap = a.cap, dcap = a.dcap, M = a.M;
    int* s_in = (int*)mx_smem;
    int* s_near = s_in + cap;
    int* s_out = s_near + cap;
    int* d_in = s_out + cap;
    float* s_leta = (float*)(d_in + dcap);
    int* s_list = (int*)(s_leta + (M > 0 ? M : 1));
    unsigned char* s_merged = (unsigned char*)(s_list + a.Kcap);
    __shared__ int s_w[MX_W];
    __shared__ float s_wf[MX_W];
    __shared__ int s_wi[MX_W];
    __shared__ int s_misc[4];
    __shared__ float s_delta;

    const phd_pose pose = a.poses[n];
    // the prior, static and dynamic, through the slab reference (bit 30: the sets X)
    const int sref = a.src[n];
    const float* S = slab_map(sref, a.map_in, a.map_x, cap);
    const float* DY = dyn_slab_map(sref, a.dmap_in, a.dmap_x, dcap);
    const int ns = min(slab_size(sref, a.size_in, a.size_x), cap);
    const int nd = min(slab_size(sref, a.dsize_in, a.dsize_x), dcap);
    int flags = 0;

    // 1. range classes, order-preserving compaction
    int Gs = 0, Gn = 0, Go = 0, Gd = 0;
    for (int base = 0; base < ns; base += MX_NT) {
        const int j = base + tid;
        const int cls = j < ns ? phd_mx_range_class(a.c, pose, S[cap + j], S[2 * cap + j]) : -1;
        int t1, t2, t0;
        const int r1 = mx_rank(cls == 1, s_w, &t1);
        if (cls == 1) s_in[Gs + r1] = j;
        const int r2 = mx_rank(cls == 2, s_w, &t2);
        if (cls == 2) s_near[Gn + r2] = j;
        const int r0 = mx_rank(cls == 0, s_w, &t0);
        if (cls == 0) s_out[Go + r0] = j;
        Gs += t1;
        Gn += t2;
        Go += t0;
    }
    for (int base = 0; base < nd; base += MX_NT) {
        const int j = base + tid;
        const int cls = j < nd ? phd_mx_range_class(a.c, pose, DY[dcap + j], DY[2 * dcap + j]) : -1;
        int t1;
        const int r1 = mx_rank(cls == 1, s_w, &t1);
        if (cls == 1) d_in[Gd + r1] = j;
        Gd += t1;
    }
    __syncthreads();

    // 2. pre-update terms of the in-range components
    phd_mx_ekf* es = (phd_mx_ekf*)(a.ekf + (size_t)n * (cap + dcap) * MX_EKF);
    phd_mx_ekf* ed = es + cap;
    for (int t = tid; t < Gs + Gd; t += MX_NT) {
        phd_mx_ekf e;
        if (t < Gs) {
            float w, m[2], c[4];
            mx_read_prior<2>(S, cap, s_in[t], w, m, c);
            phd_mx_ekf2(a.c, pose, m, c, e);
            es[t] = e;
        } else {
            float w, m[4], c[16];
            mx_read_prior<4>(DY, dcap, d_in[t - Gs], w, m, c);
            phd_mx_ekf4(a.c, pose, m, c, e);
            ed[t - Gs] = e;
        }
    }
    __syncthreads();

    // 3. normalisers (both maps) and the particle weight
    for (int m = tid; m < M; m += MX_NT) {
        const int ok_s = a.zlab[m] == PHD_MEAS_STATIC || !a.c.labeled;
        const int ok_d = a.zlab[m] == PHD_MEAS_DYNAMIC || !a.c.labeled;
        double sd = 0.0;
        float i0, i1;
        for (int t = 0; t < Gs; t++)
            sd += (double)phd_det_expf(phd_mx_logq(es[t], S[s_in[t]], a.zr[m], a.zb[m], ok_s, &i0, &i1));
        for (int t = 0; t < Gd; t++)
            sd += (double)phd_det_expf(phd_mx_logq(ed[t], DY[d_in[t]], a.zr[m], a.zb[m], ok_d, &i0, &i1));
        sd += (double)a.c.clutterDensity;
        sd += (double)a.c.birthWeight;
        if (!a.c.labeled) sd += (double)a.c.birthWeight;
        s_leta[m] = phd_mx_safe_log((float)sd);
    }
    __syncthreads();
    if (tid == 0) {
        double card = 0.0;
        for (int t = 0; t < Gs; t++) card += (double)(es[t].pd * S[s_in[t]]);
        for (int t = 0; t < Gd; t++) card += (double)(ed[t].pd * DY[d_in[t]]);
        float pw = 0.f;
        for (int m = 0; m < M; m++) pw += s_leta[m];
        s_delta = pw - (float)card;
    }

    // 4-5. static map: candidates, merge, out-of-range appended
    float* cs = a.cand + (size_t)n * a.Kcap * (MxComp<2>::F + MxComp<4>::F);
    float* cd = cs + (size_t)a.Kcap * MxComp<2>::F;
    float* so = a.map_out + (size_t)n * 7 * cap;
    int Ks = mx_candidates<2>(a, pose, S, cap, s_in, Gs, es, s_leta, s_near, Gn, PHD_MEAS_STATIC, cs, s_w);
    if (Ks > a.Kcap) {
        flags |= PHD_ST_CANDIDATE_OVERFLOW_MX;
        Ks = a.Kcap;
    }
    const int nos = mx_merge<2>(a, cs, Ks, so, cap, s_merged, s_list, s_w, s_wf, s_wi, s_misc);
    for (int t = tid; t < Go; t += MX_NT) {
        const int slot = nos + t;
        if (slot < cap)
            for (int f = 0; f < 7; f++) so[f * cap + slot] = S[f * cap + s_out[t]];
    }
    // dynamic map
    float* dout = a.dmap_out + (size_t)n * PHD_DYN_FIELDS * dcap;
    int Kd = mx_candidates<4>(a, pose, DY, dcap, d_in, Gd, ed, s_leta, nullptr, 0, PHD_MEAS_DYNAMIC, cd, s_w);
    if (Kd > a.Kcap) {
        flags |= PHD_ST_CANDIDATE_OVERFLOW_MX;
        Kd = a.Kcap;
    }
    const int nod = mx_merge<4>(a, cd, Kd, dout, dcap, s_merged, s_list, s_w, s_wf, s_wi, s_misc);
    if (tid == 0) {
        int ts = nos + Go;
        if (ts > cap || nod > dcap) flags |= PHD_ST_MAP_OVERFLOW_MX;
        a.size_out[n] = min(ts, cap);
        a.dsize_out[n] = min(nod, dcap);
        a.status[n] = flags;
        if (flags) {
            atomicOr(a.err, flags);
            atomicAdd(a.err + 3, 1);
        }
        a.delta[n] = s_delta;
        a.logw[n] += s_delta;
        a.src_reset[n] = n;
    }
}

__global__ void __launch_bounds__(256) k_predict_dynamic(int nslabs, int dcap, const float* __restrict__ din,
                                                         const int* __restrict__ dsize_in, float* __restrict__ dout,
                                                         int* __restrict__ dsize_out, phd_mx_cfg c) {
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int s = (int)(gid / dcap), k = (int)(gid % dcap);
    if (s >= nslabs) return;
    const int sz = min(max(dsize_in[s], 0), dcap);
    if (k == 0) dsize_out[s] = sz;
    if (k >= sz) return;
    const float* src = din + (size_t)s * PHD_DYN_FIELDS * dcap;
    float* dst = dout + (size_t)s * PHD_DYN_FIELDS * dcap;
    float w, m[4], p[16], mo[4], po[16], wo;
    mx_read_prior<4>(src, dcap, k, w, m, p);
    phd_mx_predict4(c, m, p, w, mo, po, &wo);
    dst[k] = wo;
    for (int i = 0; i < 4; i++) dst[(1 + i) * dcap + k] = mo[i];
    for (int i = 0; i < 16; i++) dst[(5 + i) * dcap + k] = po[i];
}

/* predictMapMixed of dynamic set X in place (no __restrict__: source and
 * destination are the same slab; a thread reads its whole component before it
 * writes it and touches no other).  One workgroup per slab of X (slots NULL),
 * or per listed slot: the slab its reference names, done by the first of the
 * consecutive slots naming it (phd_mixed_k.h). */
__global__ void __launch_bounds__(256) k_predict_dynamic_x(const int* slots, const int* src, int dcap, float* dmap_x,
                                                           const int* dsize_x, phd_mx_cfg c) {
    int s = blockIdx.x;
    if (slots) {
        const int sref = src[slots[blockIdx.x]];
        if (!slab_in_x(sref)) return;
        if (blockIdx.x > 0 && src[slots[blockIdx.x - 1]] == sref) return;
        s = slab_index(sref);
    }
    const int sz = min(max(dsize_x[s], 0), dcap);
    float* d = dmap_x + (size_t)s * PHD_DYN_FIELDS * dcap;
    for (int k = threadIdx.x; k < sz; k += blockDim.x) {
        float w, m[4], p[16], mo[4], po[16], wo;
        mx_read_prior<4>(d, dcap, k, w, m, p);
        phd_mx_predict4(c, m, p, w, mo, po, &wo);
        d[k] = wo;
        for (int i = 0; i < 4; i++) d[(1 + i) * dcap + k] = mo[i];
        for (int i = 0; i < 16; i++) d[(5 + i) * dcap + k] = po[i];
    }
}

size_t mixed_lds_bytes(int cap, int dcap, int Mcap, int Kcap) {
    return (size_t)4 * (3 * (size_t)cap + dcap) + 4 * (size_t)(Mcap > 0 ? Mcap : 1) + 4 * (size_t)Kcap +
           (size_t)Kcap + 16;
}

size_t mixed_ekf_floats(int cap, int dcap) { return (size_t)(cap + dcap) * MX_EKF; }

size_t mixed_cand_floats(int Kcap) { return (size_t)Kcap * (MxComp<2>::F + MxComp<4>::F); }

hipError_t mixed_set_lds_limit() {
    // (the static __shared__ words come out of the same 160 KB)
    return hipFuncSetAttribute((const void*)k_update_mixed, hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
}

hipError_t mixed_launch_update(const MixedArgs& a, size_t lds, hipStream_t s) {
    hipLaunchKernelGGL(k_update_mixed, dim3(a.n), dim3(MX_NT), lds, s, a);
    return hipGetLastError();
}

hipError_t mixed_launch_predict(int nslabs, int dcap, const float* din, const int* dsize_in, float* dout,
                                int* dsize_out, const phd_mx_cfg& c, hipStream_t s) {
    const long total = (long)nslabs * dcap;
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_predict_dynamic, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, nslabs, dcap, din,
                       dsize_in, dout, dsize_out, c);
    return hipGetLastError();
}

hipError_t mixed_launch_predict_x(const int* slots, int count, const int* src, int dcap, float* dmap_x,
                                  const int* dsize_x, const phd_mx_cfg& c, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_predict_dynamic_x, dim3(count), dim3(256), 0, s, slots, src, dcap, dmap_x, dsize_x, c);
    return hipGetLastError();
}

/* ---- EAP map of the dynamic maps (exp_map_dynamic, main.cpp:369-371) ----
 * computeExpectedMap over maps_dynamic (main.cpp:290-316): every particle's
 * Gaussian4D components with weight x exp(log w_n) (D8: det_expf), then
 * reduceGaussianMixture<Gaussian4D> (gm_reduce.cpp:59-132): stable priority
 * order (weight descending, concatenation index ascending; a stable radix
 * sort), seeds in that order absorb every unmerged later component at LLT
 * Mahalanobis distance < minSeparation (phd_eap_mahal4), the moments summed
 * serially in priority order by one lane (phd_eap4_*, the oracle's
 * expressions: orc_expected_map_dynamic).  Two forms of the greedy, the same
 * bytes in the same order: decision rounds over the whole GPU (k_eap4_bound ..
 * k_eap4_sum below: the static map's stages, phd_eap.hip, for 21-field
 * components), and one workgroup over the whole set (k_eap4_merge: the
 * fallback of inputs the lattice bound does not cover, and mode 1). */
/* particle blockIdx.x's weighted components into the SoA comp (21 fields of
 * stride K) at its offset: the single context's gather and the sharded pack */
__device__ __forceinline__ void eap4_gather_particle(const int* __restrict__ src, const float* __restrict__ dmap,
                                                     const float* __restrict__ dmap_x,
                                                     const int* __restrict__ off, const float* __restrict__ logw,
                                                     int dcap, long K, float* __restrict__ comp) {
    const int p = blockIdx.x;
    const float* s = dyn_slab_map(src[p], dmap, dmap_x, dcap);
    const int o = off[p], sz = off[p + 1] - o;
    const float ew = phd_det_expf(logw[p]);
    for (int k = threadIdx.x; k < sz; k += blockDim.x) {
        comp[o + k] = s[k] * ew;  // map[i].weight *= exp(weights[n]) (main.cpp:302-303)
        for (int f = 1; f < PHD_DYN_FIELDS; f++) comp[(size_t)f * K + o + k] = s[(size_t)f * dcap + k];
    }
}

__global__ void __launch_bounds__(256) k_eap4_gather(const int* __restrict__ src, const float* __restrict__ dmap,
                                                     const float* __restrict__ dmap_x,
                                                     const int* __restrict__ off, const float* __restrict__ logw,
                                                     int dcap, long K, float* __restrict__ comp) {
    eap4_gather_particle(src, dmap, dmap_x, off, logw, dcap, K, comp);
}

/* The sharded form's block of this rank ("EAP4", include/phd_capi.h): the
 * header (workgroup 0) and the gather aimed at the block's fields, stride
 * K_max — the same product, so the same bits, as the single context's SoA.
 * off[n] = K_r <= K_max (the host checked it): no entry past the block. */
__global__ void __launch_bounds__(256) k_eap4_pack(const int* __restrict__ src, const float* __restrict__ dmap,
                                                   const float* __restrict__ dmap_x,
                                                   const int* __restrict__ off, const float* __restrict__ logw,
                                                   int dcap, int n, unsigned int K_max, unsigned int* __restrict__ block) {
    if (blockIdx.x == 0 && threadIdx.x < EAP_BH_WORDS) {
        const int t = threadIdx.x;
        unsigned int v = 0;
        if (t == EAP_BH_LAYOUT) v = EAP4_BLOCK_LAYOUT;
        if (t == EAP_BH_COUNT) v = (unsigned int)off[n];
        if (t == EAP_BH_N) v = (unsigned int)n;
        if (t == EAP_BH_KMAX) v = K_max;
        block[t] = v;
    }
    eap4_gather_particle(src, dmap, dmap_x, off, logw, dcap, (long)K_max, (float*)(block + EAP_BH_WORDS));
}

__global__ void k_eap4_iota(unsigned int* a, long n) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = (unsigned int)i;
}

#define EAP4_NT 1024
__global__ void __launch_bounds__(EAP4_NT) k_eap4_merge(const float* __restrict__ comp, long K,
                                                        const unsigned int* __restrict__ ord, float T,
                                                        unsigned char* __restrict__ flag, unsigned int* __restrict__ mem,
                                                        phd_gaussian4d* __restrict__ out, int* __restrict__ nout) {
    __shared__ int s_w[EAP4_NT / 64];
    __shared__ float s_seed[PHD_DYN_FIELDS];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    for (long j = tid; j < K; j += EAP4_NT) flag[j] = 0;
    __syncthreads();
    auto fld = [&](unsigned int c, int f) { return comp[(size_t)f * K + c]; };
    int count = 0;
    long p = 0;
    while (p < K) {
        // the seed: the first unmerged priority position >= p
        long s = K;
        for (long base = p; base < K && s == K; base += EAP4_NT) {
            const long j = base + tid;
            int v = (j < K && flag[j] == 0) ? (int)(j - base) : EAP4_NT;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
            if (lane == 0) s_w[wid] = v;
            __syncthreads();
            int m = EAP4_NT;
            for (int w = 0; w < EAP4_NT / 64; w++) m = min(m, s_w[w]);
            __syncthreads();
            if (m < EAP4_NT) s = base + m;
        }
        if (s >= K) break;
        const unsigned int si = ord[s];
        if (tid < PHD_DYN_FIELDS) s_seed[tid] = fld(si, tid);
        __syncthreads();
        float sm[4], sc[16];
        for (int i = 0; i < 4; i++) sm[i] = s_seed[1 + i];
        for (int i = 0; i < 16; i++) sc[i] = s_seed[5 + i];
        // absorb the unmerged later components within T, listed in priority order
        int nm = 0;
        for (long base = s + 1; base < K; base += EAP4_NT) {
            const long j = base + tid;
            bool in = false;
            if (j < K && flag[j] == 0) {
                const unsigned int bi = ord[j];
                float bm[4], bc[16];
                for (int i = 0; i < 4; i++) bm[i] = fld(bi, 1 + i);
                for (int i = 0; i < 16; i++) bc[i] = fld(bi, 5 + i);
                in = phd_eap_mahal4(sm, sc, bm, bc) < T;
            }
            const unsigned long long b = __ballot(in);
            if (lane == 0) s_w[wid] = __popcll(b);
            __syncthreads();
            int pre = nm, tot = 0;
            for (int w = 0; w < EAP4_NT / 64; w++) {
                if (w < wid) pre += s_w[w];
                tot += s_w[w];
            }
            if (in) {
                flag[j] = 1;
                mem[pre + __popcll(b & ((1ull << lane) - 1ull))] = (unsigned int)j;
            }
            nm += tot;
            __syncthreads();
        }
        if (tid == 0) {
            phd_eap4_acc acc;
            const float sw = s_seed[0];
            phd_eap4_mean_begin(acc, sw, sm);
            for (int k = 0; k < nm; k++) {
                const unsigned int bi = ord[mem[k]];
                float bm[4];
                for (int i = 0; i < 4; i++) bm[i] = fld(bi, 1 + i);
                phd_eap4_mean_add(acc, fld(bi, 0), bm);
            }
            phd_eap4_cov_begin(acc, sw, sm, sc);
            for (int k = 0; k < nm; k++) {
                const unsigned int bi = ord[mem[k]];
                float bm[4], bc[16];
                for (int i = 0; i < 4; i++) bm[i] = fld(bi, 1 + i);
                for (int i = 0; i < 16; i++) bc[i] = fld(bi, 5 + i);
                phd_eap4_cov_add(acc, fld(bi, 0), bm, bc);
            }
            phd_eap4_finish(acc, out + count);
            flag[s] = 1;
        }
        count++;
        __syncthreads();
        p = s + 1;
    }
    if (tid == 0) *nout = count;
}

/* ---- the decision rounds: the static map's exact parallel greedy
 * (phd_eap.hip, steps 2-6 of its header) for Gaussian4D components ----
 * The lattice lies over the two position coordinates, cell side
 * R = sqrt(1.05 T Λ), Λ the largest covariance trace of the set: a pair with
 * phd_eap_mahal4 < T has |Δμ|² (all four coordinates, so the two of the
 * position too) below 1.05 T (tr_a + tr_b) / 2 <= 1.05 T Λ (DESIGN.md §6,
 * "Decision rounds": the bound for the float LLT as phd_eap_mahal4 states it, at any
 * conditioning), so merge edges only join cells that touch. */

/* the trace the bound, the records and the cull all use (one expression) */
__device__ __forceinline__ float eap4_trace(float c00, float c11, float c22, float c33) {
    return c00 + c11 + c22 + c33;
}

/* a positive variance below this (2^-60) leaves the range in which the bound's
 * rounding argument holds (products of Cholesky entries may underflow) */
#define EAP4_VAR_MIN 8.673617379884035e-19f

/* The bound pass over a prepared SoA: Λ = the largest trace, as float bits
 * (non-negative floats order as their bit patterns), and the flag of inputs
 * the bound does not cover: a non-finite field (any of the 21), a negative
 * variance (the trace would no longer bound the averaged one's row sums to a
 * few ulps) or a positive variance below EAP4_VAR_MIN.  A finite covariance
 * that is merely not positive definite is covered: its pairs' distance is NaN
 * or infinite in every form, so they never merge. */
__global__ void __launch_bounds__(256) k_eap4_bound(const float* __restrict__ comp, long K,
                                                    unsigned int* __restrict__ lam_bits, int* __restrict__ bad) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    float tr = 0.f;
    bool flag = false;
    if (i < K) {
        for (int f = 0; f < PHD_DYN_FIELDS; f++) flag |= !(fabsf(comp[(size_t)f * K + i]) < INFINITY);
        float d[4];
        for (int a = 0; a < 4; a++) {
            d[a] = comp[(size_t)(5 + 5 * a) * K + i];
            flag |= d[a] < 0.f || (d[a] > 0.f && d[a] < EAP4_VAR_MIN);
        }
        tr = eap4_trace(d[0], d[1], d[2], d[3]);
        if (flag) tr = 0.f;
    }
    if (__ballot(flag) != 0ull && (threadIdx.x & 63) == 0) atomicOr(bad, 1);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tr = fmaxf(tr, __shfl_xor(tr, o, 64));
    if ((threadIdx.x & 63) == 0 && tr > 0.f) atomicMax(lam_bits, __float_as_uint(tr));
}

/* Records in cell order t (pos_by_cell order), four planes of K float4 — what
 * the decision rounds read, 16 words: (mean 0..3) | (trace, position bits,
 * c00, c10) | (c20, c30, c11, c21) | (c31, c22, c32, c33): the lower triangle
 * of the column-major covariance, all phd_eap_mahal4 reads. */
__global__ void k_eap4_cellrec(const float* __restrict__ comp, long K, const unsigned int* __restrict__ ord,
                               const unsigned int* __restrict__ pos_by_cell, float4* __restrict__ rec) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= K) return;
    const unsigned int p = pos_by_cell[t];
    const unsigned int i = ord[p];
    auto c = [&](int k) { return comp[(size_t)(5 + k) * K + i]; };
    rec[t] = make_float4(comp[1 * K + i], comp[2 * K + i], comp[3 * K + i], comp[4 * K + i]);
    rec[K + t] = make_float4(eap4_trace(c(0), c(5), c(10), c(15)), __uint_as_float(p), c(0), c(1));
    rec[2 * K + t] = make_float4(c(2), c(3), c(5), c(6));
    rec[3 * K + t] = make_float4(c(7), c(10), c(11), c(15));
}

/* a record's planes as phd_eap_mahal4's arguments (it reads the lower triangle
 * only; the upper entries are placeholders) */
__device__ __forceinline__ void eap4_rec_args(const float4& r0, const float4& r1, const float4& r2, const float4& r3,
                                              float* m, float* c) {
    m[0] = r0.x, m[1] = r0.y, m[2] = r0.z, m[3] = r0.w;
    c[0] = r1.z, c[1] = r1.w, c[2] = r2.x, c[3] = r2.y;
    c[5] = r2.z, c[6] = r2.w, c[7] = r3.x;
    c[10] = r3.y, c[11] = r3.z;
    c[15] = r3.w;
    c[4] = c[8] = c[9] = c[12] = c[13] = c[14] = 0.f;
}

#define EAP4R_NT 256 /* positions of a work item = records of a streamed tile */

/* One synchronous decision round for one chunk of one occupied cell (work item
 * = cell, first cell-order index, count; k_eap_lfmis's layout).  state[t]
 * (cell order): -1 undecided, -2 seed, else the absorbing seed's position.
 * Every thread owns one position j of the chunk and looks for its decider: the
 * first higher-priority position k of the 3 x 3 cells (own cell first) that is
 * not absorbed and has phd_eap_mahal4(k, j) < T — the seed is the first
 * argument pair, as in k_eap4_merge.  The workgroup streams the nine cells'
 * records through LDS in tiles of ascending position, entries already absorbed
 * or past every thread's need compacted away, and stops at the first tile no
 * thread still needs.  A pair passes the isotropic cull (|Δμ|² over all four
 * coordinates below 1.05 T (tr_k + tr_j) / 2; a squared norm that overflowed
 * is not culled) before the exact distance.  j becomes a seed with no decider,
 * is absorbed when its decider is a seed, and otherwise waits for the next
 * launch (counted): nothing here waits on another workgroup.  Decisions are
 * final, so a state read in the same round only decides earlier. */
__global__ void __launch_bounds__(EAP4R_NT)
    k_eap4_lfmis(const int4* __restrict__ work, const float4* __restrict__ rec, long K, const int* __restrict__ nb9,
                 const int* __restrict__ run, float T, int* state, int* __restrict__ pending) {
    __shared__ float4 s_r[4][EAP4R_NT];
    __shared__ int s_st[EAP4R_NT];
    __shared__ int s_w[EAP4R_NT / 64], s_c[EAP4R_NT / 64];
    const int4 wk = work[blockIdx.x];
    const int c = wk.x, t = wk.y + threadIdx.x;
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const bool own = (int)threadIdx.x < wk.z;
    const bool undecided = own && __hip_atomic_load(state + t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == -1;
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 r0 = z4, r1 = z4, r2 = z4, r3 = z4;
    if (undecided) {
        r0 = rec[t];
        r1 = rec[K + t];
        r2 = rec[2 * K + t];
        r3 = rec[3 * K + t];
    }
    float jm[4], jc[16];
    eap4_rec_args(r0, r1, r2, r3, jm, jc);
    const int pj = __float_as_int(r1.y);
    int best = undecided ? pj : -1;  // the deciding position so far (pj: none); -1: nothing to find
    int bst = 0;
    const float thr = 1.05f * T * 0.5f;
    for (int rr = 0; rr < 9; rr++) {
        const int r = rr == 0 ? 4 : (rr <= 4 ? rr - 1 : rr);  // own cell first: its decider is usually there
        const int cc = nb9[(size_t)c * 9 + r];
        if (cc < 0) continue;
        const int e1 = run[cc + 1];
        for (int base = run[cc]; base < e1; base += EAP4R_NT) {
            // the largest position any thread still accepts (block max; its barrier
            // also retires the previous tile)
            int v = best;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
            if (lane == 0) s_w[wid] = v;
            __syncthreads();
            int need = s_w[0];
#pragma unroll
            for (int w = 1; w < EAP4R_NT / 64; w++) need = max(need, s_w[w]);
            const int tn = min(EAP4R_NT, e1 - base);
            const int lead = __float_as_int(rec[K + base].y);
            if (lead >= need) break;  // ascending positions: no later tile of this cell is needed either
            // the tile's entries that can decide anyone: not absorbed, below `need`
            // (compacted in position order)
            float4 q1 = z4;
            int sq = 0;
            bool keep = false;
            if ((int)threadIdx.x < tn) {
                q1 = rec[K + base + threadIdx.x];
                sq = __hip_atomic_load(state + base + threadIdx.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                keep = sq < 0 && __float_as_int(q1.y) < need;
            }
            const unsigned long long kb = __ballot(keep);
            if (lane == 0) s_c[wid] = (int)__popcll(kb);
            __syncthreads();
            int off = 0, nk = 0;
#pragma unroll
            for (int w = 0; w < EAP4R_NT / 64; w++) {
                off += w < wid ? s_c[w] : 0;
                nk += s_c[w];
            }
            if (keep) {
                off += (int)__popcll(kb & ((1ull << lane) - 1ull));
                s_r[0][off] = rec[base + threadIdx.x];
                s_r[1][off] = q1;
                s_r[2][off] = rec[2 * K + base + threadIdx.x];
                s_r[3][off] = rec[3 * K + base + threadIdx.x];
                s_st[off] = sq;
            }
            __syncthreads();
            for (int e = 0; e < nk && best >= 0; e++) {
                const float4 e0 = s_r[0][e], e1v = s_r[1][e];
                const int k = __float_as_int(e1v.y);
                if (k >= best) break;
                const float d0 = e0.x - r0.x, d1 = e0.y - r0.y, d2 = e0.z - r0.z, d3 = e0.w - r0.w;
                const float n2 = d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3;
                if (n2 >= thr * (e1v.x + r1.x) && n2 < INFINITY) continue;
                float km[4], kc[16];
                eap4_rec_args(e0, e1v, s_r[2][e], s_r[3][e], km, kc);
                if (phd_eap_mahal4(km, kc, jm, jc) < T) {
                    best = k;
                    bst = s_st[e];
                    break;
                }
            }
        }
        __syncthreads();  // (the tile arrays and s_w are rewritten next)
    }
    bool wait = false;
    if (undecided) {
        if (best == pj || bst == -2) {
            __hip_atomic_store(state + t, best == pj ? -2 : best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        } else {
            wait = true;  // the first candidate seed is still undecided
        }
    }
    const unsigned long long b = __ballot(wait);
    if (lane == 0 && b != 0ull) atomicAdd(pending, (int)__popcll(b));
}

#define EAP4_PASS 64 /* members one LDS staging pass holds (one per lane) */

/* Merged moments of seed g, one wave (a 64-thread workgroup) per seed: members
 * mem[gstart[g] .. gstart[g + 1]) in priority order, the seed first.  The wave
 * stages EAP4_PASS members at a time in LDS and lane 0 sums them serially with
 * the shared phd_eap4_* functions in k_eap4_merge's order: the mean pass over
 * the whole group, then the covariance pass.  Slot g is the seed's rank among
 * the seeds in priority order, so out[] is in emission order. */
__global__ void __launch_bounds__(64)
    k_eap4_sum(const float* __restrict__ comp, long K, const unsigned int* __restrict__ ord,
               const unsigned int* __restrict__ mem, const int* __restrict__ gstart,
               phd_gaussian4d* __restrict__ out) {
    __shared__ float s_m[PHD_DYN_FIELDS][EAP4_PASS];
    const int lane = threadIdx.x;
    const int g = blockIdx.x;
    const int a = gstart[g], b = gstart[g + 1];
    const unsigned int si = ord[mem[a]];
    phd_eap4_acc acc;
    float sw = 0.f, sm[4], sc[16];
    if (lane == 0) {
        sw = comp[si];
        for (int i = 0; i < 4; i++) sm[i] = comp[(size_t)(1 + i) * K + si];
        for (int i = 0; i < 16; i++) sc[i] = comp[(size_t)(5 + i) * K + si];
        phd_eap4_mean_begin(acc, sw, sm);
    }
    for (int pass = 0; pass < 2; pass++) {
        if (pass == 1 && lane == 0) phd_eap4_cov_begin(acc, sw, sm, sc);
        const int nf = pass == 0 ? 5 : PHD_DYN_FIELDS;  // the mean pass reads the weight and the mean only
        for (int c0 = a + 1; c0 < b; c0 += EAP4_PASS) {
            const int cn = min(EAP4_PASS, b - c0);
            if (lane < cn) {
                const unsigned int bi = ord[mem[c0 + lane]];
                for (int f = 0; f < nf; f++) s_m[f][lane] = comp[(size_t)f * K + bi];
            }
            __syncthreads();
            if (lane == 0) {
                for (int k = 0; k < cn; k++) {
                    float bm[4], bc[16];
                    for (int i = 0; i < 4; i++) bm[i] = s_m[1 + i][k];
                    if (pass == 0) {
                        phd_eap4_mean_add(acc, s_m[0][k], bm);
                    } else {
                        for (int i = 0; i < 16; i++) bc[i] = s_m[5 + i][k];
                        phd_eap4_cov_add(acc, s_m[0][k], bm, bc);
                    }
                }
            }
            __syncthreads();  // (the staging rows are rewritten next)
        }
    }
    if (lane == 0) phd_eap4_finish(acc, out + g);
}

/* ------------------------------------------------------------------ host */

#define E4CHK(expr)                      \
    do {                                 \
        hipError_t _e = (expr);          \
        if (_e != hipSuccess) {          \
            err = hipGetErrorString(_e); \
            return -1;                   \
        }                                \
    } while (0)

/* Per-particle dynamic component counts of a store, clamped to [0, dcap], as
 * n + 1 host offsets (two read-backs: the slab references, then the sizes they
 * name).  Returns the component count, -1 on a HIP error (err). */
static long eap4_offsets(hipStream_t st, const int* d_src, const int* d_dsize, const int* d_dsize_x, int n, int dcap,
                         std::vector<int>& off, std::string& err) {
    std::vector<int> src(n);
    off.assign(n + 1, 0);
    E4CHK(hipMemcpyAsync(src.data(), d_src, n * sizeof(int), hipMemcpyDeviceToHost, st));
    E4CHK(hipStreamSynchronize(st));
    int maxs = 0, maxx = -1;  // the largest slab id named in the current set / in set X
    for (int p = 0; p < n; p++) {
        if (slab_in_x(src[p]))
            maxx = std::max(maxx, slab_index(src[p]));
        else
            maxs = std::max(maxs, slab_index(src[p]));
    }
    if (maxx >= 0 && !d_dsize_x) {
        err = "a slab reference names dynamic set X, which is not allocated";
        return -1;
    }
    std::vector<int> dsz(maxs + 1), dszx(maxx + 1);
    E4CHK(hipMemcpyAsync(dsz.data(), d_dsize, (maxs + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
    if (maxx >= 0) E4CHK(hipMemcpyAsync(dszx.data(), d_dsize_x, (maxx + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
    E4CHK(hipStreamSynchronize(st));
    long K = 0;
    for (int p = 0; p < n; p++) {
        K += std::min(std::max(slab_size(src[p], dsz.data(), dszx.data()), 0), dcap);
        off[p + 1] = (int)std::min<long>(K, 0x7fffffffL);
    }
    return K;
}

/* the reduce's device buffers for K components, carved from one allocation */
struct Eap4Bufs {
    float* comp;  // 21 x K SoA weighted components (concatenation order)
    float* wsorted;
    unsigned int *i0, *ord, *mem;
    unsigned char* flag;
    phd_gaussian4d* out;
    int* nout;
    // the decision rounds
    unsigned int* misc;              // [0] Λ bits [1] fallback flag [2] occupied cells [3] positions waiting
    unsigned long long *key, *key2;  // cell keys by position / sorted; later the seed keys and slots
    int *cnt, *run, *gstart;         // cell counts (later the seed flags), cell runs, group starts
    int* nb9;                        // 9 neighbour cells of every occupied cell
    float4* rec;                     // 4 planes of K: the records in cell order
    int4* work;                      // the rounds' work items
    int *state, *state_t;            // decisions by position / by cell order
    void* tmp;  // hipcub temporary storage
    size_t tmp_bytes;
};

static size_t eap4_carve(char* base, long K, size_t tmp, Eap4Bufs* b) {
    size_t o = 0;
    auto take = [&](size_t bytes) {
        char* q = base ? base + o : nullptr;
        o = (o + bytes + 255) & ~(size_t)255;
        return q;
    };
    Eap4Bufs t;
    t.comp = (float*)take((size_t)K * PHD_DYN_FIELDS * 4);
    t.wsorted = (float*)take((size_t)K * 4);
    t.i0 = (unsigned int*)take((size_t)K * 4);
    t.ord = (unsigned int*)take((size_t)K * 4);
    t.mem = (unsigned int*)take((size_t)K * 4);
    t.flag = (unsigned char*)take((size_t)K);
    t.out = (phd_gaussian4d*)take((size_t)K * sizeof(phd_gaussian4d));
    t.nout = (int*)take(4);
    t.misc = (unsigned int*)take(8 * 4);
    t.key = (unsigned long long*)take((size_t)K * 8);
    t.key2 = (unsigned long long*)take((size_t)K * 8);
    t.cnt = (int*)take((size_t)K * 4);
    t.run = (int*)take((size_t)(K + 1) * 4);
    t.gstart = (int*)take((size_t)(K + 1) * 4);
    t.nb9 = (int*)take((size_t)K * 9 * 4);
    t.rec = (float4*)take((size_t)K * 4 * sizeof(float4));
    t.work = (int4*)take(((size_t)K + (size_t)K / EAP4R_NT + 2) * sizeof(int4));
    t.state = (int*)take((size_t)K * 4);
    t.state_t = (int*)take((size_t)K * 4);
    t.tmp = take(tmp);
    t.tmp_bytes = tmp;
    if (b) *b = t;
    return o;
}

static size_t eap4_sort_tmp(long K, hipStream_t st) {
    size_t tmp = 0;
    hipcub::DeviceRadixSort::SortPairsDescending(nullptr, tmp, (float*)nullptr, (float*)nullptr,
                                                 (unsigned int*)nullptr, (unsigned int*)nullptr, (int)K, 0, 32, st);
    // the decision rounds' sorts (by cell, by seed), the cells' run-length encode and the seeds' scan
    size_t t2 = 0;
    hipcub::DeviceRadixSort::SortPairs(nullptr, t2, (unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                       (unsigned int*)nullptr, (unsigned int*)nullptr, (int)K, 0, 64, st);
    tmp = std::max(tmp, t2);
    hipcub::DeviceRadixSort::SortPairs(nullptr, t2, (unsigned int*)nullptr, (unsigned int*)nullptr,
                                       (unsigned int*)nullptr, (unsigned int*)nullptr, (int)K, 0, 32, st);
    tmp = std::max(tmp, t2);
    hipcub::DeviceRunLengthEncode::Encode(nullptr, t2, (unsigned long long*)nullptr, (unsigned long long*)nullptr,
                                          (int*)nullptr, (int*)nullptr, (int)K, st);
    tmp = std::max(tmp, t2);
    hipcub::DeviceScan::ExclusiveSum(nullptr, t2, (int*)nullptr, (int*)nullptr, (int)K, st);
    tmp = std::max(tmp, t2);
    return tmp;
}

static int eap4_bits_for(unsigned int v) {  // radix bits covering 0..v
    int b = 1;
    while (b < 32 && (v >> b) != 0) b++;
    return b;
}

/* The decision rounds of a prepared, priority-sorted SoA of bound Λ (finite,
 * positive; T too): cells, rounds, groups and sums, the merged components left
 * in B.out in emission order.  Returns their count, -1 (err). */
static long eap4_rounds(hipStream_t st, const Eap4Bufs& B, long K, float lam, float T, int* rounds, int* cells,
                        std::string& err) {
    const int Ki = (int)K;
    const unsigned int nb = (unsigned int)((K + 255) / 256);
    size_t tb;
    const double R = std::sqrt(1.05 * (double)T * (double)lam) * 1.0001;
    const float invR = (float)(1.0 / R);
    unsigned long long* keyp = B.key;   // cell key by position, then the unique occupied cells
    unsigned long long* keys = B.key2;  // cell keys sorted
    unsigned int* pos_by_cell = B.mem;  // positions grouped by cell, ascending within a cell
    hipLaunchKernelGGL(k_eap_poskey, dim3(nb), dim3(256), 0, st, B.comp, K, B.ord, invR, keyp, B.i0);
    tb = B.tmp_bytes;
    E4CHK(hipcub::DeviceRadixSort::SortPairs(B.tmp, tb, keyp, keys, B.i0, pos_by_cell, Ki, 0, 64, st));
    tb = B.tmp_bytes;
    E4CHK(hipcub::DeviceRunLengthEncode::Encode(B.tmp, tb, keys, keyp, B.cnt, (int*)B.misc + 2, Ki, st));
    int ncell = 0;
    E4CHK(hipMemcpyAsync(&ncell, (int*)B.misc + 2, sizeof(int), hipMemcpyDeviceToHost, st));
    E4CHK(hipStreamSynchronize(st));
    // cell runs and the rounds' work items (cell, first index, count): chunks of EAP4R_NT
    std::vector<int> cnt(ncell), runh(ncell + 1, 0);
    E4CHK(hipMemcpyAsync(cnt.data(), B.cnt, ncell * sizeof(int), hipMemcpyDeviceToHost, st));
    E4CHK(hipStreamSynchronize(st));
    std::vector<int4> work;
    work.reserve((size_t)ncell + (size_t)(K / EAP4R_NT) + 1);
    for (int c = 0; c < ncell; c++) {
        runh[c + 1] = runh[c] + cnt[c];
        for (int q = 0; q < cnt[c]; q += EAP4R_NT)
            work.push_back(make_int4(c, runh[c] + q, std::min(EAP4R_NT, cnt[c] - q), 0));
    }
    E4CHK(hipMemcpyAsync(B.run, runh.data(), (ncell + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    E4CHK(hipMemcpyAsync(B.work, work.data(), work.size() * sizeof(int4), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_eap_nb9, dim3((ncell + 255) / 256), dim3(256), 0, st, keyp, ncell, B.nb9);
    hipLaunchKernelGGL(k_eap4_cellrec, dim3(nb), dim3(256), 0, st, B.comp, K, B.ord, pos_by_cell, B.rec);
    E4CHK(hipMemsetAsync(B.state_t, 0xff, K * sizeof(int), st));  // -1: undecided
    // decision rounds until no position waits: the waiting is here, between launches
    // (each round decides at least the highest-priority undecided position)
    int nr = 1;
    for (;; nr++) {
        E4CHK(hipMemsetAsync((int*)B.misc + 3, 0, sizeof(int), st));
        hipLaunchKernelGGL(k_eap4_lfmis, dim3((unsigned)work.size()), dim3(EAP4R_NT), 0, st, B.work, B.rec, K, B.nb9,
                           B.run, T, B.state_t, (int*)B.misc + 3);
        E4CHK(hipGetLastError());
        int waiting = 0;
        E4CHK(hipMemcpyAsync(&waiting, (int*)B.misc + 3, sizeof(int), hipMemcpyDeviceToHost, st));
        E4CHK(hipStreamSynchronize(st));
        if (waiting == 0) break;
        if (nr > Ki) {
            err = "decision rounds did not converge";
            return -1;
        }
    }
    hipLaunchKernelGGL(k_eap_state_pos, dim3(nb), dim3(256), 0, st, B.state_t, pos_by_cell, K, B.state);
    // seeds' slots (priority order), members grouped by seed (stable: priority order within a group)
    int* flag = B.cnt;                           // (the cell counts are dead)
    unsigned int* skey = (unsigned int*)B.key;   // seed position of every position (the cells are dead)
    int* slot = (int*)B.key + K;                 // seed slot = seeds before it
    unsigned int* skey2 = (unsigned int*)B.key2;
    unsigned int* mem = pos_by_cell;             // positions grouped by seed, ascending within a group
    hipLaunchKernelGGL(k_eap_seedkey, dim3(nb), dim3(256), 0, st, B.state, K, flag, skey);
    tb = B.tmp_bytes;
    E4CHK(hipcub::DeviceScan::ExclusiveSum(B.tmp, tb, flag, slot, Ki, st));
    int last[2] = {0, 0};
    E4CHK(hipMemcpyAsync(&last[0], slot + (K - 1), sizeof(int), hipMemcpyDeviceToHost, st));
    E4CHK(hipMemcpyAsync(&last[1], flag + (K - 1), sizeof(int), hipMemcpyDeviceToHost, st));
    hipLaunchKernelGGL(k_iota_u32, dim3(nb), dim3(256), 0, st, B.i0, K);
    tb = B.tmp_bytes;
    E4CHK(hipcub::DeviceRadixSort::SortPairs(B.tmp, tb, skey, skey2, B.i0, mem, Ki, 0,
                                             eap4_bits_for((unsigned int)(K - 1)), st));
    E4CHK(hipStreamSynchronize(st));
    const int nout = last[0] + last[1];
    hipLaunchKernelGGL(k_eap_gstart, dim3(nb), dim3(256), 0, st, skey2, slot, K, nout, B.gstart);
    hipLaunchKernelGGL(k_eap4_sum, dim3(nout), dim3(64), 0, st, B.comp, K, B.ord, mem, B.gstart, B.out);
    E4CHK(hipGetLastError());
    *rounds = nr;
    *cells = ncell;
    return nout;
}

/* The reduce of a prepared SoA (B.comp: the single context's gather, or the
 * concatenated blocks of the sharded form — both callers come through here,
 * so Λ and the flag are one function of the same bytes): the bound pass, the
 * iota and the stable descending radix sort, then the decision rounds
 * (eap4_rounds), or k_eap4_merge's one workgroup when mode is 1, the flag is
 * set, or Λ or T is not finite and positive (the static map's one_group rule);
 * the copy out.  *rounds / *cells: the decision rounds and the occupied cells
 * (1, 0 for the one-workgroup form).  Returns the component count (nothing
 * copied when out is NULL or too small), -1 (err). */
static long eap4_reduce(hipStream_t st, const Eap4Bufs& B, long K, float T, int mode, phd_gaussian4d* out,
                        long out_cap, int* rounds, int* cells, std::string& err) {
    const unsigned int nb = (unsigned int)((K + 255) / 256);
    bool one_group = mode != 0 || !(T > 0.f) || !(T < INFINITY);
    float lam = 0.f;
    if (!one_group) {
        E4CHK(hipMemsetAsync(B.misc, 0, 8 * sizeof(unsigned int), st));
        hipLaunchKernelGGL(k_eap4_bound, dim3(nb), dim3(256), 0, st, B.comp, K, B.misc, (int*)B.misc + 1);
    }
    hipLaunchKernelGGL(k_eap4_iota, dim3(nb), dim3(256), 0, st, B.i0, K);
    size_t tb = B.tmp_bytes;
    E4CHK(hipcub::DeviceRadixSort::SortPairsDescending(B.tmp, tb, B.comp, B.wsorted, B.i0, B.ord, (int)K, 0, 32, st));
    if (!one_group) {
        unsigned int misc[2];
        E4CHK(hipMemcpyAsync(misc, B.misc, sizeof(misc), hipMemcpyDeviceToHost, st));
        E4CHK(hipStreamSynchronize(st));
        memcpy(&lam, &misc[0], 4);
        one_group = misc[1] != 0 || !(lam > 0.f) || !(lam < INFINITY);
    }
    int cnt = 0;
    if (one_group) {
        hipLaunchKernelGGL(k_eap4_merge, dim3(1), dim3(EAP4_NT), 0, st, B.comp, K, B.ord, T, B.flag, B.mem, B.out,
                           B.nout);
        E4CHK(hipGetLastError());
        E4CHK(hipMemcpyAsync(&cnt, B.nout, 4, hipMemcpyDeviceToHost, st));
        E4CHK(hipStreamSynchronize(st));
        *rounds = 1;
        *cells = 0;
    } else {
        const long n = eap4_rounds(st, B, K, lam, T, rounds, cells, err);
        if (n < 0) return -1;
        cnt = (int)n;
    }
    if (out && cnt <= out_cap) {
        E4CHK(hipMemcpyAsync(out, B.out, (size_t)cnt * sizeof(phd_gaussian4d), hipMemcpyDeviceToHost, st));
        E4CHK(hipStreamSynchronize(st));
    }
    return cnt;
}

long mixed_expected_map_dynamic(hipStream_t st, const int* d_src, const float* d_dmap, const int* d_dsize,
                                const float* d_dmap_x, const int* d_dsize_x, int n, int dcap, const float* d_logw, float T, phd_gaussian4d* out, long out_cap,
                                int mode, int* rounds, int* cells, std::string& err) {
    *rounds = *cells = 0;
    std::vector<int> off;
    const long K = eap4_offsets(st, d_src, d_dsize, d_dmap_x ? d_dsize_x : nullptr, n, dcap, off, err);
    if (K <= 0) return K;
    if (K >= (1L << 31) - 1) {
        err = "dynamic expected map: more than 2^31 components";
        return -1;
    }
    const size_t tmp = eap4_sort_tmp(K, st);
    const size_t head = ((size_t)(n + 1) * 4 + 255) & ~(size_t)255;
    char* buf = nullptr;
    E4CHK(hipMalloc((void**)&buf, head + eap4_carve(nullptr, K, tmp, nullptr)));
    int* d_off = (int*)buf;
    Eap4Bufs B;
    eap4_carve(buf + head, K, tmp, &B);
    long nout = -1;
    if (hipMemcpyAsync(d_off, off.data(), (n + 1) * 4, hipMemcpyHostToDevice, st) == hipSuccess) {
        hipLaunchKernelGGL(k_eap4_gather, dim3(n), dim3(256), 0, st, d_src, d_dmap, d_dmap_x, d_off, d_logw, dcap, K,
                           B.comp);
        nout = eap4_reduce(st, B, K, T, mode, out, out_cap, rounds, cells, err);
    } else {
        err = hipGetErrorString(hipGetLastError());
    }
    (void)hipStreamSynchronize(st);  // (an error path may leave work enqueued on buf)
    hipFree(buf);
    return nout;
}

/* ------------------------------------------------- the sharded form (blocks)
 * As for the static map (phd_eap.hip): every rank packs its weighted dynamic
 * components into a block ("EAP4": header | 21 fields of stride K_max,
 * include/phd_capi.h), the caller all-gathers the blocks in rank order, every
 * rank concatenates them into the SoA the single context of all the particles
 * gathers and runs the same reduce.  The scratch stays with the context. */
struct Eap4Scratch {
    char* buf = nullptr;  // the reduce's buffers (eap4_carve), grown on demand
    size_t bytes = 0;
    int* d_off = nullptr;    // pack: n + 1 offsets
    int* pin_off = nullptr;  // their pinned source (the pack does not wait for the upload)
    int off_n = 0;
    int* heads = nullptr;  // world + 1 offsets | EAP_HS_WORDS summary words
    int heads_world = 0;
    std::vector<int> off;
    ~Eap4Scratch() {
        if (buf) (void)hipFree(buf);
        if (d_off) (void)hipFree(d_off);
        if (pin_off) (void)hipHostFree(pin_off);
        if (heads) (void)hipFree(heads);
    }
};

void eap4_free(Eap4Scratch* s) { delete s; }

size_t eap4_block_bytes(long K_max) { return eap_block_bytes_of(PHD_DYN_FIELDS, K_max); }

long eap4_shard_count(hipStream_t st, const int* d_src, const int* d_dsize, const int* d_dsize_x, int n, int dcap,
                      std::string& err) {
    std::vector<int> off;
    return eap4_offsets(st, d_src, d_dsize, d_dsize_x, n, dcap, off, err);
}

int eap4_shard_pack(Eap4Scratch** sp, hipStream_t st, const int* d_src, const float* d_dmap, const int* d_dsize,
                    const float* d_dmap_x, const int* d_dsize_x, const float* d_logw, int n, int dcap, long K_max,
                    void* d_block, std::string& err) {
    if (!*sp) *sp = new Eap4Scratch();
    Eap4Scratch& S = **sp;
    const long K_r = eap4_offsets(st, d_src, d_dsize, d_dmap_x ? d_dsize_x : nullptr, n, dcap, S.off, err);
    if (K_r < 0) return -1;
    if (K_r > K_max) {
        err = "the store holds " + std::to_string(K_r) + " dynamic components, K_max is " + std::to_string(K_max);
        return -2;
    }
    // (the stream is idle since eap4_offsets' read-back: the previous pack's upload is consumed)
    if (S.off_n < n + 1) {
        if (S.d_off) (void)hipFree(S.d_off);
        if (S.pin_off) (void)hipHostFree(S.pin_off);
        S.d_off = S.pin_off = nullptr;
        S.off_n = 0;
        E4CHK(hipMalloc((void**)&S.d_off, (size_t)(n + 1) * sizeof(int)));
        E4CHK(hipHostMalloc((void**)&S.pin_off, (size_t)(n + 1) * sizeof(int), hipHostMallocDefault));
        S.off_n = n + 1;
    }
    memcpy(S.pin_off, S.off.data(), (size_t)(n + 1) * sizeof(int));
    E4CHK(hipMemcpyAsync(S.d_off, S.pin_off, (size_t)(n + 1) * sizeof(int), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_eap4_pack, dim3(n), dim3(256), 0, st, d_src, d_dmap, d_dmap_x, (const int*)S.d_off, d_logw,
                       dcap, n, (unsigned int)K_max, (unsigned int*)d_block);
    E4CHK(hipGetLastError());
    return 0;
}

long mixed_expected_map_dynamic_blocks(Eap4Scratch** sp, hipStream_t st, const void* d_blocks, int world, int n,
                                       long K_max, float T, phd_gaussian4d* out, long out_cap, int mode, int* rounds,
                                       int* cells, std::string& err) {
    *rounds = *cells = 0;
    if (!*sp) *sp = new Eap4Scratch();
    Eap4Scratch& S = **sp;
    if (S.heads_world < world) {
        if (S.heads) (void)hipFree(S.heads);
        S.heads = nullptr;
        S.heads_world = 0;
        E4CHK(hipMalloc((void**)&S.heads, (size_t)(world + 1 + EAP_HS_WORDS) * sizeof(int)));
        S.heads_world = world;
    }
    int* d_off = S.heads;
    unsigned int* d_sum = (unsigned int*)(S.heads + world + 1);
    const size_t stride_words = eap4_block_bytes(K_max) / 4;
    eap_launch_block_heads(st, d_blocks, stride_words, world, EAP4_BLOCK_LAYOUT, n, K_max, d_off, d_sum);
    unsigned int sum[EAP_HS_WORDS];
    E4CHK(hipMemcpyAsync(sum, d_sum, sizeof(sum), hipMemcpyDeviceToHost, st));
    E4CHK(hipStreamSynchronize(st));
    if (sum[EAP_HS_REFUSED] != 0xffffffffu) {
        err = eap_refused_text(sum[EAP_HS_REFUSED]);
        return -2;
    }
    const unsigned long long total = ((unsigned long long)sum[EAP_HS_TOTAL_HI] << 32) | sum[EAP_HS_TOTAL_LO];
    if (total == 0) return 0;
    if (total >= (1ull << 31) - 1) {
        err = "the blocks hold " + std::to_string(total) + " components, 2^31 - 1 or more";
        return -2;
    }
    const long K = (long)total;
    const size_t tmp = eap4_sort_tmp(K, st);
    const size_t need = eap4_carve(nullptr, K, tmp, nullptr);
    if (S.bytes < need) {
        if (S.buf) (void)hipFree(S.buf);
        S.buf = nullptr;
        S.bytes = 0;
        E4CHK(hipMalloc((void**)&S.buf, need));
        S.bytes = need;
    }
    Eap4Bufs B;
    eap4_carve(S.buf, K, tmp, &B);
    eap_launch_concat(st, d_blocks, stride_words, PHD_DYN_FIELDS, world, K_max, d_off, K, B.comp);
    E4CHK(hipGetLastError());
    return eap4_reduce(st, B, K, T, mode, out, out_cap, rounds, cells, err);
}

#undef E4CHK

}  // namespace phd
