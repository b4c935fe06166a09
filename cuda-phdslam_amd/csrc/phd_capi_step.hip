/*
 * phd_capi_step.hip — the filter step of the C-ABI: predict, normalise / nEff /
 * resample (one block, or chunked over workgroups), predict + update enqueued
 * as one, and phd_step, which follows its StepPlan (phd_step_plan.h).
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "phd_ctx.h"

using namespace phd;

#ifndef PHD_FUSE_PREDICT_ALL
#define PHD_FUSE_PREDICT_ALL 0 /* 1: CPHD part A runs the predict at any number of workgroup rounds */
#endif

int rs_parts(phd_ctx* ctx, int n, RsParts& P) {
    const int B = (n + RS_THREADS - 1) / RS_THREADS;
    if (B > RS_MAX_CHUNKS) return fail(PHD_E_ARG, "more than 2^20 log-weights in a chunked resample");
    const size_t need = (size_t)B * (sizeof(float) + 2 * sizeof(double) + 2 * sizeof(unsigned long long)) + 64 +
                        (size_t)n * sizeof(unsigned long long);
    if (ctx->rs.d_rsx.ensure(need)) return PHD_E_HIP;
    P.cdf_rel = (unsigned long long*)ctx->rs.d_rsx.get();
    P.part_sum = (double*)(P.cdf_rel + n);
    P.part_s2 = P.part_sum + B;
    P.part_tot = (unsigned long long*)(P.part_s2 + B);
    P.part_key = P.part_tot + B;
    P.part_max = (float*)(P.part_key + B);
    return PHD_OK;
}

/* the in-launch hand-off words of k_shard_plan / k_rs_step: zeroed once, every
 * launch leaves them zero */
int ensure_sync(phd_ctx* ctx) {
    if (!ctx->rs.d_sync) {
        if (ctx->rs.d_sync.alloc(64 / sizeof(unsigned))) return PHD_E_HIP;
        HIPCHK(hipMemsetAsync(ctx->rs.d_sync, 0, 64, ctx->stream));
    }
    return PHD_OK;
}

/* The arguments of k_rs_step, phd_step's one-launch resample over n <= 16
 * chunks: every block takes the max and all chunk sums itself, the normalised
 * weights go out of place to d_tmp_logw until the search moves them.  Launches
 * nothing (the hand-off words' first zeroing apart, on the context stream): the
 * caller does, on its stream, beside part C or in part C's lead workgroup. */
static int rs_step_args(phd_ctx* ctx, float* w, int n, float* out, uint64_t seed, uint64_t step, int* parents,
                        float new_logw, RsStepArgs& a) {
    RsParts P;
    int rc = rs_parts(ctx, n, P);
    if (rc) return rc;
    if (ensure_sync(ctx)) return PHD_E_HIP;
    a = RsStepArgs{};
    a.w = w;
    a.w_out = ctx->st.d_tmp_logw;
    a.N = n;
    a.B = (n + RS_THREADS - 1) / RS_THREADS;
    a.has_meas = ctx->z.M > 0 ? 1 : 0;
    a.resample_thresh = ctx->cfg.resampleThresh;
    a.new_logw = new_logw;
    a.seed = seed;
    a.step = step;
    a.part_s2 = P.part_s2;
    a.cdf_rel = P.cdf_rel;
    a.part_tot = P.part_tot;
    a.part_key = P.part_key;
    a.sync = ctx->rs.d_sync;
    a.out = out;
    a.parents = parents;
    a.pose = ctx->st.d_pose;
    a.src = ctx->st.d_src;
    a.new_pose = ctx->st.d_tmp_pose;
    a.new_src = ctx->st.d_tmp_src;
    a.logw = w;
    a.err = ctx->d_err;
    return PHD_OK;
}

/* Normalise + nEff + decision + stratified parents of n log-weights (in place)
 * on ceil(n/1024) workgroups of stream st: k_rs_max, k_rs_sum, k_rs_cdf,
 * k_rs_search (the multi-block form of k_normalize_resample, same results bit
 * for bit).  out: [0] lse, [1] nEff, [2] decision, [4] decisions counter;
 * parents written only when the decision is 1.  With `remap`, k_rs_search also
 * writes the remapped poses / slab references of its strata into the spare
 * arrays (the identity without a resample) and the new log-weight; with
 * `fused_max` too and up to 16 chunks it is one k_rs_step launch (<= 16
 * workgroups, always resident at once).  Stream-ordered, no host
 * synchronisation. */
int launch_rs_chunks(phd_ctx* ctx, hipStream_t st, float* w, int n, float* out, uint64_t seed, uint64_t step,
                     int* parents, bool remap, float new_logw, bool fused_max, unsigned* beyond) {
    const int B = (n + RS_THREADS - 1) / RS_THREADS;
    if (fused_max && remap && B <= 16) {
        RsStepArgs a;
        int rc = rs_step_args(ctx, w, n, out, seed, step, parents, new_logw, a);
        if (rc) return rc;
        hipLaunchKernelGGL(k_rs_step, dim3(B), dim3(RS_THREADS), 0, st, a);
        HIPCHK(hipGetLastError());
        return PHD_OK;
    }
    RsParts P;
    int rc = rs_parts(ctx, n, P);
    if (rc) return rc;
    hipLaunchKernelGGL(k_rs_max, dim3(B), dim3(RS_THREADS), 0, st, (const float*)w, n, P.part_max);
    hipLaunchKernelGGL(k_rs_sum, dim3(B), dim3(RS_THREADS), 0, st, (const float*)w, n, (const float*)P.part_max, B,
                       P.part_sum, 0);
    hipLaunchKernelGGL(k_rs_cdf, dim3(B), dim3(RS_THREADS), 0, st, w, n, (const float*)P.part_max,
                       (const double*)P.part_sum, B, P.part_s2, P.cdf_rel, P.part_tot, P.part_key, out);
    hipLaunchKernelGGL(k_rs_search, dim3(B), dim3(RS_THREADS), 0, st, n, B, (const double*)P.part_s2,
                       (const unsigned long long*)P.part_tot, (const unsigned long long*)P.part_key,
                       (const unsigned long long*)P.cdf_rel, ctx->cfg.resampleThresh, ctx->z.M > 0 ? 1 : 0, seed, step,
                       parents, out, remap ? (const phd_pose*)ctx->st.d_pose : nullptr, (const int*)ctx->st.d_src,
                       ctx->st.d_tmp_pose, ctx->st.d_tmp_src, w, new_logw, (const float*)nullptr, beyond);
    HIPCHK(hipGetLastError());
    return PHD_OK;
}

PredictCfg predict_cfg(const phd_slam_config& c, int index_offset) {
    PredictCfg p;
    p.index_offset = index_offset;
    p.dt = c.dt;
    p.subdivide = c.subdividePredict > 0 ? c.subdividePredict : 1;
    p.l = c.l;
    p.h = c.h;
    p.a = c.a;
    p.b = c.b;
    p.stdAlpha = c.stdAlpha;
    p.stdEncoder = c.stdEncoder;
    p.ax = c.ax;
    p.ay = c.ay;
    p.ayaw = c.ayaw;
    return p;
}

static int check_predict(phd_ctx* ctx) {
    if (!ctx) return fail(PHD_E_ARG, "null ctx");
    if (!ctx->cfg_set) return fail(PHD_E_ARG, "phd_set_config not called");
    if (ctx->cfg.nPredictParticles > 1 && ctx->st.replay)
        return fail(PHD_E_UNSUPPORTED, "n_predict_particles > 1 in replay mode");
    return set_device(ctx);
}

/* n_predict_particles > 1 (phdPredict, phdfilter.cu:1185-1238): every live
 * particle spawns npp children (pose, slab reference, weight - log npp) before
 * the predict kernel moves each child with its own noise draw.  The live count
 * grows by npp per predict, within capacity.max_particles. */
static int expand_particles(phd_ctx* ctx) {
    const int npp = ctx->cfg.nPredictParticles;
    if (npp <= 1) return PHD_OK;
    if ((long)ctx->n * npp > ctx->nmax)
        return fail(PHD_E_CAPACITY, "n_predict_particles: " + std::to_string((long)ctx->n * npp) +
                                        " live particles exceed capacity.max_particles (" +
                                        std::to_string(ctx->nmax) + ")");
    const int m = ctx->n * npp;
    const float log_npp = std::log((float)npp);  // safeLog(nPredictParticles) in float (phdfilter.cu:1214)
    hipLaunchKernelGGL(k_expand, dim3((m + 255) / 256), dim3(256), 0, ctx->stream, ctx->n, npp,
                       (const phd_pose*)ctx->st.d_pose, (const int*)ctx->st.d_src, (const float*)ctx->st.d_logw,
                       ctx->st.d_tmp_pose, ctx->st.d_tmp_src, ctx->st.d_tmp_logw, log_npp);
    HIPCHK(hipGetLastError());
    std::swap(ctx->st.d_pose, ctx->st.d_tmp_pose);
    std::swap(ctx->st.d_src, ctx->st.d_tmp_src);
    std::swap(ctx->st.d_logw, ctx->st.d_tmp_logw);
    ctx->st.src_fresh = false;  // (children reference their parent's slab)
    ctx->n = m;
    return PHD_OK;
}

/* the resample decision's mode argument: 0 no measurements, 1 measurements,
 * 2 forced — more than 5 x n_particles live particles (main.cpp:1286) */
int rs_mode(const phd_ctx* ctx) {
    if ((long)ctx->n > 5L * ctx->n_base) return 2;
    return ctx->z.M > 0 ? 1 : 0;
}

/* predictMapMixed (one phdPredict).  All particles: every slab of the dynamic
 * set, in -> out by slab id, and — while references may name it — every slab
 * of the dynamic set X in place; a slab that several particles share (copy on
 * write after a resample, several slots of one record) is a slab still, so it
 * advances once.  Slots (a sharded step's pending slots, whose records came
 * after this step's predict was enqueued): the slabs of set X they name, once
 * each (mixed_launch_predict_x); the current set stays where it is. */
static int launch_predict_dynamic(phd_ctx* ctx, const int* slots = nullptr, int count = 0) {
    if (!ctx->mx.on) return fail(PHD_E_ARG, "feature_model 2 needs phd_enable_dynamic");
    const phd_mx_cfg mc = phd_mx_config(&ctx->cfg);
    if (slots) {
        if (ctx->mx.d_dmap_x)
            HIPCHK(mixed_launch_predict_x(slots, count, ctx->st.d_src, ctx->mx.dcap, ctx->mx.d_dmap_x, ctx->mx.d_dsize_x,
                                          mc, ctx->stream));
        return PHD_OK;
    }
    const int din = ctx->mx.dcur, dout = din ^ 1;
    HIPCHK(mixed_launch_predict(ctx->nmax, ctx->mx.dcap, ctx->mx.d_dmap[din], ctx->mx.d_dsize[din], ctx->mx.d_dmap[dout],
                                ctx->mx.d_dsize[dout], mc, ctx->stream));
    if (ctx->mx.x_live)
        HIPCHK(mixed_launch_predict_x(nullptr, (int)(ctx->mx.d_dsize_x.bytes() / sizeof(int)), nullptr, ctx->mx.dcap,
                                      ctx->mx.d_dmap_x, ctx->mx.d_dsize_x, mc, ctx->stream));
    ctx->mx.dcur = dout;
    return PHD_OK;
}

/* predict of all particles, or of `count` slots listed on the device */
static int launch_predict(phd_ctx* ctx, phd_ackerman_control u, const void* noise, uint64_t step,
                          const int* slots, int count) {
    if (count <= 0) return PHD_OK;
    if (ctx->cfg.featureModel == PHD_FEATURE_MIXED) {  // predictMapMixed with every phdPredict (phdfilter.cu:1241-1242)
        int rc = launch_predict_dynamic(ctx, slots, count);
        if (rc) return rc;
    }
    const PredictCfg pc = predict_cfg(ctx->cfg, ctx->index_offset);
    const phd_pose* pp = ctx->st.replay ? ctx->st.d_pose_prior : nullptr;
    const float* lp = ctx->st.replay ? ctx->st.d_logw_prior : nullptr;
    if (ctx->cfg.motionType == PHD_MOTION_ACKERMAN)
        hipLaunchKernelGGL(k_predict_ackerman, dim3((count + 255) / 256), dim3(256), 0, ctx->stream, ctx->st.d_pose,
                           count, u, (const phd_ackerman_noise*)noise, pc, ctx->seed, step, pp, lp, ctx->st.d_logw, slots);
    else
        hipLaunchKernelGGL(k_predict_cv, dim3((count + 255) / 256), dim3(256), 0, ctx->stream, ctx->st.d_pose, count,
                           (const phd_cv_noise*)noise, pc, ctx->seed, step, pp, lp, ctx->st.d_logw, slots);
    HIPCHK(hipGetLastError());
    return PHD_OK;
}

extern "C" {

int phd_predict_dynamic(phd_ctx* ctx) {
    if (!ctx) return fail(PHD_E_ARG, "null ctx");
    if (!ctx->cfg_set) return fail(PHD_E_ARG, "phd_set_config not called");
    if (set_device(ctx)) return PHD_E_HIP;
    return launch_predict_dynamic(ctx);
}

int phd_predict_ackerman(phd_ctx* ctx, phd_ackerman_control u, const phd_ackerman_noise* noise, uint64_t step) {
    int rc = check_predict(ctx);
    if (rc) return rc;
    if (ctx->cfg.motionType != PHD_MOTION_ACKERMAN) return fail(PHD_E_ARG, "motion_type is not Ackerman");
    rc = expand_particles(ctx);
    if (rc) return rc;
    const int n = ctx->n;  // (noise: one entry per live particle after the expansion)
    const phd_ackerman_noise* dn = nullptr;
    if (noise) {
        HIPCHK(hipMemcpyAsync(ctx->d_noise_a, noise, n * sizeof(phd_ackerman_noise), hipMemcpyHostToDevice,
                              ctx->stream));
        dn = ctx->d_noise_a;
    }
    return launch_predict(ctx, u, dn, step, nullptr, n);
}

int phd_predict_cv(phd_ctx* ctx, const phd_cv_noise* noise, uint64_t step) {
    int rc = check_predict(ctx);
    if (rc) return rc;
    if (ctx->cfg.motionType == PHD_MOTION_ACKERMAN) return fail(PHD_E_ARG, "motion_type is Ackerman, not CV");
    rc = expand_particles(ctx);
    if (rc) return rc;
    const int n = ctx->n;  // (noise: one entry per live particle after the expansion)
    const phd_cv_noise* dn = nullptr;
    if (noise) {
        HIPCHK(hipMemcpyAsync(ctx->d_noise_cv, noise, n * sizeof(phd_cv_noise), hipMemcpyHostToDevice, ctx->stream));
        dn = ctx->d_noise_cv;
    }
    return launch_predict(ctx, phd_ackerman_control{0.f, 0.f}, dn, step, nullptr, n);
}

int phd_normalize(phd_ctx* ctx, const float* lse_override) {
    if (!ctx) return fail(PHD_E_ARG, "null ctx");
    if (set_device(ctx)) return PHD_E_HIP;
    const float* d_ov = nullptr;
    if (lse_override) {
        HIPCHK(hipMemcpyAsync(ctx->d_out + 8, lse_override, sizeof(float), hipMemcpyHostToDevice, ctx->stream));
        d_ov = ctx->d_out + 8;
    }
    hipLaunchKernelGGL(k_normalize, dim3(1), dim3(1024), 0, ctx->stream, ctx->st.d_logw, ctx->n, d_ov, ctx->d_out,
                       ctx->cfg.resampleThresh, rs_mode(ctx));
    HIPCHK(hipGetLastError());
    if (lse_override) HIPCHK(hipStreamSynchronize(ctx->stream));
    return PHD_OK;
}

int phd_neff(phd_ctx* ctx, float* neff) {
    if (!ctx || !neff) return fail(PHD_E_ARG, "null argument");
    if (set_device(ctx)) return PHD_E_HIP;
    float out[2];
    HIPCHK(hipMemcpyAsync(out, ctx->d_out, 2 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    *neff = out[1];
    return PHD_OK;
}

}  // extern "C"

/* dynamic LDS of the resample kernels: the CDF when it fits (RS_LDS_MAX) */
size_t rs_lds(int n) { return n <= RS_LDS_MAX ? (size_t)n * sizeof(unsigned long long) : 0; }

/* resample the live particles into n_particles (main.cpp:1289, resampleParticles(particles, n_particles)) */
static int launch_resample(phd_ctx* ctx, const int* d_flag, const double* du, uint64_t step) {
    const float neglogn = (float)(-std::log((double)ctx->n_base));  // slamtypes.h:328
    ctx->st.src_fresh = false;  // (the resample remaps the slab references)
    hipLaunchKernelGGL(k_resample, dim3(1), dim3(1024), rs_lds(ctx->n), ctx->stream, d_flag, ctx->st.d_logw, ctx->st.d_logw,
                       ctx->n, ctx->n_base, du, ctx->seed, step, ctx->rs.d_cdf, ctx->rs.d_idx, ctx->st.d_pose, ctx->st.d_src,
                       ctx->st.d_tmp_pose, ctx->st.d_tmp_src, neglogn);
    HIPCHK(hipGetLastError());
    return PHD_OK;
}

extern "C" {

int phd_resample(phd_ctx* ctx, const double* u_host, uint64_t step, int* idx_host) {
    if (!ctx) return fail(PHD_E_ARG, "null ctx");
    if (set_device(ctx)) return PHD_E_HIP;
    const double* du = nullptr;
    if (u_host) {
        HIPCHK(hipMemcpyAsync(ctx->rs.d_u, u_host, ctx->n_base * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        du = ctx->rs.d_u;
    }
    int rc = launch_resample(ctx, nullptr, du, step);
    if (rc) return rc;
    ctx->n = ctx->n_base;
    if (idx_host) {
        HIPCHK(hipMemcpyAsync(idx_host, ctx->rs.d_idx, ctx->n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (u_host || idx_host) HIPCHK(hipStreamSynchronize(ctx->stream));
    return PHD_OK;
}

int phd_apply_resample(phd_ctx* ctx, const int* dev_idx, float new_log_weight) {
    if (!ctx || !dev_idx) return fail(PHD_E_ARG, "null argument");
    if (set_device(ctx)) return PHD_E_HIP;
    ctx->st.src_fresh = false;
    hipLaunchKernelGGL(k_apply_parents, dim3(1), dim3(1024), 0, ctx->stream, (const int*)nullptr, dev_idx, ctx->n,
                       ctx->st.d_pose, ctx->st.d_src,
                       ctx->st.d_logw, ctx->st.d_tmp_pose, ctx->st.d_tmp_src, new_log_weight);
    HIPCHK(hipGetLastError());
    return PHD_OK;
}

}  // extern "C"

/* predict (fused into the update when it pays) + update: the part of a step
 * before the cross-particle normalisation.  rs / done: launch_update's. */
int enqueue_predict_update(phd_ctx* ctx, const phd_ackerman_control* u, int do_predict, uint64_t step,
                           const int* slots, int nslots, const RsBeside* rs, UpdateDone* done) {
    const phd_slam_config& cfg = ctx->cfg;
    int rc;
    const int count = slots ? nslots : ctx->n;
    FusedPredict fp;
    // predict fused into the update launch when every particle's workgroup is
    // resident at once (saves a launch); with several rounds of workgroups the
    // serial per-particle predict would sit on each round's critical path
    const bool fuse =
        do_predict && ctx->z.M > 0 && cfg.nPredictParticles == 1 && cfg.featureModel == PHD_FEATURE_STATIC &&
        (ctx->n <= ctx->upd.resident_p || (PHD_FUSE_PREDICT_ALL && cfg.filterType == PHD_FILTER_CPHD)) &&
        ctx->upd.threads <= 512 && (cfg.filterType == PHD_FILTER_CPHD || !ctx->upd.split);
    if (fuse) {
        fp.predict = cfg.motionType == PHD_MOTION_ACKERMAN ? 1 : 2;
        if (fp.predict == 1 && !u) return fail(PHD_E_ARG, "Ackerman predict needs a control");
        fp.u = u ? *u : phd_ackerman_control{0.f, 0.f};
        fp.step = step;
    } else if (do_predict) {
        rc = check_predict(ctx);
        if (rc) return rc;
        const int sub = cfg.subdividePredict > 0 ? cfg.subdividePredict : 1;
        if (cfg.motionType == PHD_MOTION_ACKERMAN && !u) return fail(PHD_E_ARG, "Ackerman predict needs a control");
        if (cfg.nPredictParticles > 1 && slots) return fail(PHD_E_UNSUPPORTED, "n_predict_particles > 1 on slots");
        for (int k = 0; k < sub; k++) {  // (main.cpp:1248-1254: subdividePredict calls of phdPredict)
            const uint64_t s = step * (uint64_t)sub + (uint64_t)k;
            rc = expand_particles(ctx);
            if (rc) return rc;
            rc = launch_predict(ctx, u ? *u : phd_ackerman_control{0.f, 0.f}, nullptr, s, slots,
                                slots ? count : ctx->n);
            if (rc) return rc;
        }
    }
    // the step's births are placed by the update's classify from the predicted
    // pose (also when the predict is fused into the update)
    if (step_births_on(ctx) && cfg.featureModel == PHD_FEATURE_STATIC) {
        rc = launch_step_births(ctx, slots, slots ? count : ctx->n);
        if (rc) return rc;
    }
    if (ctx->z.M > 0) return launch_update(ctx, fuse ? &fp : nullptr, slots, nslots, rs, done);
    return PHD_OK;
}

extern "C" {

int phd_predict_update(phd_ctx* ctx, const phd_ackerman_control* u, int do_predict, uint64_t step,
                       float* dev_logw_out) {
    if (!ctx) return fail(PHD_E_ARG, "null ctx");
    if (!ctx->cfg_set) return fail(PHD_E_ARG, "phd_set_config not called");
    if (set_device(ctx)) return PHD_E_HIP;
    // the update writes each new log-weight to dev_logw_out as well (no copy
    // launch), when every particle is updated by the static-model kernels
    const bool mirror = dev_logw_out && ctx->z.M > 0 && ctx->cfg.featureModel == PHD_FEATURE_STATIC &&
                        ctx->cfg.nPredictParticles <= 1 && ctx->n == ctx->n_base;
    ctx->logw_mirror = mirror ? dev_logw_out : nullptr;
    UpdateDone done;
    int rc = enqueue_predict_update(ctx, u, do_predict, step, nullptr, 0, nullptr, &done);
    ctx->logw_mirror = nullptr;
    if (rc) return rc;
    if (dev_logw_out && !mirror)
        HIPCHK(hipMemcpyAsync(dev_logw_out, ctx->st.d_logw, ctx->n * sizeof(float), hipMemcpyDeviceToDevice,
                              ctx->stream));
    // phd_wait_logw promises the mirror complete: when no update marked the
    // log-weights final this call (an empty scan: no update at all) or the
    // mirror is a copy, mark them after it
    if (ctx->sh.ev_logw && (!done.logw_final || (dev_logw_out && !mirror)))
        HIPCHK(hipEventRecord(ctx->sh.ev_logw, ctx->stream));
    return PHD_OK;
}

}  // extern "C"

/* the end of a phd_step: the update's error check, then nEff and the decision
 * to the host when asked for */
static int step_read_back(phd_ctx* ctx, float* neff_out, int* resampled) {
    if (ctx->z.M > 0 && ctx->check_each_update) {
        int rc = check_err(ctx);
        if (rc) return rc;
    }
    if (!neff_out && !resampled) return PHD_OK;
    float out[3];
    HIPCHK(hipMemcpyAsync(out, ctx->d_out, 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    int f;
    memcpy(&f, &out[2], sizeof(int));
    if (neff_out) *neff_out = out[1];
    if (resampled) *resampled = f;
    return PHD_OK;
}

static_assert(kRsChunk == RS_THREADS, "phd_step_plan.h: the chunk of the resample kernels");

extern "C" {

int phd_step(phd_ctx* ctx, const phd_ackerman_control* u, int do_predict, uint64_t step, float* neff_out,
             int* resampled) {
    if (!ctx) return fail(PHD_E_ARG, "null ctx");
    if (!ctx->cfg_set) return fail(PHD_E_ARG, "phd_set_config not called");
    if (set_device(ctx)) return PHD_E_HIP;
    const phd_slam_config& cfg = ctx->cfg;
    const bool traced = ctx->tr.cap > 0;
    if (traced) {
        int rc0 = trace_supported(ctx, TRACE_STEP);
        if (rc0) return rc0;
    }
    // the step's resample form, decided before anything is enqueued
    StepFacts facts{};
    facts.n = ctx->n;
    facts.n_base = ctx->n_base;
    facts.n_predict_particles = cfg.nPredictParticles;
    facts.M = ctx->z.M;
    facts.filter_type = cfg.filterType;
    facts.feature_model = cfg.featureModel;
    facts.upd_split = ctx->upd.split;
    facts.upd_resident = ctx->upd.resident;
    facts.upd_lds = ctx->upd.lds;
    facts.rs_step_lds = rs_step_lds(ctx->upd.threads);
    facts.traced = traced;
    facts.stamps = ctx->d_stamps != nullptr;
#ifdef PHD_STAMP_PART_A
    facts.stamps = false;  // (that diagnostic build records part A: part C carries no stamps)
#endif
    facts.overlap_bits = PHD_RS_OVERLAP;
    facts.lead_on = PHD_RS_LEAD;
    const StepPlan plan = plan_step(facts);
    // normalise + nEff + device-side resample decision + resample (main.cpp:1281-1297)
    const float neglogn = (float)(-std::log((double)ctx->n));
    RsBeside rs{plan.form, {}};
    const bool with_update = plan.form == PHD_RS_FORM_LEAD || plan.form == PHD_RS_FORM_BESIDE;
    if (with_update) {  // the update launches it with part C
        if (!ctx->rs.aux) {  // (the auxiliary stream and its events: used by PHD_RS_FORM_BESIDE)
            int lo = 0, hi = 0;
            HIPCHK(hipDeviceGetStreamPriorityRange(&lo, &hi));
            if (ctx->rs.aux.create(hipStreamNonBlocking, &hi) || ctx->rs.ev_terms.create(kEvOrder) ||
                ctx->rs.ev_rs.create(kEvOrder))
                return PHD_E_HIP;
        }
        int rc0 = rs_step_args(ctx, ctx->st.d_logw, ctx->n, ctx->d_out, ctx->seed, step, ctx->rs.d_idx, neglogn, rs.a);
        if (rc0) return rc0;
        rs.a.src = nullptr;  // the update resets the slab references to the identity
    }
    UpdateDone done;
    int rc = enqueue_predict_update(ctx, u, do_predict, step, nullptr, 0, with_update ? &rs : nullptr, &done);
    if (rc) {
        // the resample may already run on the auxiliary stream (it writes the
        // log-weights, the parents and the spare pose / slab arrays): order
        // everything the caller enqueues next after it
        if (done.rs_beside) hipStreamWaitEvent(ctx->stream, ctx->rs.ev_rs, 0);
        return rc;
    }
    if (traced) {
        rc = trace_append(ctx, step);
        if (rc) return rc;
    }
    ctx->rs_form = plan.form;
    switch (plan.form) {
        case PHD_RS_FORM_SEPARATE: {
            hipLaunchKernelGGL(k_normalize, dim3(1), dim3(1024), 0, ctx->stream, ctx->st.d_logw, ctx->n,
                               (const float*)nullptr, ctx->d_out, cfg.resampleThresh, rs_mode(ctx));
            HIPCHK(hipGetLastError());
            rc = launch_resample(ctx, (const int*)(ctx->d_out + 2), nullptr, step);
            if (rc) return rc;
            int f = 0;
            rc = step_read_back(ctx, neff_out, &f);  // (the next step's launches depend on the decision)
            if (rc) return rc;
            if (f) ctx->n = ctx->n_base;
            if (resampled) *resampled = f;
            return PHD_OK;
        }
        case PHD_RS_FORM_BLOCK:
            hipLaunchKernelGGL(k_normalize_resample, dim3(1), dim3(1024), rs_lds(ctx->n), ctx->stream, ctx->st.d_logw,
                               ctx->n, ctx->d_out, cfg.resampleThresh, ctx->z.M > 0 ? 1 : 0, ctx->seed, step,
                               ctx->rs.d_cdf, ctx->rs.d_idx, ctx->st.d_pose, ctx->st.d_src, ctx->st.d_tmp_pose, ctx->st.d_tmp_src,
                               neglogn);
            HIPCHK(hipGetLastError());
            return step_read_back(ctx, neff_out, resampled);
        case PHD_RS_FORM_BESIDE:  // (ran beside part C)
            HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->rs.ev_rs, 0));
            break;
        case PHD_RS_FORM_LEAD:  // (in the lead workgroup: ordered by the stream itself, no event to wait on)
            break;
        default:  // PHD_RS_FORM_STEP / _CHUNKS: chunked over n/1024 workgroups of the context stream
            rc = launch_rs_chunks(ctx, ctx->stream, ctx->st.d_logw, ctx->n, ctx->d_out, ctx->seed, step, ctx->rs.d_idx, true,
                                  neglogn, plan.fuse_max);
            if (rc) return rc;
    }
    // the chunked forms' search wrote the remap into the spare arrays
    std::swap(ctx->st.d_pose, ctx->st.d_tmp_pose);  // identity copy when no resample was decided
    std::swap(ctx->st.d_src, ctx->st.d_tmp_src);
    ctx->st.src_fresh = false;  // (a remap, when the device decided to resample)
    return step_read_back(ctx, neff_out, resampled);
}

int phd_resample_count(phd_ctx* ctx, int* count) {
    if (!ctx || !count) return fail(PHD_E_ARG, "null argument");
    if (set_device(ctx)) return PHD_E_HIP;
    unsigned c[2];
    HIPCHK(hipMemcpyAsync(&c[0], ctx->d_out + 4, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(&c[1], ctx->d_out + 44, sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    *count = (int)(c[0] + c[1]);
    return PHD_OK;
}

int phd_last_resample_form(phd_ctx* ctx, int* form) {
    if (!ctx || !form) return fail(PHD_E_ARG, "null argument");
    *form = ctx->rs_form;
    return PHD_OK;
}

}  // extern "C"
