/*
 * phd_capi_update.hip — the update of the C-ABI: which kernel, how its launch
 * is sized (occupancy model), the launches themselves (static and mixed model),
 * the step's births, the per-update timing events, phd_update.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "phd_ctx.h"

using namespace phd;

#ifndef PHD_TIMING_EVENTS
#define PHD_TIMING_EVENTS 1 /* 0: a diagnostic build that never records the update timing events */
#endif

/* CPHD cardinality coefficients (allocated with the first CPHD use): one row
 * per slab, written by the update of the particle whose posterior slab it is. */
int ensure_cn(phd_ctx* c) {
    if (!(c->cfg_set && c->cfg.filterType == PHD_FILTER_CPHD)) return PHD_OK;
    return c->cn.d_coef.ensure((size_t)c->nmax * c->cn.stride);
}

/* cardinality doubles carried by a migration record (0 unless CPHD) */
int rec_cn_stride(const phd_ctx* c) {
    return (c->cfg_set && c->cfg.filterType == PHD_FILTER_CPHD) ? c->cn.stride : 0;
}

/* The workgroup update kernel of nt threads: part 0 the fused PHD update,
 * 1 / 2 part A / part C of the split update (CPHD: always split, with
 * k_cphd_terms between the parts; PHD: split when it pays, update_form).
 * predict: the launch that also runs the particle's predict (the fused PHD
 * update, CPHD's part A; up to 512 threads).  NULL: no such kernel. */
const void* update_kernel(int nt, int cphd, int part, int metric, int predict) {
    const int ti = nt == 256 ? 0 : nt == 512 ? 1 : 2;
    if (predict) {
        if (ti == 2) return nullptr;
        const void* p[3][2] = {{(const void*)k_update_fused_p256, (const void*)k_update_fused_p512},
                               {(const void*)k_update_fused_p256_h, (const void*)k_update_fused_p512_h},
                               {(const void*)k_update_cphd_a_p256, (const void*)k_update_cphd_a_p512}};
        return cphd ? (part == 1 ? p[2][ti] : nullptr) : (part == 0 ? p[metric == 1 ? 1 : 0][ti] : nullptr);
    }
    if (metric == 1 && part != 1) {  // the launches that hold the merge (parts A have none)
        const void* h[3][3] = {
            {(const void*)k_update_fused_256_h, (const void*)k_update_fused_512_h, (const void*)k_update_fused_1024_h},
            {(const void*)k_update_phd_c_256_h, (const void*)k_update_phd_c_512_h, (const void*)k_update_phd_c_1024_h},
            {(const void*)k_update_cphd_c_256_h, (const void*)k_update_cphd_c_512_h,
             (const void*)k_update_cphd_c_1024_h}};
        return cphd ? (part == 2 ? h[2][ti] : nullptr) : h[part == 2 ? 1 : 0][ti];
    }
    const void* k[2][3][3] = {
        {{(const void*)k_update_fused_256, (const void*)k_update_fused_512, (const void*)k_update_fused_1024},
         {(const void*)k_update_phd_a_256, (const void*)k_update_phd_a_512, (const void*)k_update_phd_a_1024},
         {(const void*)k_update_phd_c_256, (const void*)k_update_phd_c_512, (const void*)k_update_phd_c_1024}},
        {{nullptr, nullptr, nullptr},
         {(const void*)k_update_cphd_a_256, (const void*)k_update_cphd_a_512, (const void*)k_update_cphd_a_1024},
         {(const void*)k_update_cphd_c_256, (const void*)k_update_cphd_c_512, (const void*)k_update_cphd_c_1024}}};
    return k[cphd ? 1 : 0][part][ti];
}

/* LDS allocation granularity per workgroup (bytes) of the occupancy model:
 * measured on gfx950 (part C's residency timeline, stamps builds, 256 CUs): a
 * 27 120 B workgroup holds a CU to 5 (1 280 resident), a 26 864 B one to 6
 * (1 536) — consistent with 1 280-byte granules of the 160 KiB, not with the
 * 128 B this model assumed before round 5 (which had grown config 3's and 4's
 * edge pools to 27 248 B: 5 per CU, not the 6 the bench line reported) */
#ifndef PHD_LDS_GRAN
#define PHD_LDS_GRAN 1280
#endif
/* workgroups per CU of `kernel` with `lds` bytes: the LDS bound (160 KiB /
 * the layout) within the VGPR bound; hipOccupancyMaxActiveBlocksPerMultiprocessor
 * under-reports the LDS bound here (it gave 5 where 6 workgroups of 27 KB run) */
static int blocks_per_cu(const void* kernel, int nt, size_t lds) {
    int vblocks = 0;  // the VGPR / wave bound alone: the runtime's answer without LDS
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&vblocks, kernel, nt, 0) != hipSuccess || vblocks <= 0)
        vblocks = 32 / (nt / 64);
    const size_t g = PHD_LDS_GRAN;
    return (int)std::min<long>((160 * 1024) / (long)((lds + g - 1) / g * g), vblocks);
}

/* Threads per particle for the fused update.  The kernel is latency-bound, so
 * the step time is about (rounds of resident workgroups) x (per-workgroup
 * latency): residency from hipOccupancyMaxActiveBlocksPerMultiprocessor (LDS
 * layout, VGPRs, allocation granularity), relative latency measured at
 * config 3 (256 threads 1.25, 512 threads 1.0, 1024 threads ~0.85).
 * Returns the configuration by value (the requests carried over from the
 * context's): threads == 0 when none fits (the last error says why, code
 * PHD_E_CAPACITY).  The context is not written. */
static UpdLaunch configure_update_launch(const phd_ctx* c, int req) {
    const phd_capacity& cap = c->cap;
    const int cphd = c->cfg_set && c->cfg.filterType == PHD_FILTER_CPHD ? 1 : 0;
    // the kernels that hold the merge differ by metric (registers, hence residency)
    const int metric = c->cfg_set && c->cfg.distanceMetric == 1 ? 1 : 0;
    int ncu = 0;
    hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, c->device);
    if (ncu <= 0) ncu = 1;
    int best = 0, best_blocks = 0, best_split = 0;
    double best_cost = 1e300;
    size_t best_lds = 0;
    int best_ep = c->upd.epool;
    // forms: the fused PHD update (one launch), or split into part A and part C
    // (CPHD always: its terms sit between the parts)
    for (int split = cphd ? 1 : 0; split <= 1; split++) {
        if (!cphd && c->upd.form_req && split != c->upd.form_req - 1) continue;
        for (int nt = UPD_THREADS_MIN; nt <= UPD_THREADS_MAX; nt *= 2) {
            const int pc = split ? 2 : 0;  // the launch whose layout holds the merge
            // edge pool: the minimal one, grown while the workgroups per CU stay the same
            auto lds_of = [&](int e) {
                return upd_lds_layout(cap.map_capacity, cap.max_measurements, cap.candidate_capacity,
                                      cap.survivor_capacity, e, nt, cphd, pc)
                    .total;
            };
            const void* kc = update_kernel(nt, cphd, pc, metric);
            // minimal edge pool: one edge per candidate (+16 for CPHD): the births
            // join the detected landmarks' clusters — config 4's shard overflowed a
            // pool of K / 2 + 32 in 48 % of its particle-updates (serial greedy), and
            // config 3 with the step's births has up to 795 edges of 807 candidates
            // (K = 832: a pool of 800 fell back to the serial greedy in 3 of 1.2 M
            // particle-updates, 848 in none)
            int ep = c->upd.epool_req > 0 ? c->upd.epool_req : cap.candidate_capacity + (cphd ? 16 : 0);
            const size_t l0 = lds_of(ep);
            if (l0 > 160 * 1024) continue;
            const int b0 = blocks_per_cu(kc, nt, l0);
            while (!c->upd.epool_req && ep + 16 <= upd_epool(cap.candidate_capacity) &&
                   blocks_per_cu(kc, nt, lds_of(ep + 16)) >= b0)
                ep += 16;
            const size_t lds = lds_of(ep);
            const int blocks = blocks_per_cu(kc, nt, lds);
            if (blocks < 1) continue;
            // per-workgroup latency relative to 512 threads (config 3 measurements:
            // 256 threads 1.25, 512 1.0, 1024 ~0.85); part A ~0.4 and part C ~0.6
            // of the whole update (config 3: A 66 us, C 160 us minus the CPHD-only work)
            const double lat = nt == 256 ? 1.25 : nt == 512 ? 1.0 : 0.85;
            const long resident = (long)blocks * ncu;
            double cost = (double)((c->n + resident - 1) / resident) * lat;
            if (split) {
                const size_t la = upd_lds_layout(cap.map_capacity, cap.max_measurements, cap.candidate_capacity,
                                                 cap.survivor_capacity, ep, nt, cphd, 1)
                                      .total;
                const int ba = blocks_per_cu(update_kernel(nt, cphd, 1), nt, la);
                if (ba < 1) continue;
                const long ra = (long)ba * ncu;
                cost = 0.6 * cost + 0.4 * (double)((c->n + ra - 1) / ra) * lat;
            }
            if (req ? (nt == req && (best == 0 || cost < best_cost)) : cost < best_cost) {
                best = nt;
                best_cost = cost;
                best_blocks = blocks;
                best_lds = lds;
                best_ep = ep;
                best_split = split;
            }
        }
    }
    if (!best) {
        const size_t need = upd_lds_layout(cap.map_capacity, cap.max_measurements, cap.candidate_capacity,
                                           cap.survivor_capacity, c->upd.epool, UPD_THREADS_MIN, cphd, cphd ? 2 : 0)
                                .total;
        fail(PHD_E_CAPACITY, "capacities need " + std::to_string(need) + " B of LDS (> 160 KiB)");
        UpdLaunch none;
        none.threads = 0;
        return none;
    }
    UpdLaunch L = c->upd;
    L.threads = best;
    L.cphd = cphd;
    L.metric = metric;
    L.split = best_split;
    L.threads_req = req;
    L.lds = best_lds;
    L.lds_a = best_split ? upd_lds_layout(cap.map_capacity, cap.max_measurements, cap.candidate_capacity,
                                               cap.survivor_capacity, best_ep, best, cphd, 1)
                                    .total
                              : 0;
    L.epool = best_ep;
    L.resident = best_blocks * ncu;
    L.resident_a = best_split ? blocks_per_cu(update_kernel(best, cphd, 1), best, L.lds_a) * ncu : 0;
    // the fused-predict forms (CPHD: part A; PHD: the fused update) carry the
    // predict's registers: phd_step fuses the predict only when every particle's
    // workgroup of THAT launch is resident at once
    const void* kp = update_kernel(best, cphd, best_split ? 1 : 0, metric, 1);  // (none: split PHD, 1024 threads)
    L.resident_p = kp ? blocks_per_cu(kp, best, best_split ? L.lds_a : L.lds) * ncu : 0;
    return L;
}

int apply_update_launch(phd_ctx* c, int threads_req) {
    UpdLaunch L = configure_update_launch(c, threads_req);
    if (!L.threads) return PHD_E_CAPACITY;
    c->upd = std::move(L);
    return PHD_OK;
}

static DevCfg dev_cfg(const phd_slam_config& c) {
    DevCfg d;
    d.minRange = c.minRange;
    d.maxRange = c.maxRange;
    d.maxBearing = c.maxBearing;
    d.stdRange = c.stdRange;
    d.stdBearing = c.stdBearing;
    d.pd = c.pd;
    d.kappa = c.clutterDensity;
    d.birthWeight = c.birthWeight;
    d.birthNoiseFactor = c.birthNoiseFactor;
    d.minFeatureWeight = c.minFeatureWeight;
    d.minSeparation = c.minSeparation;
    d.log_birth = c.birthWeight <= 0 ? -FLT_MAX : phd_det_logf(c.birthWeight);  // (D17: the oracle's bits)
    d.log_2pi = (double)std::log((float)(2 * M_PI));
    const double kb = (double)c.clutterDensity + (double)c.birthWeight;
    if (c.minFeatureWeight > 0 && kb > 0)
        d.lq_keep_thresh = (float)(std::log((double)c.minFeatureWeight) + std::log(kb) - 0.5);
    else
        d.lq_keep_thresh = -INFINITY;
    d.labeled = c.labeledMeasurements ? 1 : 0;
    d.cphd_rate = (double)c.clutterRate;
    d.cphd_lrate = c.clutterRate > 0 ? std::log((double)c.clutterRate) : -INFINITY;
    d.cphd_lck = d.cphd_lrate - std::log((double)c.clutterDensity);
    d.cphd_log1mpd = 1 - c.pd <= 0 ? -FLT_MAX : std::log(1 - c.pd);
    d.log_minfw = c.minFeatureWeight > 0 ? std::log(c.minFeatureWeight) : -INFINITY;
    d.cphd_thr0 = (float)((std::log((double)c.minFeatureWeight) + std::log((double)c.clutterDensity) - 2.5) *
                          1.4426950408889634);
    d.cphd_leta_min = (float)(std::log((double)c.clutterDensity) - 2.0);
    {
        // PHD: η_m >= κ + β, so a term below (κ + β) 2^-40 moves it by < 2^-40
        // relative.  CPHD: Λ_m = rate Σ q / κ enters as (1 + Λ_m x): terms below
        // κ / rate 2^-48 move it by < 2^-48 absolute each.  The two-level fixed
        // point resolves 2^-70: the floor never goes below -72.
        const bool cphd = c.filterType == PHD_FILTER_CPHD;
        const double kb = cphd ? (double)c.clutterDensity / std::max((double)c.clutterRate, 1.0)
                               : (double)c.clutterDensity + (double)c.birthWeight;
        double fl = kb > 0 ? std::log2(kb) - (cphd ? 48.0 : 40.0) : -72.0;
        fl = std::max(fl, -72.0);
        const double thr0 = cphd ? (double)d.cphd_thr0 : (double)d.lq_keep_thresh * 1.4426950408889634;
        d.walk_floor = (float)std::min(fl, thr0 - 1.0);  // every listable pair is walked
    }
    return d;
}

/* Mixed static + dynamic update (feature_model 2; phd_mixed.hip) of every
 * particle, or (slots != NULL) a re-update of `nslots` listed slots with the
 * sets of the last launch: same input sets, same output sets, cur and dcur
 * unchanged (a sharded step's overflow recovery, as launch_update's).  Every
 * prior is read through its slab reference, the sets X included. */
static int launch_update_mixed(phd_ctx* ctx, const int* slots, int nslots) {
    const phd_slam_config& cfg = ctx->cfg;
    if (!ctx->mx.on) return fail(PHD_E_ARG, "feature_model 2 needs phd_enable_dynamic");
    if (cfg.filterType != PHD_FILTER_PHD) return fail(PHD_E_UNSUPPORTED, "feature_model 2 with the CPHD filter");
    if (cfg.particleWeighting != 0) return fail(PHD_E_UNSUPPORTED, "particle_weighting != 0 is not implemented");
    if (cfg.distanceMetric == 1)
        return fail(PHD_E_UNSUPPORTED,
                    "feature_model 2 with distance_metric 1: the reference's Hellinger distance of 4-D components is "
                    "the constant 0 (device_math.cuh:366-371), which would merge every dynamic component into one");
    if (cfg.distanceMetric != 0) return fail(PHD_E_UNSUPPORTED, "distance_metric must be 0 (Mahalanobis)");
    if (ctx->st.replay) return fail(PHD_E_UNSUPPORTED, "feature_model 2 in replay mode");
    if (ctx->st.d_map_x && !ctx->mx.d_dmap_x)  // (static records received before phd_enable_dynamic)
        return fail(PHD_E_ARG, "feature_model 2: migrated particles without dynamic maps (phd_enable_dynamic comes first)");
    const int grid = slots ? nslots : ctx->n;
    if (grid <= 0) return PHD_OK;
    const int in_set = slots ? ctx->st.cur ^ 1 : ctx->st.cur, out_set = in_set ^ 1;
    const int din = slots ? ctx->mx.dcur ^ 1 : ctx->mx.dcur, dout = din ^ 1;
    MixedArgs a;
    a.n = grid;
    a.slots = slots;
    a.map_x = ctx->st.d_map_x;
    a.size_x = ctx->st.d_size_x;
    a.dmap_x = ctx->mx.d_dmap_x;
    a.dsize_x = ctx->mx.d_dsize_x;
    a.cap = ctx->cap.map_capacity;
    a.dcap = ctx->mx.dcap;
    a.M = ctx->z.M;
    a.Kcap = ctx->cap.candidate_capacity;
    a.src = ctx->st.d_src;
    a.src_reset = ctx->st.d_src;
    a.map_in = ctx->st.d_map[in_set];
    a.map_out = ctx->st.d_map[out_set];
    a.size_in = ctx->st.d_size[in_set];
    a.size_out = ctx->st.d_size[out_set];
    a.dmap_in = ctx->mx.d_dmap[din];
    a.dmap_out = ctx->mx.d_dmap[dout];
    a.dsize_in = ctx->mx.d_dsize[din];
    a.dsize_out = ctx->mx.d_dsize[dout];
    a.poses = ctx->st.d_pose;
    a.logw = ctx->st.d_logw;
    a.delta = ctx->d_delta;
    a.status = ctx->d_status;
    a.err = ctx->d_err;
    a.zr = ctx->z.zr;
    a.zb = ctx->z.zb;
    a.zlab = ctx->z.zlab;
    a.c = phd_mx_config(&cfg);
    a.ekf = ctx->mx.d_ekf;
    a.cand = ctx->mx.d_cand;
    const size_t lds = mixed_lds_bytes(a.cap, a.dcap, ctx->cap.max_measurements, a.Kcap);
    if (lds > 150 * 1024) return fail(PHD_E_CAPACITY, "feature_model 2: capacities exceed the 150 KB LDS budget");
    const bool timed = PHD_TIMING_EVENTS && !ctx->tm.ev_a.empty() && !slots && ctx->tm.tick++ % ctx->tm.stride == 0;
    const int ei = ctx->tm.next;
    if (timed) HIPCHK(hipEventRecord(ctx->tm.ev_a[ei], ctx->stream));
    HIPCHK(mixed_launch_update(a, lds, ctx->stream));
    if (timed) {
        HIPCHK(hipEventRecord(ctx->tm.ev_b[ei], ctx->stream));
        ctx->tm.next = (ei + 1) % (int)ctx->tm.ev_a.size();
        if (ctx->tm.used < (int)ctx->tm.ev_a.size()) ctx->tm.used++;
    }
    if (slots) return PHD_OK;
    ctx->st.cur = out_set;
    ctx->mx.dcur = dout;
    ctx->mx.x_live = false;  // every reference is the identity again: none names the sets X
    return PHD_OK;
}

/* Trailing workgroups of an update launch that run at the highest wave
 * priority (UpdateArgs.prio): the ones dispatched last finish the launch, and
 * while they share SIMDs with earlier workgroups (which have slack) their
 * instructions issue first, so the launch drains sooner.  Default: the last
 * 20 % of the grid (measured at config 3: +1.3 % for 40 %; with the
 * last-written-first part C order 25 % is +0.2 % over 40 %, 55 % -1.5 %,
 * 20 % +1.0 % over 25 %, 15 % -0.5 %; four graded levels were no better;
 * round 4 close: 20 % = 35 %, none -1.3 %, profiles/r04fin_c3_prio_tail.txt). */
#ifndef UPD_PRIO_TAIL_PCT
#define UPD_PRIO_TAIL_PCT 20
#endif
static int prio_tail(int grid, int resident) {
    if (grid <= resident) return 0;
    return (int)((long)grid * UPD_PRIO_TAIL_PCT / 100);
}

/* The fused update of every particle, or (slots != NULL) a re-update of
 * `nslots` listed slots with the sets of the last launch (a sharded step's
 * overflow recovery: same input slabs, same output slabs, cur unchanged).
 * rs: the step's resample to launch with part C, as its plan says. */
int launch_update(phd_ctx* ctx, const FusedPredict* fused, const int* slots, int nslots, const RsBeside* rs,
                  UpdateDone* done) {
    UpdateDone done_here;
    if (!done) done = &done_here;
    const phd_slam_config& cfg = ctx->cfg;
    if (cfg.featureModel == PHD_FEATURE_MIXED) {
        return launch_update_mixed(ctx, slots, nslots);
    }
    if (cfg.featureModel != PHD_FEATURE_STATIC)
        return fail(PHD_E_UNSUPPORTED,
                    "feature_model 1 (dynamic only): the reference's update is a stub (phdfilter.cu:3663-3671)");
    if (cfg.distanceMetric != 0 && cfg.distanceMetric != 1)
        return fail(PHD_E_UNSUPPORTED, "distance_metric must be 0 (Mahalanobis) or 1 (Hellinger)");
    const int metric = cfg.distanceMetric;  // the merge's distance: selects the kernels that hold the merge
    const bool cphd = cfg.filterType == PHD_FILTER_CPHD;
    if (cfg.filterType != PHD_FILTER_PHD && !cphd) return fail(PHD_E_UNSUPPORTED, "unknown filter_type");
    if (cphd) {
        if (ctx->z.M > PHD_CPHD_MAX_M)
            return fail(PHD_E_UNSUPPORTED, "CPHD update supports at most " + std::to_string(PHD_CPHD_MAX_M) +
                                               " measurements per step");
        if (cfg.maxCardinality < 0) return fail(PHD_E_ARG, "CPHD needs max_cardinality >= 0");
        const int nl = std::max(cfg.maxCardinality, ctx->cap.max_measurements) + 2;
        if (ctx->cn.lfact_n < nl) {
            std::vector<double> lf(nl);
            lf[0] = 0;
            for (int i = 1; i < nl; i++) lf[i] = lf[i - 1] + std::log((double)i);  // as the oracle
            if (ctx->cn.d_lfact.alloc(nl)) return PHD_E_HIP;
            HIPCHK(hipMemcpyAsync(ctx->cn.d_lfact, lf.data(), nl * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            HIPCHK(hipStreamSynchronize(ctx->stream));
            ctx->cn.lfact_n = nl;
        }
        if (ensure_cn(ctx)) return PHD_E_HIP;
    }
    if (cfg.particleWeighting != 0)
        return fail(PHD_E_UNSUPPORTED, "particle_weighting != 0 is not implemented on the device path");
    // phd_set_config sizes the launch for the filter's and the metric's kernels (registers,
    // LDS layout); a mismatch here is its failure, reported again
    if (ctx->upd.cphd != (cphd ? 1 : 0) || ctx->upd.metric != metric)
        return ctx->upd.cfg_error.empty()
                   ? fail(PHD_E_ARG, "internal: update launch not configured for this filter/metric")
                   : fail(PHD_E_CAPACITY, ctx->upd.cfg_error);
    // the first launch (part A of the split update, else the whole update), which runs a fused predict
    const void* k_first = update_kernel(ctx->upd.threads, cphd, ctx->upd.split ? 1 : 0, metric, fused ? 1 : 0);
    if (!k_first) return fail(PHD_E_ARG, "internal: no fused-predict kernel for this update form");
    if (rs && (slots || !ctx->upd.split)) return fail(PHD_E_ARG, "internal: a step's resample without a full split update");
    const int in_set = ctx->st.replay ? 0 : (slots ? ctx->st.cur ^ 1 : ctx->st.cur);
    const int out_set = in_set ^ 1;
    const int grid = slots ? nslots : ctx->n;
    if (grid <= 0) return PHD_OK;
    UpdateArgs a{};
    a.n = ctx->n;
    a.slots = slots;
    a.first = 0;
    a.order = 0;
    a.cap = ctx->cap.map_capacity;
    a.M = ctx->z.M;
    a.Mcap = ctx->cap.max_measurements;
    a.Kcap = ctx->cap.candidate_capacity;
    a.Scap = ctx->cap.survivor_capacity;
    a.Epool = ctx->upd.epool;
    a.plreq = ctx->upd.plreq;
    a.Bbuckets = ctx->upd.split
                     ? upd_lds_layout(a.cap, a.Mcap, a.Kcap, a.Scap, a.Epool, ctx->upd.threads, cphd, 2).B
                     : upd_buckets(a.Kcap, 0);
    a.merge_mode = ctx->merge_mode;
    a.src = ctx->st.replay ? nullptr : ctx->st.d_src;
    a.src_reset = ctx->st.d_src;
    a.map_x = ctx->st.d_map_x;
    a.size_x = ctx->st.d_size_x;
    a.map_in = ctx->st.d_map[in_set];
    a.map_out = ctx->st.d_map[out_set];
    a.size_in = ctx->st.d_size[in_set];
    a.size_out = ctx->st.d_size[out_set];
    a.poses = ctx->st.d_pose;
    a.logw = ctx->st.d_logw;
    a.logw_out = slots ? nullptr : ctx->logw_mirror;  // (a partial update leaves the rest of the mirror stale)
    a.delta = ctx->d_delta;
    a.zr = ctx->z.zr;
    a.zb = ctx->z.zb;
    a.zok = ctx->z.zok;
    a.zs = ctx->z.zs;
    a.zbin = ctx->z.zbin;
    a.Mv = ctx->z.Mv;
    a.zwide = ctx->z.zwide;
    a.status = ctx->d_status;
    a.err = ctx->d_err;
    a.stamps = ctx->d_stamps;
    a.pc = predict_cfg(cfg, ctx->index_offset);
    a.pseed = ctx->seed;
    if (fused) {  // (else no predict: zeros)
        a.predict = fused->predict;
        a.pu = fused->u;
        a.pstep = fused->step;
        a.pose_prior = ctx->st.replay ? ctx->st.d_pose_prior : nullptr;
        a.logw_prior = ctx->st.replay ? ctx->st.d_logw_prior : nullptr;
    }
    a.births = ctx->z.births_now > 0 ? ctx->z.d_births : nullptr;
    a.Mb = ctx->z.births_now;
    a.bzr = ctx->z.births_zr;
    a.bzb = ctx->z.births_zb;
    a.bzvi = ctx->z.births_zvi;
    ctx->z.births_now = 0;  // (consumed by this update)
    a.cn_coef = cphd ? ctx->cn.d_coef : nullptr;
    a.hand = nullptr;
    if (ctx->upd.split) {
        const size_t hb = (size_t)ctx->nmax * cphd_hand_layout(ctx->cap.map_capacity, ctx->cap.max_measurements,
                                                             ctx->cap.survivor_capacity)
                                               .stride;
        if (ctx->cn.d_hand.ensure(hb)) return PHD_E_HIP;
        a.hand = ctx->cn.d_hand;
    }
    a.cn_stride = ctx->cn.stride;
    a.lfact = ctx->cn.d_lfact;
    a.Nmax = cfg.maxCardinality;
    a.c = dev_cfg(cfg);
    const bool timed =
        PHD_TIMING_EVENTS && !ctx->tm.ev_a.empty() && !slots && ctx->tm.tick++ % ctx->tm.stride == 0;
    const int ei = ctx->tm.next;
    if (timed) HIPCHK(hipEventRecord(ctx->tm.ev_a[ei], ctx->stream));
    hipStream_t st = ctx->stream;
    const dim3 block(ctx->upd.threads);
    a.prio = prio_tail(grid, ctx->upd.resident);
    if (ctx->upd.split) {
        // part A -> (CPHD: the terms, one wave per particle) -> part C through the
        // handoff (the diagnostic phase stamps record part C)
        UpdateArgs aa = a;
        aa.stamps = nullptr;
#ifdef PHD_STAMP_PART_A
        aa.stamps = a.stamps;  // diagnostic stamps build: record part A instead
        a.stamps = nullptr;
#endif
        // CPHD's part A runs the particle's predict when fused (the CPHD update is
        // three launches: the predict's registers cost part A nothing that matters);
        // the split PHD update's never (enqueue_predict_update: its own launch)
        aa.prio = prio_tail(grid, ctx->upd.resident_a);
        hipLaunchKernelGGL((void (*)(UpdateArgs))k_first, dim3(grid), block, ctx->upd.lds_a, st, aa);
        // the fused predict is done: the later launches read the predicted poses
        a.predict = 0;
        a.pose_prior = nullptr;
        a.logw_prior = nullptr;
        // the terms and part C read part A's handoff and prior slab: last-written
        // first, XCD-preserving (upd_particle)
        a.order = 1;
        if (cphd)
            hipLaunchKernelGGL(k_cphd_terms, dim3(grid), dim3(64), cphd_terms_lds(ctx->cap.max_measurements), st,
                               a);
        if (ctx->sh.ev_logw) {  // the log-weights are final (phd_wait_logw)
            hipEventRecord(ctx->sh.ev_logw, st);
            done->logw_final = true;
        }
        // the step's resample, now that the log-weights are final: part C reads
        // neither them nor the arrays the resample writes
        int lead = 0;
        if (rs && rs->form == PHD_RS_FORM_LEAD) {  // in part C's lead workgroups: ordered by the stream itself
            a.rs_lead = lead = RS_LEAD_WGS;
            a.rs = rs->a;
        } else if (rs) {  // PHD_RS_FORM_BESIDE: on the auxiliary stream
            hipEventRecord(ctx->rs.ev_terms, st);
            hipStreamWaitEvent(ctx->rs.aux, ctx->rs.ev_terms, 0);
            hipLaunchKernelGGL(k_rs_step, dim3(rs->a.B), dim3(RS_THREADS), 0, ctx->rs.aux, rs->a);
            hipEventRecord(ctx->rs.ev_rs, ctx->rs.aux);
            done->rs_beside = true;
        }
        hipLaunchKernelGGL((void (*)(UpdateArgs))update_kernel(ctx->upd.threads, cphd, 2, metric), dim3(grid + lead),
                           block, ctx->upd.lds, st, a);
        if (cphd) ctx->cn.valid = true;
    } else {
        hipLaunchKernelGGL((void (*)(UpdateArgs))k_first, dim3(grid), block, ctx->upd.lds, st, a);
    }
    HIPCHK(hipGetLastError());
    if (ctx->sh.ev_logw && !done->logw_final) {  // (the fused update: its log-weights at its end)
        HIPCHK(hipEventRecord(ctx->sh.ev_logw, st));
        done->logw_final = true;
    }
    if (!slots) ctx->st.src_fresh = true;  // part C reset every slab reference to the identity
    if (timed) {
        HIPCHK(hipEventRecord(ctx->tm.ev_b[ei], ctx->stream));
        ctx->tm.next = (ei + 1) % (int)ctx->tm.ev_a.size();
        if (ctx->tm.used < (int)ctx->tm.ev_a.size()) ctx->tm.used++;
    }
    if (!slots) ctx->st.cur = out_set;
    return PHD_OK;
}

/* the step adds births (phd_set_step_births; by default with CPHD, whose
 * update array has no birth terms: phdfilter.cu.bak:738-870) */
bool step_births_on(const phd_ctx* ctx) {
    return ctx->z.births_req < 0 ? ctx->cfg.filterType == PHD_FILTER_CPHD : ctx->z.births_req != 0;
}

extern "C" {

int phd_set_step_births(phd_ctx* ctx, int on) {
    if (!ctx || on < -1 || on > 1) return fail(PHD_E_ARG, "bad arguments to phd_set_step_births");
    ctx->z.births_req = on;
    return PHD_OK;
}

int phd_step_births(phd_ctx* ctx, int* on) {
    if (!ctx || !on) return fail(PHD_E_ARG, "null argument");
    *on = step_births_on(ctx) ? 1 : 0;
    return PHD_OK;
}

}  // extern "C"

/* the scan the step's births come from: its raw rows, measurement count and
 * valid count (false: no births this step) */
static bool birth_rows(const phd_ctx* ctx, const float** zr, const float** zb, const int** zok, int* Mr, int* Mv) {
    if (!step_births_on(ctx) || ctx->cfg.featureModel != PHD_FEATURE_STATIC) return false;  // (mixed: update terms)
    const bool own = ctx->st.replay;  // replay: the fixed scan is also the previous one
    if (!own && !ctx->z.have_prev) return false;
    *Mr = own ? ctx->z.M : ctx->z.M_prev;
    *Mv = own ? ctx->z.Mv : ctx->z.Mv_prev;
    if (*Mr <= 0 || *Mv <= 0) return false;
    const ZBlk Z = zblk_layout();
    const unsigned char* rows = own ? ctx->z.blk : ctx->z.prev;
    *zr = (const float*)(rows + Z.zr);
    *zb = (const float*)(rows + Z.zb);
    *zok = (const int*)(rows + Z.zok);
    return true;
}

/* The step's births, after its predict: the previous scan's valid measurements
 * (replay: the replayed scan's own).  With an update this step the update's
 * classify places them itself after each particle's map (UpdateArgs::births:
 * this only arms it); with no measurements they are appended to the maps by
 * k_add_births, as the reference does without an update. */
int launch_step_births(phd_ctx* ctx, const int* slots, int count) {
    ctx->z.births_now = 0;
    if (count <= 0) return PHD_OK;
    const float *zr = nullptr, *zb = nullptr;
    const int* zok = nullptr;
    int Mr = 0, Mv = 0;
    if (!birth_rows(ctx, &zr, &zb, &zok, &Mr, &Mv)) return PHD_OK;
    if (ctx->z.M <= 0) {
        // no update this step: the births join the maps themselves.  Pending
        // slots (a sharded settle on an empty scan) take the sets a slot update
        // takes (launch_update): their records (set X) -> their slabs of the
        // current set, which the step's own births launch wrote
        const int in_set = slots ? ctx->st.cur ^ 1 : ctx->st.cur, out_set = slots ? ctx->st.cur : ctx->st.cur ^ 1;
        hipLaunchKernelGGL(k_add_births, dim3(count), dim3(256), 0, ctx->stream, ctx->st.d_src, slots, count,
                           ctx->cap.map_capacity, (const float*)ctx->st.d_map[in_set], (const int*)ctx->st.d_size[in_set],
                           (const float*)ctx->st.d_map_x, (const int*)ctx->st.d_size_x, ctx->st.d_map[out_set],
                           ctx->st.d_size[out_set], (const phd_pose*)ctx->st.d_pose, zr, zb, zok, Mr, dev_cfg(ctx->cfg),
                           ctx->d_status, ctx->d_err);
        HIPCHK(hipGetLastError());
        if (!slots) {
            hipLaunchKernelGGL(k_iota, dim3((ctx->n + 255) / 256), dim3(256), 0, ctx->stream, ctx->st.d_src, ctx->n);
            HIPCHK(hipGetLastError());
            ctx->st.cur = out_set;
        }
        return PHD_OK;
    }
    if (ctx->z.d_births.ensure((size_t)ctx->nmax * 7 * ctx->cap.map_capacity)) return PHD_E_HIP;
    const ZBlk Z = zblk_layout();
    const unsigned char* rows = (const unsigned char*)zr - Z.zr;
    ctx->z.births_zr = zr;
    ctx->z.births_zb = zb;
    ctx->z.births_zvi = (const int*)(rows + Z.zvi);
    ctx->z.births_now = Mv;
    return PHD_OK;
}

extern "C" {

/* CPHD births through the prediction (phd_capi.h). */
int phd_add_births(phd_ctx* ctx, const phd_measurement* z, int n_measure) {
    if (!ctx || n_measure < 0 || (n_measure > 0 && !z)) return fail(PHD_E_ARG, "bad arguments to phd_add_births");
    if (!ctx->cfg_set) return fail(PHD_E_ARG, "phd_set_config not called");
    if (ctx->st.replay) return fail(PHD_E_ARG, "phd_add_births: not in replay mode");
    if (ctx->z.births_req < 0)
        ctx->z.births_req = 0;  // the caller's loop places the births (the pre-step-births API): from now on
    if (step_births_on(ctx))
        return fail(PHD_E_ARG, "phd_add_births: phd_set_step_births(ctx, 1) asked the step to add the births of "
                               "the previous scan itself");
    if (n_measure == 0) return PHD_OK;
    if (set_device(ctx)) return PHD_E_HIP;
    // the previous scan's measurements through phd_set_measurements' device rows
    // (they replace the context's measurements: set the update's afterwards)
    int rc = phd_set_measurements(ctx, z, n_measure);
    if (rc) return rc;
    const int M = ctx->z.M;
    const int in_set = ctx->st.cur, out_set = in_set ^ 1;
    hipLaunchKernelGGL(k_add_births, dim3(ctx->n), dim3(256), 0, ctx->stream, ctx->st.d_src, (const int*)nullptr, ctx->n,
                       ctx->cap.map_capacity, (const float*)ctx->st.d_map[in_set], (const int*)ctx->st.d_size[in_set],
                       (const float*)ctx->st.d_map_x, (const int*)ctx->st.d_size_x, ctx->st.d_map[out_set],
                       ctx->st.d_size[out_set], (const phd_pose*)ctx->st.d_pose, (const float*)ctx->z.zr,
                       (const float*)ctx->z.zb, (const int*)ctx->z.zok, M, dev_cfg(ctx->cfg), ctx->d_status,
                       ctx->d_err);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_iota, dim3((ctx->n + 255) / 256), dim3(256), 0, ctx->stream, ctx->st.d_src, ctx->n);
    HIPCHK(hipGetLastError());
    ctx->st.cur = out_set;
    if (ctx->check_each_update) return check_err(ctx);
    return PHD_OK;
}

int phd_enable_timing(phd_ctx* ctx, int max_records) {
    if (!ctx) return fail(PHD_E_ARG, "null ctx");
    if (set_device(ctx)) return PHD_E_HIP;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->tm.ev_a.clear();
    ctx->tm.ev_b.clear();
    ctx->tm.next = ctx->tm.used = 0;
    ctx->tm.tick = 0;
    for (int i = 0; i < max_records; i++) {
        Event a, b;
        if (a.create(kEvTime) || b.create(kEvTime)) return PHD_E_HIP;
        ctx->tm.ev_a.push_back(std::move(a));
        ctx->tm.ev_b.push_back(std::move(b));
    }
    return PHD_OK;
}

int phd_set_timing_stride(phd_ctx* ctx, int stride) {
    if (!ctx || stride < 1) return fail(PHD_E_ARG, "bad arguments to phd_set_timing_stride");
    ctx->tm.stride = stride;
    ctx->tm.tick = 0;
    return PHD_OK;
}

int phd_update_timing(phd_ctx* ctx, float* total_ms, int* count) {
    if (!ctx || !total_ms) return fail(PHD_E_ARG, "null argument");
    if (set_device(ctx)) return PHD_E_HIP;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    float tot = 0.f;
    for (int i = 0; i < ctx->tm.used; i++) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, ctx->tm.ev_a[i], ctx->tm.ev_b[i]));
        tot += ms;
    }
    *total_ms = tot;
    if (count) *count = ctx->tm.used;
    ctx->tm.used = 0;
    ctx->tm.next = 0;
    return PHD_OK;
}

}  // extern "C"

int check_err(phd_ctx* ctx) {
    int err = 0;
    HIPCHK(hipMemcpyAsync(&err, ctx->d_err, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (err) {
        hipMemsetAsync(ctx->d_err, 0, sizeof(int), ctx->stream);
        std::string m = "update capacity exceeded:";
        if (err & PHD_ST_SURVIVOR_OVERFLOW) m += " survivor_capacity";
        if (err & PHD_ST_CANDIDATE_OVERFLOW) m += " candidate_capacity";
        if (err & PHD_ST_MAP_OVERFLOW) m += " map_capacity";
        if (err & PHD_ST_ETA_RANGE) m += " likelihood range (a term >= 2^20)";
        if (err & PHD_ST_WAIT_TIMEOUT) m += " (a one-launch resample wait timed out: not every workgroup was resident)";
        return fail(PHD_E_CAPACITY, m);
    }
    return PHD_OK;
}

extern "C" {

int phd_update(phd_ctx* ctx) {
    if (!ctx) return fail(PHD_E_ARG, "null ctx");
    if (!ctx->cfg_set) return fail(PHD_E_ARG, "phd_set_config not called");
    if (set_device(ctx)) return PHD_E_HIP;
    if (ctx->z.M == 0) return PHD_OK;  // run_synth skips the update when |Z| == 0 (main.cpp:1260)
    int rc = launch_update(ctx);
    if (rc) return rc;
    if (ctx->check_each_update) return check_err(ctx);
    return PHD_OK;
}

int phd_last_update_ms(phd_ctx* ctx, float* ms) {
    if (!ctx || !ms) return fail(PHD_E_ARG, "null argument");
    if (ctx->tm.used == 0) return fail(PHD_E_ARG, "timing not enabled (phd_enable_timing) or no update recorded");
    const int i = (ctx->tm.next + (int)ctx->tm.ev_a.size() - 1) % (int)ctx->tm.ev_a.size();
    HIPCHK(hipEventSynchronize(ctx->tm.ev_b[i]));
    HIPCHK(hipEventElapsedTime(ms, ctx->tm.ev_a[i], ctx->tm.ev_b[i]));
    return PHD_OK;
}

}  // extern "C"
