/*
 * phd_capi_trace.hip — the per-scan estimate trace of the C-ABI (phd_trace.hip
 * holds its kernels): enable, the append of phd_step, reads, and the pack /
 * append pairs of the sharded step (static and mixed).
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "phd_ctx.h"

using namespace phd;

static void trace_free(phd_ctx* c) { c->tr = Trace{}; }  // (the rings release with the old value)

/* what the trace does not cover (phd_trace_enable, and again at every traced
 * step: the configuration may change in between).  sharded: the trace of a
 * sharded step (phd_trace_shard_pack), which reads migrated slabs but not every
 * rank's cardinality rows; phd_step's own reads no migrated slab.
 * phd_trace_enable asks for neither: the context may serve either step. */
int trace_supported(const phd_ctx* ctx, TraceUse use) {
    if (ctx->tr.mixed) {
        // a mixed-model trace (phd_trace_enable_mixed): the model and the dynamic
        // capacity its rings and launches were sized for
        if (ctx->cfg.featureModel != PHD_FEATURE_MIXED)
            return fail(PHD_E_UNSUPPORTED,
                        "feature_model changed after phd_trace_enable_mixed: enable the trace again");
        if (!ctx->mx.on || ctx->mx.dcap != ctx->tr.dcap)
            return fail(PHD_E_UNSUPPORTED,
                        "the dynamic capacity changed after phd_trace_enable_mixed: enable the trace again");
    } else if (ctx->cfg.featureModel != PHD_FEATURE_STATIC)
        return fail(PHD_E_UNSUPPORTED, "the estimate trace supports the static feature model only");
    if (ctx->cfg.nPredictParticles > 1 || ctx->n != ctx->n_base)
        return fail(PHD_E_UNSUPPORTED, "the estimate trace does not support n_predict_particles > 1");
    if (use == TRACE_STEP && ctx->st.d_map_x)
        return fail(PHD_E_UNSUPPORTED, "phd_step's estimate trace does not support migrated (sharded) slabs");
    if (use == TRACE_SHARDED && ctx->tr.d_card && (ctx->cfg.mapEstimate & 2))
        return fail(PHD_E_UNSUPPORTED,
                    "the sharded estimate trace does not support PHD_TRACE_CARD_DIST with map_estimate & 2 (the "
                    "expected rows are a sequential sum over every rank's particles)");
    if ((ctx->tr.flags & PHD_TRACE_CARD_DIST) &&
        (ctx->cfg.filterType != PHD_FILTER_CPHD || ctx->cfg.maxCardinality + 1 != ctx->tr.K))
        return fail(PHD_E_UNSUPPORTED, "PHD_TRACE_CARD_DIST needs the CPHD configuration it was enabled with");
    if (ctx->tr.d_card && (ctx->cfg.mapEstimate & 2) && !ctx->tr.d_card_all)
        return fail(PHD_E_UNSUPPORTED, "map_estimate changed after phd_trace_enable: enable the trace again");
    return PHD_OK;
}

/* One entry of the trace from the state between the update and the resample
 * (phd_trace.hip): stream-ordered, nothing waits on the host. */
int trace_append(phd_ctx* ctx, uint64_t step) {
    auto& T = ctx->tr;
    const size_t slot = (size_t)(T.count % T.cap);
    TraceArgs a{};
    a.logw = ctx->st.d_logw;
    a.pose = ctx->st.d_pose;
    a.src = ctx->st.d_src;
    a.map_in = ctx->st.d_map[ctx->st.cur];
    a.size_in = ctx->st.d_size[ctx->st.cur];
    a.map_x = ctx->st.d_map_x;
    a.size_x = ctx->st.d_size_x;
    a.n = ctx->n;
    a.cap = ctx->cap.map_capacity;
    a.step = step;
    a.M = ctx->z.M;
    a.has_meas = rs_mode(ctx);
    a.resample_thresh = ctx->cfg.resampleThresh;
    a.err = ctx->d_err;
    a.w_norm = T.d_w;
    a.part = T.d_part;
    a.hand = T.d_hand;
    a.rec = T.d_rec + slot;
    a.snap = T.d_snap ? T.d_snap + slot * (size_t)T.snap_cap : nullptr;
    a.snap_cap = T.snap_cap;
    a.K = T.K;
    if (T.mixed) {  // the dynamic set that is current after the update (or, on an empty scan, the predict)
        a.dmap = ctx->mx.d_dmap[ctx->mx.dcur];
        a.dsize = ctx->mx.d_dsize[ctx->mx.dcur];
        a.dcap = ctx->mx.dcap;
        a.dpart = T.d_dpart;
        a.drec = T.d_drec + slot;
        a.dsnap = T.d_dsnap ? T.d_dsnap + slot * (size_t)T.dsnap_cap : nullptr;
        a.dsnap_cap = T.dsnap_cap;
    }
    trace_launch_stage1(a, ctx->stream);
    if (T.d_card && ctx->cn.valid) {
        float* entry = T.d_card + slot * (size_t)T.K;
        if ((ctx->cfg.mapEstimate & 2) && ctx->n > 1) {  // Σ exp(w_n) cn_n (recoverSlamState's expected form)
            hipLaunchKernelGGL(k_cphd_cardinality, dim3(ctx->n), dim3(256), 0, ctx->stream, (const int*)ctx->st.d_src,
                               (const double*)ctx->cn.d_coef, (const double*)ctx->cn.d_x, ctx->cn.stride,
                               ctx->cn.d_lfact, T.K - 1, ctx->n, T.d_card_all);
            a.card = entry;
            a.card_all = T.d_card_all;
        } else {  // the arg-max particle's row: stage 1 left its slab reference
            hipLaunchKernelGGL(k_cphd_cardinality, dim3(1), dim3(256), 0, ctx->stream,
                               (const int*)(T.d_hand + TRACE_H_SLAB), (const double*)ctx->cn.d_coef,
                               (const double*)ctx->cn.d_x, ctx->cn.stride, ctx->cn.d_lfact, T.K - 1, 1, entry);
        }
    }
    trace_launch_stage2(a, ctx->stream);
    HIPCHK(hipGetLastError());
    T.count++;
    return PHD_OK;
}

/* phd_trace_enable, and with mixed (phd_trace_enable_mixed) the dyn ring beside it */
static int trace_enable(phd_ctx* ctx, int capacity, int map_snapshot_cap, int dyn_snapshot_cap, unsigned flags,
                        bool mixed) {
    const std::string who = mixed ? "phd_trace_enable_mixed" : "phd_trace_enable";
    if (!ctx || capacity < 0 || map_snapshot_cap < 0 || dyn_snapshot_cap < 0)
        return fail(PHD_E_ARG, "bad arguments to " + who);
    if (set_device(ctx)) return PHD_E_HIP;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    trace_free(ctx);
    if (capacity == 0) return PHD_OK;
    if (!ctx->cfg_set) return fail(PHD_E_ARG, "phd_set_config not called");
    if (flags & ~(unsigned)PHD_TRACE_CARD_DIST) return fail(PHD_E_ARG, "unknown trace flags");
    if (mixed) {
        if (!PHD_TRACE_DYN)
            return fail(PHD_E_UNSUPPORTED, "this build has the dynamic trace stages compiled out (PHD_TRACE_DYN 0)");
        if (ctx->cfg.featureModel != PHD_FEATURE_MIXED)
            return fail(PHD_E_UNSUPPORTED, "phd_trace_enable_mixed needs feature_model 2 (phd_trace_enable serves the static model)");
        if (!ctx->mx.on) return fail(PHD_E_ARG, "phd_trace_enable_mixed: phd_enable_dynamic not called");
        if (flags & PHD_TRACE_CARD_DIST)
            return fail(PHD_E_UNSUPPORTED, "PHD_TRACE_CARD_DIST on a mixed trace: feature_model 2 has no CPHD filter");
    }
    auto& T = ctx->tr;
    T.mixed = mixed;
    T.dcap = mixed ? ctx->mx.dcap : 0;
    T.flags = flags;
    T.K = (flags & PHD_TRACE_CARD_DIST) ? ctx->cfg.maxCardinality + 1 : 0;
    int rc = trace_supported(ctx, TRACE_ENABLE);
    if ((flags & PHD_TRACE_CARD_DIST) && !rc && T.K < 1) rc = fail(PHD_E_ARG, "CPHD needs max_cardinality >= 0");
    if (rc) {
        trace_free(ctx);
        return rc;
    }
    const size_t N = (size_t)ctx->nmax;
    const size_t parts = (N + TRACE_PB - 1) / TRACE_PB;
    const size_t dsnap_n = (size_t)capacity * dyn_snapshot_cap;
    rc = T.d_rec.alloc(capacity) || T.d_w.alloc(N) || T.d_part.alloc(parts) || T.d_hand.alloc(TRACE_H_WORDS) ||
         (map_snapshot_cap > 0 && T.d_snap.alloc((size_t)capacity * map_snapshot_cap)) ||
         (T.K && (T.d_card.alloc((size_t)capacity * T.K) || T.d_card_row.alloc(T.K))) ||
         (T.K && (ctx->cfg.mapEstimate & 2) && T.d_card_all.alloc(N * T.K)) ||
         (mixed && (T.d_drec.alloc(capacity) || T.d_dpart.alloc(parts) ||
                    (dyn_snapshot_cap > 0 && T.d_dsnap.alloc(dsnap_n))));
    if (rc) {
        const std::string msg = who + ": " + last_error();
        trace_free(ctx);
        return fail(PHD_E_HIP, msg);
    }
    hipError_t e = hipMemsetAsync(T.d_rec, 0, (size_t)capacity * sizeof(phd_trace_record), ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(T.d_hand, 0, TRACE_H_WORDS * sizeof(int), ctx->stream);
    // status_errors counts from here: the counter as it stands is the baseline
    if (e == hipSuccess)
        e = hipMemcpyAsync(T.d_hand + TRACE_H_ERRPREV, ctx->d_err + 3, sizeof(int), hipMemcpyDeviceToDevice,
                           ctx->stream);
    if (e == hipSuccess && T.d_snap)
        e = hipMemsetAsync(T.d_snap, 0, (size_t)capacity * map_snapshot_cap * sizeof(phd_gaussian2d), ctx->stream);
    if (e == hipSuccess && T.d_card) e = hipMemsetAsync(T.d_card, 0, (size_t)capacity * T.K * sizeof(float), ctx->stream);
    if (mixed) {
        if (e == hipSuccess)
            e = hipMemsetAsync(T.d_drec, 0, (size_t)capacity * sizeof(phd_trace_dyn_record), ctx->stream);
        if (e == hipSuccess && T.d_dsnap) e = hipMemsetAsync(T.d_dsnap, 0, dsnap_n * sizeof(phd_gaussian4d), ctx->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        trace_free(ctx);
        return fail(PHD_E_HIP, who + ": " + hipGetErrorString(e));
    }
    T.snap_cap = map_snapshot_cap;
    T.dsnap_cap = mixed ? dyn_snapshot_cap : 0;
    T.cap = capacity;  // (on from here)
    return PHD_OK;
}

extern "C" {

int phd_trace_enable(phd_ctx* ctx, int capacity, int map_snapshot_cap, unsigned flags) {
    return trace_enable(ctx, capacity, map_snapshot_cap, 0, flags, false);
}

int phd_trace_enable_mixed(phd_ctx* ctx, int capacity, int map_snapshot_cap, int dyn_snapshot_cap, unsigned flags) {
    return trace_enable(ctx, capacity, map_snapshot_cap, dyn_snapshot_cap, flags, true);
}

int phd_trace_count(phd_ctx* ctx, long* written_total) {
    if (!ctx || !written_total) return fail(PHD_E_ARG, "null argument");
    *written_total = ctx->tr.count;
    return PHD_OK;
}

int phd_trace_read(phd_ctx* ctx, long first, int count, phd_trace_record* records, phd_gaussian2d* maps,
                   float* card) {
    if (!ctx || count < 0 || (count > 0 && !records)) return fail(PHD_E_ARG, "bad arguments to phd_trace_read");
    const auto& T = ctx->tr;
    if (T.cap <= 0) return fail(PHD_E_ARG, "the estimate trace is off (phd_trace_enable)");
    if (first < 0 || first + count > T.count) return fail(PHD_E_ARG, "trace records not written yet");
    if (first < T.count - T.cap) return fail(PHD_E_ARG, "trace records already overwritten");
    if (maps && !T.d_snap) return fail(PHD_E_ARG, "the trace has no map snapshots");
    if (card && !T.d_card) return fail(PHD_E_ARG, "the trace has no cardinality distributions");
    if (count == 0) return PHD_OK;
    if (set_device(ctx)) return PHD_E_HIP;
    // the range is one run of the ring, or two where it wraps
    const size_t s0 = (size_t)(first % T.cap);
    const size_t c0 = std::min((size_t)count, (size_t)T.cap - s0), c1 = (size_t)count - c0;
    auto pull = [&](void* dst, const void* ring, size_t entry) -> hipError_t {
        hipError_t e = hipMemcpyAsync(dst, (const char*)ring + s0 * entry, c0 * entry, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && c1)
            e = hipMemcpyAsync((char*)dst + c0 * entry, ring, c1 * entry, hipMemcpyDeviceToHost, ctx->stream);
        return e;
    };
    HIPCHK(pull(records, T.d_rec, sizeof(phd_trace_record)));
    if (maps) HIPCHK(pull(maps, T.d_snap, (size_t)T.snap_cap * sizeof(phd_gaussian2d)));
    if (card) HIPCHK(pull(card, T.d_card, (size_t)T.K * sizeof(float)));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PHD_OK;
}

int phd_trace_read_dynamic(phd_ctx* ctx, long first, int count, phd_trace_dyn_record* records, phd_gaussian4d* dmaps) {
    if (!ctx || count < 0 || (count > 0 && !records)) return fail(PHD_E_ARG, "bad arguments to phd_trace_read_dynamic");
    const auto& T = ctx->tr;
    if (T.cap <= 0 || !T.mixed) return fail(PHD_E_ARG, "the mixed estimate trace is off (phd_trace_enable_mixed)");
    if (first < 0 || first + count > T.count) return fail(PHD_E_ARG, "trace records not written yet");
    if (first < T.count - T.cap) return fail(PHD_E_ARG, "trace records already overwritten");
    if (dmaps && !T.d_dsnap) return fail(PHD_E_ARG, "the trace has no dynamic map snapshots");
    if (count == 0) return PHD_OK;
    if (set_device(ctx)) return PHD_E_HIP;
    // the range is one run of the ring, or two where it wraps (as phd_trace_read)
    const size_t s0 = (size_t)(first % T.cap);
    const size_t c0 = std::min((size_t)count, (size_t)T.cap - s0), c1 = (size_t)count - c0;
    auto pull = [&](void* dst, const void* ring, size_t entry) -> hipError_t {
        hipError_t e = hipMemcpyAsync(dst, (const char*)ring + s0 * entry, c0 * entry, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && c1)
            e = hipMemcpyAsync((char*)dst + c0 * entry, ring, c1 * entry, hipMemcpyDeviceToHost, ctx->stream);
        return e;
    };
    HIPCHK(pull(records, T.d_drec, sizeof(phd_trace_dyn_record)));
    if (dmaps) HIPCHK(pull(dmaps, T.d_dsnap, (size_t)T.dsnap_cap * sizeof(phd_gaussian4d)));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PHD_OK;
}

int phd_trace_shape_dynamic(phd_ctx* ctx, int* dyn_snapshot_cap) {
    if (!ctx) return fail(PHD_E_ARG, "null ctx");
    if (dyn_snapshot_cap) *dyn_snapshot_cap = ctx->tr.dsnap_cap;
    return PHD_OK;
}

int phd_trace_shape(phd_ctx* ctx, int* capacity, int* map_snapshot_cap, int* card_k) {
    if (!ctx) return fail(PHD_E_ARG, "null ctx");
    if (capacity) *capacity = ctx->tr.cap;
    if (map_snapshot_cap) *map_snapshot_cap = ctx->tr.snap_cap;
    if (card_k) *card_k = ctx->tr.d_card ? ctx->tr.K : 0;
    return PHD_OK;
}

int phd_trace_shard_block_bytes(int n, int map_snapshot_cap, int K, size_t* bytes) {
    if (n < 1 || map_snapshot_cap < 0 || K < 0 || !bytes) return fail(PHD_E_ARG, "bad arguments to phd_trace_shard_block_bytes");
    *bytes = trace_block_words(n, map_snapshot_cap, K) * sizeof(float);
    return PHD_OK;
}

int phd_trace_shard_block_bytes_mixed(int n, int map_snapshot_cap, int dyn_snapshot_cap, size_t* bytes) {
    if (n < 1 || map_snapshot_cap < 0 || dyn_snapshot_cap < 0 || !bytes)
        return fail(PHD_E_ARG, "bad arguments to phd_trace_shard_block_bytes_mixed");
    *bytes = trace_block_words_mixed(n, map_snapshot_cap, dyn_snapshot_cap) * sizeof(float);
    return PHD_OK;
}

}  // extern "C"

/* the arguments the three stages of a sharded trace share; a mixed trace's
 * carry the dynamic sets (the one current after the update and set X) too */
static TraceShardArgs trace_shard_args(phd_ctx* ctx, const float* dev_w_all, int world, int rank) {
    auto& T = ctx->tr;
    const size_t slot = (size_t)(T.count % T.cap);
    TraceShardArgs a{};
    a.w_all = dev_w_all;
    a.world = world;
    a.rank = rank;
    a.pose = ctx->st.d_pose;
    a.src = ctx->st.d_src;
    a.map_in = ctx->st.d_map[ctx->st.cur];
    a.size_in = ctx->st.d_size[ctx->st.cur];
    a.map_x = ctx->st.d_map_x;
    a.size_x = ctx->st.d_size_x;
    a.n = ctx->n;
    a.cap = ctx->cap.map_capacity;
    a.M = ctx->z.M;
    a.has_meas = rs_mode(ctx);
    a.resample_thresh = ctx->cfg.resampleThresh;
    a.err = ctx->d_err;
    a.hand = T.d_hand;
    a.snap_cap = T.snap_cap;
    a.K = T.d_card ? T.K : 0;
    a.block_words = trace_block_words(ctx->n, a.snap_cap, a.K);
    a.rec = T.d_rec + slot;
    a.snap = T.d_snap ? T.d_snap + slot * (size_t)T.snap_cap : nullptr;
    a.card = T.d_card ? T.d_card + slot * (size_t)T.K : nullptr;
    if (T.mixed) {
        a.dmap = ctx->mx.d_dmap[ctx->mx.dcur];
        a.dsize = ctx->mx.d_dsize[ctx->mx.dcur];
        a.dmap_x = ctx->mx.d_dmap_x;
        a.dsize_x = ctx->mx.d_dsize_x;
        a.dcap = ctx->mx.dcap;
        a.dsnap_cap = T.dsnap_cap;
        a.block_words = trace_block_words_mixed(ctx->n, a.snap_cap, a.dsnap_cap);
        a.drec = T.d_drec + slot;
        a.dsnap = T.d_dsnap ? T.d_dsnap + slot * (size_t)T.dsnap_cap : nullptr;
    }
    return a;
}

/* mixed: the call is one of the _mixed pair, which serves a trace enabled by
 * phd_trace_enable_mixed and no other; the static pair the other way round */
static int trace_shard_check(phd_ctx* ctx, const void* dev_w_all, const void* dev_block, int world, int rank,
                             const char* who, bool mixed) {
    if (!ctx || !dev_w_all || !dev_block || world < 1 || world > 1024 || rank < 0 || rank >= world ||
        (long long)world * ctx->n > (long long)RS_MAX_CHUNKS * RS_THREADS)
        return fail(PHD_E_ARG, std::string("bad arguments to ") + who);
    if (!ctx->cfg_set || ctx->tr.cap <= 0)
        return fail(PHD_E_ARG, mixed ? "the mixed estimate trace is off (phd_trace_enable_mixed)"
                                     : "the estimate trace is off (phd_trace_enable)");
    if (ctx->tr.mixed && !mixed)
        return fail(PHD_E_UNSUPPORTED, std::string(who) + ": a mixed trace (phd_trace_enable_mixed) — the sharded step "
                                       "of feature_model 2 is traced by phd_trace_shard_pack_mixed / _append_mixed");
    if (!ctx->tr.mixed && mixed)
        return fail(PHD_E_ARG, std::string(who) + ": the trace was enabled by phd_trace_enable (a static trace: "
                               "phd_trace_shard_pack / _append); the mixed calls need phd_trace_enable_mixed");
    return PHD_OK;
}

static int trace_shard_pack(phd_ctx* ctx, const float* dev_w_all, int world, int rank, uint64_t step, void* dev_block,
                            const char* who, bool mixed) {
    int rc = trace_shard_check(ctx, dev_w_all, dev_block, world, rank, who, mixed);
    if (rc) return rc;
    rc = trace_supported(ctx, TRACE_SHARDED);
    if (rc) return rc;
    if (ctx->tr.shard_packed)
        return fail(PHD_E_ARG, mixed ? "phd_trace_shard_append_mixed the previous block first"
                                     : "phd_trace_shard_append the previous block first");
    if (mixed && ctx->st.d_map_x && !ctx->mx.d_dmap_x)  // (static records received before phd_enable_dynamic)
        return fail(PHD_E_ARG, std::string(who) + ": migrated particles without dynamic maps (phd_enable_dynamic comes first)");
    if (set_device(ctx)) return PHD_E_HIP;
    auto& T = ctx->tr;
    if (ctx->sh.stream) {
        // the caller gathered dev_w_all on the plan stream (beside part C): the
        // trace runs on the context stream, after the update and after that gather
        if (!ctx->tr.ev_trace && ctx->tr.ev_trace.create(kEvOrder)) return PHD_E_HIP;
        HIPCHK(hipEventRecord(ctx->tr.ev_trace, ctx->sh.stream));
        HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->tr.ev_trace, 0));
    }
    TraceShardArgs a = trace_shard_args(ctx, dev_w_all, world, rank);
    a.step = step;
    a.block = (float*)dev_block;
    trace_launch_shard_weights(a, ctx->stream);
    if (T.d_card && ctx->cn.valid) {  // the arg-max particle's row, where this rank owns it (stage 1 left its slab)
        hipLaunchKernelGGL(k_cphd_cardinality, dim3(1), dim3(256), 0, ctx->stream,
                           (const int*)(T.d_hand + TRACE_H_SLAB), (const double*)ctx->cn.d_coef,
                           (const double*)ctx->cn.d_x, ctx->cn.stride, ctx->cn.d_lfact, T.K - 1, 1, T.d_card_row);
        a.card_row = T.d_card_row;
    }
    trace_launch_shard_pack(a, ctx->stream);
    HIPCHK(hipGetLastError());
    T.shard_packed = true;
    return PHD_OK;
}

static int trace_shard_append(phd_ctx* ctx, const float* dev_w_all, const void* dev_blocks_all, int world, int rank,
                              const char* who, bool mixed) {
    int rc = trace_shard_check(ctx, dev_w_all, dev_blocks_all, world, rank, who, mixed);
    if (rc) return rc;
    if (!ctx->tr.shard_packed)
        return fail(PHD_E_ARG, mixed ? "phd_trace_shard_append_mixed without phd_trace_shard_pack_mixed"
                                     : "phd_trace_shard_append without phd_trace_shard_pack");
    if (set_device(ctx)) return PHD_E_HIP;
    TraceShardArgs a = trace_shard_args(ctx, dev_w_all, world, rank);
    a.blocks = (const float*)dev_blocks_all;
    trace_launch_shard_finish(a, ctx->stream);
    HIPCHK(hipGetLastError());
    ctx->tr.shard_packed = false;
    ctx->tr.count++;
    return PHD_OK;
}

extern "C" {

int phd_trace_shard_pack(phd_ctx* ctx, const float* dev_w_all, int world, int rank, uint64_t step, void* dev_block) {
    return trace_shard_pack(ctx, dev_w_all, world, rank, step, dev_block, "phd_trace_shard_pack", false);
}

int phd_trace_shard_append(phd_ctx* ctx, const float* dev_w_all, const void* dev_blocks_all, int world, int rank) {
    return trace_shard_append(ctx, dev_w_all, dev_blocks_all, world, rank, "phd_trace_shard_append", false);
}

int phd_trace_shard_pack_mixed(phd_ctx* ctx, const float* dev_w_all, int world, int rank, uint64_t step,
                               void* dev_block) {
    return trace_shard_pack(ctx, dev_w_all, world, rank, step, dev_block, "phd_trace_shard_pack_mixed", true);
}

int phd_trace_shard_append_mixed(phd_ctx* ctx, const float* dev_w_all, const void* dev_blocks_all, int world,
                                 int rank) {
    return trace_shard_append(ctx, dev_w_all, dev_blocks_all, world, rank, "phd_trace_shard_append_mixed", true);
}

}  // extern "C"
