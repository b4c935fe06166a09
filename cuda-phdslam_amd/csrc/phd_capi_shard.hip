/*
 * phd_capi_shard.hip — the sharded (multi-GPU) step of the C-ABI: the global
 * and the sharded resample, the sync-free plan with its poll, the receives into
 * set X, pack / unpack of migration records, the log-weight copies.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "phd_ctx.h"
#include "phd_records.h"

using namespace phd;

/* migration slab set X (+ its cardinality rows), allocated on first receive */
static int ensure_x(phd_ctx* c) {
    if (!c->st.d_map_x) {
        if (c->st.d_map_x.alloc((size_t)c->n * 7 * c->cap.map_capacity) || c->st.d_size_x.alloc(c->n)) return PHD_E_HIP;
        HIPCHK(hipMemsetAsync(c->st.d_size_x, 0, c->n * sizeof(int), c->stream));
    }
    if (rec_cn_stride(c) && c->cn.d_x.ensure((size_t)c->n * c->cn.stride)) return PHD_E_HIP;
    if (rec_dcap(c)) {  // mixed: the dynamic twin; from here on references may name it
        if (ensure_dyn_x(c)) return PHD_E_HIP;
        c->mx.x_live = true;
    }
    return ensure_cn(c);
}

int ensure_dyn_x(phd_ctx* c) {
    if (c->mx.d_dmap_x) return PHD_OK;
    if (c->mx.d_dmap_x.alloc((size_t)c->n * PHD_DYN_FIELDS * c->mx.dcap) || c->mx.d_dsize_x.alloc(c->n)) return PHD_E_HIP;
    HIPCHK(hipMemsetAsync(c->mx.d_dsize_x, 0, c->n * sizeof(int), c->stream));
    return PHD_OK;
}

/* The record kernels (phd_records.hip) see the store through this, as it is
 * when the launch is enqueued. */
static RecordStore record_store(const phd_ctx* c) {
    RecordStore S;
    S.cap = c->cap.map_capacity;
    S.cn_stride = rec_cn_stride(c);
    S.dcap = rec_dcap(c);
    S.src = c->st.d_src;
    S.map_in = c->st.d_map[c->st.cur];
    S.size_in = c->st.d_size[c->st.cur];
    S.map_x = c->st.d_map_x;
    S.size_x = c->st.d_size_x;
    S.cn = c->cn.d_coef;
    S.cn_x = c->cn.d_x;
    S.dmap_in = c->mx.d_dmap[c->mx.dcur];
    S.dsize_in = c->mx.d_dsize[c->mx.dcur];
    S.dmap_x = c->mx.d_dmap_x;
    S.dsize_x = c->mx.d_dsize_x;
    S.pose = c->st.d_pose;
    S.logw = c->st.d_logw;
    return S;
}

/* What is refused of a sharded resample, whatever its form.  The mixed model
 * (feature_model 2, PHD) takes part once phd_enable_dynamic was called. */
static int shard_supported(const phd_ctx* ctx) {
    if (ctx->cfg.nPredictParticles > 1 || ctx->n != ctx->n_base)
        return fail(PHD_E_UNSUPPORTED, "sharded resample with n_predict_particles > 1 (shards hold n_particles each)");
    if (ctx->cfg.featureModel == PHD_FEATURE_MIXED) {
        if (ctx->cfg.filterType != PHD_FILTER_PHD) return fail(PHD_E_UNSUPPORTED, "feature_model 2 with the CPHD filter");
        if (!ctx->mx.on) return fail(PHD_E_ARG, "feature_model 2 needs phd_enable_dynamic");
    } else if (ctx->cfg.featureModel != PHD_FEATURE_STATIC) {
        return fail(PHD_E_UNSUPPORTED, "sharded resample with feature_model != 0");
    }
    return PHD_OK;
}

/* The caller sized its record buffers by phd_record_bytes: a mixed record of
 * another dynamic capacity than it last returned would not fit them. */
static int record_size_known(const phd_ctx* ctx) {
    if (rec_dcap(ctx) && rec_dcap(ctx) != ctx->sh.rec_dcap)
        return fail(PHD_E_ARG, "the record size changed (feature_model 2: dynamic capacity " +
                                   std::to_string(rec_dcap(ctx)) + ", phd_record_bytes last reported " +
                                   std::to_string(ctx->sh.rec_dcap) +
                                   "): call phd_enable_dynamic first, then size the record buffers by phd_record_bytes");
    return PHD_OK;
}

extern "C" {

__global__ void k_fill(float* a, int n, float v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = v;
}

int phd_set_index_offset(phd_ctx* ctx, int offset) {
    if (!ctx || offset < 0) return fail(PHD_E_ARG, "bad arguments");
    ctx->index_offset = offset;
    return PHD_OK;
}

int phd_fill_log_weights(phd_ctx* ctx, float value) {
    if (!ctx) return fail(PHD_E_ARG, "null ctx");
    if (set_device(ctx)) return PHD_E_HIP;
    hipLaunchKernelGGL(k_fill, dim3((ctx->n + 255) / 256), dim3(256), 0, ctx->stream, ctx->st.d_logw, ctx->n, value);
    HIPCHK(hipGetLastError());
    return PHD_OK;
}

int phd_global_resample(phd_ctx* ctx, float* dev_w_all, int n_total, int offset, uint64_t seed, uint64_t step,
                        int* dev_parents, float* neff, int* resampled) {
    if (!ctx || !dev_w_all || !dev_parents || n_total < ctx->n || offset < 0 || offset + ctx->n > n_total)
        return fail(PHD_E_ARG, "bad arguments to phd_global_resample");
    if (int rc0 = shard_supported(ctx)) return rc0;
    if (set_device(ctx)) return PHD_E_HIP;
    if (ctx->rs.d_cdf_g.ensure(n_total)) return PHD_E_HIP;
    float* out = ctx->d_out + 40;
    hipLaunchKernelGGL(k_normalize, dim3(1), dim3(1024), 0, ctx->stream, dev_w_all, n_total, (const float*)nullptr, out,
                       ctx->cfg.resampleThresh, ctx->z.M > 0 ? 1 : 0);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(ctx->st.d_logw, dev_w_all + offset, ctx->n * sizeof(float), hipMemcpyDeviceToDevice,
                          ctx->stream));
    const float neglogn = (float)(-std::log((double)n_total));
    hipLaunchKernelGGL(k_resample, dim3(1), dim3(1024), rs_lds(n_total), ctx->stream, (const int*)(out + 2), dev_w_all, dev_w_all,
                       n_total, n_total, (const double*)nullptr, seed, step, ctx->rs.d_cdf_g, dev_parents, (phd_pose*)nullptr,
                       (int*)nullptr, (phd_pose*)nullptr, (int*)nullptr, neglogn);
    HIPCHK(hipGetLastError());
    float h[3];
    HIPCHK(hipMemcpyAsync(h, out, 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (neff) *neff = h[1];
    if (resampled) memcpy(resampled, &h[2], sizeof(int));
    return PHD_OK;
}

}  // extern "C"

/* plan buffers of a sharded step for `world` ranks (device + pinned read-back) */
static int ensure_mig(phd_ctx* ctx, int world) {
    const size_t words = (size_t)(3 * world + MIG_TAIL);
    if (ctx->sh.d_mig.ensure(words)) return PHD_E_HIP;
    if (ctx->sh.h_mig.bytes() < words * sizeof(int)) {  // host-mapped, coherent: the tail writes the plan's counts into it (no copy launch)
        ctx->sh.h_mig_dev = nullptr;
        if (ctx->sh.h_mig.alloc(words, hipHostMallocMapped | hipHostMallocCoherent)) return PHD_E_HIP;
        HIPCHK(hipHostGetDevicePointer((void**)&ctx->sh.h_mig_dev, ctx->sh.h_mig, 0));
        memset(ctx->sh.h_mig, 0, ctx->sh.h_mig.bytes());
        ctx->sh.seq = 0;
        ctx->sh.h_mig_world = world;
    }
    if (ctx->sh.h_mig_world != world) {
        // the poll's sequence word sits at 3 world + MIG_SEQ: under another world
        // that slot held a count of an earlier plan, which could equal the next
        // sequence number — clear the buffer once the earlier plans are done
        HIPCHK(hipStreamSynchronize(ctx->stream));
        memset(ctx->sh.h_mig, 0, ctx->sh.h_mig.bytes());
        ctx->sh.h_mig_world = world;
    }
    if (ctx->sh.d_pend.ensure(ctx->n)) return PHD_E_HIP;
    if (ensure_sync(ctx)) return PHD_E_HIP;
    if (!ctx->sh.max_blocks) {
        int per_cu = 0, ncu = 0;
        HIPCHK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)k_shard_plan, RS_THREADS, 0));
        HIPCHK(hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, ctx->device));
        // one workgroup per CU whatever the query says beyond that: the query can
        // be one high, and a grid that is not resident at once would stall its waits
        ctx->sh.max_blocks = per_cu > 0 ? std::max(ncu, 1) : -1;
    }
    return PHD_OK;
}

/* The sharded plan (global normalise / nEff / decision / parents, then this
 * rank's migration plan and remap): one k_shard_plan launch when its
 * ceil(N/1024) workgroups can all be resident (every config here: <= 256), else
 * the k_rs_* chain + k_shard_tail; on stream st. */
static int launch_shard_plan(phd_ctx* ctx, hipStream_t st, float* dev_w_all, int world, int rank, uint64_t seed,
                             uint64_t step, int* dev_parents, int* dev_keep_src, int* dev_send_src, int* dev_recv_rec,
                             float new_log_weight, int block_records, bool chain = false, bool with_src = true) {
    const int n_total = world * ctx->n;
    const int B = (n_total + RS_THREADS - 1) / RS_THREADS;
    float* out = ctx->d_out + 40;
    const int* src = with_src ? (const int*)ctx->st.d_src : nullptr;  // (NULL: the identity)
    if (!chain && B <= ctx->sh.max_blocks) {
        RsParts P;
        int rc = rs_parts(ctx, n_total, P);
        if (rc) return rc;
        ShardPlanArgs a;
        a.w = dev_w_all;
        a.N = n_total;
        a.B = B;
        a.n = ctx->n;
        a.world = world;
        a.rank = rank;
        a.has_meas = ctx->z.M > 0 ? 1 : 0;
        a.block_records = block_records;
        a.resample_thresh = ctx->cfg.resampleThresh;
        a.new_logw = new_log_weight;
        a.seed = seed;
        a.step = step;
        a.part_sum = P.part_sum;
        a.part_s2 = P.part_s2;
        a.cdf_rel = P.cdf_rel;
        a.part_tot = P.part_tot;
        a.part_key = P.part_key;
        a.sync = ctx->rs.d_sync;
        a.out = out;
        a.parents = dev_parents;
        a.mig = ctx->sh.d_mig;
        a.mig_host = ctx->sh.h_mig_dev;
        a.stamps = ctx->d_stamps;  // (allocated by phd_debug_stamps only)
        a.seq = ++ctx->sh.seq;
        a.keep_src = dev_keep_src;
        a.send_src = dev_send_src;
        a.recv_rec = dev_recv_rec;
        a.pending = ctx->sh.d_pend;
        a.pose = ctx->st.d_pose;
        a.src = src;
        a.new_pose = ctx->st.d_tmp_pose;
        a.new_src = ctx->st.d_tmp_src;
        a.logw_local = ctx->st.d_logw;
        hipLaunchKernelGGL(k_shard_plan, dim3(B), dim3(RS_THREADS), 0, st, a);
        HIPCHK(hipGetLastError());
        return PHD_OK;
    }
    int rc = launch_rs_chunks(ctx, st, dev_w_all, n_total, out, seed, step, dev_parents, false, 0.f, false,
                              ctx->rs.d_sync + PLAN_BEYOND);
    if (rc) return rc;
    hipLaunchKernelGGL(k_shard_tail, dim3(1), dim3(RS_THREADS), 0, st, (const float*)dev_w_all, ctx->n,
                       world, rank, (const float*)out, (const int*)dev_parents, ctx->rs.d_sync, ctx->sh.d_mig,
                       ctx->sh.h_mig_dev, dev_keep_src, dev_send_src, dev_recv_rec, (const phd_pose*)ctx->st.d_pose, src,
                       ctx->st.d_tmp_pose, ctx->st.d_tmp_src, ctx->st.d_logw, new_log_weight, block_records, ctx->sh.d_pend,
                       ++ctx->sh.seq);
    HIPCHK(hipGetLastError());
    return PHD_OK;
}

extern "C" {

int phd_shard_resample(phd_ctx* ctx, float* dev_w_all, int world, int rank, uint64_t seed, uint64_t step,
                       int* dev_parents, int* dev_keep_src, int* dev_send_src, int* dev_recv_rec,
                       void* dev_send_records, int send_capacity, float new_log_weight, int* demand,
                       int* send_records, int* recv_records, float* neff, int* resampled) {
    if (!ctx || !dev_w_all || !dev_parents || !dev_keep_src || !dev_send_src || !dev_recv_rec || !demand ||
        !send_records || !recv_records || world < 1 || world > 1024 || rank < 0 || rank >= world ||
        (long long)world * ctx->n > (long long)RS_MAX_CHUNKS * RS_THREADS || send_capacity < 0 || (send_capacity > 0 && !dev_send_records))
        return fail(PHD_E_ARG, "bad arguments to phd_shard_resample");
    if (int rc0 = shard_supported(ctx)) return rc0;
    if (send_capacity > 0)
        if (int rc0 = record_size_known(ctx)) return rc0;
    if (set_device(ctx)) return PHD_E_HIP;
    const int n_total = world * ctx->n;
    if (ensure_mig(ctx, world)) return PHD_E_HIP;
    // the global part and this rank's plan (k_shard_plan, or the k_rs_* chain + k_shard_tail)
    int rc = launch_shard_plan(ctx, ctx->stream, dev_w_all, world, rank, seed, step, dev_parents, dev_keep_src,
                               dev_send_src, dev_recv_rec, new_log_weight, ctx->n);
    if (rc) return rc;
    if (send_capacity > 0) {
        if (ensure_cn(ctx)) return PHD_E_HIP;
        // records this rank sends (count on the device) from the pre-resample
        // store; they carry the new log-weight
        HIPCHK(records_pack(record_store(ctx), std::min(send_capacity, 256), (const int*)(ctx->sh.d_mig + 3 * world),
                            (const int*)dev_send_src, send_capacity, 1, new_log_weight, (float*)dev_send_records,
                            ctx->stream));
    }
    int* h = ctx->sh.h_mig;  // (written by the plan's tail)
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (h[3 * world + MIG_TIMEOUT])
        return fail(PHD_E_HIP, "phd_shard_resample: the one-launch plan lost residency (a wait timed out)");
    float o[2];
    memcpy(o, h + 3 * world + MIG_LSE, sizeof(o));
    const int flag = h[3 * world + MIG_FLAG];
    if (flag) {  // the remapped poses / slab references become the store
        std::swap(ctx->st.d_pose, ctx->st.d_tmp_pose);
        std::swap(ctx->st.d_src, ctx->st.d_tmp_src);
        ctx->st.src_fresh = false;
    }
    if (neff) *neff = o[1];
    if (resampled) *resampled = flag;
    memcpy(demand, h, world * sizeof(int));
    memcpy(send_records, h + world, world * sizeof(int));
    memcpy(recv_records, h + 2 * world, world * sizeof(int));
    if (h[3 * world] > send_capacity)
        return fail(PHD_E_CAPACITY, "phd_shard_resample: send buffer smaller than this rank's surplus records");
    return PHD_OK;
}

/* Sync-free sharded plan (see phd_capi.h). */
int phd_shard_resample_async(phd_ctx* ctx, float* dev_w_all, int world, int rank, uint64_t seed, uint64_t step,
                             int* dev_parents, int* dev_keep_src, int* dev_send_src, int* dev_recv_rec,
                             void* dev_send_blocks, int block_records, void* dev_overflow, int overflow_capacity,
                             float new_log_weight) {
    if (!ctx || !dev_w_all || !dev_parents || !dev_keep_src || !dev_send_src || !dev_recv_rec || world < 1 ||
        world > 1024 || rank < 0 || rank >= world || block_records < 0 || overflow_capacity < 0 ||
        (long long)world * ctx->n > (long long)RS_MAX_CHUNKS * RS_THREADS ||
        (world > 1 && block_records > 0 && !dev_send_blocks) || (overflow_capacity > 0 && !dev_overflow))
        return fail(PHD_E_ARG, "bad arguments to phd_shard_resample_async");
    if (ctx->sh.open) return fail(PHD_E_ARG, "phd_shard_poll the previous plan first");
    if (int rc0 = shard_supported(ctx)) return rc0;
    if (int rc0 = record_size_known(ctx)) return rc0;  // (before anything is enqueued: nothing is written)
    if (set_device(ctx)) return PHD_E_HIP;
    if (ensure_mig(ctx, world)) return PHD_E_HIP;
    if (ensure_cn(ctx)) return PHD_E_HIP;
    int rc;
    if (ctx->sh.stream) {
        // the plan beside part C (phd_set_plan_stream): on the plan stream, after
        // the caller's all-gather there (which waited for phd_wait_logw); with
        // every slab reference the identity (the step's update resets them) it
        // reads none (src NULL), so part C may still be writing them.  The launch
        // chain, not the one-launch plan: its workgroups need not be resident at
        // once beside part C's, and its latency is hidden.  The pack, which reads
        // the posterior maps, waits for it on the context stream.
        if (!ctx->sh.ev_plan && ctx->sh.ev_plan.create(kEvOrder)) return PHD_E_HIP;
        // (no update since the last remap: after the whole stream; a traced step:
        // after its trace, which reads dev_w_all before the plan normalises it in place)
        if (!ctx->st.src_fresh || ctx->tr.cap > 0) {
            HIPCHK(hipEventRecord(ctx->sh.ev_plan, ctx->stream));
            HIPCHK(hipStreamWaitEvent(ctx->sh.stream, ctx->sh.ev_plan, 0));
        }
        rc = launch_shard_plan(ctx, ctx->sh.stream, dev_w_all, world, rank, seed, step, dev_parents, dev_keep_src,
                               dev_send_src, dev_recv_rec, new_log_weight, block_records, true, !ctx->st.src_fresh);
        if (rc) return rc;
        if (PHD_PLAN_WAIT_KERNEL) {
            // the pack / the next step wait for the plan inside the context
            // stream (k_wait_plan polls the tail's sequence word), not through
            // a cross-stream event (its barrier packet: ~15 us of idle stream)
            hipLaunchKernelGGL(k_wait_plan, dim3(1), dim3(64), 0, ctx->stream,
                               (const int*)(ctx->sh.h_mig_dev + 3 * world + MIG_SEQ), ctx->sh.seq,
                               ctx->rs.d_sync + PLAN_TIMEOUT);
            HIPCHK(hipGetLastError());
        } else {
            HIPCHK(hipEventRecord(ctx->sh.ev_plan, ctx->sh.stream));
            HIPCHK(hipStreamWaitEvent(ctx->stream, ctx->sh.ev_plan, 0));
        }
    } else {
        rc = launch_shard_plan(ctx, ctx->stream, dev_w_all, world, rank, seed, step, dev_parents, dev_keep_src,
                               dev_send_src, dev_recv_rec, new_log_weight, block_records);
        if (rc) return rc;
    }
    if (world > 1)  // records from the pre-resample store (the pointers are swapped below)
        HIPCHK(records_pack_blocks(record_store(ctx), std::min(ctx->n, 256), (const int*)ctx->sh.d_mig, world,
                                   (const int*)dev_send_src, block_records, overflow_capacity, new_log_weight,
                                   (float*)dev_send_blocks, (float*)dev_overflow,
                                   ctx->sh.h_mig_dev + 3 * world + MIG_OVF_CAP, ctx->stream));
    // the tail wrote the remapped store (the identity without a resample): swap it in
    std::swap(ctx->st.d_pose, ctx->st.d_tmp_pose);
    std::swap(ctx->st.d_src, ctx->st.d_tmp_src);
    ctx->st.src_fresh = false;
    // (the counts reach h_mig from the tail directly; the host polls the plan's
    // sequence number there: no event record, whose system-scope release would
    // cost the stream a gap)
    ctx->sh.ovf_cap = overflow_capacity;
    ctx->sh.open = true;
    ctx->sh.world = world;
    ctx->sh.rank = rank;
    return PHD_OK;
}

int phd_wait_logw(phd_ctx* ctx, void* stream) {
    if (!ctx || !stream) return fail(PHD_E_ARG, "bad arguments to phd_wait_logw");
    if (set_device(ctx)) return PHD_E_HIP;
    if (!ctx->sh.ev_logw) {
        // first call: from here on every update marks its log-weights final;
        // until one has, the whole stream
        if (ctx->sh.ev_logw.create(kEvOrder)) return PHD_E_HIP;
        HIPCHK(hipEventRecord(ctx->sh.ev_logw, ctx->stream));
    }
    HIPCHK(hipStreamWaitEvent((hipStream_t)stream, ctx->sh.ev_logw, 0));
    return PHD_OK;
}

int phd_set_plan_stream(phd_ctx* ctx, void* stream) {
    if (!ctx) return fail(PHD_E_ARG, "null ctx");
    if (set_device(ctx)) return PHD_E_HIP;
    if (stream && !ctx->sh.ev_logw) {
        if (ctx->sh.ev_logw.create(kEvOrder)) return PHD_E_HIP;
        HIPCHK(hipEventRecord(ctx->sh.ev_logw, ctx->stream));
    }
    ctx->sh.stream = (hipStream_t)stream;
    return PHD_OK;
}

int phd_shard_receive_blocks(phd_ctx* ctx, const void* dev_recv_blocks, int block_records, const int* dev_recv_rec) {
    if (!ctx || !dev_recv_rec || block_records < 0 || (block_records > 0 && !dev_recv_blocks) || !ctx->sh.world)
        return fail(PHD_E_ARG, "bad arguments to phd_shard_receive_blocks");
    if (set_device(ctx)) return PHD_E_HIP;
    if (int rc0 = record_size_known(ctx)) return rc0;
    if (ensure_x(ctx)) return PHD_E_HIP;
    ctx->st.src_fresh = false;
    HIPCHK(records_unpack_blocks(record_store(ctx), std::min(ctx->n, 256), (const float*)dev_recv_blocks,
                                 (const float*)nullptr, block_records, 0, (const int*)ctx->sh.d_mig, ctx->sh.world,
                                 ctx->sh.rank, dev_recv_rec, ctx->n, ctx->stream));
    return PHD_OK;
}

int phd_shard_poll(phd_ctx* ctx, int* demand, int* send_records, int* recv_records, int* pending, float* neff,
                   int* resampled) {
    if (!ctx || !ctx->sh.open) return fail(PHD_E_ARG, "no sharded plan to poll");
    if (set_device(ctx)) return PHD_E_HIP;
    const int w = ctx->sh.world;
    const int* h = ctx->sh.h_mig;
    {
        // the plan's tail stores its sequence number last (system-scope release)
        const auto t0 = std::chrono::steady_clock::now();
        for (unsigned spin = 0;; spin++) {
            if ((unsigned)__atomic_load_n(h + 3 * w + MIG_SEQ, __ATOMIC_ACQUIRE) == ctx->sh.seq) break;
            if ((spin & 1023u) == 1023u) {
                const hipError_t q = hipStreamQuery(ctx->stream);
                if (q != hipSuccess && q != hipErrorNotReady) {
                    ctx->sh.open = false;
                    return fail(PHD_E_HIP, std::string("phd_shard_poll: ") + hipGetErrorString(q));
                }
                if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(60)) {
                    ctx->sh.open = false;
                    return fail(PHD_E_HIP, "phd_shard_poll: the plan did not complete within 60 s");
                }
            }
        }
    }
    ctx->sh.open = false;
    if (demand) memcpy(demand, h, w * sizeof(int));
    if (send_records) memcpy(send_records, h + w, w * sizeof(int));
    if (recv_records) memcpy(recv_records, h + 2 * w, w * sizeof(int));
    ctx->sh.pend_count = h[3 * w + MIG_PENDING];
    if (pending) *pending = ctx->sh.pend_count;
    if (neff) memcpy(neff, h + 3 * w + MIG_NEFF, sizeof(float));
    if (resampled) *resampled = h[3 * w + MIG_FLAG];
    if (h[3 * w + MIG_TIMEOUT])
        return fail(PHD_E_HIP, "phd_shard_resample_async: the one-launch plan lost residency (a wait timed out)");
    if (h[3 * w + MIG_OVF_SEND] > ctx->sh.ovf_cap)  // (what k_pack_blocks flags, from the counts)
        return fail(PHD_E_CAPACITY, "phd_shard_resample_async: overflow buffer smaller than the records beyond the blocks");
    return PHD_OK;
}

int phd_shard_receive_overflow(phd_ctx* ctx, const void* dev_recv_overflow, int block_records,
                               const int* dev_recv_rec) {
    if (!ctx || !dev_recv_rec || !ctx->sh.world || ctx->sh.open)
        return fail(PHD_E_ARG, "bad arguments to phd_shard_receive_overflow (poll the plan first)");
    if (ctx->sh.pend_count == 0) return PHD_OK;
    if (!dev_recv_overflow) return fail(PHD_E_ARG, "phd_shard_receive_overflow: pending slots need the records");
    if (set_device(ctx)) return PHD_E_HIP;
    if (int rc0 = record_size_known(ctx)) return rc0;
    ctx->st.src_fresh = false;
    if (ensure_x(ctx)) return PHD_E_HIP;  // (the sets X exist since the blocks' receive; mixed: marks them live again)
    HIPCHK(records_unpack_blocks(record_store(ctx), std::min(ctx->n, 256), (const float*)nullptr,
                                 (const float*)dev_recv_overflow, block_records, 1, (const int*)ctx->sh.d_mig,
                                 ctx->sh.world, ctx->sh.rank, dev_recv_rec, ctx->n, ctx->stream));
    return PHD_OK;
}

int phd_update_pending(phd_ctx* ctx, const phd_ackerman_control* u, int do_predict, uint64_t step,
                       float* dev_logw_out) {
    if (!ctx || !ctx->cfg_set) return fail(PHD_E_ARG, "bad arguments to phd_update_pending");
    if (ctx->sh.pend_count == 0) return PHD_OK;
    if (set_device(ctx)) return PHD_E_HIP;
    int rc = enqueue_predict_update(ctx, u, do_predict, step, ctx->sh.d_pend, ctx->sh.pend_count);
    if (rc) return rc;
    if (dev_logw_out)
        HIPCHK(hipMemcpyAsync(dev_logw_out, ctx->st.d_logw, ctx->n * sizeof(float), hipMemcpyDeviceToDevice,
                              ctx->stream));
    if (ctx->sh.ev_logw) HIPCHK(hipEventRecord(ctx->sh.ev_logw, ctx->stream));  // (the mirror is complete here)
    // the pending slots (the only references off the identity) were re-updated;
    // (mixed: its update does not keep this flag, the plan always reads the references)
    if (ctx->cfg.featureModel == PHD_FEATURE_STATIC) ctx->st.src_fresh = true;
    return PHD_OK;
}

int phd_shard_receive(phd_ctx* ctx, const void* dev_records, const int* dev_recv_rec, int n_slots, int first_slot) {
    if (!ctx || n_slots < 0 || first_slot < 0 || first_slot + n_slots > ctx->n ||
        (n_slots > 0 && (!dev_records || !dev_recv_rec)))
        return fail(PHD_E_ARG, "bad arguments to phd_shard_receive");
    if (n_slots == 0) return PHD_OK;
    if (set_device(ctx)) return PHD_E_HIP;
    if (int rc0 = record_size_known(ctx)) return rc0;
    if (ensure_x(ctx)) return PHD_E_HIP;
    HIPCHK(records_unpack_slots(record_store(ctx), (const float*)dev_records, dev_recv_rec, n_slots, first_slot,
                                ctx->stream));
    return PHD_OK;
}

int phd_copy_log_weights(phd_ctx* ctx, float* dev_dst) {
    if (!ctx || !dev_dst) return fail(PHD_E_ARG, "null argument");
    if (set_device(ctx)) return PHD_E_HIP;
    HIPCHK(hipMemcpyAsync(dev_dst, ctx->st.d_logw, ctx->n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    return PHD_OK;
}

int phd_set_log_weights(phd_ctx* ctx, const float* dev_src) {
    if (!ctx || !dev_src) return fail(PHD_E_ARG, "null argument");
    if (set_device(ctx)) return PHD_E_HIP;
    HIPCHK(hipMemcpyAsync(ctx->st.d_logw, dev_src, ctx->n * sizeof(float), hipMemcpyDeviceToDevice, ctx->stream));
    return PHD_OK;
}

int phd_record_bytes(const phd_ctx* ctx, size_t* bytes) {
    if (!ctx || !bytes) return fail(PHD_E_ARG, "null argument");
    const int dcap = rec_dcap(ctx);
    *bytes = record_words_mixed(ctx->cap.map_capacity, rec_cn_stride(ctx), dcap) * sizeof(float);
    // what the caller now sizes its buffers for (record_size_known); not part of the filter's state
    const_cast<phd_ctx*>(ctx)->sh.rec_dcap = dcap;
    return PHD_OK;
}

int phd_record_layout_bytes(int map_capacity, int cn_stride, int dyn_capacity, size_t* bytes) {
    if (map_capacity < 0 || cn_stride < 0 || dyn_capacity < 0 || !bytes)
        return fail(PHD_E_ARG, "bad arguments to phd_record_layout_bytes");
    *bytes = record_words_mixed(map_capacity, cn_stride, dyn_capacity) * sizeof(float);
    return PHD_OK;
}

int phd_pack_particles(phd_ctx* ctx, const int* dev_src_idx, int count, void* dev_records) {
    if (!ctx || (count > 0 && (!dev_src_idx || !dev_records))) return fail(PHD_E_ARG, "bad arguments");
    if (count <= 0) return PHD_OK;
    if (set_device(ctx)) return PHD_E_HIP;
    if (int rc0 = record_size_known(ctx)) return rc0;
    if (ensure_cn(ctx)) return PHD_E_HIP;
    HIPCHK(records_pack(record_store(ctx), count, (const int*)nullptr, dev_src_idx, count, 0, 0.f, (float*)dev_records,
                        ctx->stream));
    return PHD_OK;
}

int phd_unpack_particles(phd_ctx* ctx, const void* dev_records, const int* dev_dst_idx, int count) {
    if (!ctx || (count > 0 && (!dev_dst_idx || !dev_records))) return fail(PHD_E_ARG, "bad arguments");
    if (count <= 0) return PHD_OK;
    if (count > ctx->n) return fail(PHD_E_ARG, "more migrants than particles");
    if (set_device(ctx)) return PHD_E_HIP;
    if (int rc0 = record_size_known(ctx)) return rc0;
    if (ensure_x(ctx)) return PHD_E_HIP;
    HIPCHK(records_unpack(record_store(ctx), (const float*)dev_records, dev_dst_idx, count, ctx->stream));
    return PHD_OK;
}

}  // extern "C"
