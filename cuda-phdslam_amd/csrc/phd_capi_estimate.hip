/*
 * phd_capi_estimate.hip — estimates read from the store: expected pose, the
 * EAP expected map (static, dynamic, the sharded blocks of both), cardinalities,
 * LSE parts.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "phd_ctx.h"

using namespace phd;

extern "C" {

int phd_cardinality_distribution(phd_ctx* ctx, float* cn_host) {
    if (!ctx || !cn_host) return fail(PHD_E_ARG, "null argument");
    if (!ctx->cn.valid) return fail(PHD_E_ARG, "no CPHD update has run on this context");
    if (set_device(ctx)) return PHD_E_HIP;
    const int Nmax = ctx->cfg.maxCardinality;
    const size_t bytes = (size_t)ctx->n * (Nmax + 1) * sizeof(float);
    DevBuf<float> d;  // (released after the read-back below)
    if (d.alloc((size_t)ctx->n * (Nmax + 1))) return PHD_E_HIP;
    hipLaunchKernelGGL(k_cphd_cardinality, dim3(ctx->n), dim3(256), 0, ctx->stream, (const int*)ctx->st.d_src,
                       (const double*)ctx->cn.d_coef, (const double*)ctx->cn.d_x, ctx->cn.stride,
                       ctx->cn.d_lfact, Nmax, ctx->n, d);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(cn_host, d, bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(PHD_E_HIP, std::string("phd_cardinality_distribution: ") + hipGetErrorString(e));
    return PHD_OK;
}

int phd_expected_pose(phd_ctx* ctx, phd_pose* pose, int* map_particle) {
    if (!ctx) return fail(PHD_E_ARG, "null ctx");
    if (set_device(ctx)) return PHD_E_HIP;
    hipLaunchKernelGGL(k_expected_pose, dim3(1), dim3(1024), 0, ctx->stream, ctx->st.d_logw, ctx->st.d_pose, ctx->n,
                       ctx->d_out + 16);
    HIPCHK(hipGetLastError());
    float out[7];
    HIPCHK(hipMemcpyAsync(out, ctx->d_out + 16, 7 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (pose) memcpy(pose, out, sizeof(phd_pose));
    if (map_particle) memcpy(map_particle, &out[6], sizeof(int));
    return PHD_OK;
}

int phd_cardinalities(phd_ctx* ctx, float* cn_host) {
    if (!ctx || !cn_host) return fail(PHD_E_ARG, "null argument");
    if (set_device(ctx)) return PHD_E_HIP;
    hipLaunchKernelGGL(k_cardinality, dim3((ctx->n + 3) / 4), dim3(256), 0, ctx->stream, ctx->st.d_src,
                       ctx->st.d_map[ctx->st.cur], ctx->st.d_size[ctx->st.cur], ctx->st.d_map_x, ctx->st.d_size_x, ctx->n,
                       ctx->cap.map_capacity, ctx->d_cn);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(cn_host, ctx->d_cn, ctx->n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PHD_OK;
}

/* EAP expected map (computeExpectedMap main.cpp:290-316 + reduceGaussianMixture
 * gm_reduce.cpp:59-132) of the current store, on the device (phd_eap.hip). */
int phd_expected_map(phd_ctx* ctx, phd_gaussian2d* out, long out_cap, long* n_out) {
    if (!ctx || !n_out) return fail(PHD_E_ARG, "null argument");
    if (!ctx->cfg_set) return fail(PHD_E_ARG, "phd_set_config first");
    if (set_device(ctx)) return PHD_E_HIP;
    std::string err;
    const long nout = eap_run(&ctx->eap, ctx->stream, ctx->st.d_src, ctx->st.d_map[ctx->st.cur], ctx->st.d_size[ctx->st.cur],
                              ctx->st.d_map_x, ctx->st.d_size_x, ctx->st.d_logw, ctx->n, ctx->cap.map_capacity,
                              ctx->cfg.minSeparation, out, out ? out_cap : 0, &ctx->eap_groups, err);
    if (nout < 0) return fail(PHD_E_HIP, "expected map: " + err);
    *n_out = nout;
    if (nout > 0 && (!out || nout > out_cap))
        return fail(PHD_E_CAPACITY, "expected map has " + std::to_string(nout) + " components; out_cap too small");
    return PHD_OK;
}

/* EAP map of the dynamic maps (feature_model 2): recoverSlamState's
 * exp_map_dynamic (main.cpp:369-371) on the device (phd_mixed.hip). */
int phd_expected_map_dynamic(phd_ctx* ctx, phd_gaussian4d* out, long out_cap, long* n_out) {
    if (!ctx || !n_out) return fail(PHD_E_ARG, "null argument");
    if (!ctx->cfg_set) return fail(PHD_E_ARG, "phd_set_config first");
    if (!ctx->mx.on) return fail(PHD_E_ARG, "phd_enable_dynamic not called");
    if (set_device(ctx)) return PHD_E_HIP;
    std::string err;
    const long nout = mixed_expected_map_dynamic(ctx->stream, ctx->st.d_src, ctx->mx.d_dmap[ctx->mx.dcur],
                                                 ctx->mx.d_dsize[ctx->mx.dcur], ctx->mx.d_dmap_x, ctx->mx.d_dsize_x,
                                                 ctx->n, ctx->mx.dcap, ctx->st.d_logw,
                                                 ctx->cfg.minSeparation, out, out ? out_cap : 0, ctx->eap4_mode,
                                                 &ctx->eap4_rounds, &ctx->eap4_cells, err);
    if (nout < 0) return fail(PHD_E_HIP, "dynamic expected map: " + err);
    *n_out = nout;
    if (nout > 0 && (!out || nout > out_cap))
        return fail(PHD_E_CAPACITY, "dynamic expected map has " + std::to_string(nout) + " components; out_cap too small");
    return PHD_OK;
}

int phd_expected_map_groups(phd_ctx* ctx, int* groups) {
    if (!ctx || !groups) return fail(PHD_E_ARG, "null argument");
    *groups = ctx->eap_groups;
    return PHD_OK;
}

int phd_expected_map_dynamic_groups(phd_ctx* ctx, int* rounds, int* cells) {
    if (!ctx || !rounds || !cells) return fail(PHD_E_ARG, "null argument");
    *rounds = ctx->eap4_rounds;
    *cells = ctx->eap4_cells;
    return PHD_OK;
}

int phd_set_expected_map_dynamic_mode(phd_ctx* ctx, int mode) {
    if (!ctx || (mode != 0 && mode != 1)) return fail(PHD_E_ARG, "bad arguments to phd_set_expected_map_dynamic_mode");
    ctx->eap4_mode = mode;
    return PHD_OK;
}

/* ---- the EAP expected map of a sharded filter (phd_eap.hip: blocks) ---- */

static int eap_shard_check(phd_ctx* ctx, const char* who) {
    if (!ctx) return fail(PHD_E_ARG, std::string("null ctx in ") + who);
    if (!ctx->cfg_set) return fail(PHD_E_ARG, "phd_set_config first");
    // a mixed context's static maps live in the same slab sets and migration set as a
    // static context's: the pack and the reduce are the same
    const bool mixed = ctx->cfg.featureModel == PHD_FEATURE_MIXED && ctx->mx.on;
    if (ctx->cfg.featureModel != PHD_FEATURE_STATIC && !mixed)
        return fail(PHD_E_UNSUPPORTED, std::string(who) + " with feature_model != 0 (feature_model 2: after "
                                                          "phd_enable_dynamic only)");
    return PHD_OK;
}

/* world blocks of block_bytes each must lie inside the allocation dev_blocks
 * points into (where the runtime knows it): no header is read past the
 * caller's buffer */
static int blocks_fit(const void* dev_blocks, int world, long K_max, size_t block_bytes, const char* who) {
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, (hipDeviceptr_t)dev_blocks) == hipSuccess && base) {
        const size_t room = size - (size_t)((const char*)dev_blocks - (const char*)base);
        if ((size_t)world * block_bytes > room)
            return fail(PHD_E_ARG, std::string(who) + ": " + std::to_string(world) + " blocks of K_max " +
                                       std::to_string(K_max) + " do not fit the buffer (" + std::to_string(room) +
                                       " bytes from dev_blocks)");
    } else {
        (void)hipGetLastError();
    }
    return PHD_OK;
}

int phd_eap_shard_count(phd_ctx* ctx, long* K_local) {
    int rc = eap_shard_check(ctx, "phd_eap_shard_count");
    if (rc) return rc;
    if (!K_local) return fail(PHD_E_ARG, "null argument");
    if (set_device(ctx)) return PHD_E_HIP;
    std::string err;
    const long k = eap_shard_count(&ctx->eap, ctx->stream, ctx->st.d_src, ctx->st.d_size[ctx->st.cur], ctx->st.d_size_x, ctx->n, err);
    if (k < 0) return fail(PHD_E_HIP, "phd_eap_shard_count: " + err);
    *K_local = k;
    return PHD_OK;
}

int phd_eap_shard_block_bytes(long K_max, size_t* bytes) {
    if (K_max < 0 || !bytes) return fail(PHD_E_ARG, "bad arguments to phd_eap_shard_block_bytes");
    *bytes = eap_block_bytes(K_max);
    return PHD_OK;
}

int phd_eap_shard_pack(phd_ctx* ctx, long K_max, void* dev_block) {
    int rc = eap_shard_check(ctx, "phd_eap_shard_pack");
    if (rc) return rc;
    if (K_max < 0 || K_max >= (1L << 31) - 1 || !dev_block || ((uintptr_t)dev_block & 15))
        return fail(PHD_E_ARG, "bad arguments to phd_eap_shard_pack (K_max in [0, 2^31 - 1), a 16-byte aligned block)");
    if (set_device(ctx)) return PHD_E_HIP;
    std::string err;
    rc = eap_shard_pack(&ctx->eap, ctx->stream, ctx->st.d_src, ctx->st.d_map[ctx->st.cur], ctx->st.d_size[ctx->st.cur], ctx->st.d_map_x,
                        ctx->st.d_size_x, ctx->st.d_logw, ctx->n, ctx->cap.map_capacity, K_max, dev_block, err);
    if (rc == -2) return fail(PHD_E_ARG, "phd_eap_shard_pack: " + err);
    if (rc) return fail(PHD_E_HIP, "phd_eap_shard_pack: " + err);
    return PHD_OK;
}

int phd_expected_map_blocks(phd_ctx* ctx, const void* dev_blocks, int world, long K_max, phd_gaussian2d* out,
                            long out_cap, long* n_out) {
    int rc = eap_shard_check(ctx, "phd_expected_map_blocks");
    if (rc) return rc;
    if (!n_out || !dev_blocks || ((uintptr_t)dev_blocks & 15) || world < 1 || world > EAP_MAX_WORLD || K_max < 0 ||
        K_max >= (1L << 31) - 1)
        return fail(PHD_E_ARG, "bad arguments to phd_expected_map_blocks (world in [1, 1024], K_max in [0, 2^31 - 1), "
                               "16-byte aligned blocks)");
    if (set_device(ctx)) return PHD_E_HIP;
    rc = blocks_fit(dev_blocks, world, K_max, eap_block_bytes(K_max), "phd_expected_map_blocks");
    if (rc) return rc;
    std::string err;
    const long nout = eap_run_blocks(&ctx->eap, ctx->stream, dev_blocks, world, ctx->n, K_max, ctx->cfg.minSeparation,
                                     out, out ? out_cap : 0, &ctx->eap_groups, err);
    if (nout == -2) return fail(PHD_E_ARG, "phd_expected_map_blocks: " + err);
    if (nout < 0) return fail(PHD_E_HIP, "expected map: " + err);
    *n_out = nout;
    if (nout > 0 && (!out || nout > out_cap))
        return fail(PHD_E_CAPACITY, "expected map has " + std::to_string(nout) + " components; out_cap too small");
    return PHD_OK;
}

/* ---- the EAP map of the dynamic maps of a sharded mixed filter (phd_mixed.hip: blocks) ---- */

static int eap_dyn_check(phd_ctx* ctx, const char* who) {
    if (!ctx) return fail(PHD_E_ARG, std::string("null ctx in ") + who);
    if (!ctx->cfg_set) return fail(PHD_E_ARG, std::string(who) + ": phd_set_config first");
    if (!ctx->mx.on) return fail(PHD_E_ARG, std::string(who) + ": phd_enable_dynamic not called");
    return PHD_OK;
}

int phd_eap_dyn_shard_count(phd_ctx* ctx, long* K_local) {
    int rc = eap_dyn_check(ctx, "phd_eap_dyn_shard_count");
    if (rc) return rc;
    if (!K_local) return fail(PHD_E_ARG, "null argument");
    if (set_device(ctx)) return PHD_E_HIP;
    std::string err;
    const long k = eap4_shard_count(ctx->stream, ctx->st.d_src, ctx->mx.d_dsize[ctx->mx.dcur],
                                    ctx->mx.d_dsize_x, ctx->n, ctx->mx.dcap, err);
    if (k < 0) return fail(PHD_E_HIP, "phd_eap_dyn_shard_count: " + err);
    *K_local = k;
    return PHD_OK;
}

int phd_eap_dyn_shard_block_bytes(long K_max, size_t* bytes) {
    if (K_max < 0 || !bytes) return fail(PHD_E_ARG, "bad arguments to phd_eap_dyn_shard_block_bytes");
    *bytes = eap4_block_bytes(K_max);
    return PHD_OK;
}

int phd_eap_dyn_shard_pack(phd_ctx* ctx, long K_max, void* dev_block) {
    int rc = eap_dyn_check(ctx, "phd_eap_dyn_shard_pack");
    if (rc) return rc;
    if (K_max < 0 || K_max >= (1L << 31) - 1 || !dev_block || ((uintptr_t)dev_block & 15))
        return fail(PHD_E_ARG,
                    "bad arguments to phd_eap_dyn_shard_pack (K_max in [0, 2^31 - 1), a 16-byte aligned block)");
    if (set_device(ctx)) return PHD_E_HIP;
    std::string err;
    rc = eap4_shard_pack(&ctx->eap4, ctx->stream, ctx->st.d_src, ctx->mx.d_dmap[ctx->mx.dcur],
                         ctx->mx.d_dsize[ctx->mx.dcur], ctx->mx.d_dmap_x, ctx->mx.d_dsize_x, ctx->st.d_logw, ctx->n,
                         ctx->mx.dcap, K_max, dev_block, err);
    if (rc == -2) return fail(PHD_E_ARG, "phd_eap_dyn_shard_pack: " + err);
    if (rc) return fail(PHD_E_HIP, "phd_eap_dyn_shard_pack: " + err);
    return PHD_OK;
}

int phd_expected_map_dynamic_blocks(phd_ctx* ctx, const void* dev_blocks, int world, long K_max, phd_gaussian4d* out,
                                    long out_cap, long* n_out) {
    int rc = eap_dyn_check(ctx, "phd_expected_map_dynamic_blocks");
    if (rc) return rc;
    if (!n_out || !dev_blocks || ((uintptr_t)dev_blocks & 15) || world < 1 || world > EAP_MAX_WORLD || K_max < 0 ||
        K_max >= (1L << 31) - 1)
        return fail(PHD_E_ARG, "bad arguments to phd_expected_map_dynamic_blocks (world in [1, 1024], K_max in "
                               "[0, 2^31 - 1), 16-byte aligned blocks)");
    if (set_device(ctx)) return PHD_E_HIP;
    rc = blocks_fit(dev_blocks, world, K_max, eap4_block_bytes(K_max), "phd_expected_map_dynamic_blocks");
    if (rc) return rc;
    std::string err;
    const long nout = mixed_expected_map_dynamic_blocks(&ctx->eap4, ctx->stream, dev_blocks, world, ctx->n, K_max,
                                                        ctx->cfg.minSeparation, out, out ? out_cap : 0, ctx->eap4_mode,
                                                 &ctx->eap4_rounds, &ctx->eap4_cells, err);
    if (nout == -2) return fail(PHD_E_ARG, "phd_expected_map_dynamic_blocks: " + err);
    if (nout < 0) return fail(PHD_E_HIP, "dynamic expected map: " + err);
    *n_out = nout;
    if (nout > 0 && (!out || nout > out_cap))
        return fail(PHD_E_CAPACITY, "dynamic expected map has " + std::to_string(nout) + " components; out_cap too small");
    return PHD_OK;
}

/* Local LSE parts for a cross-rank log-sum-exp: out_host[0] = max, out_host[1] = Σexp(w - max). */
int phd_lse_parts(phd_ctx* ctx, float* out_host) {
    if (!ctx || !out_host) return fail(PHD_E_ARG, "null argument");
    if (set_device(ctx)) return PHD_E_HIP;
    hipLaunchKernelGGL(k_lse_parts, dim3(1), dim3(1024), 0, ctx->stream, ctx->st.d_logw, ctx->n, ctx->d_out + 32);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out_host, ctx->d_out + 32, 2 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PHD_OK;
}

}  // extern "C"
