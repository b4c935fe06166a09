/*
 * phd_capi_ctx.hip — the context of the C-ABI (include/phd_capi.h): create /
 * destroy, configuration, stream and seed, load and export of the store (static
 * and dynamic), the measurement upload, the status and error counters, the
 * tuning setters and getters.
 */
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "phd_ctx.h"

using namespace phd;

static thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}
const std::string& last_error() { return g_last_error; }

int set_device(phd_ctx* c) {
    HIPCHK(hipSetDevice(c->device));
    return PHD_OK;
}

extern "C" {

const char* phd_version(void) { return "phdslam-mi355x 0.1 (gfx950)"; }
const char* phd_last_error(void) { return g_last_error.c_str(); }

int phd_device_count(int* count) {
    if (!count) return fail(PHD_E_ARG, "count is NULL");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) c = 0;
    *count = c;
    return PHD_OK;
}

__global__ void k_iota(int* a, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) a[i] = i;
}

/* the store, the scan block and the scratch every context has from the start */
static int alloc_fixed(phd_ctx* c) {
    const size_t N = (size_t)c->nmax;
    const ZBlk Z = zblk_layout();
    for (int b = 0; b < 2; b++)
        if (c->st.d_map[b].alloc(N * 7 * (size_t)c->cap.map_capacity) || c->st.d_size[b].alloc(N)) return PHD_E_HIP;
    if (c->st.d_src.alloc(N) || c->st.d_pose.alloc(N) || c->st.d_logw.alloc(N) || c->st.d_tmp_pose.alloc(N) ||
        c->st.d_tmp_src.alloc(N) || c->st.d_tmp_logw.alloc(N) || c->d_delta.alloc(N) || c->d_status.alloc(N) ||
        c->d_err.alloc(4) || c->z.blk.alloc(Z.bytes) || c->d_noise_a.alloc(N) || c->d_noise_cv.alloc(N) ||
        c->rs.d_cdf.alloc(N) || c->rs.d_idx.alloc(N) || c->rs.d_u.alloc(N) || c->d_out.alloc(64) || c->d_cn.alloc(N))
        return PHD_E_HIP;
    c->z.zr = (float*)(c->z.blk + Z.zr);
    c->z.zb = (float*)(c->z.blk + Z.zb);
    c->z.zok = (int*)(c->z.blk + Z.zok);
    c->z.zlab = (int*)(c->z.blk + Z.zlab);
    c->z.zs = (float4*)(c->z.blk + Z.zs);
    c->z.zbin = (unsigned short*)(c->z.blk + Z.zbin);
    return PHD_OK;
}

int phd_ctx_create(phd_ctx** out, int device, int n_particles, const phd_capacity* capin) {
    if (!out || n_particles <= 0) return fail(PHD_E_ARG, "bad arguments to phd_ctx_create");
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(PHD_E_NODEVICE, "no HIP device visible");
    if (device < 0 || device >= ndev) return fail(PHD_E_ARG, "device index out of range");
    phd_capacity cap = capin ? *capin : phd_capacity{};
    if (cap.max_particles < n_particles) cap.max_particles = n_particles;
    if (cap.map_capacity <= 0) cap.map_capacity = 1024;
    if (cap.max_measurements <= 0) cap.max_measurements = 256;
    if (cap.max_measurements > 256) cap.max_measurements = 256;
    if (cap.candidate_capacity <= 0) cap.candidate_capacity = cap.map_capacity + 4 * cap.max_measurements;
    if (cap.survivor_capacity <= 0) cap.survivor_capacity = 4 * cap.max_measurements;
    if (cap.map_capacity > 32767 || cap.candidate_capacity > 16383)
        return fail(PHD_E_ARG, "map_capacity must be <= 32767 and candidate_capacity <= 16383");
    cap.survivor_capacity = (cap.survivor_capacity + 3) & ~3;  // rank sort reads keys 4 at a time
    phd_ctx* c = new phd_ctx();  // (every failure below: delete c releases what exists)
    c->device = device;
    c->n = n_particles;
    c->n_base = n_particles;
    c->nmax = cap.max_particles;
    c->cap = cap;
    c->upd.epool = upd_epool(cap.candidate_capacity);
    c->cn.stride = cap.max_measurements + 8;
    const size_t N = (size_t)c->nmax;
    if (set_device(c) || alloc_fixed(c)) {
        delete c;
        return PHD_E_HIP;
    }
    if (c->stream.create(hipStreamNonBlocking)) {
        delete c;
        return fail(PHD_E_HIP, "hipStreamCreate failed");
    }
    hipMemsetAsync(c->st.d_size[0], 0, N * sizeof(int), c->stream);
    hipMemsetAsync(c->st.d_size[1], 0, N * sizeof(int), c->stream);
    hipMemsetAsync(c->d_err, 0, 4 * sizeof(int), c->stream);
    hipMemsetAsync(c->d_out, 0, 64 * sizeof(float), c->stream);
    hipMemsetAsync(c->st.d_logw, 0, N * sizeof(float), c->stream);
    hipMemsetAsync(c->st.d_pose, 0, N * sizeof(phd_pose), c->stream);
    hipLaunchKernelGGL(k_iota, dim3((c->nmax + 255) / 256), dim3(256), 0, c->stream, c->st.d_src, c->nmax);
    for (int nt = UPD_THREADS_MIN; nt <= UPD_THREADS_MAX; nt *= 2)
        for (int cp = 0; cp < 2; cp++)
            for (int part = cp; part < 3; part++)
                for (int metric = 0; metric < (part == 1 ? 1 : 2); metric++)
                    for (int predict = 0; predict < 2; predict++)
                        if (const void* k = update_kernel(nt, cp, part, metric, predict))
                            hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    hipFuncSetAttribute((const void*)k_resample, hipFuncAttributeMaxDynamicSharedMemorySize, 8 * RS_LDS_MAX);
    hipFuncSetAttribute((const void*)k_normalize_resample, hipFuncAttributeMaxDynamicSharedMemorySize,
                        8 * RS_LDS_MAX);
    // a limit a kernel cannot take only caps its launches (checked at launch):
    // do not leave it as the runtime's last error for the next launch check
    (void)hipGetLastError();
    if (apply_update_launch(c, 0) != PHD_OK) {
        delete c;
        return PHD_E_CAPACITY;  // (the last error: the configuration's)
    }
    if (hipStreamSynchronize(c->stream) != hipSuccess) {
        delete c;
        return fail(PHD_E_HIP, "initialisation failed");
    }
    *out = c;
    return PHD_OK;
}

int phd_ctx_destroy(phd_ctx* ctx) {
    delete ctx;  // ~phd_ctx waits for the stream first
    return PHD_OK;
}

int phd_ctx_info(const phd_ctx* ctx, int* n_particles, phd_capacity* cap) {
    if (!ctx) return fail(PHD_E_ARG, "null ctx");
    if (n_particles) *n_particles = ctx->n;
    if (cap) *cap = ctx->cap;
    return PHD_OK;
}

int phd_set_config(phd_ctx* ctx, const phd_slam_config* cfg) {
    if (!ctx || !cfg) return fail(PHD_E_ARG, "null argument");
    ctx->cfg = *cfg;
    ctx->cfg_set = true;
    const int cphd = cfg->filterType == PHD_FILTER_CPHD ? 1 : 0;
    const int metric = cfg->distanceMetric == 1 ? 1 : 0;
    if (cphd != ctx->upd.cphd || metric != ctx->upd.metric) {
        // the CPHD kernels have their own LDS layout and occupancy, the
        // Hellinger kernels their own registers
        if (set_device(ctx)) return PHD_E_HIP;
        int rc = apply_update_launch(ctx, ctx->upd.threads_req);
        ctx->upd.cfg_error = rc ? g_last_error : std::string();  // (the launch stays sized for the old kernels)
        if (rc) return rc;
    }
    return PHD_OK;
}

int phd_set_stream(phd_ctx* ctx, void* s) {
    if (!ctx) return fail(PHD_E_ARG, "null ctx");
    if (s) {
        if (ctx->stream.owned() && ctx->stream) hipStreamSynchronize(ctx->stream);
        ctx->stream.borrow(s == PHD_STREAM_NULL ? (hipStream_t)0 : (hipStream_t)s);  // (destroys the owned one)
    }
    return PHD_OK;
}

void* phd_get_stream(phd_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int phd_synchronize(phd_ctx* ctx) {
    if (!ctx) return fail(PHD_E_ARG, "null ctx");
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PHD_OK;
}

int phd_set_seed(phd_ctx* ctx, uint64_t seed) {
    if (!ctx) return fail(PHD_E_ARG, "null ctx");
    ctx->seed = seed;
    return PHD_OK;
}

int phd_load_particles(phd_ctx* ctx, int n, const phd_pose* poses, const float* logw, const phd_gaussian2d* maps,
                       const int* offsets) {
    if (!ctx || n <= 0 || n > ctx->nmax || !poses || !logw || !offsets)
        return fail(PHD_E_ARG, "bad arguments to phd_load_particles");
    if (set_device(ctx)) return PHD_E_HIP;
    ctx->n = n;  // the live count (n_particles, or up to capacity.max_particles)
    const int cap = ctx->cap.map_capacity;
    std::vector<float> slab((size_t)n * 7 * cap, 0.f);
    std::vector<int> sizes(n);
    for (int p = 0; p < n; p++) {
        const int sz = offsets[p + 1] - offsets[p];
        if (sz < 0 || sz > cap) return fail(PHD_E_CAPACITY, "particle map exceeds map_capacity");
        sizes[p] = sz;
        float* s = slab.data() + (size_t)p * 7 * cap;
        for (int k = 0; k < sz; k++) {
            const phd_gaussian2d& g = maps[offsets[p] + k];
            s[k] = g.weight;
            s[1 * cap + k] = g.mean[0];
            s[2 * cap + k] = g.mean[1];
            s[3 * cap + k] = g.cov[0];
            s[4 * cap + k] = g.cov[1];
            s[5 * cap + k] = g.cov[2];
            s[6 * cap + k] = g.cov[3];
        }
    }
    ctx->st.cur = 0;
    ctx->st.replay = false;
    HIPCHK(hipMemcpyAsync(ctx->st.d_map[0], slab.data(), slab.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->st.d_size[0], sizes.data(), n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->st.d_pose, poses, n * sizeof(phd_pose), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->st.d_logw, logw, n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_iota, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, ctx->st.d_src, n);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PHD_OK;
}

int phd_set_poses(phd_ctx* ctx, int n, const phd_pose* poses) {
    if (!ctx || n != ctx->n || !poses) return fail(PHD_E_ARG, "bad arguments to phd_set_poses");
    if (set_device(ctx)) return PHD_E_HIP;
    HIPCHK(hipMemcpyAsync(ctx->st.d_pose, poses, n * sizeof(phd_pose), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PHD_OK;
}

/* Host image of the current state: slab reference table + the sets it references. */
struct HostState {
    std::vector<int> src, size_cur, size_x;
    std::vector<float> map_cur, map_x;
};

static int fetch_state(phd_ctx* ctx, HostState& h, bool with_maps) {
    // slabs of the current set: a resample after n_predict_particles > 1 may
    // leave live particles referencing slabs beyond the live count
    const int n = ctx->n, ns = ctx->nmax, cap = ctx->cap.map_capacity;
    h.src.resize(n);
    h.size_cur.resize(ns);
    HIPCHK(hipMemcpyAsync(h.src.data(), ctx->st.d_src, n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(h.size_cur.data(), ctx->st.d_size[ctx->st.cur], ns * sizeof(int), hipMemcpyDeviceToHost,
                          ctx->stream));
    if (ctx->st.d_size_x) {
        h.size_x.resize(n);
        HIPCHK(hipMemcpyAsync(h.size_x.data(), ctx->st.d_size_x, n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    }
    if (with_maps) {
        h.map_cur.resize((size_t)ns * 7 * cap);
        HIPCHK(hipMemcpyAsync(h.map_cur.data(), ctx->st.d_map[ctx->st.cur], h.map_cur.size() * sizeof(float),
                              hipMemcpyDeviceToHost, ctx->stream));
        if (ctx->st.d_map_x) {
            h.map_x.resize((size_t)n * 7 * cap);
            HIPCHK(hipMemcpyAsync(h.map_x.data(), ctx->st.d_map_x, h.map_x.size() * sizeof(float), hipMemcpyDeviceToHost,
                                  ctx->stream));
        }
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PHD_OK;
}

static inline int host_size(const HostState& h, int p) {
    return slab_size(h.src[p], h.size_cur.data(), h.size_x.data());
}

int phd_export_particles(phd_ctx* ctx, int n, phd_pose* poses, float* logw, int* sizes) {
    if (!ctx || n != ctx->n) return fail(PHD_E_ARG, "bad arguments to phd_export_particles");
    if (set_device(ctx)) return PHD_E_HIP;
    if (poses) HIPCHK(hipMemcpyAsync(poses, ctx->st.d_pose, n * sizeof(phd_pose), hipMemcpyDeviceToHost, ctx->stream));
    if (logw) HIPCHK(hipMemcpyAsync(logw, ctx->st.d_logw, n * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HostState h;
    int rc = fetch_state(ctx, h, false);
    if (rc) return rc;
    if (sizes)
        for (int p = 0; p < n; p++) sizes[p] = host_size(h, p);
    return PHD_OK;
}

int phd_export_maps(phd_ctx* ctx, int n, const int* offsets, phd_gaussian2d* maps) {
    if (!ctx || n != ctx->n || !offsets || !maps) return fail(PHD_E_ARG, "bad arguments to phd_export_maps");
    if (set_device(ctx)) return PHD_E_HIP;
    const int cap = ctx->cap.map_capacity;
    HostState h;
    int rc = fetch_state(ctx, h, true);
    if (rc) return rc;
    for (int p = 0; p < n; p++) {
        const float* s = slab_map(h.src[p], h.map_cur.data(), h.map_x.data(), cap);
        const int sz = offsets[p + 1] - offsets[p];
        if (sz != host_size(h, p)) return fail(PHD_E_ARG, "offsets do not match the current map sizes");
        for (int k = 0; k < sz; k++) {
            phd_gaussian2d& g = maps[offsets[p] + k];
            g.weight = s[k];
            g.mean[0] = s[1 * cap + k];
            g.mean[1] = s[2 * cap + k];
            g.cov[0] = s[3 * cap + k];
            g.cov[1] = s[4 * cap + k];
            g.cov[2] = s[5 * cap + k];
            g.cov[3] = s[6 * cap + k];
        }
    }
    return PHD_OK;
}

/* ---- mixed static + dynamic feature model (feature_model 2) ---- */
int phd_enable_dynamic(phd_ctx* ctx, int dyn_capacity) {
    if (!ctx || dyn_capacity <= 0) return fail(PHD_E_ARG, "bad arguments to phd_enable_dynamic");
    if (set_device(ctx)) return PHD_E_HIP;
    if (ctx->mx.on && ctx->mx.dcap == dyn_capacity) return PHD_OK;
    ctx->mx = Mixed{};  // (another capacity: the old sets go before the new ones come)
    const size_t ns = (size_t)ctx->nmax;
    for (int k = 0; k < 2; k++) {
        if (ctx->mx.d_dmap[k].alloc(ns * PHD_DYN_FIELDS * dyn_capacity) || ctx->mx.d_dsize[k].alloc(ns))
            return PHD_E_HIP;
        HIPCHK(hipMemsetAsync(ctx->mx.d_dsize[k], 0, ns * sizeof(int), ctx->stream));
    }
    if (ctx->mx.d_ekf.alloc(ns * mixed_ekf_floats(ctx->cap.map_capacity, dyn_capacity)) ||
        ctx->mx.d_cand.alloc(ns * mixed_cand_floats(ctx->cap.candidate_capacity)))
        return PHD_E_HIP;
    HIPCHK(mixed_set_lds_limit());
    ctx->mx.on = true;
    ctx->mx.dcap = dyn_capacity;
    ctx->mx.dcur = 0;
    // a context that holds migrated slabs: its references with bit 30 name the
    // dynamic set X as well — resized with the rest (empty, like the new sets),
    // so none of them is left stale
    if (ctx->st.d_map_x && ensure_dyn_x(ctx)) return PHD_E_HIP;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PHD_OK;
}

int phd_load_dynamic_maps(phd_ctx* ctx, int n, const phd_gaussian4d* maps, const int* offsets) {
    if (!ctx || n != ctx->n || !offsets || (offsets[n] > 0 && !maps))
        return fail(PHD_E_ARG, "bad arguments to phd_load_dynamic_maps");
    if (!ctx->mx.on) return fail(PHD_E_ARG, "phd_enable_dynamic not called");
    if (set_device(ctx)) return PHD_E_HIP;
    // particle i must own slab i (as after phd_load_particles or an update)
    std::vector<int> src(n);
    HIPCHK(hipMemcpyAsync(src.data(), ctx->st.d_src, n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    for (int p = 0; p < n; p++)
        if (src[p] != p)
            return fail(PHD_E_ARG, "phd_load_dynamic_maps: particles share slabs (load after phd_load_particles or an update)");
    const int dcap = ctx->mx.dcap;
    std::vector<float> slab((size_t)n * PHD_DYN_FIELDS * dcap, 0.f);
    std::vector<int> sizes(n);
    for (int p = 0; p < n; p++) {
        const int sz = offsets[p + 1] - offsets[p];
        if (sz < 0 || sz > dcap) return fail(PHD_E_CAPACITY, "dynamic map exceeds the dynamic capacity");
        sizes[p] = sz;
        float* sl = slab.data() + (size_t)p * PHD_DYN_FIELDS * dcap;
        for (int k = 0; k < sz; k++) {
            const phd_gaussian4d& g = maps[offsets[p] + k];
            sl[k] = g.weight;
            for (int i = 0; i < 4; i++) sl[(1 + i) * dcap + k] = g.mean[i];
            for (int i = 0; i < 16; i++) sl[(5 + i) * dcap + k] = g.cov[i];
        }
    }
    HIPCHK(hipMemcpyAsync(ctx->mx.d_dmap[ctx->mx.dcur], slab.data(), slab.size() * sizeof(float), hipMemcpyHostToDevice,
                          ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->mx.d_dsize[ctx->mx.dcur], sizes.data(), n * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->mx.x_live = false;  // (every reference is the identity, checked above: none names set X)
    return PHD_OK;
}

/* Host image of the dynamic migration set X (sizes, and the maps when asked
 * for); both stay empty before the first receive.  The copies are enqueued:
 * the caller synchronises. */
static int fetch_dyn_x(phd_ctx* ctx, std::vector<int>& size_x, std::vector<float>* map_x) {
    if (!ctx->mx.d_dsize_x) return PHD_OK;
    const size_t nx = ctx->mx.d_dsize_x.bytes() / sizeof(int);
    size_x.resize(nx);
    HIPCHK(hipMemcpyAsync(size_x.data(), ctx->mx.d_dsize_x, nx * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (map_x) {
        map_x->resize(nx * PHD_DYN_FIELDS * ctx->mx.dcap);
        HIPCHK(hipMemcpyAsync(map_x->data(), ctx->mx.d_dmap_x, map_x->size() * sizeof(float), hipMemcpyDeviceToHost,
                              ctx->stream));
    }
    return PHD_OK;
}

/* every reference that names set X names a slab the dynamic set X has */
static int check_dyn_refs(const phd_ctx* ctx, const std::vector<int>& src, const std::vector<int>& size_x) {
    for (int r : src)
        if (slab_in_x(r) && (size_t)slab_index(r) >= size_x.size())
            return fail(PHD_E_ARG, "a slab reference names a slab the dynamic migration set X does not have");
    return PHD_OK;
}

int phd_dynamic_sizes(phd_ctx* ctx, int* sizes) {
    if (!ctx || !sizes) return fail(PHD_E_ARG, "null argument");
    if (!ctx->mx.on) return fail(PHD_E_ARG, "phd_enable_dynamic not called");
    if (set_device(ctx)) return PHD_E_HIP;
    const int n = ctx->n;
    std::vector<int> src(n), dsz(ctx->nmax), dszx;
    HIPCHK(hipMemcpyAsync(src.data(), ctx->st.d_src, n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(dsz.data(), ctx->mx.d_dsize[ctx->mx.dcur], ctx->nmax * sizeof(int), hipMemcpyDeviceToHost,
                          ctx->stream));
    if (int rc = fetch_dyn_x(ctx, dszx, nullptr)) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (int rc = check_dyn_refs(ctx, src, dszx)) return rc;
    for (int p = 0; p < n; p++) sizes[p] = slab_size(src[p], dsz.data(), dszx.data());
    return PHD_OK;
}

int phd_export_dynamic_maps(phd_ctx* ctx, int n, const int* offsets, phd_gaussian4d* maps) {
    if (!ctx || n != ctx->n || !offsets || (offsets[n] > 0 && !maps))
        return fail(PHD_E_ARG, "bad arguments to phd_export_dynamic_maps");
    if (!ctx->mx.on) return fail(PHD_E_ARG, "phd_enable_dynamic not called");
    if (set_device(ctx)) return PHD_E_HIP;
    const int dcap = ctx->mx.dcap;
    std::vector<int> src(n), dsz(ctx->nmax), dszx;
    std::vector<float> all((size_t)ctx->nmax * PHD_DYN_FIELDS * dcap), allx;
    HIPCHK(hipMemcpyAsync(src.data(), ctx->st.d_src, n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(dsz.data(), ctx->mx.d_dsize[ctx->mx.dcur], ctx->nmax * sizeof(int), hipMemcpyDeviceToHost,
                          ctx->stream));
    HIPCHK(hipMemcpyAsync(all.data(), ctx->mx.d_dmap[ctx->mx.dcur], all.size() * sizeof(float), hipMemcpyDeviceToHost,
                          ctx->stream));
    if (int rc = fetch_dyn_x(ctx, dszx, &allx)) return rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (int rc = check_dyn_refs(ctx, src, dszx)) return rc;
    for (int p = 0; p < n; p++) {
        const int sz = offsets[p + 1] - offsets[p];
        if (sz != slab_size(src[p], dsz.data(), dszx.data()))
            return fail(PHD_E_ARG, "offsets do not match the current dynamic map sizes");
        const float* sl = dyn_slab_map(src[p], (const float*)all.data(), (const float*)allx.data(), dcap);
        for (int k = 0; k < sz; k++) {
            phd_gaussian4d& g = maps[offsets[p] + k];
            g.weight = sl[k];
            for (int i = 0; i < 4; i++) g.mean[i] = sl[(1 + i) * dcap + k];
            for (int i = 0; i < 16; i++) g.cov[i] = sl[(5 + i) * dcap + k];
        }
    }
    return PHD_OK;
}

int phd_slab_sizes(phd_ctx* ctx, int* sizes) {
    if (!ctx || !sizes) return fail(PHD_E_ARG, "null argument");
    if (set_device(ctx)) return PHD_E_HIP;
    HIPCHK(hipMemcpyAsync(sizes, ctx->st.d_size[ctx->st.cur], ctx->n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PHD_OK;
}

int phd_set_replay(phd_ctx* ctx, int on) {
    if (!ctx) return fail(PHD_E_ARG, "null ctx");
    if (set_device(ctx)) return PHD_E_HIP;
    if (on) {
        if (ctx->st.cur != 0) return fail(PHD_E_ARG, "phd_set_replay must follow phd_load_particles");
        if (ctx->n != ctx->n_base) return fail(PHD_E_UNSUPPORTED, "replay mode needs n_particles live particles");
        if (ctx->st.d_pose_prior.ensure(ctx->n) || ctx->st.d_logw_prior.ensure(ctx->n)) return PHD_E_HIP;
        HIPCHK(hipMemcpyAsync(ctx->st.d_pose_prior, ctx->st.d_pose, ctx->n * sizeof(phd_pose), hipMemcpyDeviceToDevice,
                              ctx->stream));
        HIPCHK(hipMemcpyAsync(ctx->st.d_logw_prior, ctx->st.d_logw, ctx->n * sizeof(float), hipMemcpyDeviceToDevice,
                              ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    ctx->st.replay = on != 0;
    return PHD_OK;
}

/* phdUpdateSynth's measurement upload (phdfilter.cu:3389-3400: clamp to 256,
 * cudaMemcpyToSymbol(Z)): the measurements, labels, and the bearing-sorted
 * valid ones with their 256-bin table for the banded pair walk, staged in a
 * pinned ring slot and sent as ONE stream-ordered copy.  No host wait: the slot
 * is reused PHD_ZRING calls later, after the event of its copy (long
 * complete); the device block is overwritten in stream order, after every
 * earlier launch that reads it. */
int phd_set_measurements(phd_ctx* ctx, const phd_measurement* z, int n_measure) {
    if (!ctx || n_measure < 0 || (n_measure > 0 && !z)) return fail(PHD_E_ARG, "bad arguments to phd_set_measurements");
    if (!ctx->cfg_set) return fail(PHD_E_ARG, "phd_set_config not called");
    if (set_device(ctx)) return PHD_E_HIP;
    int M = std::min(n_measure, 256);  // phdfilter.cu:3390-3394
    if (M > ctx->cap.max_measurements) return fail(PHD_E_CAPACITY, "more measurements than max_measurements");
    const ZBlk Z = zblk_layout();
    if (!ctx->z.h_ring) {
        if (ctx->z.h_ring.alloc(PHD_ZRING * Z.bytes)) return PHD_E_HIP;
        for (auto& e : ctx->z.ev_ring)
            if (e.create(hipEventDisableTiming)) return PHD_E_HIP;
    }
    if (ctx->z.sets > 0) {
        // the current scan becomes the previous one (the step's births, CPHD):
        // its raw rows, copied in stream order ahead of the new upload
        if (ctx->z.prev.ensure(Z.zlab)) return PHD_E_HIP;
        if (ctx->z.M > 0) HIPCHK(hipMemcpyAsync(ctx->z.prev, ctx->z.blk, Z.zlab, hipMemcpyDeviceToDevice, ctx->stream));
        ctx->z.M_prev = ctx->z.M;
        ctx->z.Mv_prev = ctx->z.Mv;
        ctx->z.have_prev = true;
    }
    ctx->z.sets++;
    const int slot = ctx->z.ring_next;
    ctx->z.ring_next = (slot + 1) % PHD_ZRING;
    if (ctx->z.ring_used[slot]) HIPCHK(hipEventSynchronize(ctx->z.ev_ring[slot]));  // the copy PHD_ZRING calls ago (done long since)
    unsigned char* h = ctx->z.h_ring + (size_t)slot * Z.bytes;
    float* zr = (float*)(h + Z.zr);
    float* zb = (float*)(h + Z.zb);
    int* zok = (int*)(h + Z.zok);
    int* zlab = (int*)(h + Z.zlab);
    int* zvi = (int*)(h + Z.zvi);
    float4* zs = (float4*)(h + Z.zs);
    unsigned short* zbin = (unsigned short*)(h + Z.zbin);
    int Mv = 0, zwide = 0;
    for (int m = 0; m < M; m++) {
        zr[m] = z[m].range;
        zb[m] = z[m].bearing;
        zok[m] = (z[m].label == PHD_MEAS_STATIC || !ctx->cfg.labeledMeasurements) ? 1 : 0;
        zlab[m] = z[m].label;
        if (!(std::fabs(zb[m]) < 3.f)) zwide = 1;
        if (!zok[m]) continue;
        zvi[Mv] = m;
        // bearing-sorted valid measurements for the banded pair loop (key = bearing wrapped to [-pi, pi))
        double key = std::fmod((double)zb[m] + M_PI, 2 * M_PI);
        if (key < 0) key += 2 * M_PI;
        key -= M_PI;
        float kf = (float)key;
        if (kf >= (float)M_PI) kf = -(float)M_PI;
        float idx;
        std::memcpy(&idx, &m, sizeof(int));
        zs[Mv++] = make_float4(zr[m], zb[m], idx, kf);
    }
    std::stable_sort(zs, zs + Mv, [](const float4& x, const float4& y) { return x.w < y.w; });
    for (int b = 0, k = 0; b < PHD_ZBINS; b++) {
        const float edge = (float)(-M_PI + b * (2 * M_PI / PHD_ZBINS));
        while (k < Mv && zs[k].w < edge) k++;
        zbin[b] = (unsigned short)k;
    }
    if (M > 0) {
        HIPCHK(hipMemcpyAsync(ctx->z.blk, h, Z.bytes, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipEventRecord(ctx->z.ev_ring[slot], ctx->stream));
        ctx->z.ring_used[slot] = true;
    }
    ctx->z.M = M;
    ctx->z.Mv = Mv;
    ctx->z.zwide = zwide;
    return PHD_OK;
}

/* Turn the per-update capacity check (one 4-B D2H + sync) on/off; the bench
 * turns it off inside the timed loop and checks once at the end. */
int phd_set_check_each_update(phd_ctx* ctx, int on) {
    if (!ctx) return fail(PHD_E_ARG, "null ctx");
    ctx->check_each_update = on != 0;
    return PHD_OK;
}

/* Diagnostic: copy the per-workgroup phase stamps of the last update (PHD_STAMPS builds). */
int phd_debug_stamps(phd_ctx* ctx, unsigned long long* host, int enable) {
    if (!ctx) return fail(PHD_E_ARG, "null ctx");
    if (set_device(ctx)) return PHD_E_HIP;
    if (enable && !ctx->d_stamps) {
        if (ctx->d_stamps.alloc((size_t)ctx->nmax * PHD_STAMP_SLOTS)) return PHD_E_HIP;
        HIPCHK(hipMemsetAsync(ctx->d_stamps, 0, (size_t)ctx->nmax * PHD_STAMP_SLOTS * sizeof(unsigned long long), ctx->stream));
    }
    if (host && ctx->d_stamps) {
        HIPCHK(hipMemcpyAsync(host, ctx->d_stamps, (size_t)ctx->n * PHD_STAMP_SLOTS * sizeof(unsigned long long),
                              hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
    }
    return PHD_OK;
}

int phd_set_update_threads(phd_ctx* ctx, int threads) {
    if (!ctx || !(threads == 0 || threads == 256 || threads == 512 || threads == 1024))
        return fail(PHD_E_ARG, "threads must be 0 (automatic), 256, 512 or 1024");
    if (set_device(ctx)) return PHD_E_HIP;
    return apply_update_launch(ctx, threads);
}

int phd_set_edge_pool(phd_ctx* ctx, int pool) {
    if (!ctx || pool < 0 || pool > 32768) return fail(PHD_E_ARG, "edge pool must be 0 (automatic) .. 32768");
    if (set_device(ctx)) return PHD_E_HIP;
    const int old = ctx->upd.epool_req;
    ctx->upd.epool_req = pool;
    const int rc = apply_update_launch(ctx, ctx->upd.threads_req);
    if (rc) ctx->upd.epool_req = old;
    return rc;
}

int phd_set_pair_list_cap(phd_ctx* ctx, int pairs) {
    if (!ctx || pairs < 0) return fail(PHD_E_ARG, "pair-list cap must be >= 0 (0: the layout's)");
    ctx->upd.plreq = pairs;
    return PHD_OK;
}

int phd_set_update_form(phd_ctx* ctx, int form) {
    if (!ctx || form < 0 || form > 2) return fail(PHD_E_ARG, "form must be 0 (automatic), 1 (fused) or 2 (split)");
    if (set_device(ctx)) return PHD_E_HIP;
    const int old = ctx->upd.form_req;
    ctx->upd.form_req = form;
    const int rc = apply_update_launch(ctx, ctx->upd.threads_req);
    if (rc) ctx->upd.form_req = old;
    return rc;
}

int phd_update_form(phd_ctx* ctx, int* split) {
    if (!ctx || !split) return fail(PHD_E_ARG, "null argument");
    *split = ctx->upd.split;
    return PHD_OK;
}

int phd_update_threads(phd_ctx* ctx, int* threads, size_t* lds_bytes, int* resident) {
    if (!ctx) return fail(PHD_E_ARG, "null context");
    if (threads) *threads = ctx->upd.threads;
    if (lds_bytes) *lds_bytes = ctx->upd.lds;
    if (resident) *resident = ctx->upd.resident;
    return PHD_OK;
}

int phd_set_merge_mode(phd_ctx* ctx, int mode) {
    if (!ctx || mode < 0 || mode > 1) return fail(PHD_E_ARG, "bad arguments");
    ctx->merge_mode = mode;
    return PHD_OK;
}

int phd_merge_fallbacks(phd_ctx* ctx, int* count) {
    if (!ctx || !count) return fail(PHD_E_ARG, "null argument");
    if (set_device(ctx)) return PHD_E_HIP;
    int v[2];
    HIPCHK(hipMemcpyAsync(v, ctx->d_err, 2 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    *count = v[1];
    HIPCHK(hipMemsetAsync(ctx->d_err + 1, 0, sizeof(int), ctx->stream));
    return PHD_OK;
}

/* read and clear one of the counters after the sticky error word */
static int take_counter(phd_ctx* ctx, int k, int* count) {
    if (!ctx || !count) return fail(PHD_E_ARG, "null argument");
    if (set_device(ctx)) return PHD_E_HIP;
    int v = 0;
    HIPCHK(hipMemcpyAsync(&v, ctx->d_err + k, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    *count = v;
    HIPCHK(hipMemsetAsync(ctx->d_err + k, 0, sizeof(int), ctx->stream));
    // (the trace's status_errors is the counter's growth per step: restart its baseline too)
    if (k == 3 && ctx->tr.d_hand)
        HIPCHK(hipMemsetAsync(ctx->tr.d_hand + TRACE_H_ERRPREV, 0, sizeof(int), ctx->stream));
    return PHD_OK;
}

int phd_status_errors(phd_ctx* ctx, int* count) { return take_counter(ctx, 3, count); }

int phd_particle_status(phd_ctx* ctx, int* host_status) {
    if (!ctx || !host_status) return fail(PHD_E_ARG, "null argument");
    if (set_device(ctx)) return PHD_E_HIP;
    HIPCHK(hipMemcpyAsync(host_status, ctx->d_status, ctx->n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return PHD_OK;
}

int phd_merge_pair_overflows(phd_ctx* ctx, int* count) {
    if (!ctx || !count) return fail(PHD_E_ARG, "null argument");
    if (set_device(ctx)) return PHD_E_HIP;
    int v = 0;
    HIPCHK(hipMemcpyAsync(&v, ctx->d_err + 2, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    *count = v;
    HIPCHK(hipMemsetAsync(ctx->d_err + 2, 0, sizeof(int), ctx->stream));
    return PHD_OK;
}

int phd_check_errors(phd_ctx* ctx) {
    if (!ctx) return fail(PHD_E_ARG, "null ctx");
    if (set_device(ctx)) return PHD_E_HIP;
    return check_err(ctx);
}

}  // extern "C"
