/*
 * phd_ctx.h — the context behind include/phd_capi.h and what the host units
 * (phd_capi_*.hip) share: the last error, struct phd_ctx grouped by the unit
 * that owns each part, and the helpers one unit calls in another.  Host only:
 * no kernel unit includes it.
 *
 * The reference allocates, uploads, launches, downloads and frees inside every
 * phdPredict / phdUpdateSynth call (phdfilter.cu:1080-1257, :3336-3761) and
 * interleaves ~4 small memcpys per particle (:3227-3257).  Here the store lives
 * in HBM for the lifetime of the context; a filter step is a handful of
 * asynchronous launches on one stream with no host round trip.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "phd_capi.h"
#include "phd_kernels.h"
#include "phd_mixed_k.h"
#include "phd_own.h"
#include "phd_slab.h"
#include "phd_step_plan.h"
#include "phd_trace.h"

#pragma GCC visibility push(hidden)

/* the calling thread's last error, as fail (phd_own.h) set it */
const std::string& last_error();

#define HIPCHK(expr)                                                                         \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess)                                                                \
            return fail(PHD_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e));       \
    } while (0)

/* Events that only order work on this device (the overlap's cross-stream
 * hand-offs) or only time it: recorded without the system-scope fence, which
 * writes back and invalidates the caches at every record and costs the stream
 * a gap of several microseconds.  (The host reads the sharded plan's counts
 * after polling the sequence word the plan stores last with a system-scope
 * release: no event there either.) */
#ifndef PHD_EV_DEVICE_SCOPE
#define PHD_EV_DEVICE_SCOPE 1
#endif
static constexpr unsigned kEvOrder = hipEventDisableTiming | (PHD_EV_DEVICE_SCOPE ? hipEventDisableSystemFence : 0u);
static constexpr unsigned kEvTime = PHD_EV_DEVICE_SCOPE ? hipEventDisableSystemFence : hipEventDefault;

/* the measurement block: zr | zb | zok | zvi (the valid measurements' indices
 * in order) | zlab (256 each) | zs (256 float4) | zbin; [zr, zlab) is what the
 * step's births read (kept for the previous scan) */
#define PHD_ZRING 4
struct ZBlk {
    size_t zr, zb, zok, zvi, zlab, zs, zbin, bytes;
};
inline ZBlk zblk_layout() {
    ZBlk L;
    L.zr = 0;
    L.zb = L.zr + 256 * sizeof(float);
    L.zok = L.zb + 256 * sizeof(float);
    L.zvi = L.zok + 256 * sizeof(int);
    L.zlab = L.zvi + 256 * sizeof(int);
    L.zs = L.zlab + 256 * sizeof(int);
    L.zbin = L.zs + 256 * sizeof(float4);
    L.bytes = L.zbin + PHD_ZBINS * sizeof(unsigned short);
    return L;
}

/* Device store (phd_capi_ctx.hip loads and exports it; the update, the
 * resamples and the shard receives rewrite it).  Two slab sets (ping-pong
 * between updates) plus a migration set X; particle n's map is slab d_src[n]
 * of set `cur` (bit 30 -> set X).  Resampling rewrites d_src (copy-on-write),
 * never the slabs. */
struct Store {
    int cur = 0;
    phd::DevBuf<float> d_map[2];
    phd::DevBuf<int> d_size[2];
    phd::DevBuf<float> d_map_x;  // set X, allocated on the first receive (phd_capi_shard.hip)
    phd::DevBuf<int> d_size_x;
    phd::DevBuf<int> d_src;
    phd::DevBuf<phd_pose> d_pose;
    phd::DevBuf<float> d_logw;
    phd::DevBuf<phd_pose> d_tmp_pose;  // spares: a remap writes them, then they are swapped in
    phd::DevBuf<int> d_tmp_src;
    phd::DevBuf<float> d_tmp_logw;
    // replay mode (bench): fixed prior in set 0 + saved poses / log-weights
    bool replay = false;
    phd::DevBuf<phd_pose> d_pose_prior;
    phd::DevBuf<float> d_logw_prior;
    bool src_fresh = false;  // every slab reference is the identity (a full update since the last remap)
};

/* The scan (phd_set_measurements, phd_capi_ctx.hip) and the step's births from
 * the previous one (phd_capi_update.hip).  One device block (zr .. zbin are
 * views into it, zblk_layout) filled by ONE copy from a pinned host ring, so
 * phd_set_measurements never waits for the device (a slot is reused PHD_ZRING
 * calls later, after its event). */
struct Scan {
    phd::DevBuf<unsigned char> blk;
    float *zr = nullptr, *zb = nullptr;
    int *zok = nullptr, *zlab = nullptr;
    float4* zs = nullptr;            // valid measurements sorted by wrapped bearing
    unsigned short* zbin = nullptr;  // bearing-bin index into zs
    int M = 0, Mv = 0;
    int zwide = 0;  // some |measurement bearing| >= 3 (see UpdateArgs::zwide)
    phd::PinnedBuf<unsigned char> h_ring;
    phd::Event ev_ring[PHD_ZRING];
    bool ring_used[PHD_ZRING] = {};
    int ring_next = 0;
    int sets = 0;  // phd_set_measurements calls so far
    // the previous scan's raw rows (zr | zb | zok, zblk_layout) for the step's
    // births (CPHD: births through the prediction from the previous scan)
    phd::DevBuf<unsigned char> prev;
    int M_prev = 0, Mv_prev = 0;
    bool have_prev = false;
    int births_req = -1;         // -1: with the filter type (CPHD on), 0 off, 1 on (phd_set_step_births)
    phd::DevBuf<float> d_births;  // the step's birth slabs, nmax x 7 x map_capacity (written by the classify)
    int births_now = 0;          // the next launch_update places this many births per particle (0: none)
    const float *births_zr = nullptr, *births_zb = nullptr;  // ... from these rows
    const int* births_zvi = nullptr;
};

/* How the update is launched: the requests (setters) and what
 * configure_update_launch (phd_capi_update.hip) sized from them.  Replaced as
 * a whole, and only by a configuration that succeeded. */
struct UpdLaunch {
    int threads_req = 0;  // 0 = automatic
    int form_req = 0;     // PHD form requested: 0 automatic, 1 fused, 2 split (phd_set_update_form)
    int epool_req = 0;    // merge edge pool requested (phd_set_edge_pool; 0: the occupancy model's)
    int plreq = 0;        // culled-pair list cap (phd_set_pair_list_cap; 0: the layout's)
    int threads = 256;    // threads per particle of the fused update
    int cphd = 0;         // sized for the CPHD kernels
    int metric = 0;       // the merge distance it was sized for (its kernels' registers)
    int split = 0;        // the update runs as part A + part C (CPHD: always, with the terms between)
    int epool = 0;
    size_t lds = 0;       // LDS of the fused update / of part C
    size_t lds_a = 0;     // ... of part A
    int resident = 0;     // update workgroups resident at once on the device
    int resident_a = 0;   // the same for part A
    int resident_p = 0;   // the same for the launch that carries a fused predict (its own registers)
    std::string cfg_error;  // phd_set_config could not size the launch for its filter / metric (updates report it)
};

/* CPHD state (phd_capi_update.hip), allocated with the first CPHD use */
struct Cphd {
    phd::DevBuf<unsigned char> d_hand;  // per-particle handoff between the launches of a split update
    phd::DevBuf<double> d_coef;         // cardinality coefficients, nmax x stride (row = slab of the current set)
    phd::DevBuf<double> d_x;            // their rows for migration set X
    int stride = 0;
    phd::DevBuf<double> d_lfact;  // log n!, n = 0..lfact_n-1
    int lfact_n = 0;
    bool valid = false;  // a CPHD update has produced coefficients
};

/* resample scratch (phd_capi_step.hip; d_cdf_g: the global resample's) */
struct Resample {
    phd::DevBuf<unsigned long long> d_cdf, d_cdf_g;
    phd::DevBuf<int> d_idx;
    phd::DevBuf<double> d_u;
    phd::DevBuf<unsigned char> d_rsx;  // chunk partials + chunk-relative CDF (rs_parts)
    phd::DevBuf<unsigned> d_sync;      // k_shard_plan's / k_rs_step's hand-off words (PLAN_*), zero between launches
    // PHD_RS_FORM_BESIDE: the step's k_rs_step runs on `aux` beside part C, after
    // ev_terms (the log-weights final); ev_rs orders the context stream after it
    phd::Stream aux;
    phd::Event ev_terms, ev_rs;
};

/* The sharded step (phd_capi_shard.hip): plan buffers, the open plan's state.
 * ev_logw marks the last update's log-weights final (after the CPHD terms /
 * the split part A, else after the update: phd_wait_logw); the plan runs on
 * `stream` (phd_set_plan_stream, borrowed) and ev_plan orders the pack after it. */
struct ShardPlan {
    phd::DevBuf<int> d_mig;      // per-rank demand of a sharded resample
    phd::PinnedBuf<int> h_mig;   // host-mapped copy of d_mig, written by the plan's tail itself
    int* h_mig_dev = nullptr;    // its device address
    int h_mig_world = 0;         // world of the plans h_mig holds (its sequence word's slot depends on it)
    phd::DevBuf<int> d_pend;     // pending slots (records beyond the fixed blocks)
    bool open = false;           // a plan's counts not yet polled
    unsigned seq = 0;            // sequence number of the last plan launched (h_mig[3 world + MIG_SEQ] when done)
    int ovf_cap = 0;             // overflow capacity of the open plan (records)
    int world = 0, rank = 0;
    int pend_count = 0;          // pending slots of the last polled plan
    int max_blocks = 0;          // workgroups of k_shard_plan resident at once (0: not queried)
    int rec_dcap = 0;            // dynamic capacity of the record size phd_record_bytes last returned (0: the static record)
    phd::Event ev_logw, ev_plan;
    hipStream_t stream = nullptr;
};

/* per-update kernel timing (HIP events on the context stream; phd_capi_update.hip) */
struct Timing {
    std::vector<phd::Event> ev_a, ev_b;
    int next = 0, used = 0;
    int stride = 1, tick = 0;  // events around every stride-th update
};

/* mixed feature model (feature_model 2, phd_enable_dynamic): dynamic slab sets
 * (same slab ids as the static sets, own ping-pong index) + scratch */
struct Mixed {
    bool on = false;
    int dcap = 0, dcur = 0;
    phd::DevBuf<float> d_dmap[2];
    phd::DevBuf<int> d_dsize[2];
    // dynamic migration set X, the twin of Store::d_map_x / d_size_x (same slab
    // ids: bit 30 of d_src[p] selects both), allocated with the first receive
    // on a mixed context (phd_capi_shard.hip)
    phd::DevBuf<float> d_dmap_x;
    phd::DevBuf<int> d_dsize_x;
    bool x_live = false;  // a receive since the last full update: references may name set X (the predict advances it)
    phd::DevBuf<float> d_ekf, d_cand;
};

/* per-scan estimate trace (phd_capi_trace.hip): device rings of `cap` entries,
 * `count` appended so far (entry count % cap is written next), and the scratch
 * the two stages of phd_trace.hip hand each other */
struct Trace {
    int cap = 0, snap_cap = 0, K = 0;
    unsigned flags = 0;
    long count = 0;
    phd::DevBuf<phd_trace_record> d_rec;
    phd::DevBuf<phd_gaussian2d> d_snap;
    phd::DevBuf<float> d_card;
    phd::DevBuf<float> d_card_all;  // every particle's rows (the expected form, map_estimate & 2)
    phd::DevBuf<float> d_w;
    phd::DevBuf<double> d_part;
    phd::DevBuf<int> d_hand;
    phd::DevBuf<float> d_card_row;  // sharded trace: the arg-max particle's row before it is packed
    bool shard_packed = false;      // phd_trace_shard_pack enqueued, its phd_trace_shard_append not yet
    // mixed-model trace (phd_trace_enable_mixed): the parallel dyn ring, the
    // dynamic snapshots and the dynamic capacity it was enabled with
    bool mixed = false;
    int dsnap_cap = 0, dcap = 0;
    phd::DevBuf<phd_trace_dyn_record> d_drec;
    phd::DevBuf<phd_gaussian4d> d_dsnap;
    phd::DevBuf<double> d_dpart;
    phd::Event ev_trace;  // sharded trace: the gathered log-weights (plan stream) before the pack
};

struct phd_ctx {
    int device = 0;
    int n = 0;        // live particles (grows by n_predict_particles per predict until a resample)
    int n_base = 0;   // the filter's particle count (phd_ctx_create): a resample draws this many
    int nmax = 0;     // allocated particles: max(n_base, capacity.max_particles)
    phd_capacity cap{};
    phd::Stream stream;  // first of the owners: released last (phd_set_stream borrows the caller's)
    phd_slam_config cfg{};
    bool cfg_set = false;
    uint64_t seed = 0x5eed5eedULL;
    int merge_mode = 0;
    bool check_each_update = true;
    int index_offset = 0;  // global id of local particle 0 (noise counter)
    int rs_form = 0;       // PHD_RS_FORM_*: what the last phd_step launched (phd_last_resample_form)
    float* logw_mirror = nullptr;  // the next full update also writes its log-weights here (phd_predict_update)
    Store st;
    Scan z;
    UpdLaunch upd;
    Cphd cn;
    Resample rs;
    ShardPlan sh;
    Timing tm;
    Mixed mx;
    Trace tr;
    // scratch of no one stage
    phd::DevBuf<float> d_delta;
    phd::DevBuf<int> d_status;
    phd::DevBuf<int> d_err;  // error bits, serial-merge fallbacks, pair-list overflow walks, error statuses
    phd::DevBuf<phd_ackerman_noise> d_noise_a;
    phd::DevBuf<phd_cv_noise> d_noise_cv;
    phd::DevBuf<float> d_out;  // [0]=lse [1]=neff [2]=resample flag ...
    phd::DevBuf<float> d_cn;
    phd::DevBuf<unsigned long long> d_stamps;  // diagnostic builds (PHD_STAMPS)
    phd::EapScratch* eap = nullptr;  // expected-map scratch (phd_eap.hip), allocated on first use
    int eap_groups = 0;
    phd::Eap4Scratch* eap4 = nullptr;  // the dynamic maps' blocks form (phd_mixed.hip), allocated on first use
    int eap4_mode = 0;  // the dynamic expected map: 0 decision rounds, 1 the one workgroup only
    int eap4_rounds = 0, eap4_cells = 0;  // of the last dynamic expected map (single or blocks form)

    /* waits for the context stream, then the members release (the stream last) */
    ~phd_ctx() {
        (void)hipSetDevice(device);
        if (stream) (void)hipStreamSynchronize(stream);
        if (eap) phd::eap_free(eap);
        if (eap4) phd::eap4_free(eap4);
    }
};

/* ---- helpers one unit calls in another (defined in the unit named) ---- */

/* phd_capi_ctx.hip */
int set_device(phd_ctx* c);

/* phd_capi_update.hip */
int ensure_cn(phd_ctx* c);            // the CPHD cardinality rows, with the first CPHD use
int rec_cn_stride(const phd_ctx* c);  // cardinality doubles carried by a migration record (0 unless CPHD)
const void* update_kernel(int nt, int cphd, int part, int metric = 0, int predict = 0);
int apply_update_launch(phd_ctx* c, int threads_req);  // sizes the launch; c->upd changes only on success
int check_err(phd_ctx* ctx);
bool step_births_on(const phd_ctx* ctx);
int launch_step_births(phd_ctx* ctx, const int* slots, int count);
struct FusedPredict {
    int predict;  // 1 Ackerman, 2 CV
    phd_ackerman_control u;
    uint64_t step;
};
/* The one-launch resample of a phd_step that its update launch carries
 * (StepPlan): PHD_RS_FORM_LEAD in part C's lead workgroups, PHD_RS_FORM_BESIDE
 * on the auxiliary stream beside part C. */
struct RsBeside {
    int form;
    phd::RsStepArgs a;
};
/* what an update launch tells its callers */
struct UpdateDone {
    bool logw_final = false;  // it recorded ev_logw (the log-weights final: phd_wait_logw)
    bool rs_beside = false;   // the resample runs on `aux`: the context stream has to wait for ev_rs
};
int launch_update(phd_ctx* ctx, const FusedPredict* fused = nullptr, const int* slots = nullptr, int nslots = 0,
                  const RsBeside* rs = nullptr, UpdateDone* done = nullptr);

/* phd_capi_shard.hip */
/* dynamic capacity a migration record carries: 0 unless feature_model 2 (with
 * the PHD filter: the mixed model has no CPHD, so no cardinality rows) after
 * phd_enable_dynamic — then the record is record_words_mixed (phd_records.h) */
inline int rec_dcap(const phd_ctx* c) {
    return c->cfg_set && c->cfg.featureModel == PHD_FEATURE_MIXED && c->cfg.filterType == PHD_FILTER_PHD && c->mx.on
               ? c->mx.dcap
               : 0;
}
/* the dynamic migration set X beside the static one, sized like it (n slabs,
 * empty): with the first receive, and when phd_enable_dynamic changes the
 * capacity of a context that holds migrated slabs */
int ensure_dyn_x(phd_ctx* c);

/* phd_capi_step.hip */
phd::PredictCfg predict_cfg(const phd_slam_config& c, int index_offset);
int rs_mode(const phd_ctx* ctx);
size_t rs_lds(int n);
/* chunk partials + chunk-relative CDF of a chunked resample over n entries */
struct RsParts {
    unsigned long long* cdf_rel;
    double *part_sum, *part_s2;
    unsigned long long *part_tot, *part_key;
    float* part_max;
};
int rs_parts(phd_ctx* ctx, int n, RsParts& P);
int ensure_sync(phd_ctx* ctx);
int launch_rs_chunks(phd_ctx* ctx, hipStream_t st, float* w, int n, float* out, uint64_t seed, uint64_t step,
                     int* parents, bool remap = false, float new_logw = 0.f, bool fused_max = false,
                     unsigned* beyond = nullptr);
int enqueue_predict_update(phd_ctx* ctx, const phd_ackerman_control* u, int do_predict, uint64_t step,
                           const int* slots = nullptr, int nslots = 0, const RsBeside* rs = nullptr,
                           UpdateDone* done = nullptr);

/* phd_capi_trace.hip */
enum TraceUse { TRACE_ENABLE, TRACE_STEP, TRACE_SHARDED };
int trace_supported(const phd_ctx* ctx, TraceUse use);
int trace_append(phd_ctx* ctx, uint64_t step);

#pragma GCC visibility pop

extern "C" __global__ void k_iota(int* a, int n);  // phd_capi_ctx.hip
