/*
 * phd_trace.h — launch interface of the per-scan estimate trace (phd_trace.hip),
 * called by phd_step (phd_capi_step.hip) between the update and the resample, and
 * of its sharded form, called by phd_trace_shard_pack / phd_trace_shard_append.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "phd_types.h"

namespace phd {

/* particles per workgroup of the cardinality stage (4 waves, 8 particles each) */
#define TRACE_PB 32

/* 1: the dynamic half of the mixed-model trace (phd_trace_enable_mixed) is
 * compiled in; 0 leaves the static trace's kernels as they were without it */
#ifndef PHD_TRACE_DYN
#define PHD_TRACE_DYN 1
#endif
/* dynamic components per workgroup of the snapshot transpose (4 waves, one strip of 64 each) */
#define TRACE_DSNAP_PB 256

/* scratch words the stages hand each other (TraceArgs::hand) */
#define TRACE_H_PARTICLE 0 /* arg-max particle */
#define TRACE_H_SLAB 1     /* its slab reference (src[particle]) */
#define TRACE_H_ERRPREV 2  /* the status-error counter after the previous traced step */
#define TRACE_H_LSE 3      /* sharded trace: the log-sum-exp of the gathered log-weights (float bits) */
#define TRACE_H_WORDS 4

struct TraceArgs {
    /* the store, as k_cardinality reads it */
    const float* logw; /* un-normalised log-weights of the scan */
    const phd_pose* pose;
    const int* src;
    const float* map_in;
    const int* size_in;
    const float* map_x;
    const int* size_x;
    int n, cap;
    /* the scan */
    uint64_t step;
    int M, has_meas;
    float resample_thresh;
    const int* err; /* the context's error words ([3]: error statuses) */
    /* scratch */
    float* w_norm; /* n normalised log-weights (stage 1 -> stage 2) */
    double* part;  /* ceil(n / TRACE_PB) partial sums of card_expected */
    int* hand;     /* TRACE_H_* */
    /* this scan's ring entries */
    phd_trace_record* rec;
    phd_gaussian2d* snap; /* NULL: no snapshot */
    int snap_cap;
    /* cardinality distribution (NULL: off): the entry, and for the expected
     * form (map_estimate & 2) every particle's rows, n x K */
    float* card;
    const float* card_all;
    int K;
    /* the dynamic half of a mixed-model scan (dmap NULL: a static trace): the
     * dynamic slab set that is current after the update, [w | m0..m3 | c0..c15]
     * x dcap per slab, addressed by the same slab references as the static set */
    const float* dmap;
    const int* dsize;
    int dcap;
    double* dpart;             /* ceil(n / TRACE_PB) partial sums of the dynamic card_expected */
    phd_trace_dyn_record* drec; /* this scan's entry of the dyn ring */
    phd_gaussian4d* dsnap;      /* NULL: no dynamic snapshot */
    int dsnap_cap;
};

/* Stage 1 (weights final, parents not applied): one 1024-thread workgroup. */
void trace_launch_stage1(const TraceArgs& a, hipStream_t st);
/* Stage 2 (posterior maps written): cardinalities by blocks of particles, then
 * the fixed-order combine, the snapshot and the expected cardinality rows; with
 * a.dmap set also the dynamic half (same grid of k_trace_card, 1 + ceil(dsnap_cap
 * / TRACE_DSNAP_PB) more workgroups of k_trace_finish). */
void trace_launch_stage2(const TraceArgs& a, hipStream_t st);

/* ---- the trace of a sharded step (phd_trace_shard_pack / _append, phd_capi.h) ----
 * Every rank writes one fixed-size block, a flat run of 32-bit words:
 *   [0, 16)                 header, TRACE_BH_*; the other words zero
 *   [16, 16 + 6n)           the n local poses
 *   [.., + n)               the n local cardinalities, (float) Σ_j w_j
 *   [.., + 7 snap_cap)      the arg-max particle's map snapshot, phd_gaussian2d words
 *   [.., + K)               its cardinality row
 * rounded up to 4 words.  Snapshot and row are zero on the ranks that do not
 * own the arg-max particle.  The all-gathered blocks sit in rank order.
 * A mixed-model trace (phd_trace_shard_pack_mixed, K = 0) puts its dynamic half
 * behind those words, before the rounding:
 *   [.., + n)               the n local dynamic cardinalities, (float) Σ_j w_j
 *   [.., + 21 dsnap_cap)    the arg-max particle's dynamic snapshot, phd_gaussian4d words
 * the whole rounded up to 4 words; the snapshot is zero off the owner. */
#define TRACE_BH_WORDS 16
#define TRACE_BH_ERR 0   /* growth of the rank's status-error counter since its previous traced step */
#define TRACE_BH_OWNER 1 /* 1 on the rank that owns the arg-max particle */
#define TRACE_BH_SIZE 2  /* owner: components of that particle's map */
#define TRACE_BH_CARD 3  /* owner: its cardinality (float) */
#define TRACE_BH_DSIZE 4 /* mixed, owner: components of that particle's dynamic map */
#define TRACE_BH_DCARD 5 /* mixed, owner: its dynamic cardinality (float) */

inline size_t trace_block_words(int n, int snap_cap, int K) {
    const size_t w = TRACE_BH_WORDS + (size_t)(6 + 1) * n + (size_t)7 * snap_cap + (size_t)K;
    return (w + 3) & ~(size_t)3;
}
/* words of a block in front of its dynamic half (the static block, not rounded) */
inline size_t trace_block_dyn_offset(int n, int snap_cap, int K) {
    return TRACE_BH_WORDS + (size_t)(6 + 1) * n + (size_t)7 * snap_cap + (size_t)K;
}
inline size_t trace_block_words_mixed(int n, int snap_cap, int dsnap_cap) {
    const size_t w = trace_block_dyn_offset(n, snap_cap, 0) + (size_t)n + (size_t)21 * dsnap_cap;
    return (w + 3) & ~(size_t)3;
}

struct TraceShardArgs {
    const float* w_all; /* the world * n gathered un-normalised log-weights, rank order */
    int world, rank;
    /* this rank's store, as k_cardinality reads it */
    const phd_pose* pose;
    const int* src;
    const float* map_in;
    const int* size_in;
    const float* map_x;
    const int* size_x;
    int n, cap;
    /* the scan */
    uint64_t step;
    int M, has_meas;
    float resample_thresh;
    const int* err;
    int* hand;             /* TRACE_H_* */
    const float* card_row; /* the cardinality row of slab hand[TRACE_H_SLAB] (NULL: none) */
    int snap_cap, K;
    size_t block_words;
    float* block;        /* pack: this rank's block */
    const float* blocks; /* finish: the world gathered blocks */
    /* this scan's ring entries */
    phd_trace_record* rec;
    phd_gaussian2d* snap;
    float* card;
    /* the dynamic half of a mixed-model scan (dmap NULL: a static trace): the
     * dynamic slab set that is current after the update and the dynamic set X
     * (NULL until the first receive: no reference names it), addressed by the
     * same slab references as the static sets */
    const float* dmap;
    const int* dsize;
    const float* dmap_x;
    const int* dsize_x;
    int dcap, dsnap_cap;
    phd_trace_dyn_record* drec; /* this scan's entry of the dyn ring */
    phd_gaussian4d* dsnap;      /* NULL: no dynamic snapshot */
};

/* Stage 1 (w_all gathered): one 1024-thread workgroup, k_trace_weights'
 * arithmetic over all world * n entries; starts the record. */
void trace_launch_shard_weights(const TraceShardArgs& a, hipStream_t st);
/* Stage 2 (posterior maps written, before the plan's remap): this rank's block;
 * with a.dmap set the mixed form of the kernel, which also writes the dynamic half. */
void trace_launch_shard_pack(const TraceShardArgs& a, hipStream_t st);
/* Stage 4 (blocks gathered): the cross-rank sums in the single context's order
 * and the owner's entries; completes the record (a.dmap set: and the dyn
 * record and snapshot, by one more workgroup). */
void trace_launch_shard_finish(const TraceShardArgs& a, hipStream_t st);

}  // namespace phd
