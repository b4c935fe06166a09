/*
 * phd_trace.h — launch interface of the per-scan estimate trace (phd_trace.hip),
 * called by phd_step (phd_capi.hip) between the update and the resample.
 */
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "phd_types.h"

namespace phd {

/* particles per workgroup of the cardinality stage (4 waves, 8 particles each) */
#define TRACE_PB 32

/* scratch words the stages hand each other (TraceArgs::hand) */
#define TRACE_H_PARTICLE 0 /* arg-max particle */
#define TRACE_H_SLAB 1     /* its slab reference (src[particle]) */
#define TRACE_H_ERRPREV 2  /* the status-error counter after the previous traced step */
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
};

/* Stage 1 (weights final, parents not applied): one 1024-thread workgroup. */
void trace_launch_stage1(const TraceArgs& a, hipStream_t st);
/* Stage 2 (posterior maps written): cardinalities by blocks of particles, then
 * the fixed-order combine, the snapshot and the expected cardinality rows. */
void trace_launch_stage2(const TraceArgs& a, hipStream_t st);

}  // namespace phd
