/* phd_step_plan.h — which resample form a phd_step takes, decided once from
 * plain values before anything is enqueued (phd_capi_step.hip follows the plan).
 * Host C++17, no HIP: tests/step_plan_harness.cpp builds it by itself. */
#pragma once

#include <cstddef>

#include "phd_capi.h"

namespace phd {

/* entries per workgroup of the chunked resample (phd_capi_step.hip asserts it RS_THREADS) */
constexpr int kRsChunk = 1024;

struct StepFacts {
    int n;                    // live particles at the step's start
    int n_base;               // the filter's particle count (a resample draws this many)
    int n_predict_particles;  // children per predict (> 1: the live count grows with the step's predict)
    int M;                    // measurements of the step's scan
    int filter_type;          // PHD_FILTER_*
    int feature_model;        // PHD_FEATURE_*
    int upd_split;            // the update runs as part A + part C
    int upd_resident;         // part C workgroups resident at once
    size_t upd_lds;           // part C's dynamic LDS
    size_t rs_step_lds;       // rs_step_lds(upd_threads): what the lead workgroup's resample takes of it
    bool traced;              // phd_trace_enable: the step appends a trace entry
    bool stamps;              // part C records diagnostic stamps (PHD_STAMPS builds)
    int overlap_bits;         // PHD_RS_OVERLAP
    int lead_on;              // PHD_RS_LEAD
};

struct StepPlan {
    int form;       // PHD_RS_FORM_*
    bool fuse_max;  // the chunked forms: no k_rs_max launch
};

inline StepPlan plan_step(const StepFacts& f) {
    StepPlan p;
    // chunked normalise up to 16 chunks: each block takes the max of all
    // entries itself instead of a k_rs_max launch (same max, same bits)
    p.fuse_max = f.n <= 16 * kRsChunk;
    if (f.n_predict_particles > 1 || f.n != f.n_base) {
        // live count above n_particles: the resample draws n_particles children
        // and the next step's launches depend on the decision, so it is read
        // back (one host synchronisation per step in this mode)
        p.form = PHD_RS_FORM_SEPARATE;
        return p;
    }
    if (f.n <= 2 * kRsChunk) {  // one launch: a single block is fastest here
        p.form = PHD_RS_FORM_BLOCK;
        return p;
    }
    // PHD_RS_OVERLAP: the one-launch resample beside part C of a CPHD step (its
    // log-weights are final after the terms launch, bit 1) or of a split PHD
    // step (final after part A, bit 2); the fused PHD update has no part C and
    // leaves it to the main stream.  Its workgroups wait out part C on their
    // CUs, so only while part C is a few rounds of resident workgroups (config
    // 4's per-GPU shard, 2.7 rounds: 3 409 -> 3 504 steps/s; config 5's, 16
    // rounds: 674 -> 645).
    // A traced step (phd_trace_enable) reads the poses and the log-weights the
    // resample rewrites: its resample runs after the update and the trace.
    const bool overlap =
        !f.traced &&
        (f.filter_type == PHD_FILTER_CPHD ? (f.overlap_bits & 1) != 0 : f.upd_split && (f.overlap_bits & 2) != 0) &&
        (long)f.n <= 4L * f.upd_resident && p.fuse_max && f.M > 0 && f.feature_model == PHD_FEATURE_STATIC;
    if (!overlap) {
        p.form = p.fuse_max ? PHD_RS_FORM_STEP : PHD_RS_FORM_CHUNKS;
        return p;
    }
    // PHD_RS_LEAD: part C's lead workgroup runs it (rs_step_block): the launch
    // gets RS_LEAD_WGS workgroups in front (the others return at once, so every
    // particle keeps its XCD) and no event crosses streams.  The diagnostic
    // stamps build indexes its records by workgroup: it keeps the second
    // stream.  Part C's LDS must hold rs_step_block's tables: with small
    // capacities it does not, and the resample takes the second stream too.
    p.form = f.lead_on && !f.stamps && f.upd_lds >= f.rs_step_lds ? PHD_RS_FORM_LEAD : PHD_RS_FORM_BESIDE;
    return p;
}

}  // namespace phd
