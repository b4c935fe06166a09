/*
 * phd_records.h — the migration record of the sharded step: its layout, the
 * view of a context's store its kernels work on, and their launches
 * (phd_records.hip).  One record format and one set of kernels for the static
 * PHD, the CPHD and the mixed static + dynamic store.
 *
 * Record, 32-bit words:
 *   [pose 6 | logw | size | map PHD_NF * cap]   rows [w | mx | my | P00 | P10 |
 *                                               P01 | P11] of cap floats, the
 *                                               first `size` of each live
 *   [cn_stride doubles]                         CPHD: cardinality coefficients
 * and, with a dynamic capacity (feature_model 2 after phd_enable_dynamic,
 * dcap > 0), padded to a multiple of 4 words, the dynamic part
 *   [dsize | 3 reserved words (0) | dmap PHD_DYN_FIELDS * dcap]
 * (rows [w | m0..m3 | c0..c15] of dcap floats, the first dsize of each live),
 * the whole padded to a multiple of 4 words again: in a 16-byte aligned buffer
 * every record, every dynamic part and (dcap a multiple of 4) every row starts
 * on 16 bytes.  dcap == 0: the static / CPHD record ends after its first part.
 */
#pragma once
#include <hip/hip_runtime.h>

#include "phd_slab.h"
#include "phd_types.h"

#define PHD_REC_DYN_HEAD 4 /* words before the dynamic rows */

namespace phd {

__host__ __device__ inline size_t record_words(int cap, int cn_stride) {
    return 8 + (size_t)PHD_NF * cap + 2 * (size_t)cn_stride;
}
__host__ __device__ inline size_t record_dyn_offset(int cap, int cn_stride) {
    return (record_words(cap, cn_stride) + 3) & ~(size_t)3;
}
__host__ __device__ inline size_t record_words_mixed(int cap, int cn_stride, int dcap) {
    if (dcap <= 0) return record_words(cap, cn_stride);
    return (record_dyn_offset(cap, cn_stride) + PHD_REC_DYN_HEAD + (size_t)PHD_DYN_FIELDS * dcap + 3) & ~(size_t)3;
}

/* What the record kernels see of a context.  Records are written from the
 * slab a particle's reference names (the current sets or the sets X) and read
 * into the sets X.  Static PHD: cn_stride == 0 and dcap == 0 (cn / dynamic
 * pointers unused); CPHD: cn_stride > 0; mixed PHD: dcap > 0. */
struct RecordStore {
    int cap, cn_stride, dcap;
    int* src;
    const float* map_in;  // current static set
    const int* size_in;
    float* map_x;         // static set X
    int* size_x;
    const double* cn;     // cardinality rows of the current set / of set X
    double* cn_x;
    const float* dmap_in; // current dynamic set
    const int* dsize_in;
    float* dmap_x;        // dynamic set X
    int* dsize_x;
    phd_pose* pose;
    float* logw;
};

/* Each launches the kernel's form for S.dcap (with or without the dynamic
 * part) on stream s: one 256-thread workgroup per record at a time. */

/* Records src_idx[0 .. count) -> rec; `dcount` (device) overrides `count` when
 * given (records beyond it are not written); `grid` workgroups stride over the
 * records.  logw_set != 0 writes logw_value as the record's log-weight (a
 * sharded resample's -log N). */
hipError_t records_pack(const RecordStore& S, int grid, const int* dcount, const int* src_idx, int count, int logw_set,
                        float logw_value, float* rec, hipStream_t s);
/* Record r -> slab r of the sets X; particle dst_idx[r] points at it. */
hipError_t records_unpack(const RecordStore& S, const float* rec, const int* dst_idx, int count, hipStream_t s);
/* Slot first_slot + i takes record slot_rec[i]: the first of the consecutive
 * slots of a record copies its maps into slab slot_rec[i] of the sets X, every
 * slot of the record points at that slab. */
hipError_t records_unpack_slots(const RecordStore& S, const float* rec, const int* slot_rec, int nslots, int first_slot,
                                hipStream_t s);
/* The sender's records in fixed blocks: record t of send_src (grouped by
 * destination, mig[world + d] each) is the r-th record to rank d: block slot
 * d * block_records + r, or — beyond the block — position
 * Σ_{d' < d} max(sent_d' - K, 0) + r - K of the overflow buffer (ovf_flag[0] =
 * 1 and the record dropped when that is past ovf_capacity).  Records carry
 * logw_value. */
hipError_t records_pack_blocks(const RecordStore& S, int grid, const int* mig, int world, const int* send_src,
                               int block_records, int ovf_capacity, float logw_value, float* blocks, float* ovf,
                               int* ovf_flag, hipStream_t s);
/* Receive side: deficit slot mig[rank] + i of n takes record recv_rec[i]
 * (numbered in source-rank order, mig[2 world + s] from source s), from the
 * fixed blocks (overflow == 0) or from the received overflow buffer (!= 0; the
 * other pass's records are skipped), addressed as records_pack_blocks wrote
 * them; maps as records_unpack_slots. */
hipError_t records_unpack_blocks(const RecordStore& S, int grid, const float* blocks, const float* ovf,
                                 int block_records, int overflow, const int* mig, int world, int rank,
                                 const int* recv_rec, int n, hipStream_t s);

}  // namespace phd
