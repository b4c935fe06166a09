/*
 * phd_records.hip — the migration records of the sharded step on gfx950: the
 * record codec, the block / overflow addressing and the five kernels that move
 * particles between a context's store and record buffers (layout and launch
 * interface: phd_records.h).  One 256-thread workgroup handles one record at a
 * time.  Every kernel comes with (DYN) and without the dynamic part; the
 * static form carries no dynamic code.
 */
#include <hip/hip_runtime.h>

#include <cstdint>

#include "phd_kernels.h" /* MIG_*: the plan's counts the block forms read */
#include "phd_records.h"

namespace phd {

/* ---- codec ---- */

/* The first sz components of nf rows (row stride `stride` on both sides), one
 * float at a time; consecutive threads take consecutive components of a row. */
__device__ __forceinline__ void copy_rows(float* __restrict__ d, const float* __restrict__ s, int nf, int stride,
                                          int sz) {
    for (int f = 0; f < nf; f++)
        for (int k = threadIdx.x; k < sz; k += blockDim.x) d[f * stride + k] = s[f * stride + k];
}

/* The first sz components of the PHD_DYN_FIELDS rows of a dynamic map (row
 * stride dcap on both sides): whole quads of a row as float4 when both sides
 * and the stride are 16-byte aligned, the up to three components left of each
 * row (or everything, unaligned) one float at a time.  Consecutive threads
 * take consecutive quads / components of a row. */
__device__ __forceinline__ void copy_dyn_rows(float* __restrict__ d, const float* __restrict__ s, int dcap, int sz) {
    const bool vec = (dcap & 3) == 0 && ((((uintptr_t)d) | ((uintptr_t)s)) & 15) == 0;
    const int nq = vec ? sz >> 2 : 0;
    for (int i = threadIdx.x; i < PHD_DYN_FIELDS * nq; i += blockDim.x) {
        const int f = i / nq, q = i - f * nq;
        ((float4*)(d + (size_t)f * dcap))[q] = ((const float4*)(s + (size_t)f * dcap))[q];
    }
    const int t0 = nq << 2, nt = sz - t0;
    for (int i = threadIdx.x; i < PHD_DYN_FIELDS * nt; i += blockDim.x) {
        const int f = i / nt, k = t0 + (i - f * nt);
        d[(size_t)f * dcap + k] = s[(size_t)f * dcap + k];
    }
}

template <bool DYN>
__device__ __forceinline__ size_t rec_words(const RecordStore& S) {
    return DYN ? record_words_mixed(S.cap, S.cn_stride, S.dcap) : record_words(S.cap, S.cn_stride);
}

/* One workgroup writes particle p's record at o, from the slabs its reference names. */
template <bool DYN>
__device__ __forceinline__ void record_write(const RecordStore& S, float* __restrict__ o, int p, float logw) {
    const int sref = S.src[p];
    const int sz = slab_size(sref, S.size_in, S.size_x);
    if (threadIdx.x == 0) {
        const float* pf = (const float*)&S.pose[p];
        for (int k = 0; k < 6; k++) o[k] = pf[k];
        o[6] = logw;
        ((int*)o)[7] = sz;
    }
    copy_rows(o + 8, slab_map(sref, S.map_in, (const float*)S.map_x, S.cap), PHD_NF, S.cap, sz);
    if (S.cn_stride) {  // CPHD cardinality coefficients travel with the particle
        double* co = (double*)(o + 8 + (size_t)PHD_NF * S.cap);
        const double* cs = slab_cn(sref, S.cn, S.cn_x, S.cn_stride);
        for (int k = threadIdx.x; k < S.cn_stride; k += blockDim.x) co[k] = cs[k];
    }
    if (DYN) {
        const int dsz = min(max(slab_size(sref, S.dsize_in, S.dsize_x), 0), S.dcap);
        float* od = o + record_dyn_offset(S.cap, S.cn_stride);
        if (threadIdx.x < PHD_REC_DYN_HEAD) ((int*)od)[threadIdx.x] = threadIdx.x == 0 ? dsz : 0;
        copy_dyn_rows(od + PHD_REC_DYN_HEAD, dyn_slab_map(sref, S.dmap_in, (const float*)S.dmap_x, S.dcap), S.dcap, dsz);
    }
}

/* One workgroup reads the record at o into particle p, which then refers to
 * slab xs of the sets X; with_map: this workgroup also fills that slab (the
 * first of the particles that share the record). */
template <bool DYN>
__device__ __forceinline__ void record_read(const RecordStore& S, const float* __restrict__ o, int p, int xs,
                                            bool with_map) {
    const int sz = min(max(((const int*)o)[7], 0), S.cap);  // a record never carries more than cap
    if (threadIdx.x == 0) {
        float* pd = (float*)&S.pose[p];
        for (int k = 0; k < 6; k++) pd[k] = o[k];
        S.logw[p] = o[6];
        S.src[p] = xs | PHD_SLAB_X;
        if (with_map) S.size_x[xs] = sz;
    }
    if (!with_map) return;
    copy_rows(S.map_x + (size_t)xs * PHD_NF * S.cap, o + 8, PHD_NF, S.cap, sz);
    if (S.cn_stride) {
        const double* ci = (const double*)(o + 8 + (size_t)PHD_NF * S.cap);
        for (int k = threadIdx.x; k < S.cn_stride; k += blockDim.x) S.cn_x[(size_t)xs * S.cn_stride + k] = ci[k];
    }
    if (DYN) {
        const float* od = o + record_dyn_offset(S.cap, S.cn_stride);
        const int dsz = min(max(((const int*)od)[0], 0), S.dcap);  // ... nor more than dcap
        if (threadIdx.x == 0) S.dsize_x[xs] = dsz;
        copy_dyn_rows(S.dmap_x + (size_t)xs * PHD_DYN_FIELDS * S.dcap, od + PHD_REC_DYN_HEAD, S.dcap, dsz);
    }
}

/* ---- block / overflow addressing ----
 * A rank's records are numbered grouped by peer, cnt[q] of peer q (the sender:
 * mig + world, by destination; the receiver: mig + 2 world, by source).  Record
 * t is the r-th of its peer: block slot peer * K + r when r < K, else position
 * ovf_first + r - K of the overflow buffer, ovf_first = Σ_{q < peer} max(cnt[q] - K, 0). */
struct RecordSlot {
    int peer, r, ovf_first;
};
__device__ __forceinline__ RecordSlot record_slot(const int* __restrict__ cnt, int world, int K, int t) {
    int q = 0, first = 0, ofirst = 0;
    while (q < world - 1 && t >= first + cnt[q]) {
        first += cnt[q];
        ofirst += max(cnt[q] - K, 0);
        q++;
    }
    return RecordSlot{q, t - first, ofirst};
}

/* ---- kernels (phd_records.h: records_*) ---- */

template <bool DYN>
__global__ void __launch_bounds__(256) k_pack(RecordStore S, const int* __restrict__ dcount,
                                              const int* __restrict__ src_idx, int count, int logw_set,
                                              float logw_value, float* __restrict__ rec) {
    if (dcount) count = min(*dcount, count);
    const size_t rw = rec_words<DYN>(S);
    for (int r = blockIdx.x; r < count; r += gridDim.x) {
        const int p = src_idx[r];
        record_write<DYN>(S, rec + (size_t)r * rw, p, logw_set ? logw_value : S.logw[p]);
    }
}

template <bool DYN>
__global__ void __launch_bounds__(256) k_unpack(RecordStore S, const float* __restrict__ rec,
                                                const int* __restrict__ dst_idx, int count) {
    const int r = blockIdx.x;
    if (r >= count) return;
    record_read<DYN>(S, rec + (size_t)r * rec_words<DYN>(S), dst_idx[r], r, true);
}

template <bool DYN>
__global__ void __launch_bounds__(256) k_unpack_slots(RecordStore S, const float* __restrict__ rec,
                                                      const int* __restrict__ slot_rec, int nslots, int first_slot) {
    const int i = blockIdx.x;
    if (i >= nslots) return;
    const int r = slot_rec[i];
    record_read<DYN>(S, rec + (size_t)r * rec_words<DYN>(S), first_slot + i, r, !(i > 0 && slot_rec[i - 1] == r));
}

template <bool DYN>
__global__ void __launch_bounds__(256) k_pack_blocks(RecordStore S, const int* __restrict__ mig, int world,
                                                     const int* __restrict__ send_src, int block_records,
                                                     int ovf_capacity, float logw_value, float* __restrict__ blocks,
                                                     float* __restrict__ ovf, int* __restrict__ ovf_flag) {
    const int count = mig[3 * world + MIG_SENT];
    const size_t rw = rec_words<DYN>(S);
    const int K = block_records;
    for (int t = blockIdx.x; t < count; t += gridDim.x) {
        const RecordSlot a = record_slot(mig + world, world, K, t);
        float* o;
        if (a.r < K) {
            o = blocks + ((size_t)a.peer * K + a.r) * rw;
        } else {
            const int oi = a.ovf_first + a.r - K;
            if (oi >= ovf_capacity) {
                if (threadIdx.x == 0) ovf_flag[0] = 1;
                continue;
            }
            o = ovf + (size_t)oi * rw;
        }
        record_write<DYN>(S, o, send_src[t], logw_value);
    }
}

/* Strided over a grid of min(n, 256) workgroups (the deficit is read on the
 * device): a step that moves nothing costs one short wave each. */
template <bool DYN>
__global__ void __launch_bounds__(256) k_unpack_blocks(RecordStore S, const float* __restrict__ blocks,
                                                       const float* __restrict__ ovf, int block_records, int overflow,
                                                       const int* __restrict__ mig, int world, int rank,
                                                       const int* __restrict__ recv_rec, int n) {
    const int d = min(mig[rank], n);
    const int K = block_records;
    const size_t rw = rec_words<DYN>(S);
    for (int i = blockIdx.x; d + i < n; i += gridDim.x) {
        const int rho = recv_rec[i];
        const RecordSlot a = record_slot(mig + 2 * world, world, K, rho);
        if ((a.r >= K) != (overflow != 0)) continue;  // the other pass's record
        const float* o =
            a.r < K ? blocks + ((size_t)a.peer * K + a.r) * rw : ovf + (size_t)(a.ovf_first + a.r - K) * rw;
        record_read<DYN>(S, o, d + i, rho, !(i > 0 && recv_rec[i - 1] == rho));
    }
}

/* ---- launches ---- */

#define REC_LAUNCH(K, grid, s, ...)                                                           \
    do {                                                                                      \
        if (S.dcap > 0)                                                                       \
            hipLaunchKernelGGL(K<true>, dim3(grid), dim3(256), 0, s, S, __VA_ARGS__);         \
        else                                                                                  \
            hipLaunchKernelGGL(K<false>, dim3(grid), dim3(256), 0, s, S, __VA_ARGS__);        \
        return hipGetLastError();                                                             \
    } while (0)

hipError_t records_pack(const RecordStore& S, int grid, const int* dcount, const int* src_idx, int count, int logw_set,
                        float logw_value, float* rec, hipStream_t s) {
    REC_LAUNCH(k_pack, grid, s, dcount, src_idx, count, logw_set, logw_value, rec);
}

hipError_t records_unpack(const RecordStore& S, const float* rec, const int* dst_idx, int count, hipStream_t s) {
    REC_LAUNCH(k_unpack, count, s, rec, dst_idx, count);
}

hipError_t records_unpack_slots(const RecordStore& S, const float* rec, const int* slot_rec, int nslots, int first_slot,
                                hipStream_t s) {
    REC_LAUNCH(k_unpack_slots, nslots, s, rec, slot_rec, nslots, first_slot);
}

hipError_t records_pack_blocks(const RecordStore& S, int grid, const int* mig, int world, const int* send_src,
                               int block_records, int ovf_capacity, float logw_value, float* blocks, float* ovf,
                               int* ovf_flag, hipStream_t s) {
    REC_LAUNCH(k_pack_blocks, grid, s, mig, world, send_src, block_records, ovf_capacity, logw_value, blocks, ovf,
               ovf_flag);
}

hipError_t records_unpack_blocks(const RecordStore& S, int grid, const float* blocks, const float* ovf,
                                 int block_records, int overflow, const int* mig, int world, int rank,
                                 const int* recv_rec, int n, hipStream_t s) {
    REC_LAUNCH(k_unpack_blocks, grid, s, blocks, ovf, block_records, overflow, mig, world, rank, recv_rec, n);
}

#undef REC_LAUNCH

}  // namespace phd
