/*
 * phd_slab.h — the one place that decodes a slab reference and that knows the
 * particle record's layout.  Particle p's map is slab `src[p]` of the index
 * table: 7 SoA rows of `cap` floats
 * [w | mx | my | P00 | P10 | P01 | P11] in the current set or in set X.
 */
#pragma once
#include <hip/hip_runtime.h>

#include "phd_types.h"

#define PHD_NF 7 /* fields per component */

/* slab reference encoding in the index table: bit 30 selects the migration set X */
#define PHD_SLAB_X 0x40000000
#define PHD_SLAB_MASK 0x3fffffff

namespace phd {

__host__ __device__ inline bool slab_in_x(int sref) { return (sref & PHD_SLAB_X) != 0; }
__host__ __device__ inline int slab_index(int sref) { return sref & PHD_SLAB_MASK; }

/* the map rows / component count / cardinality coefficients a reference names */
template <class T>
__host__ __device__ inline T* slab_map(int sref, T* map_in, T* map_x, int cap) {
    return (slab_in_x(sref) ? map_x : map_in) + (size_t)slab_index(sref) * PHD_NF * cap;
}
__host__ __device__ inline int slab_size(int sref, const int* size_in, const int* size_x) {
    return slab_in_x(sref) ? size_x[slab_index(sref)] : size_in[slab_index(sref)];
}
__host__ __device__ inline const double* slab_cn(int sref, const double* cn, const double* cn_x, int cn_stride) {
    return (slab_in_x(sref) ? cn_x : cn) + (size_t)slab_index(sref) * cn_stride;
}

struct Slab { const float* map; int size; };
__device__ __forceinline__ Slab slab_of(int sref, const float* map_in, const int* size_in, const float* map_x,
                                        const int* size_x, int cap) {
    return Slab{slab_map(sref, map_in, map_x, cap), slab_size(sref, size_in, size_x)};
}

/* Particle record (cross-rank migration): [pose 6 | logw | size | map 7*cap]
 * 32-bit words, then (CPHD contexts) cn_stride doubles of cardinality
 * coefficients. */
__host__ __device__ inline size_t record_words(int cap, int cn_stride) {
    return 8 + (size_t)PHD_NF * cap + 2 * (size_t)cn_stride;
}

/* Mixed contexts (feature_model 2 after phd_enable_dynamic, dcap > 0): the
 * record above, padded to a multiple of 4 words, then the dynamic part
 *   [dsize | 3 reserved words (0) | dmap PHD_DYN_FIELDS * dcap]
 * (rows [w | m0..m3 | c0..c15] of dcap floats, the first dsize of each live),
 * the whole padded to a multiple of 4 words again: in a 16-byte aligned buffer
 * every record, every dynamic part and (dcap a multiple of 4) every row starts
 * on 16 bytes.  dcap == 0: the static / CPHD record, unchanged. */
#define PHD_DYN_FIELDS 21
#define PHD_REC_DYN_HEAD 4 /* words before the dynamic rows */
/* the dynamic map a reference names: the slab of the same id in the current
 * dynamic set or in dynamic set X (its size: slab_size on the dynamic sizes) */
template <class T>
__host__ __device__ inline T* dyn_slab_map(int sref, T* dmap_in, T* dmap_x, int dcap) {
    return (slab_in_x(sref) ? dmap_x : dmap_in) + (size_t)slab_index(sref) * PHD_DYN_FIELDS * dcap;
}
__host__ __device__ inline size_t record_dyn_offset(int cap, int cn_stride) {
    return (record_words(cap, cn_stride) + 3) & ~(size_t)3;
}
__host__ __device__ inline size_t record_words_mixed(int cap, int cn_stride, int dcap) {
    if (dcap <= 0) return record_words(cap, cn_stride);
    return (record_dyn_offset(cap, cn_stride) + PHD_REC_DYN_HEAD + (size_t)PHD_DYN_FIELDS * dcap + 3) & ~(size_t)3;
}

/* One workgroup writes particle `ps`'s record at o: its map `s`, and its
 * cardinality coefficients `cs` when cn_stride != 0. */
__device__ __forceinline__ void record_write(float* o, int cap, int cn_stride, const phd_pose* ps, float logw,
                                             const Slab& s, const double* cs) {
    if (threadIdx.x == 0) {
        const float* pf = (const float*)ps;
        for (int k = 0; k < 6; k++) o[k] = pf[k];
        o[6] = logw;
        ((int*)o)[7] = s.size;
    }
    for (int f = 0; f < PHD_NF; f++)
        for (int k = threadIdx.x; k < s.size; k += blockDim.x) o[8 + f * cap + k] = s.map[f * cap + k];
    if (cn_stride) {  // CPHD cardinality coefficients travel with the particle
        double* co = (double*)(o + 8 + (size_t)PHD_NF * cap);
        for (int k = threadIdx.x; k < cn_stride; k += blockDim.x) co[k] = cs[k];
    }
}

/* One workgroup reads the record at o into particle p, which then refers to
 * migration slab xs of set X; with_map: this workgroup also fills that slab
 * (the first of the particles that share the record). */
__device__ __forceinline__ void record_read(const float* o, int cap, int cn_stride, int p, int xs, bool with_map,
                                            float* map_x, int* size_x, int* src, phd_pose* pose, float* logw,
                                            double* cn_x) {
    const int sz = min(max(((const int*)o)[7], 0), cap);  // a record never carries more than cap
    if (threadIdx.x == 0) {
        float* pd = (float*)&pose[p];
        for (int k = 0; k < 6; k++) pd[k] = o[k];
        logw[p] = o[6];
        src[p] = xs | PHD_SLAB_X;
        if (with_map) size_x[xs] = sz;
    }
    if (!with_map) return;
    float* d = map_x + (size_t)xs * PHD_NF * cap;
    for (int f = 0; f < PHD_NF; f++)
        for (int k = threadIdx.x; k < sz; k += blockDim.x) d[f * cap + k] = o[8 + f * cap + k];
    if (cn_stride) {
        const double* ci = (const double*)(o + 8 + (size_t)PHD_NF * cap);
        for (int k = threadIdx.x; k < cn_stride; k += blockDim.x) cn_x[(size_t)xs * cn_stride + k] = ci[k];
    }
}

}  // namespace phd
