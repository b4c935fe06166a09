/*
 * phd_slab.h — the one place that decodes a slab reference (the migration
 * record's layout: phd_records.h).  Particle p's map is slab `src[p]` of the index
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

/* floats of one dynamic component (mixed contexts): rows [w | m0..m3 | c0..c15] */
#define PHD_DYN_FIELDS 21
/* the dynamic map a reference names: the slab of the same id in the current
 * dynamic set or in dynamic set X (its size: slab_size on the dynamic sizes) */
template <class T>
__host__ __device__ inline T* dyn_slab_map(int sref, T* dmap_in, T* dmap_x, int dcap) {
    return (slab_in_x(sref) ? dmap_x : dmap_in) + (size_t)slab_index(sref) * PHD_DYN_FIELDS * dcap;
}

}  // namespace phd
