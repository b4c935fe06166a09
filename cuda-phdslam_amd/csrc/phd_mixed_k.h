/*
 * phd_mixed_k.h — launch interface of the mixed static + dynamic feature model
 * kernels (phd_mixed.hip; SURVEY.md §8(f) rank 4, feature_model = 2).
 *
 * Dynamic maps live in their own ping-pong slab sets, indexed by the same slab
 * id as the static maps (particle n's maps are slab d_src[n] of each set), so
 * resampling and the n_predict_particles spawn (index remaps of d_src) carry
 * them with no copy.  Dynamic slab: SoA [w | m0..m3 | c0..c15] x dcap floats.
 */
#ifndef PHD_MIXED_K_H
#define PHD_MIXED_K_H

#include <hip/hip_runtime.h>

#include <string>

#include "phd_mixed.h"
#include "phd_slab.h"
#include "phd_types.h"

namespace phd {

/* (PHD_DYN_FIELDS, the floats of one dynamic component: phd_slab.h) */
/* status bits (phd_kernels.h PHD_ST_CANDIDATE_OVERFLOW / PHD_ST_MAP_OVERFLOW) */
#define PHD_ST_CANDIDATE_OVERFLOW_MX 2
#define PHD_ST_MAP_OVERFLOW_MX 4

struct MixedArgs {
    int n;            // particles (one workgroup each)
    int cap, dcap;    // static / dynamic slab capacities
    int M, Kcap;      // measurements, candidate capacity per map
    const int* slots; // NULL: block b does particle b; else particle slots[b] (n blocks)
    const int* src;   // slab reference of particle p: the input sets, or (bit 30) the sets X
    int* src_reset;   // posterior of particle p -> output slab p
    const float* map_in;
    float* map_out;
    const int* size_in;
    int* size_out;
    const float* map_x;  // static migration set X (NULL before the first receive)
    const int* size_x;
    const float* dmap_in;
    float* dmap_out;
    const int* dsize_in;
    int* dsize_out;
    const float* dmap_x;  // dynamic migration set X
    const int* dsize_x;
    const phd_pose* poses;
    float* logw;
    float* delta;
    int* status;
    int* err;
    const float* zr;
    const float* zb;
    const int* zlab;
    phd_mx_cfg c;
    float* ekf;       // per particle (cap + dcap) x 32 floats
    float* cand;      // per particle Kcap x (7 + 21) floats
};

/* dynamic LDS bytes of k_update_mixed */
size_t mixed_lds_bytes(int cap, int dcap, int Mcap, int Kcap);
/* per-particle global scratch (floats) */
size_t mixed_ekf_floats(int cap, int dcap);
size_t mixed_cand_floats(int Kcap);

hipError_t mixed_launch_update(const MixedArgs& a, size_t lds, hipStream_t s);
/* one predictMapMixed over `nslabs` slabs: set in -> set out */
hipError_t mixed_launch_predict(int nslabs, int dcap, const float* din, const int* dsize_in, float* dout,
                                int* dsize_out, const phd_mx_cfg& c, hipStream_t s);
/* predictMapMixed of the dynamic migration set X, in place (each thread reads
 * and writes its own component only).  slots == NULL: every one of the `count`
 * slabs of X.  Else one workgroup per listed slot, `count` of them: the slab
 * the slot's reference names in X, predicted by the first of the consecutive
 * slots that name it (a sharded plan lists its pending slots in slot order and
 * the slots of one record are consecutive: once per slab); a slot that does
 * not refer to X is left alone (its slab of the current set went with the
 * full predict). */
hipError_t mixed_launch_predict_x(const int* slots, int count, const int* src, int dcap, float* dmap_x,
                                  const int* dsize_x, const phd_mx_cfg& c, hipStream_t s);
hipError_t mixed_set_lds_limit();

/* EAP map of the dynamic maps of n particles (exp_map_dynamic): the component
 * count (nothing copied when out is NULL or too small), -1 on a HIP error;
 * d_dmap_x / d_dsize_x: the dynamic set X (NULL: no reference names it).
 * mode 0: decision rounds over the whole GPU (the one workgroup for inputs the
 * lattice bound does not cover), 1: the one workgroup only — the same bytes.
 * *rounds / *cells: the decision rounds and occupied lattice cells of this
 * call (1, 0 for the one-workgroup form; 0, 0 for an empty set). */
long mixed_expected_map_dynamic(hipStream_t st, const int* d_src, const float* d_dmap, const int* d_dsize,
                                const float* d_dmap_x, const int* d_dsize_x, int n, int dcap, const float* d_logw, float T, phd_gaussian4d* out, long out_cap,
                                int mode, int* rounds, int* cells, std::string& err);

/* The sharded form (the "EAP4" block: include/phd_capi.h).  eap4_shard_count:
 * the dynamic components of the store, clamped per particle to dcap (-1: a HIP
 * error).  eap4_shard_pack: this rank's block, enqueued after the same
 * read-back; 0, -1 on a HIP error, -2 when the store holds more than K_max
 * components (nothing is then written).  mixed_expected_map_dynamic_blocks:
 * the map of `world` gathered blocks, as mixed_expected_map_dynamic; -2 when a
 * header is refused (err names the rank; no field is read) or the blocks hold
 * 2^31 - 1 components or more.  The scratch is the context's, grown on demand
 * (eap4_free releases it). */
struct Eap4Scratch;
void eap4_free(Eap4Scratch* s);
size_t eap4_block_bytes(long K_max);
long eap4_shard_count(hipStream_t st, const int* d_src, const int* d_dsize, const int* d_dsize_x, int n, int dcap,
                      std::string& err);
int eap4_shard_pack(Eap4Scratch** sp, hipStream_t st, const int* d_src, const float* d_dmap, const int* d_dsize,
                    const float* d_dmap_x, const int* d_dsize_x, const float* d_logw, int n, int dcap, long K_max,
                    void* d_block, std::string& err);
long mixed_expected_map_dynamic_blocks(Eap4Scratch** sp, hipStream_t st, const void* d_blocks, int world, int n,
                                       long K_max, float T, phd_gaussian4d* out, long out_cap, int mode, int* rounds,
                                       int* cells, std::string& err);

}  // namespace phd

#endif /* PHD_MIXED_K_H */
