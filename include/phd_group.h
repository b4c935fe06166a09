/*
 * phd_group.h — one host process driving a particle-sharded filter over N
 * GPUs of one node through RCCL (ncclCommInitAll + grouped calls over xGMI),
 * C ABI.  The same sync-free step as phdslam/dist.py (ShardedFilter.step),
 * for C / C++ callers of phdfilter.h / phd_capi.h that have no PyTorch:
 *
 *   per step k, every rank r (each call on rank r's context stream):
 *     1. phd_predict_update(ctx_r, u, 1, k, w_local_r)
 *     2. settle step k-1's plan: phd_shard_poll; records beyond the fixed
 *        blocks go point to point (grouped ncclSend / ncclRecv), then
 *        phd_shard_receive_overflow + phd_update_pending on the slots they feed
 *     3. ncclAllGather of the n log-weights (grouped over the ranks)
 *     3t. (phd_group_trace_enable / _mixed) phd_trace_shard_pack, ncclAllGather
 *        of the trace blocks, phd_trace_shard_append (the _mixed pair for the
 *        mixed model): the scan's estimate record
 *     4. phd_shard_resample_async (global normalise / nEff / decision /
 *        parents, identical on every rank; plan; fixed blocks packed)
 *     5. equal-split all-to-all of the blocks (grouped ncclSend / ncclRecv)
 *     6. phd_shard_receive_blocks
 *
 * The reference has no multi-GPU path (main.cpp:1446 prints the device count
 * only); this is SURVEY.md §8(e).  Built as libphdslam_group.so (it links
 * RCCL; libphdslam.so itself does not, so a PyTorch process never loads two
 * RCCL copies).
 */
#ifndef PHD_GROUP_H
#define PHD_GROUP_H
#include <stddef.h>
#include <stdint.h>

#include "phd_capi.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct phd_group phd_group;

/* world contexts, ctxs[r] created on device devices[r] with the same particle
 * count n, configuration and capacities, each loaded with its shard.  The
 * group sets each context's predict index offset (r * n) and creates one RCCL
 * communicator per device (ncclCommInitAll).  seed: the resample seed shared
 * by every rank (phdslam.dist.ShardedFilter's default 0x9e3779b97f4a7c15);
 * block_records: particle records per peer in the fixed all-to-all blocks.
 * The update form (phd_set_update_form / phd_set_update_threads) must be fixed
 * before this call: the plan stream beside part C is set up only for a split
 * update found here.  A later change of form stays correct (the all-gather
 * waits on phd_wait_logw, which every form records) but loses or gains no
 * overlap until the group is re-created.  The record buffers are sized here by
 * phd_record_bytes: on a mixed context (feature_model 2) phd_enable_dynamic
 * comes before this call, and the group is re-created after another dynamic
 * capacity (the step then fails with PHD_E_ARG, nothing written). */
int phd_group_create(phd_group** out, int world, phd_ctx* const* ctxs, const int* devices, int block_records,
                     uint64_t seed);
/* One process per GPU: this process's shard `ctx` (on `device`) as rank `rank`
 * of a `world`-rank group whose RCCL communicator comes from ncclCommInitRank
 * with `unique_id` — the 128 bytes phd_group_unique_id wrote on one rank, handed
 * to every rank by the caller (e.g. a torch.distributed broadcast).  Every rank
 * calls this, then phd_group_step once per step: the whole sharded step of
 * ShardedFilter (phdslam/dist.py) in one C call.  Same seed / block_records on
 * every rank; the update form is fixed before the call (as phd_group_create). */
int phd_group_unique_id(void* out, size_t bytes);
int phd_group_create_rank(phd_group** out, phd_ctx* ctx, int device, int world, int rank, const void* unique_id,
                          int block_records, uint64_t seed);
int phd_group_destroy(phd_group* g);
/* One sharded filter step (predict with control u — NULL for CV — update,
 * global normalise / nEff / resample, migration).  Returns with every rank's
 * work enqueued; *neff / *resampled (optional) receive the PREVIOUS step's plan
 * (its counts are polled here), 0 / -1 on the first step. */
int phd_group_step(phd_group* g, const phd_ackerman_control* u, uint64_t step, float* neff, int* resampled);
/* The per-scan estimate trace (phd_trace_enable, phd_capi.h) on the sharded
 * step: enables it on every context of the group with these arguments
 * (capacity 0: off) and allocates the trace blocks.  Every phd_group_step then
 * appends the scan's record — the one a single context of all world * n
 * particles writes — to every rank's ring: read it with phd_trace_read /
 * phd_trace_count on any rank's context.  A traced step runs its plan after
 * the trace instead of beside part C.  Synchronises (an allocation). */
int phd_group_trace_enable(phd_group* g, int capacity, int map_snapshot_cap, unsigned flags);
/* The same for the mixed model (phd_trace_enable_mixed on every context,
 * feature_model 2 after phd_enable_dynamic): every phd_group_step then appends
 * the scan's phd_trace_record and phd_trace_dyn_record, through
 * phd_trace_shard_pack_mixed / ncclAllGather of the blocks /
 * phd_trace_shard_append_mixed; read them with phd_trace_read and
 * phd_trace_read_dynamic.  capacity 0 (here or in phd_group_trace_enable): off. */
int phd_group_trace_enable_mixed(phd_group* g, int capacity, int map_snapshot_cap, int dyn_snapshot_cap,
                                 unsigned flags);
/* Settle the last plan (no update follows): the contexts' stores are final. */
int phd_group_flush(phd_group* g);
/* The EAP expected map of the whole filter (phd_capi.h: "the EAP expected map
 * of a sharded filter"): what phd_expected_map returns on a single context of
 * all world * n particles in rank order, bit for bit.  Settles the open plan
 * (as phd_group_flush), ncclAllGather of the ranks' component counts, K_max
 * their maximum, phd_eap_shard_pack, one ncclAllGather of the blocks, and
 * phd_expected_map_blocks on every rank of this process; out / out_cap / n_out
 * as phd_expected_map (rank 0's copy in the one-process form; every process
 * of the phd_group_create_rank form calls it and receives the same map).
 * The blocks are allocated here, 28 K_max + 64 bytes per rank, and kept.
 * Synchronises. */
int phd_group_expected_map(phd_group* g, phd_gaussian2d* out, long out_cap, long* n_out);
/* The EAP map of the dynamic maps of the whole mixed filter (feature_model 2
 * after phd_enable_dynamic; phd_capi.h: "the EAP map of the dynamic maps of a
 * sharded mixed filter"): what phd_expected_map_dynamic returns on a single
 * mixed context of all world * n particles in rank order, byte for byte.  The
 * phases of phd_group_expected_map on buffers of its own: the settle,
 * ncclAllGather of the counts (phd_eap_dyn_shard_count), phd_eap_dyn_shard_pack,
 * one ncclAllGather of the blocks (84 K_max + 64 bytes per rank, kept), and
 * phd_expected_map_dynamic_blocks on every rank of this process (the decision
 * rounds over each rank's whole GPU; phd_set_expected_map_dynamic_mode and
 * phd_expected_map_dynamic_groups on a rank's context select the form and
 * report its rounds and cells).  On such a group phd_group_expected_map returns the static expected map.  Synchronises. */
int phd_group_expected_map_dynamic(phd_group* g, phd_gaussian4d* out, long out_cap, long* n_out);
/* Counters over the steps so far: [0] resamples, [1] migrated particles,
 * [2] records sent, [3] records beyond the fixed blocks, [4] pending slots. */
int phd_group_stats(const phd_group* g, long long* out5);
/* Wait for every rank's stream. */
int phd_group_synchronize(phd_group* g);
/* Text of the last phd_group_* failure of this thread. */
const char* phd_group_last_error(void);

/* Host-side transport plan of the records beyond the fixed blocks (the layout
 * of the block pack and unpack, record_slot of phd_records.hip): the sender's
 * overflow buffer holds, per destination d in rank order, its records block_records .. send_records[d]-1;
 * the receiver's, per source s in rank order, records block_records ..
 * recv_records[s]-1.  Writes (peer, byte offset, byte count) triples — at most
 * world each — and their numbers.  Pure host arithmetic (no device). */
int phd_group_overflow_slices(int world, const int* send_records, const int* recv_records, int block_records,
                              size_t record_bytes, long long* send_slices, int* n_send, long long* recv_slices,
                              int* n_recv);

#ifdef __cplusplus
}
#endif
#endif
