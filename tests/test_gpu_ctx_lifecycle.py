"""Teardown of a context (phd_ctx_destroy): contexts are created, driven until
every lazily allocated resource exists, and destroyed, over and over; the
device's free memory must not shrink by as much as one context's particle
store.  What a context holds is released by its owners (csrc/phd_own.h), not
by a list: a buffer that nobody releases shows here as growth per cycle.

The cap is one particle store (two slab sets of n x 7 x map_capacity floats):
every cycle allocates that and more, so eight leaked cycles would exceed it
eight times over, while the runtime's own caching (code objects, the first
events and streams) is paid in the warm-up cycle before the first reading.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, CAP, M = 256, 256, 8
CYCLES = 8
STORE_BYTES = 2 * N * 7 * CAP * 4


def _cphd_cycle(torch, bufs):
    """A CPHD context with timing, the trace, the expected map, the cardinality
    distribution and one phd_shard_receive into set X."""
    import phdslam
    c, poses, lw, maps, offs, z = phdslam.config_scenario(3, n=N, G=16, M=M)
    f = phdslam.PHDFilter(N, c, map_capacity=CAP, max_measurements=M)
    f.set_seed(11)
    f.set_check_each_update(False)
    f.load(poses, lw, maps, offs)
    f.enable_timing(4)
    f.enable_trace(4, map_snapshot_cap=8, card_dist=True)
    for k in range(2):  # (the second scan has a previous one: the step's births)
        f.set_measurements(z)
        f.step((0.0, 0.0), do_predict=k > 0, step=k)
    assert f.trace_count() == 2
    assert len(f.expected_map()) > 0
    assert f.cardinality_distribution().shape == (N, c.maxCardinality + 1)
    # every particle's record back into its own slot, through migration set X
    rec, idx = bufs
    assert rec.numel() >= N * f.record_bytes()
    f.pack(idx.data_ptr(), N, rec.data_ptr())
    f.shard_receive(rec.data_ptr(), idx.data_ptr(), N, 0)
    assert len(f.cardinalities()) == N
    f.check_errors()
    f.close()


def _mixed_cycle(torch, bufs):
    """A mixed-model context (phd_enable_dynamic) with the mixed trace."""
    import phdslam
    from phdslam.scenario import mixed_config, mixed_scenario
    c = mixed_config()
    poses, sm, so, dm, do, z = mixed_scenario(c, N, 12, 6, M)
    f = phdslam.PHDFilter(N, c, map_capacity=CAP, max_measurements=M)
    f.set_seed(11)
    f.set_check_each_update(False)
    f.enable_dynamic(32)
    f.load(poses, np.full(N, -np.log(np.float32(N)), np.float32), sm, so)
    f.load_dynamic(dm, do)
    f.enable_timing(4)
    f.enable_trace_mixed(4, map_snapshot_cap=8, dyn_snapshot_cap=8)
    for k in range(2):
        f.set_measurements(z)
        f.step((0.0, 0.0), do_predict=k > 0, step=k)
    assert f.trace_count() == 2
    f.expected_map()
    f.expected_map_dynamic()
    f.check_errors()
    f.close()


@pytest.mark.parametrize("cycle", [_cphd_cycle, _mixed_cycle], ids=["cphd", "mixed"])
def test_create_drive_destroy_releases_everything(gpu, cycle):
    import torch
    dev = torch.device("cuda", 0)
    # the test's own buffers exist before the first reading (a record: pose, weight, size, map, cardinality row)
    bufs = (torch.zeros(N * (7 * CAP + M + 64) * 8, dtype=torch.uint8, device=dev),
            torch.arange(N, dtype=torch.int32, device=dev))
    cycle(torch, bufs)  # warm-up: what the runtime keeps after the first use
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info(dev)[0]
    for _ in range(CYCLES):
        cycle(torch, bufs)
    torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info(dev)[0]
    print(f"free before {free0} after {free1} growth {free0 - free1} cap {STORE_BYTES}")
    assert free0 - free1 < STORE_BYTES, (free0, free1)
