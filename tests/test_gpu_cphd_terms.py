"""GPU parity of the CPHD terms kernel (k_cphd_terms) at the edges of its
unrolled elementary-symmetric-function chains, against the CPU oracle.

The fast form (cphd_fast64: M <= 64 and a complete cardinality series) runs its
chains over all 64 lanes whatever M is — the steps of measurements m >= M
multiply by λ'_m = 0 — in two halves of 32 measurements and batches of 8.  The
rest of the suite holds M = 16, 40 and 64 only.  Tolerance: parity.RTOL (1e-5).
"""
import numpy as np
import pytest

from test_gpu_parity import _check_cardinality, _check_update

pytestmark = pytest.mark.gpu


# 1, 2: the single measurement and the smallest case with a chain step;
# 7, 8, 9: the edges of the batches of 8; 31, 32, 33: the edges of the two
# halves; 63: the last step with a zero multiplier; 64: the full wave and the
# lane-0 k = 64 term
@pytest.mark.parametrize("M", [1, 2, 7, 8, 9, 31, 32, 33, 63, 64])
def test_cphd_terms_fast_form_chain_edges(gpu, M):
    """maxCardinality = 1023 against λ ≈ tens: the closed-form series applies,
    so the fast form runs.  Posterior maps, Δ log w = <Ψ0,p> and the log
    cardinality distribution against the oracle's direct formulas."""
    import phdslam
    n, G = 8, 64
    c, poses, lw, maps, offs, z = phdslam.config_scenario(3, n=n, G=G, M=M)
    assert c.filterType == 1
    c.maxCardinality = 1023
    cap = dict(map_capacity=256, candidate_capacity=512, survivor_capacity=256, max_measurements=M)
    _check_update(c, poses, lw, maps, offs, z, f"cphd terms fast M{M}", **cap)
    _check_cardinality(c, n, poses, lw, maps, offs, z, **cap)


def test_cphd_terms_general_form_below_64(gpu):
    """maxCardinality just above the predicted mean cardinality λ = Σ w: the
    Chernoff check of the closed form fails and the general form (cphd_wave)
    sums the truncated series, here with its M <= 64 chains (M = 24: one full
    segment of 16 measurements and one of 8)."""
    import phdslam
    n, G, M = 8, 96, 24
    c, poses, lw, maps, offs, z = phdslam.config_scenario(3, n=n, G=G, M=M)
    lam = float(np.max([maps[offs[p]:offs[p + 1]]["weight"].sum() for p in range(n)]))
    c.maxCardinality = int(np.ceil(lam)) + 2
    cap = dict(map_capacity=256, candidate_capacity=512, survivor_capacity=256, max_measurements=M)
    _check_update(c, poses, lw, maps, offs, z, f"cphd terms general nmax {c.maxCardinality} lambda {lam:.1f}", **cap)
    _check_cardinality(c, n, poses, lw, maps, offs, z, **cap)
