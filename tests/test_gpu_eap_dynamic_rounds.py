"""The dynamic expected map as decision rounds over the whole GPU
(phd_expected_map_dynamic, mode 0: k_eap4_bound, the lattice cells,
k_eap4_lfmis, k_eap4_sum; phd_mixed.hip) against the one-workgroup form (mode
1: k_eap4_merge) and the oracle (orc_expected_map_dynamic).

Every case is compared three ways, by byte equality in emission order and
n_out: mode 0 against mode 1, mode 0 against the oracle, mode 1 against the
oracle.  No tolerance is involved: the distance and the moment sums are header
functions shared by all three (include/phd_mixed.h), the rounds add only
scheduling.  Round counts depend on scheduling, so only 1 <= rounds <= K is
asserted; the occupied cells are a function of the input and are asserted.

The stores are tests/eap_dynamic_cases.py's (held to what they are named for
by tests/test_eap_dynamic_cases.py on the CPU); their sizes sit at the kernel's
constants - 1, + 0, + 1 (CHUNK = TILE = 256, PASS = 64).
"""
import numpy as np
import pytest

import eap_dynamic_cases as edc
import pyoracle
import test_gpu_mixed_sharded as tms
from phdslam.scenario import mixed_config, mixed_scenario

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a).tobytes()


def _same(a, b, what):
    assert len(a) == len(b), f"{what}: {len(a)} vs {len(b)} components"
    if _bits(a) != _bits(b):
        i = next(k for k in range(len(a)) if _bits(a[k:k + 1]) != _bits(b[k:k + 1]))
        raise AssertionError(f"{what}: first difference at output {i}: {a[i]} vs {b[i]}")


def load_case(cs):
    """A mixed context holding the case's store (three static components per
    particle beside the dynamic maps)."""
    cfg = mixed_config(minSeparation=cs["T"])
    n = len(cs["sizes"])
    poses, sm, sof, _, _, _ = mixed_scenario(cfg, n, 3, 1, 4, seed=77)
    f = tms._filter(cfg, n, dcap=edc.DCAP)
    tms._load(f, poses, cs["lw"], sm, sof, cs["comps"], edc.offsets(cs))
    return cfg, f


def both_modes(f):
    """(mode 0 map, (rounds, cells)), (mode 1 map, (rounds, cells))"""
    out = []
    for mode in (0, 1):
        f.set_expected_map_dynamic_mode(mode)
        out.append((f.expected_map_dynamic().copy(), f.expected_map_dynamic_groups()))
    f.set_expected_map_dynamic_mode(0)
    return out


def held(cs, name):
    cfg, f = load_case(cs)
    (m0, (r0, c0)), (m1, (r1, c1)) = both_modes(f)
    f.close()
    ref = pyoracle.expected_map_dynamic(cfg, cs["lw"], cs["comps"], edc.offsets(cs))
    K = len(cs["comps"])
    print(f"{name}: K {K} n_out {len(m0)} / {len(m1)} / {len(ref)} rounds {r0} cells {c0}")
    _same(m0, m1, f"{name}: rounds vs one workgroup")
    _same(m0, ref, f"{name}: rounds vs oracle")
    _same(m1, ref, f"{name}: one workgroup vs oracle")
    if cs["n_out"] is not None:
        assert len(m0) == cs["n_out"]
    if K == 0:
        assert (r0, c0) == (0, 0) and (r1, c1) == (0, 0)
        return
    assert (r1, c1) == (1, 0), "mode 1 is the one-workgroup form"
    if cs["fallback"]:
        assert (r0, c0) == (1, 0), "the one-workgroup form serves this input"
        return
    assert c0 > 0 and 1 <= r0 <= K
    if cs["cells"] is not None:
        assert c0 == cs["cells"]
    if cs["multi_cell"]:
        assert c0 > 1
    assert c0 == len(np.unique(edc.cell_keys(cs["comps"], cs["T"]), axis=0))


@pytest.mark.parametrize("name", sorted(edc.CASES))
def test_rounds_equal_one_workgroup_and_oracle(gpu, name):
    held(edc.CASES[name](), name)


def test_mixed_scenario_after_two_updates(gpu):
    """A mixed_scenario store of 128 particles x about 24 dynamic components
    (K about 3 000) after two updates with normalised weights."""
    cfg = mixed_config()
    n = 128
    poses, sm, sof, dm, dof, z = mixed_scenario(cfg, n, 30, 24, 24)
    f = tms._filter(cfg, n, dcap=edc.DCAP)
    lw = np.log(np.random.default_rng(5).dirichlet(np.ones(n))).astype(np.float32)
    tms._load(f, poses, lw, sm, sof, dm, dof)
    for _ in range(2):
        f.update(z)
        f.normalize()
    _, gw, _, _ = f.export(with_maps=False)
    gd, gdo = f.export_dynamic()
    (m0, (r0, c0)), (m1, g1) = both_modes(f)
    f.close()
    ref = pyoracle.expected_map_dynamic(cfg, gw, gd, gdo)
    K = int(gdo[-1])
    print(f"mixed_scenario: K {K} n_out {len(m0)} rounds {r0} cells {c0}")
    assert 2500 <= K <= 8192 and 0 < len(ref) < K
    _same(m0, m1, "rounds vs one workgroup")
    _same(m0, ref, "rounds vs oracle")
    _same(m1, ref, "one workgroup vs oracle")
    assert g1 == (1, 0) and c0 > 1 and 1 <= r0 <= K
