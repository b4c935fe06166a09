"""The hand-built stores of tests/eap_dynamic_cases.py do what they are named
for: the oracle (orc_expected_map_dynamic) on each gives the output count the
case was constructed for, a chain chains, k clusters give k outputs, and the
generators' own assertions (cells, distances) hold.  CPU only.
"""
import numpy as np
import pytest

import eap_dynamic_cases as edc
import pyoracle
from phdslam.scenario import mixed_config


def oracle_map(cs):
    cfg = mixed_config(minSeparation=cs["T"])
    return pyoracle.expected_map_dynamic(cfg, cs["lw"], cs["comps"], edc.offsets(cs))


@pytest.mark.parametrize("name", sorted(edc.CASES))
def test_case_does_what_it_is_named_for(built, name):
    cs = edc.CASES[name]()
    K = len(cs["comps"])
    ref = oracle_map(cs)
    assert len(ref) <= K
    if cs["n_out"] is not None:
        assert len(ref) == cs["n_out"], f"{name}: the oracle emits {len(ref)} of {K}"
    elif K:
        assert 0 < len(ref), name
    if cs["cells"] is not None and K and not cs["fallback"]:
        assert len(np.unique(edc.cell_keys(cs["comps"], cs["T"]), axis=0)) == cs["cells"], name
    if cs["multi_cell"]:
        assert len(np.unique(edc.cell_keys(cs["comps"], cs["T"]), axis=0)) > 1, name


def test_chain_merges_the_head_and_keeps_the_tail(built):
    """A absorbs B; C, within T of B only, is emitted on its own with its weight."""
    for axis in ("x", "y", "diagonal", "velocity"):
        cs = edc.chain(axis)
        ref = oracle_map(cs)
        ew = np.exp(cs["lw"].astype(np.float64)[0])
        w = cs["comps"]["weight"].astype(np.float64) * ew
        assert abs(ref["weight"][0] - (w[0] + w[1])) < 1e-6 and abs(ref["weight"][2] - w[2]) < 1e-6, axis


def test_merging_cases_merge_some_not_all(built):
    for name in ("one_cell_256", "neighbour_stream_256", "rank_one_1e+06", "zero_weights", "empty_between"):
        cs = edc.CASES[name]()
        ref = oracle_map(cs)
        assert 1 < len(ref) < len(cs["comps"]), f"{name}: {len(ref)} of {len(cs['comps'])}"


def test_big_groups_hold_the_members_they_name(built):
    for members in (edc.PASS - 1, edc.PASS, edc.PASS + 1):
        cs = edc.big_group(members)
        ref = oracle_map(cs)
        ew = np.exp(np.float64(cs["lw"][0]))
        want = cs["comps"]["weight"][:members + 1].astype(np.float64).sum() * ew
        assert abs(ref["weight"][0] - want) < 1e-5 * want, members
