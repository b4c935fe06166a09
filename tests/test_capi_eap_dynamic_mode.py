"""phd_expected_map_dynamic_groups and phd_set_expected_map_dynamic_mode
(include/phd_capi.h): exported and bound, their argument checks, and what a
fresh context reports.  The checks of a null context need no device.
"""
import ctypes

import numpy as np
import pytest

SYMBOLS = ("phd_expected_map_dynamic_groups", "phd_set_expected_map_dynamic_mode")


def test_symbols_exported_and_bound(built):
    import phdslam
    from phdslam._lib import SIGNATURES
    L = phdslam.lib()
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym
        assert sym in SIGNATURES, sym
    from phdslam.dist import GroupRank, ShardedFilter
    for cls in (phdslam.PHDFilter, ShardedFilter, GroupRank):
        assert hasattr(cls, "expected_map_dynamic_groups") and hasattr(cls, "set_expected_map_dynamic_mode"), cls


def test_null_context_is_refused(built):
    import phdslam
    L = phdslam.lib()
    E_ARG = phdslam._lib.PHD_E_ARG
    r, c = ctypes.c_int(-7), ctypes.c_int(-7)
    assert L.phd_expected_map_dynamic_groups(None, ctypes.byref(r), ctypes.byref(c)) == E_ARG
    assert (r.value, c.value) == (-7, -7)
    assert L.phd_last_error()
    for mode in (0, 1, 2):
        assert L.phd_set_expected_map_dynamic_mode(None, mode) == E_ARG


@pytest.mark.gpu
def test_argument_checks_and_a_fresh_context(gpu):
    import phdslam
    import test_gpu_mixed_sharded as tms
    from phdslam.scenario import mixed_config
    L = phdslam.lib()
    E_ARG, OK = phdslam._lib.PHD_E_ARG, phdslam._lib.PHD_OK
    f = tms._filter(mixed_config(), 4, dcap=8)
    h = f.handle
    r, c = ctypes.c_int(-7), ctypes.c_int(-7)
    # before any map: 0, 0
    assert L.phd_expected_map_dynamic_groups(h, ctypes.byref(r), ctypes.byref(c)) == OK
    assert (r.value, c.value) == (0, 0) and f.expected_map_dynamic_groups() == (0, 0)
    # null outputs: refused, the other output untouched
    r.value = c.value = -7
    assert L.phd_expected_map_dynamic_groups(h, None, ctypes.byref(c)) == E_ARG
    assert L.phd_expected_map_dynamic_groups(h, ctypes.byref(r), None) == E_ARG
    assert (r.value, c.value) == (-7, -7)
    # a mode outside {0, 1}: refused, the mode kept
    for bad in (-1, 2, 7):
        assert L.phd_set_expected_map_dynamic_mode(h, bad) == E_ARG
        with pytest.raises(phdslam._lib.PHDError):
            f.set_expected_map_dynamic_mode(bad)
    for good in (1, 0):
        assert L.phd_set_expected_map_dynamic_mode(h, good) == OK
    # an empty store: the map is empty and the diagnostics stay 0, 0
    assert len(f.expected_map_dynamic()) == 0 and f.expected_map_dynamic_groups() == (0, 0)
    f.close()
