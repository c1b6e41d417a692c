"""Host (no GPU): the capacity horizon of every precompiled tracking policy's LDS layout (hilo_nmpc_layout_capacity) obeys the rule
it is defined by - the footprint at the capacity horizon fits the 40 KB - 64 B that let four instances share the 160 KB of a CU
(csrc/hilo_ocp.h::VEC_BUDGET), the footprint one horizon further does not."""
import ctypes as C

import pytest

from hilo_mpc_amd import _lib
from hilo_mpc_amd.model import ZOO

BUDGET = 40 * 1024 - 64
TRACKED = ['chemostat4', 'pendulum4', 'bioreactor3', 'chemostat4_gp', 'robot6', 'cstr3']   # HILO_NMPC_MODELS of csrc/hilo_nmpc.hip


@pytest.mark.parametrize('taylor', [0, 1], ids=['sym', 'taylor'])
@pytest.mark.parametrize('name', TRACKED)
def test_capacity_horizon_is_the_largest_that_fits_40_kb(name, taylor):
    n, at_cap, beyond = C.c_int(), C.c_longlong(), C.c_longlong()
    _lib.check(_lib.lib().hilo_nmpc_layout_capacity(ZOO[name][0], taylor, C.byref(n), C.byref(at_cap), C.byref(beyond)))
    print(name, 'taylor' if taylor else 'sym', 'capacity horizon', n.value, 'bytes', at_cap.value, 'next', beyond.value)
    assert n.value >= 1
    assert 0 < at_cap.value <= BUDGET < beyond.value


def test_unknown_model_is_refused():
    n, a, b = C.c_int(), C.c_longlong(), C.c_longlong()
    assert _lib.lib().hilo_nmpc_layout_capacity(ZOO['lti'][0], 0, C.byref(n), C.byref(a), C.byref(b)) != 0
