"""GPU: the capacity LDS layout of the precompiled tracking policies (csrc/hilo_ocp.h::OcpCapLayout, csrc/hilo_nmpc.hip::
nmpc_launch_pb) against the run-time layout of the SAME build, and a solve with the phase profile switched on against one without.

Only addresses differ between the two layouts and only bookkeeping between a profiled and a plain solve: no product and no order of
a sum changes, so every output must be equal BIT FOR BIT - `x` (v), `f`, `lam_g`, the returned input, status, iteration count, KKT error
and the fused plant step's `x_next`.  There is no tolerance in this file.

`HILO_OCP_LAYOUT=runtime` is read at every launch like `HILO_NMPC_TAYLOR`: it is set around the solves of the forced run only.
Horizons: 1, 2, 3 (the Riccati sweep is unrolled by two and has an odd-horizon head), the capacity horizon NCAP of the policy, one
below it, and NCAP + 1, where the default launch itself falls back to the run-time layout.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests.problems import C2, C4, c2_x0, product_gp, product_nmpc
from tests.test_sym_phase_gpu import CSTR3, PENDULUM

pytestmark = pytest.mark.gpu

KEYS = ('x', 'f', 'lam_g', 'status', 'iter_count', 'kkt_error')
B = 8


def _ncap(model_id, taylor):
    from hilo_mpc_amd import _lib
    n, a, b = C.c_int(), C.c_longlong(), C.c_longlong()
    _lib.check(_lib.lib().hilo_nmpc_layout_capacity(model_id, int(taylor), C.byref(n), C.byref(a), C.byref(b)))
    return n.value


def _c2_batch():
    """Eight chemostat starts: the benchmark's spread, one far from the reference (product P = 6 against the reference 2, substrate
    nearly used up) and one whose optimal first inputs sit on their bounds (no product and no biomass to speak of: feed at the limit)."""
    x0 = c2_x0(B)
    x0[6] = [.02, 5., 0., 0.]
    x0[7] = [.5, 10., 6., .2]
    return x0


BIOREACTOR = dict(model='bioreactor3', dt=.5, N=5, order=4, stage_states=[([1], [10.], [1.5])], stage_inputs=[([0], [1.], None)],
                  terminal_states=[([1], [10.], [1.5])], x_lb=[0, 0, 0], u_lb=[0.], u_ub=[.5], x_guess=[25., 1., 1.], u_guess=[.1],
                  p=[.1, 25., .2, .001, .5, .5])
ROBOT = dict(model='robot6', dt=.1, N=5, order=4, stage_states=[([0, 2], [10., 10.], [1., .5])], stage_inputs=[([0, 1], [.1, .1], None)],
             terminal_states=[([0, 2], [10., 10.], [1., .5])], u_lb=[-2., -2.], u_ub=[2., 2.], x_guess=[0.] * 6, u_guess=[0., 0.], p=[])


def _x0_of(spec):
    name = spec['model']
    if name.startswith('chemostat4'):
        return _c2_batch()
    rng = np.random.default_rng(3)
    base = {'pendulum4': [.5, 0., .3, 0.], 'cstr3': [.6, .4, 430.], 'bioreactor3': [25., 1., 1.], 'robot6': [0., .5, 0., .2, .3, 0.]}[name]
    scale = .02 if name == 'cstr3' else .2
    return np.array(base) * (1 + scale * rng.uniform(-1, 1, (B, len(base)))) + (0. if name != 'robot6' else .05 * rng.uniform(-1, 1, (B, 6)))


def _two_steps(spec, x0, forced, taylor, gp=None):
    """Cold solve from x0, then a warm-started solve from the fused plant step's answer; every output of both."""
    nmpc = product_nmpc(spec, gp=gp)
    p = spec['p'] or None
    xn = torch.zeros(B, x0.shape[1], dtype=torch.float64, device='cuda')
    fused = nmpc.set_plant_buffer(xn)
    out = []
    if forced:
        os.environ['HILO_OCP_LAYOUT'] = 'runtime'
    if taylor:
        os.environ['HILO_NMPC_TAYLOR'] = '1'
    try:
        x = x0
        for _ in range(2):
            u = nmpc.optimize(x, cp=p)
            torch.cuda.synchronize()
            r = {k: nmpc._nlp_solution[k].cpu().numpy().copy() for k in KEYS}
            r['u0'] = np.asarray(u.cpu().numpy() if torch.is_tensor(u) else u).copy()
            r['x_next'] = (xn if fused else nmpc.plant_step(x, u, cp=p)).cpu().numpy().copy()
            out.append(r)
            x = r['x_next']
    finally:
        os.environ.pop('HILO_OCP_LAYOUT', None)
        os.environ.pop('HILO_NMPC_TAYLOR', None)
    return out


def _assert_same_bits(a, b, what):
    for step, (ra, rb) in enumerate(zip(a, b)):
        for k in ra:
            va, vb = np.ascontiguousarray(ra[k]), np.ascontiguousarray(rb[k])
            assert va.dtype == vb.dtype and va.shape == vb.shape, (what, step, k)
            assert va.tobytes() == vb.tobytes(), (what, step, k, int(np.sum(va != vb)))


@pytest.mark.parametrize('taylor', [False, True], ids=['sym', 'taylor'])
@pytest.mark.parametrize('horizon', ['1', '2', '3', 'ncap-1', 'ncap', 'ncap+1'])
def test_chemostat4_capacity_layout_equals_runtime_layout(horizon, taylor):
    ncap = _ncap(3, taylor)
    assert ncap >= 4
    N = {'ncap-1': ncap - 1, 'ncap': ncap, 'ncap+1': ncap + 1}.get(horizon) or int(horizon)
    spec = dict(C2, N=N)
    x0 = _c2_batch()
    cap = _two_steps(spec, x0, forced=False, taylor=taylor)
    run = _two_steps(spec, x0, forced=True, taylor=taylor)
    print(f"N {N} (capacity {ncap}) taylor {taylor}: status {cap[0]['status'].tolist()} {cap[1]['status'].tolist()}  iterations "
          f"{cap[0]['iter_count'].tolist()} {cap[1]['iter_count'].tolist()}  u0 {cap[1]['u0'].tolist()}")
    _assert_same_bits(cap, run, (N, taylor))
    assert np.all(np.isin(cap[0]['status'], (1, 2))), cap[0]['status']
    if horizon == 'ncap':   # the premises of the batch, at the horizon next to the benchmark's: an input bound is active at a
        # solution (the whole input trajectory is part of x), and the far start is a different problem from the benchmark's spread
        Nu = N * 2
        uu = cap[0]['x'][:, -Nu:]
        assert np.any(np.minimum(np.abs(uu - 0.), np.abs(uu - 1.)) < 1e-6)
        assert cap[0]['iter_count'][7] != cap[0]['iter_count'][0] or abs(cap[0]['f'][7] - cap[0]['f'][0]) > 1.


FURTHER = {'pendulum4': dict(PENDULUM, N=5), 'cstr3': dict(CSTR3, N=4), 'bioreactor3': BIOREACTOR, 'robot6': ROBOT,
           'chemostat4_gp': dict(C4, N=5)}


@pytest.mark.parametrize('taylor', [False, True], ids=['sym', 'taylor'])
@pytest.mark.parametrize('name', list(FURTHER))
def test_further_policies_capacity_layout_equals_runtime_layout(name, taylor):
    spec = FURTHER[name]
    gp = product_gp() if name == 'chemostat4_gp' else None
    x0 = _x0_of(spec)
    cap = _two_steps(spec, x0, forced=False, taylor=taylor, gp=gp)
    run = _two_steps(spec, x0, forced=True, taylor=taylor, gp=gp)
    print(f"{name} taylor {taylor}: status {cap[0]['status'].tolist()} iterations {cap[0]['iter_count'].tolist()}")
    _assert_same_bits(cap, run, (name, taylor))
    assert np.any(cap[0]['iter_count'] > 0)


@pytest.mark.parametrize('forced', [False, True], ids=['capacity', 'runtime'])
def test_profiled_kernel_returns_the_product_kernels_bits(forced):
    """A solve while a profile buffer is set (hilo_nmpc_profile) against a plain one, in both layouts; and the ten counters it leaves:
    at least one factorisation per iteration of instance 0, every slot positive."""
    spec = dict(C2)
    x0 = _c2_batch()
    plain = _two_steps(spec, x0, forced=forced, taylor=False)
    nmpc = product_nmpc(spec)
    xn = torch.zeros(B, 4, dtype=torch.float64, device='cuda')
    assert nmpc.set_plant_buffer(xn)
    nmpc.phase_profile(True)
    prof, x = [], x0
    if forced:
        os.environ['HILO_OCP_LAYOUT'] = 'runtime'
    try:
        for _ in range(2):
            u = nmpc.optimize(x, cp=spec['p'])
            torch.cuda.synchronize()
            r = {k: nmpc._nlp_solution[k].cpu().numpy().copy() for k in KEYS}
            r['u0'] = np.asarray(u.cpu().numpy() if torch.is_tensor(u) else u).copy()
            r['x_next'] = xn.cpu().numpy().copy()
            prof.append(r)
            x = r['x_next']
            counters = nmpc.phase_profile(True)
            ends = nmpc.phase_profile_ends()
            print('counters', counters, ends, 'iterations of instance 0', int(r['iter_count'][0]))
            assert counters['n_factorizations'] >= int(r['iter_count'][0])
            assert all(v > 0 for v in counters.values()) and all(v > 0 for v in ends.values()) and len(counters) + len(ends) == 10
    finally:
        os.environ.pop('HILO_OCP_LAYOUT', None)
        nmpc.phase_profile(False)
    _assert_same_bits(plain, prof, ('profile', forced))
