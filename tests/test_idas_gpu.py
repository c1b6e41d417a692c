"""GPU: variable-order implicit integration of models with algebraic states, `Model.setup(solver='idas')`
(csrc/hilo_integrate.h `idas_interval` in [x; z], one instance per lane), through `Model.rollout` / `step` / `simulate` and the
plant of a `SimpleControlLoop`.

The accuracy rule is that of tests/dae_reference.py, for x and for z separately: the error against the tight solution of the reduced
equation, relative to |.| + abstol / reltol, is at most 10 times the larger of the error of scipy's BDF on the reduced equation at
the same tolerances and the disagreement of two tight solutions.  Each test prints the figures it asserts on."""
import ctypes

import numpy as np
import pytest
import torch

from hilo_mpc_amd import Model, SimpleControlLoop, _lib
from tests import dae_reference as dr
from tests import sim_reference as sr

pytestmark = pytest.mark.gpu

TOLS = [(1e-6, 1e-8), (1e-9, 1e-11)]
SCALE = np.array([1., 1.2, .8])          # the three instances of a case: initial states (Robertson: the rate constant k1) scaled


def _instances(case):
    x0, u, p, dt, steps = dr.CASES[case]
    X0 = np.tile(np.asarray(x0, dtype=float), (3, 1))
    P = np.tile(np.asarray(p, dtype=float), (3, 1))
    if case.startswith('robertson_dae'):
        P[:, 0] *= SCALE
    else:
        X0 *= SCALE[:, None]
    return X0, np.tile(np.asarray(u, dtype=float), (3, 1)), P, dt, steps


def _args(U, P):
    return (U if U.shape[-1] else None), (P if P.shape[-1] else None)


def _sequence(case):
    X0, _, P, dt, steps = _instances(case)
    U = np.stack([dr.sequence(case, steps, seed=5 + i) for i in range(3)], axis=1)      # [steps, 3, 1]
    return X0, U, P, dt, steps


@pytest.fixture(scope='module')
def refs():
    """Every reference of this module, once, in worker processes: (case, instance) -> one result per tolerance."""
    keys, jobs = [], []
    for case in sorted(dr.CASES):
        X0, U, P, dt, steps = _instances(case)
        for i in range(3):
            keys.append((case, i))
            jobs.append((case, X0[i], U[i], P[i], dt, steps, TOLS))
    for case in dr.SEQUENCE_CASES:
        X0, U, P, dt, steps = _sequence(case)
        for i in range(3):
            keys.append((case + ':seq', i))
            jobs.append((case, X0[i], U[:, i], P[i], dt, steps, TOLS))
    return dict(zip(keys, dr.run_jobs(jobs)))


def _model(case, i_tol=0, **opts):
    rtol, atol = TOLS[i_tol]
    return dr.symbolic_model(case).setup(dt=dr.CASES[case][3], solver='idas', solver_options=dict(reltol=rtol, abstol=atol, **opts))


def _check(tag, case, refs_of, x, z, U, P, steps, rtol, atol, i_tol):
    worst = 0.
    for i in range(x.shape[1]):
        b = refs_of(i)[i_tol]
        ex, ez, ratio = dr.check(case, x[:, i], z[:, i], b, rtol, atol)
        res = dr.residual(case, x[:, i], z[:, i], U[:, i] if U.ndim == 3 else U[i], P[i], steps)
        print(f"{tag} instance {i} rtol={rtol:g}: error x {ex:.3e} (admissible {b['adm_x']:.3e}), z {ez:.3e} (admissible "
              f"{b['adm_z']:.3e}), ratio {ratio:.3f}, residual {res:.1e}")
        assert ex <= b['adm_x'] and ez <= b['adm_z'], (tag, i)
        assert res <= 1e-10, (tag, i)
        worst = max(worst, ratio)
    return worst


@pytest.mark.parametrize('i_tol', [0, 1])
@pytest.mark.parametrize('case', sorted(dr.CASES))
def test_idas_accuracy_with_held_inputs(refs, case, i_tol):
    rtol, atol = TOLS[i_tol]
    X0, U, P, dt, steps = _instances(case)
    m = _model(case, i_tol)
    u, p = _args(U, P)
    x, y, z, stats = m.rollout(X0, u, p, steps=steps, return_z=True, return_stats=True)
    nz = dr.NZ[m.name]
    assert x.shape == (steps + 1, 3, m.n_x) and z.shape == (steps + 1, 3, nz) and y.shape == (steps, 3, 1 + nz)
    print(f"{case}: status {stats['status'].tolist()}, accepted {stats['n_accepted'].tolist()}, rejected {stats['n_rejected'].tolist()}, "
          f"rhs {stats['n_rhs'].tolist()}; scipy BDF steps {[int(refs[(case, i)][i_tol]['counts'][0]) for i in range(3)]}")
    assert not stats['status'].any()
    _check(case, case, lambda i: refs[(case, i)], x, z, U, P, steps, rtol, atol, i_tol)
    # the measurement is taken on the recorded pair
    np.testing.assert_array_equal(y[:, :, 0], x[1:, :, 0])
    np.testing.assert_array_equal(y[:, :, 1:], z[1:])
    if case == 'lin1':
        t = dt * np.arange(steps + 1)[:, None]
        assert np.max(np.abs(x[:, :, 0] / (X0[:, 0] * np.exp(t)) - 1.)) <= 100. * rtol


@pytest.mark.parametrize('case', dr.SEQUENCE_CASES)
def test_idas_accuracy_with_an_input_sequence(refs, case):
    i_tol = 1
    rtol, atol = TOLS[i_tol]
    X0, U, P, dt, steps = _sequence(case)
    m = _model(case, i_tol)
    x, y, z, stats = m.rollout(X0, U, None, steps=steps, return_z=True, return_stats=True)
    assert not stats['status'].any()
    _check(case + ' sequence', case, lambda i: refs[(case + ':seq', i)], x, z, U, P, steps, rtol, atol, i_tol)


def test_stiff_dae_over_long_intervals_against_the_fixed_step_map(refs):
    """Robertson's kinetics at dt = 100: 'idas' meets the rule; the same model without a solver - eight classic Runge-Kutta steps
    per interval with a nested Newton iteration - is recorded next to it."""
    case, i_tol = 'robertson_dae_long', 0
    rtol, atol = TOLS[i_tol]
    X0, U, P, dt, steps = _instances(case)
    x, y, z, stats = _model(case, i_tol).rollout(X0, None, P, steps=steps, return_z=True, return_stats=True)
    assert not stats['status'].any()
    _check(case, case, lambda i: refs[(case, i)], x, z, U, P, steps, rtol, atol, i_tol)
    xm, _ = dr.symbolic_model(case).setup(dt=dt).rollout(X0, None, P, steps=steps)
    for i in range(3):
        b = refs[(case, i)][i_tol]
        em = sr.rel_err(xm[:, i], b['x'], rtol, atol) if np.isfinite(xm[:, i]).all() else np.inf
        print(f"{case} instance {i}: the fixed-step map is off by {em:.3e} (admissible {b['adm_x']:.3e})")


def _edge_batch(n):
    rng = np.random.default_rng(23)
    return np.array([.5, 1.]) * (1 + .2 * rng.uniform(-1, 1, (n, 2))), rng.uniform(-.3, .6, (n, 1))


def test_batch_edges_and_lane_independence():
    """130 instances - two full waves and a partial one - each with its own u and x0: no value crosses lanes, so an instance's rows
    do not depend on the batch it is computed in."""
    m = _model('alg_u', 1)
    steps = 4
    X0, U = _edge_batch(130)
    out = {n: m.rollout(X0[:n], U[:n], steps=steps, return_z=True, return_stats=True) for n in (63, 65, 130)}
    x, y, z, stats = out[130]
    assert not stats['status'].any() and np.isfinite(x).all() and np.isfinite(z).all()
    for n in (63, 65):
        for a, b in zip(out[n][:3], out[130][:3]):
            np.testing.assert_array_equal(a, b[:, :n])
    for i in (0, 63, 64, 129):
        x1, y1, z1 = m.rollout(X0[i:i + 1], U[i:i + 1], steps=steps, return_z=True)
        np.testing.assert_array_equal(x1[:, 0], x[:, i])
        np.testing.assert_array_equal(z1[:, 0], z[:, i])
        np.testing.assert_array_equal(y1[:, 0], y[:, i])


def test_device_tensors_and_the_consistent_start():
    m = _model('cubic', 1)
    dev = torch.device('cuda')
    X0 = torch.tensor([[2.], [1.], [-3.]], dtype=torch.float64, device=dev)
    U = torch.full((3, 1), .5, dtype=torch.float64, device=dev)
    Z0 = torch.tensor([[50.], [-40.], [1e3]], dtype=torch.float64, device=dev)      # far from the roots
    x, y, z = m.rollout(X0, U, steps=3, z0=Z0, return_z=True)
    assert all(isinstance(v, torch.Tensor) and v.device.type == 'cuda' for v in (x, y, z))
    assert len({v.data_ptr() for v in (x, y, z, X0, U, Z0)}) == 6
    z0 = z[0, :, 0].cpu().numpy()
    assert np.max(np.abs(z0 ** 3 + z0 - X0[:, 0].cpu().numpy())) <= 1e-10 * (1. + np.max(np.abs(z0)))
    xa, ya, za = m.rollout(X0, U, steps=3, return_z=True)                                # from the model's guess
    np.testing.assert_allclose(z.cpu().numpy(), za.cpu().numpy(), rtol=1e-9)
    np.testing.assert_allclose(x.cpu().numpy(), xa.cpu().numpy(), rtol=1e-9)


def test_max_num_steps_ends_the_instance():
    case = 'robertson_dae'
    X0, U, P, dt, steps = _instances(case)
    x, y, z, stats = _model(case, 0, max_num_steps=3).rollout(X0, None, P, steps=steps, return_z=True, return_stats=True)
    assert (stats['status'] == 1).all()
    for i in range(3):
        bad = np.isnan(x[:, i, 0])
        assert bad[-1] and not bad[0] and np.all(np.diff(bad.astype(int)) >= 0)
        assert np.array_equal(np.isnan(x[:, i]).all(axis=1), bad) and np.array_equal(np.isnan(z[:, i]).all(axis=1), bad)
        assert np.array_equal(np.isnan(y[:, i]).all(axis=1), bad[1:]) and np.isfinite(x[~bad, i]).all() and np.isfinite(z[~bad, i]).all()


def test_no_consistent_start_ends_that_instance_alone():
    """0 = z^2 - p has no root for p = -1: status 3 for that row, NaN from row 1 of x and row 0 of z; the others are not affected."""
    m = Model(name='noroot')
    x, z, p = m.set_dynamical_states(['x']), m.set_algebraic_states(['z']), m.set_parameters(['p'])
    m.set_dynamical_equations([-x[0] + z[0]])
    m.set_algebraic_equations([z[0] * z[0] - p[0] + 0. * x[0]])
    m.set_measurement_equations([x[0] + z[0]])
    m.setup(dt=.2, solver='idas')
    X0 = np.array([[1.], [2.], [3.], [4.]])
    P = np.array([[4.], [-1.], [9.], [1.]])
    Z0 = np.ones((4, 1))                                   # (dg/dz vanishes at the model's guess 0)
    xs, ys, zs, stats = m.rollout(X0, None, P, steps=3, z0=Z0, return_z=True, return_stats=True)
    assert stats['status'].tolist() == [0, 3, 0, 0] and stats['n_accepted'][1] == 0
    assert xs[0, 1, 0] == 2. and np.isnan(xs[1:, 1]).all() and np.isnan(zs[:, 1]).all() and np.isnan(ys[:, 1]).all()
    ok = [0, 2, 3]
    np.testing.assert_allclose(zs[:, ok, 0], np.tile([2., 3., 1.], (4, 1)), rtol=1e-12)
    xo, yo, zo = m.rollout(X0[ok], None, P[ok], steps=3, z0=Z0[ok], return_z=True)
    np.testing.assert_array_equal(xs[:, ok], xo)
    np.testing.assert_array_equal(zs[:, ok], zo)
    np.testing.assert_array_equal(ys[:, ok], yo)


def test_step_is_the_one_interval_rollout():
    m = _model('alg_u', 0)
    X0, U, _, _, _ = _instances('alg_u')
    xn, yn = m.step(X0, U)
    x, y = m.rollout(X0, U, steps=1)
    np.testing.assert_array_equal(xn, x[1])
    np.testing.assert_array_equal(yn, y[0])


def test_two_simulate_calls_in_a_row(refs):
    case, i_tol = 'alg_u', 1
    rtol, atol = TOLS[i_tol]
    X0, U, P, dt, steps = _instances(case)
    m = _model(case, i_tol)
    m.set_initial_conditions(X0, 0., z0=np.zeros((3, 2)))
    m.simulate(u=U, steps=4)
    m.simulate(u=U, steps=steps - 4)
    sol = m.solution
    assert sol['x'].shape == (steps + 1, 3, 2) and sol['z'].shape == (steps + 1, 3, 2) and sol['z:f'].shape == (3, 2)
    assert not sol['status'].any()
    _check(case + ' simulate', case, lambda i: refs[(case, i)], sol['x'], sol['z'], U, P, steps, rtol, atol, i_tol)


def test_control_loop_with_an_idas_plant():
    class Constant:
        def call(self, x=None, p=None):
            return np.full((x.shape[0], 1), .3)
    m = _model('alg_u', 0)
    X0, U, _, _, _ = _instances('alg_u')
    sol = SimpleControlLoop(m, Constant()).run(3, X0)
    x, _ = m.rollout(X0, np.full((3, 1), .3), steps=1)
    assert sol['x'].shape == (4, 3, 2) and np.isfinite(sol['x']).all()
    np.testing.assert_array_equal(sol['x'][1], x[1])
    # the second interval starts its Newton iteration at the algebraic states the first one ended with
    x1, _, z1 = m.rollout(X0, np.full((3, 1), .3), steps=1, return_z=True)
    x2, _ = m.rollout(x1[1], np.full((3, 1), .3), steps=1, z0=z1[1])
    np.testing.assert_array_equal(sol['x'][2], x2[1])


def test_nine_states_are_refused_by_the_library_and_by_setup():
    m = Model(name='wide9')
    x = m.set_dynamical_states([f'x{i}' for i in range(6)])
    z = m.set_algebraic_states(['a', 'b', 'c'])
    m.set_dynamical_equations([-x[i] + z[i % 3] for i in range(6)])
    m.set_algebraic_equations([z[i] - x[i] for i in range(3)])
    m.set_measurement_equations([x[0]])
    with pytest.raises(NotImplementedError, match="at most 8 differential and algebraic states together"):
        m.setup(dt=.1, solver='idas')
    m.setup(dt=.1)
    h = m._plant_handle()
    opts = _lib.SimOpts()
    opts.method = 3
    X0 = torch.zeros(1, 6, dtype=torch.float64, device=h._dev)
    X = torch.empty(2, 1, 6, dtype=torch.float64, device=h._dev)
    rc = _lib.lib().hilo_model_rollout_dae(h._handle, ctypes.byref(opts), 1, 1, X0.data_ptr(), None, None, 0, 0, X.data_ptr(), None, None,
                                           None, None)
    assert rc == -4 and b'up to 8 differential and algebraic states together; the model has 6 + 3' in _lib.lib().hilo_last_error()
    # ... and a model without algebraic states, and another method
    o = Model('pendulum4').setup(dt=.1)
    ho = o._plant_handle()
    rc = _lib.lib().hilo_model_rollout_dae(ho._handle, ctypes.byref(opts), 1, 1, X0.data_ptr(), None, None, 0, 0, X.data_ptr(), None, None,
                                           None, None)
    assert rc == -4 and b'has none' in _lib.lib().hilo_last_error()
    opts.method = 2
    rc = _lib.lib().hilo_model_rollout_dae(h._handle, ctypes.byref(opts), 1, 1, X0.data_ptr(), None, None, 0, 0, X.data_ptr(), None, None,
                                           None, None)
    assert rc == -4 and b'HILO_SIM_IDAS alone' in _lib.lib().hilo_last_error()
