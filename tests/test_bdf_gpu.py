"""GPU: variable-order implicit integration, `Model.setup(solver='bdf')` (csrc/hilo_integrate.h `bdf_interval`, one instance per
lane), through `Model.rollout` / `Model.step`.

The accuracy bound is that of tests/stiff_reference.py: the error against the tight solution, relative to |x| + abstol / reltol, is
at most 10 times the larger of the error of scipy's BDF on the same instance at the same tolerances (given the exact Jacobian) and
the disagreement of two tight solutions.  The batch is 130 instances - two full waves and a partial one - with the initial states
(and Robertson's rate constants) perturbed by +-10 %; 8 instances at the edges of the waves are compared with scipy.  Each test
prints the figures it asserts on."""
import numpy as np
import pytest
import torch

from hilo_mpc_amd import Model
from tests import sim_reference as sr
from tests import stiff_reference as st

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-8, 1e-10
OPTS = {'reltol': RTOL, 'abstol': ATOL}
B = 130
IDX = np.array([0, 1, 63, 64, 65, 127, 128, 129])
STEPS = 10


def _robertson():
    m = Model(name='robertson3')
    x = m.set_dynamical_states(['a', 'b', 'c'])
    k = m.set_parameters(['k1', 'k2', 'k3'])
    m.set_dynamical_equations([-k[0] * x[0] + k[2] * x[1] * x[2], k[0] * x[0] - k[2] * x[1] * x[2] - k[1] * x[1] * x[1],
                               k[1] * x[1] * x[1]])
    m.set_measurement_equations([x[0] + x[2], x[1]])
    return m


def _vdp():
    m = Model(name='vdp2')
    x = m.set_dynamical_states(['x', 'v'])
    mu = m.set_parameters(['mu'])
    m.set_dynamical_equations([x[1], mu[0] * ((1. - x[0] * x[0]) * x[1]) - x[0]])
    m.set_measurement_equations([x[0]])
    return m


def _square():
    m = Model(name='square')
    x = m.set_dynamical_states(['x'])
    m.set_dynamical_equations([x[0] * x[0]])
    m.set_measurement_equations([x[0]])
    return m


def _measure(name, x, U, P, dt):
    if name == 'robertson3':
        return np.stack([x[:, 0] + x[:, 2], x[:, 1]], axis=1)
    if name == 'vdp2':
        return x[:, :1]
    return sr.oracle_model(name).h(x, U, P, dt)


BUILD = {'robertson3': _robertson, 'vdp2': _vdp, 'chemostat4': lambda: Model('chemostat4'), 'pendulum4': lambda: Model('pendulum4')}


def _batch(case, n=B, seed=17):
    x0, u, p, _, _ = st.CASES[case]
    rng = np.random.default_rng(seed)
    X0 = np.asarray(x0) * (1 + .1 * rng.uniform(-1, 1, (n, len(x0))))
    if case == 'pendulum4':                               # (three of the four nominal states are zero)
        X0 = X0 + .03 * rng.uniform(-1, 1, (n, 4))
    U = np.asarray(u, dtype=float) * (1 + .1 * rng.uniform(-1, 1, (n, len(u))))
    P = np.tile(np.asarray(p, dtype=float), (n, 1))
    if case.startswith('robertson3'):
        P = P * (1 + .1 * rng.uniform(-1, 1, P.shape))
    return X0, U, P


def _args(U, P):
    return (U if U.shape[-1] else None), (P if P.shape[-1] else None)


def _check_against_bound(tag, x, ref, admissible, e_bdf, e_tight, rtol=RTOL, atol=ATOL):
    """x, ref [steps + 1, n, nx]"""
    worst = 0.
    for i in range(ref.shape[1]):
        err = sr.rel_err(x[:, i], ref[:, i], rtol, atol)
        worst = max(worst, err / max(e_bdf[i], e_tight[i]))
        assert err <= admissible[i], (tag, i, err, admissible[i])
    print(f"{tag}: largest error / max(scipy BDF's error, tight solutions' disagreement) over {ref.shape[1]} instances: {worst:.2f} "
          f"(BDF errors {e_bdf.min():.2e} .. {e_bdf.max():.2e})")


@pytest.mark.parametrize('case', ['robertson3', 'vdp2', 'chemostat4', 'pendulum4'])
def test_bdf_accuracy_against_tight_solution(case):
    """robertson3 and vdp2 are written as expressions (the run-time compiled kernel), chemostat4 and pendulum4 are the library's."""
    dt = st.CASES[case][3]
    m = BUILD[case]().setup(dt=dt, solver='bdf', solver_options=OPTS)
    X0, U, P = _batch(case)
    u, p = _args(U, P)
    x, y, stats = m.rollout(X0, u, p, steps=STEPS, return_stats=True)
    assert x.shape == (STEPS + 1, B, m.n_x) and y.shape == (STEPS, B, m.n_y)
    assert not stats['status'].any()
    ref, admissible, e_bdf, e_tight, counts = st.bounds_batch(case, X0[IDX], U[IDX], P[IDX], dt, STEPS, RTOL, ATOL)
    print(f"{case}: rhs evaluations {stats['n_rhs'].min()} .. {stats['n_rhs'].max()}, accepted {stats['n_accepted'].min()} .. "
          f"{stats['n_accepted'].max()}, rejected {stats['n_rejected'].min()} .. {stats['n_rejected'].max()}; on the 8 instances "
          f"accepted : scipy's {stats['n_accepted'][IDX].tolist()} : {counts[:, 0].tolist()}, rhs : nfev "
          f"{stats['n_rhs'][IDX].tolist()} : {counts[:, 1].tolist()}")
    _check_against_bound(case, x[:, IDX], ref, admissible, e_bdf, e_tight)
    # the measurements are those of the returned states
    for k in (0, STEPS - 1):
        np.testing.assert_allclose(y[k], _measure(case, x[k + 1], U, P, dt), rtol=1e-12, atol=1e-300)
    # step() is a one-interval roll-out - bitwise - and nothing is carried between calls.  (The first row of the 10-interval
    # roll-out is NOT that number: with the inputs held only the end of the roll-out clips a step, the first instant is read off
    # the interpolant of a step that passed it; both are within the bound.)
    xs, ys = m.step(X0, u, p)
    x1, y1 = m.rollout(X0, u, p, steps=1)
    np.testing.assert_array_equal(xs, x1[1])
    np.testing.assert_array_equal(ys, y1[0])
    for j, i in enumerate(IDX):
        assert sr.rel_err(xs[i], ref[1, j], RTOL, ATOL) <= admissible[j]


def test_bdf_with_an_input_sequence():
    """Robertson's k1 jumps at every sampling instant: every interval is an integration of its own, as scipy restarted there."""
    dt = st.CASES['robertson3'][3]
    m = _robertson().setup(dt=dt, solver='bdf', solver_options=OPTS)
    X0, _, P = _batch('robertson3')
    Ps = np.tile(P[None], (STEPS, 1, 1))
    Ps[:, :, 0] *= np.random.default_rng(4).uniform(.5, 2., (STEPS, B))
    x, y, stats = m.rollout(X0, None, Ps, steps=STEPS, return_stats=True)
    assert not stats['status'].any()
    ref, admissible, e_bdf, e_tight, counts = st.bounds_batch('robertson3', X0[IDX], np.zeros((len(IDX), 0)), Ps[:, IDX], dt, STEPS,
                                                              RTOL, ATOL)
    print(f"accepted : scipy's {stats['n_accepted'][IDX].tolist()} : {counts[:, 0].tolist()}")
    _check_against_bound('robertson3, parameter sequence', x[:, IDX], ref, admissible, e_bdf, e_tight)


def test_an_instance_does_not_depend_on_its_wave():
    """Bitwise: instance 65 alone, or inside the batch among lanes of other orders and step counts."""
    dt = st.CASES['robertson3'][3]
    m = _robertson().setup(dt=dt, solver='bdf', solver_options=OPTS)
    X0, _, P = _batch('robertson3')
    x, y, stats = m.rollout(X0, None, P, steps=STEPS, return_stats=True)
    wave = slice(64, 128)
    assert len(np.unique(stats['n_accepted'][wave])) > 1 or len(np.unique(stats['n_rhs'][wave])) > 1      # the wave IS mixed
    xi, yi, si = m.rollout(X0[65:66], None, P[65:66], steps=STEPS, return_stats=True)
    np.testing.assert_array_equal(xi[:, 0], x[:, 65])
    np.testing.assert_array_equal(yi[:, 0], y[:, 65])
    assert all(si[k][0] == stats[k][65] for k in stats)


def test_bdf_goes_on_where_the_explicit_pair_gives_up():
    """robertson3_long (dt = 100) at the default options: about 2e5 attempted steps per interval for the explicit pair."""
    case = 'robertson3_long'
    dt = st.CASES[case][3]
    X0, U, P = _batch(case, 4)
    xe, _, se = _robertson().setup(dt=dt, solver='dopri5').rollout(X0, None, P, steps=STEPS, return_stats=True)
    assert (se['status'] == 1).all() and np.isnan(xe[1:]).all()          # HILO_SIM_STATUS_MAX_STEPS in the first interval
    x, _, stats = _robertson().setup(dt=dt, solver='bdf').rollout(X0, None, P, steps=STEPS, return_stats=True)
    assert not stats['status'].any()
    ref, admissible, e_bdf, e_tight, counts = st.bounds_batch(case, X0, U, P, dt, STEPS, 1e-6, 1e-8)
    print(f"dopri5: attempted {(se['n_accepted'] + se['n_rejected']).tolist()}; bdf: accepted {stats['n_accepted'].tolist()}, rhs "
          f"{stats['n_rhs'].tolist()} (scipy {counts[:, 0].tolist()}, {counts[:, 1].tolist()})")
    _check_against_bound(case, x, ref, admissible, e_bdf, e_tight, 1e-6, 1e-8)


def test_failure_is_contained():
    """dx/dt = x^2 over [0, 2]: one instance from +1 (the solution 1 / (1 - t) leaves at t = 1) among instances started near -1."""
    m = _square().setup(dt=.25, solver='bdf', solver_options=OPTS)
    n, steps = 70, 8
    X0 = -1. - .1 * np.random.default_rng(5).uniform(0, 1, (n, 1))
    X0[0] = 1.
    x, y, stats = m.rollout(X0, steps=steps, return_stats=True)          # returned: the call itself is HILO_OK
    t = .25 * np.arange(steps + 1)
    assert stats['status'][0] in (1, 2) and not stats['status'][1:].any()
    print("failed instance: status", stats['status'][0], "attempted steps", stats['n_accepted'][0] + stats['n_rejected'][0])
    assert np.isfinite(x[t < 1., 0]).all() and np.isnan(x[t > 1., 0]).all() and np.isnan(y[t[1:] > 1., 0]).all()
    assert np.isfinite(x[:, 1:]).all()
    near = [1, 63, 64, n - 1]
    none = np.zeros((len(near), 0))
    ref, admissible, e_bdf, e_tight, _ = st.bounds_batch('square', X0[near], none, none, .25, steps, RTOL, ATOL)
    np.testing.assert_allclose(ref[:, :, 0], 1. / (1. / X0[None, near, 0] - t[:, None]), rtol=1e-11)
    _check_against_bound('square', x[:, near], ref, admissible, e_bdf, e_tight)
    for i in near:
        xi, _, si = m.rollout(X0[i:i + 1], steps=steps, return_stats=True)
        np.testing.assert_array_equal(xi[:, 0], x[:, i])
        assert si['status'][0] == 0


def test_the_library_refuses_method_2_on_a_discretised_handle():
    import ctypes as C
    from hilo_mpc_amd import _lib
    from hilo_mpc_amd._device import ptr, stream_ptr
    P4 = [100., 4., 1., 0.]
    m = Model('chemostat4').discretize('rk4').setup(dt=1.)
    h = m._plant_handle()
    dev = h._dev
    x0 = torch.tensor([[.1, 40., .5, .2]], dtype=torch.float64, device=dev)
    up = torch.tensor([[.1, .2] + P4], dtype=torch.float64, device=dev)
    X = torch.empty(3, 1, 4, dtype=torch.float64, device=dev)
    opts = _lib.SimOpts(2, 0, 0., 0., 0.)
    rc = _lib.lib().hilo_model_rollout(h._handle, C.byref(opts), 1, 2, ptr(x0), ptr(up), 6, 0, ptr(X), None, None, stream_ptr(dev))
    assert rc == -4 and b'HILO_SIM_BDF integrates a continuous model' in _lib.lib().hilo_last_error()
