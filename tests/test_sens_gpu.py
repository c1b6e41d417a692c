"""GPU: forward sensitivities of the error-controlled roll-out (`Model.rollout(..., sensitivities=)`, `hilo_model_rollout_sens`):
one instance on a team of T lanes, T the smallest power of two >= the number of columns NS.

The accuracy bound is that of tests/sens_reference.py: the error of the augmented trajectory [x; vec S] against the tight scipy
solution (DOP853 at 1e-13), relative to |.| + abstol / reltol, is at most 10 times the larger of scipy RK45's error on the same
augmented instance at the same tolerances and the disagreement of DOP853 and Radau at the case's nominal instance.  The sizes are
the smallest that reach every path of the team layout: a batch of 70 leaves the last wave partly filled for every T, NS = 5 leaves
three lanes of a team idle, NS = 4 and NS = 1 fill theirs.  Each test prints the figures it asserts on."""
import functools

import numpy as np
import pytest
import torch

from hilo_mpc_amd import Model
from tests import sens_reference as sn
from tests import sim_reference as sr
from tests.test_rollout_gpu import ACCURACY, _batch

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-8, 1e-10
OPTS = {'reltol': RTOL, 'abstol': ATOL}
B, STEPS = 70, 5
SUBSET = np.linspace(0, B - 1, 8).astype(int)           # the first and the last instance of the batch among them


def _columns(sens_part, groups):
    """{'g': [rows, B, n, n_g]} -> the kernel's layout [rows, B, NS, n], columns in the order of `groups`"""
    return np.concatenate([np.asarray(sens_part[g]).transpose(0, 1, 3, 2) for g in groups], axis=2)


def _check(tag, x, S, ref, admissible, e45, e_tight):
    """x [rows, n, nx], S [rows, n, NS, nx], ref [rows, n, nx (1 + NS)]"""
    w = sn.join(x, S)
    worst = 0.
    for i in range(ref.shape[1]):
        err = sr.rel_err(w[:, i], ref[:, i], RTOL, ATOL)
        worst = max(worst, err / max(e45[i], e_tight))
        assert err <= admissible[i], (tag, i, err, admissible[i])
    print(f"{tag}: largest error / max(RK45's error, DOP853 vs Radau) over {ref.shape[1]} instances: {worst:.2f} "
          f"(RK45 errors {e45.min():.2e} .. {e45.max():.2e}, DOP853 vs Radau {e_tight:.2e})")


@functools.lru_cache(maxsize=None)
def _accuracy_run(name):
    """The roll-out of the accuracy test, shared with the test of the measurement columns."""
    build, rhs_name, case, dt = ACCURACY[name]
    m = build().setup(dt=dt, solver='dopri5', solver_options=OPTS)
    X0, U, P = _batch(case, B)
    x, y, st, sens = m.rollout(X0, U, P if P.shape[1] else None, steps=STEPS, return_stats=True, sensitivities=True)
    return m, (X0, U, P), x, y, st, sens


@pytest.mark.parametrize('name', sorted(ACCURACY))
def test_accuracy_against_tight_solution(name):
    """pendulum4: NS 5, T 8, three idle lanes; chemostat4: NS 10, T 16; cstr3 as expressions (run-time compiled): NS 4 = T."""
    _, rhs_name, case, dt = ACCURACY[name]
    m, (X0, U, P), x, y, st, sens = _accuracy_run(name)
    groups = sn.groups_of(sr.oracle_model(rhs_name))
    ns = sn.n_columns(sr.oracle_model(rhs_name), groups)
    assert list(sens['x']) == list(groups) and ns == {'pendulum4': 5, 'chemostat4': 10, 'cstr3_expressions': 4}[name]
    assert x.shape == (STEPS + 1, B, m.n_x) and y.shape == (STEPS, B, m.n_y)
    assert not st['status'].any()
    np.testing.assert_array_equal(st['n_rhs'], 6 * (st['n_accepted'] + st['n_rejected']) + 2)
    print(f"{name}: augmented rhs evaluations {st['n_rhs'].min()} .. {st['n_rhs'].max()}, rejected share "
          f"{st['n_rejected'].sum() / (st['n_accepted'].sum() + st['n_rejected'].sum()):.3f}")
    np.testing.assert_array_equal(x[0], X0)
    S = _columns(sens['x'], groups)
    seed = np.zeros((ns, m.n_x))
    seed[:m.n_x] = np.eye(m.n_x)
    np.testing.assert_array_equal(S[0], np.tile(seed, (B, 1, 1)))                     # row 0 is the seed
    ref, admissible, e45, e_tight = sn.bounds_batch(rhs_name, groups, X0[SUBSET], U[SUBSET], P[SUBSET], dt, STEPS, RTOL, ATOL,
                                                    nominal_case=case)
    _check(name, x[:, SUBSET], S[:, SUBSET], ref, admissible, e45, e_tight)


@pytest.mark.parametrize('name,groups,big', [('pendulum4', ('u',), 65), ('chemostat4', ('x0',), 17)])
def test_team_sizes_at_their_edges(name, groups, big):
    """pendulum4 with ('u',): NS 1, a team of one lane, 64 instances per wave; chemostat4 with ('x0',): NS 4 = T, 16 per wave.  A
    batch of one (a wave with one team) and one of 64 / T + 1 (a second wave with one team); every instance within the bound."""
    _, rhs_name, case, dt = ACCURACY[name]
    steps = 3
    m = Model(name).setup(dt=dt, solver='dopri5', solver_options=OPTS)
    X0, U, P = _batch(case, big)
    ref, admissible, e45, e_tight = sn.bounds_batch(rhs_name, groups, X0, U, P, dt, steps, RTOL, ATOL, nominal_case=case)
    for n in (1, big):
        x, y, st, sens = m.rollout(X0[:n], U[:n], P[:n] if P.shape[1] else None, steps=steps, return_stats=True, sensitivities=groups)
        assert not st['status'].any() and list(sens['x']) == list(groups)
        np.testing.assert_array_equal(st['n_rhs'], 6 * (st['n_accepted'] + st['n_rejected']) + 2)
        _check(f"{name} {groups} B={n}", x, _columns(sens['x'], groups), ref[:, :n], admissible[:n], e45[:n], e_tight)


def test_an_instance_does_not_depend_on_its_neighbours():
    """Bitwise: alone (one team in the wave), or at position 37 among 70 different instances whose teams take other numbers of
    steps in the same wave."""
    m = Model('pendulum4').setup(dt=.5, solver='dopri5', solver_options=OPTS)
    rng = np.random.default_rng(13)
    X0 = rng.uniform(-1, 1, (B, 4)) * np.array([.5, .5, 3., 3.])
    U = rng.uniform(-5, 5, (B, 1))
    x, y, st, sens = m.rollout(X0, U, steps=STEPS, return_stats=True, sensitivities=True)
    assert not st['status'].any() and st['n_accepted'].max() > st['n_accepted'].min()       # the batch IS mixed
    x1, y1, st1, sens1 = m.rollout(X0[37:38], U[37:38], steps=STEPS, return_stats=True, sensitivities=True)
    np.testing.assert_array_equal(x1[:, 0], x[:, 37])
    np.testing.assert_array_equal(y1[:, 0], y[:, 37])
    for part in ('x', 'y'):
        for g in ('x0', 'u'):
            np.testing.assert_array_equal(sens1[part][g][:, 0], sens[part][g][:, 37])
    assert all(st1[k][0] == st[k][37] for k in st)


@pytest.mark.parametrize('name', ['chemostat4', 'cstr3_expressions'])
def test_measurement_columns(name):
    """sens['y'] = h_x S + h_theta with the oracle's derivatives at the returned states (cstr3 measures the reaction rate, a
    nonlinear function of all three states); the tolerance of the measurement check in tests/test_rollout_gpu.py."""
    _, rhs_name, case, dt = ACCURACY[name]
    m, (X0, U, P), x, y, st, sens = _accuracy_run(name)
    groups = sn.groups_of(sr.oracle_model(rhs_name))
    S, SY = _columns(sens['x'], groups), _columns(sens['y'], groups)
    assert SY.shape == (STEPS, B, S.shape[2], m.n_y)
    worst = 0.
    for i in SUBSET:
        for k in range(STEPS):
            want = sn.meas_sens(rhs_name, groups, x[k + 1, i], S[k + 1, i], U[i], P[i])
            np.testing.assert_allclose(SY[k, i], want, rtol=1e-9, atol=1e-12)
            worst = max(worst, float(np.max(np.abs(SY[k, i] - want) / (1e-9 * np.abs(want) + 1e-12))))
    print(f"{name}: largest |sens y - (h_x S + h_theta)| / (1e-9 |.| + 1e-12): {worst:.3f}")


def test_input_sequence_with_the_x0_and_p_columns():
    """Inputs that change at every sampling instant: the x0 and p columns go on across the instants (NS 8, T 8); 'u' is refused."""
    m = Model('chemostat4').setup(dt=4., solver='dopri5', solver_options=OPTS)
    n, groups = 20, ('x0', 'p')
    X0, U0, P = _batch('chemostat4', n)
    U = U0[None] * (1 + .5 * np.random.default_rng(7).uniform(-1, 1, (STEPS, n, 2)))
    x, y, st, sens = m.rollout(X0, U, P, steps=STEPS, return_stats=True, sensitivities=groups)
    assert not st['status'].any()
    np.testing.assert_array_equal(st['n_rhs'], 6 * (st['n_accepted'] + st['n_rejected']) + STEPS + 1)   # a first slope per interval
    sub = np.array([0, 7, 13, 19])
    ref, admissible, e45, e_tight = sn.bounds_batch('chemostat4', groups, X0[sub], U[:, sub], P[sub], 4., STEPS, RTOL, ATOL,
                                                    nominal_case='chemostat4')
    _check("chemostat4, input sequence, ('x0', 'p')", x[:, sub], _columns(sens['x'], groups)[:, sub], ref, admissible, e45, e_tight)
    with pytest.raises(ValueError, match="input sequence"):
        m.rollout(X0, U, P, steps=STEPS, sensitivities=('u',))
    with pytest.raises(ValueError, match="input sequence"):
        m.rollout(X0, U, P, steps=STEPS, sensitivities=True)


def test_time_variant_model_against_the_closed_form():
    """dx/dt = -a x + u sin(w t) from t0 = 1.5 with the input held:
        x(t) = E x0 + u [(a sin wt - w cos wt) - E (a sin wt0 - w cos wt0)] / (a^2 + w^2),  E = exp(-a (t - t0)),
    and its derivatives with respect to x0, u, a, w by sympy.  The error is measured in units of reltol (|value| + abstol / reltol).
    A bound of 100 such units follows from the method: the controller holds the LOCAL error of a step, in the norm over all five
    components, below reltol x scale; the global error at a sampling instant is at most the sum of the local errors of the steps
    before it (the flow contracts: a > 0), and the roll-out takes fewer than 100 steps (asserted).  Measured on an MI355X: 1.93
    units, at most 73 attempted steps - far inside, so the bound asserted is 10 x the measured value, 20 units."""
    import sympy as sp
    m = Model(name='decay_forced')
    m.set_parameters(['a', 'w'])
    m.set_equations("dx/dt = -a*x(t) + u(k)*sin(w*t)\ny(k) = x(t)")
    dt, steps, t0 = .5, 6, 1.5
    m.setup(dt=dt, solver='dopri5', solver_options=OPTS)
    n = 9
    rng = np.random.default_rng(5)
    X0, U, P = rng.uniform(.5, 2., (n, 1)), rng.uniform(-2., 2., (n, 1)), np.column_stack([rng.uniform(.3, 2., n), rng.uniform(.5, 4., n)])
    x, y, st, sens = m.rollout(X0, U, P, steps=steps, return_stats=True, t0=t0, sensitivities=True)
    assert not st['status'].any() and (st['n_accepted'] + st['n_rejected']).max() < 100
    x0s, us, a, w, t = sp.symbols('x0 u a w t')
    E = sp.exp(-a * (t - t0))
    xs = E * x0s + us * ((a * sp.sin(w * t) - w * sp.cos(w * t)) - E * (a * sp.sin(w * t0) - w * sp.cos(w * t0))) / (a**2 + w**2)
    fn = sp.lambdify((x0s, us, a, w, t), [xs] + [xs.diff(s) for s in (x0s, us, a, w)], modules='numpy')
    tt = t0 + dt * np.arange(steps + 1)
    want = np.array([[fn(X0[i, 0], U[i, 0], P[i, 0], P[i, 1], tk) for i in range(n)] for tk in tt], dtype=float)   # [rows, n, 5]
    got = np.concatenate([x, sens['x']['x0'][:, :, :, 0], sens['x']['u'][:, :, :, 0], sens['x']['p'][:, :, 0, :]], axis=2)
    assert got.shape == want.shape == (steps + 1, n, 5)
    margin = float(np.max(np.abs(got - want) / (np.abs(want) + ATOL / RTOL))) / RTOL
    print(f"decay_forced: largest error / (reltol (|value| + abstol / reltol)) = {margin:.2f} (bound 20), attempted steps at most "
          f"{(st['n_accepted'] + st['n_rejected']).max()}")
    assert margin <= 20.
    np.testing.assert_array_equal(y, x[1:])                                   # y = x, and its columns are the state's
    np.testing.assert_array_equal(sens['y']['p'], sens['x']['p'][1:])
    # the start time matters: from t0 = 0 the trajectory is another one
    x_0, _ = m.rollout(X0, U, P, steps=steps)
    assert np.max(np.abs(x_0 - x)) > 1e-2


def test_failure_is_contained():
    """dx/dt = x^2 as expressions over [0, 2] with max_num_steps 50: from 1 the solution 1 / (1 - t) leaves at t = 1 and
    dx/dx0 = 1 / (1 - t)^2 with it; from -1 both go on, -1 / (1 + t) and 1 / (1 + t)^2.  Three failing instances among five that
    finish.  Every loop of the kernel is bounded by max_num_steps per interval."""
    m = Model(name='square')
    xs = m.set_dynamical_states(['x'])
    m.set_dynamical_equations([xs[0] * xs[0]])
    m.set_measurement_equations([xs[0]])
    m.setup(dt=.25, solver='dopri5', solver_options=dict(OPTS, max_num_steps=50))
    steps = 8
    X0 = np.array([[1.], [-1.], [-1.], [1.], [-1.], [-1.], [1.], [-1.]])
    bad = X0[:, 0] > 0
    x, y, st, sens = m.rollout(X0, steps=steps, return_stats=True, sensitivities=True)
    assert list(sens['x']) == ['x0'] and sens['x']['x0'].shape == (steps + 1, 8, 1, 1)
    assert (st['status'][bad] != 0).all() and (st['status'][~bad] == 0).all()
    assert ((st['n_accepted'] + st['n_rejected']) <= steps * 50).all()
    print("failing instances: status", st['status'][bad], "attempted steps", (st['n_accepted'] + st['n_rejected'])[bad])
    t = .25 * np.arange(steps + 1)
    S, SY = sens['x']['x0'][:, :, 0, 0], sens['y']['x0'][:, :, 0, 0]
    np.testing.assert_array_equal(np.isnan(S), np.isnan(x[:, :, 0]))          # NaN in S exactly where it is in x
    np.testing.assert_array_equal(np.isnan(SY), np.isnan(x[1:, :, 0]))
    assert np.isnan(x[t > 1.][:, bad]).all() and np.isfinite(x[t < 1.][:, bad]).all()
    nan_rows = np.isnan(x[:, bad, 0])
    assert (np.diff(nan_rows.astype(int), axis=0) >= 0).all()                 # from the interval not reached onwards
    assert np.isfinite(x[:, ~bad]).all() and np.isfinite(S[:, ~bad]).all()
    np.testing.assert_allclose(x[:, ~bad, 0], np.tile(-1. / (1. + t)[:, None], (1, 5)), rtol=1e-6)
    np.testing.assert_allclose(S[:, ~bad], np.tile(1. / (1. + t)[:, None] ** 2, (1, 5)), rtol=1e-6)
    np.testing.assert_allclose(x[t < 1.][:, bad, 0], np.tile(1. / (1. - t[t < 1.])[:, None], (1, 3)), rtol=1e-6)
    # the call returned; the next one on the same handle works
    x2, _, st2, _ = m.rollout(-np.ones((2, 1)), steps=steps, return_stats=True, sensitivities=True)
    assert not st2['status'].any()
    np.testing.assert_array_equal(x2[:, 0], x[:, 1])


def test_device_tensors_and_one_step():
    """Device tensors in, device tensors out (permuted views of the kernel's buffers); `step(..., sensitivities=True)` is row 1 of
    the roll-out bit for bit."""
    m = Model('chemostat4').setup(dt=4., solver='dopri5', solver_options=OPTS)
    n = 6
    X0, U, P = _batch('chemostat4', n)
    x, y, sens = m.rollout(X0, U, P, steps=3, sensitivities=True)
    dev = torch.device('cuda')
    xt, yt, st = m.rollout(torch.as_tensor(X0, device=dev), torch.as_tensor(U, device=dev), torch.as_tensor(P, device=dev), steps=3,
                           sensitivities=True)
    assert xt.is_cuda and yt.is_cuda
    np.testing.assert_array_equal(xt.cpu().numpy(), x)
    for part in ('x', 'y'):
        for g in ('x0', 'u', 'p'):
            assert st[part][g].is_cuda and st[part][g].shape == sens[part][g].shape
            np.testing.assert_array_equal(st[part][g].cpu().numpy(), sens[part][g])
    assert st['x']['u'].stride() == (n * 40, 40, 1, 4)                        # a view of [rows, B, 10, 4]
    xn, yn, s1 = m.step(X0, U, P, sensitivities=True)
    np.testing.assert_array_equal(xn, x[1])
    np.testing.assert_array_equal(yn, y[0])
    for g in ('x0', 'u', 'p'):
        np.testing.assert_array_equal(s1['x'][g], sens['x'][g][1])
        np.testing.assert_array_equal(s1['y'][g], sens['y'][g][0])


def test_the_library_refuses_a_discrete_handle():
    """hilo_model_rollout_sens on a discretised handle: HILO_ENOTSUP (Python's own check keeps a user from reaching it)."""
    import ctypes as C
    from hilo_mpc_amd import _lib
    from hilo_mpc_amd._device import ptr, stream_ptr
    m = Model('chemostat4').discretize('rk4').setup(dt=1.)
    h = m._plant_handle()
    dev = h._dev
    x0 = torch.tensor([[.1, 40., .5, .2]], dtype=torch.float64, device=dev)
    up = torch.tensor([[.1, .2, 100., 4., 1., 0.]], dtype=torch.float64, device=dev)
    X = torch.empty(3, 1, 4, dtype=torch.float64, device=dev)
    SX = torch.empty(3, 1, 10, 4, dtype=torch.float64, device=dev)
    opts = _lib.SimOpts(1, 0, 0., 0., 0.)
    rc = _lib.lib().hilo_model_rollout_sens(h._handle, C.byref(opts), 1, 2, ptr(x0), ptr(up), 6, 0, 7, ptr(X), None, ptr(SX), None, None,
                                            stream_ptr(dev))
    assert rc == -4 and b'HILO_SIM_DOPRI5 integrates a continuous model' in _lib.lib().hilo_last_error()
    opts.method = 2
    rc = _lib.lib().hilo_model_rollout_sens(h._handle, C.byref(opts), 1, 2, ptr(x0), ptr(up), 6, 0, 7, ptr(X), None, ptr(SX), None, None,
                                            stream_ptr(dev))
    assert rc == -4 and b'HILO_SIM_DOPRI5 alone' in _lib.lib().hilo_last_error()
