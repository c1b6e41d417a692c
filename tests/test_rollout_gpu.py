"""GPU: error-controlled integration (`Model.setup(solver='dopri5')`) and one-launch roll-outs (`Model.rollout`).

The accuracy bound is that of tests/sim_reference.py: the error against the tight scipy solution (DOP853 at 1e-13), relative to
|x| + abstol / reltol, is at most 10 times the larger of scipy RK45's error on the same instance at the same tolerances and the
disagreement of the two tight solutions (DOP853 against Radau).  Each test prints the figures it asserts on."""
import numpy as np
import pytest
import torch

from hilo_mpc_amd import Model
from tests import sim_reference as sr

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-8, 1e-10
OPTS = {'reltol': RTOL, 'abstol': ATOL}
SUBSET = np.linspace(0, 4095, 32).astype(int)
P4 = [100., 4., 1., 0.]


def _cstr3_expressions():
    from tests.problems import symbolic_model
    return symbolic_model('cstr3')


# model under test, reference right-hand side, nominal (x0, u, p), dt
ACCURACY = {
    'pendulum4': (lambda: Model('pendulum4'), 'pendulum4', 'pendulum4', .5),
    'chemostat4': (lambda: Model('chemostat4'), 'chemostat4', 'chemostat4', 4.),
    'cstr3_expressions': (_cstr3_expressions, 'cstr3', 'cstr3_heated', 10.),
}


def _batch(case, B, seed=11):
    x0, u, p, _, _ = sr.CASES[case]
    rng = np.random.default_rng(seed)
    X0 = np.asarray(x0) * (1 + .1 * rng.uniform(-1, 1, (B, len(x0))))
    if case == 'pendulum4':                               # (three of the four nominal states are zero)
        X0 = X0 + .03 * rng.uniform(-1, 1, (B, 4))
    U = np.asarray(u) * (1 + .1 * rng.uniform(-1, 1, (B, len(u))))
    P = np.tile(np.asarray(p, dtype=float), (B, 1))
    return X0, U, P


def _check_against_bound(tag, x, ref, admissible, e45, e_tight):
    """x, ref [steps + 1, n, nx]"""
    worst = 0.
    for i in range(ref.shape[1]):
        err = sr.rel_err(x[:, i], ref[:, i], RTOL, ATOL)
        worst = max(worst, err / max(e45[i], e_tight[i]))
        assert err <= admissible[i], (tag, i, err, admissible[i])
    print(f"{tag}: largest error / max(RK45's error, DOP853 vs Radau) over {ref.shape[1]} instances: {worst:.2f} "
          f"(RK45 errors {e45.min():.2e} .. {e45.max():.2e})")


@pytest.mark.parametrize('name', sorted(ACCURACY))
def test_dopri5_accuracy_against_tight_solution(name):
    """4096 instances, 10 sampling intervals; 32 of them against scipy (the measured ratios: DESIGN.md 5.2b)."""
    build, rhs_name, case, dt = ACCURACY[name]
    steps, B = 10, 4096
    m = build().setup(dt=dt, solver='dopri5', solver_options=OPTS)
    X0, U, P = _batch(case, B)
    x, y, st = m.rollout(X0, U, P if P.shape[1] else None, steps=steps, return_stats=True)
    assert x.shape == (steps + 1, B, m.n_x) and y.shape == (steps, B, m.n_y)
    assert not st['status'].any()                                   # max_num_steps at its default does not bind
    print(f"{name}: rhs evaluations {st['n_rhs'].min()} .. {st['n_rhs'].max()}, accepted {st['n_accepted'].min()} .. "
          f"{st['n_accepted'].max()}, rejected share {st['n_rejected'].sum() / (st['n_accepted'].sum() + st['n_rejected'].sum()):.3f}")
    np.testing.assert_array_equal(st['n_rhs'], 6 * (st['n_accepted'] + st['n_rejected']) + 2)
    ref, admissible, e45, e_tight = sr.bounds_batch(rhs_name, X0[SUBSET], U[SUBSET], P[SUBSET], dt, steps, RTOL, ATOL)
    _check_against_bound(name, x[:, SUBSET], ref, admissible, e45, e_tight)
    # the measurements are those of the states at the sampling instants
    om = sr.oracle_model(rhs_name)
    for k in (0, steps - 1):
        np.testing.assert_allclose(y[k, SUBSET], om.h(x[k + 1, SUBSET], U[SUBSET], P[SUBSET], dt), rtol=1e-9, atol=1e-12)
    # one sampling interval through step(): the first row of the roll-out (the same kernel from the same state)
    xs, ys = m.step(X0[SUBSET], U[SUBSET], P[SUBSET] if P.shape[1] else None)
    np.testing.assert_array_equal(xs, x[1, SUBSET])


def _text_model():
    m = Model(name='toy_text_u', discrete=True)
    m.set_inputs(['u'])                 # (in a discrete model `u(k)` cannot be told from a state: declared)
    m.set_equations(equations=['x(k+1) = x(k)/2 + 25*dt*x(k)/(1 + x(k)^2) + a*u(k)', 'y(k) = x(k)^2/20'])
    return m.setup(dt=.1)


@pytest.mark.parametrize('which', ['chemostat4_rk4', 'discrete_text'])
@pytest.mark.parametrize('sequence', [False, True])
def test_rollout_equals_repeated_steps(which, sequence):
    """The roll-out with the handle's own map against 20 calls of Model.step: one map compiled into two kernels, the tolerance
    tests/test_zz_late_gpu.py uses for that."""
    steps, B = 20, 200
    rng = np.random.default_rng(5)
    if which == 'chemostat4_rk4':
        m = Model('chemostat4').discretize('rk4').setup(dt=1.)
        X0 = np.array([.1, 40., .5, .2]) * (1 + .1 * rng.uniform(-1, 1, (B, 4)))
        U = rng.uniform(0, .3, (steps, B, 2))
        p = P4
    else:
        m = _text_model()
        X0 = rng.uniform(-6, 6, (B, 1))
        U = rng.uniform(-1, 1, (steps, B, 1))
        p = [.3]
    if not sequence:
        U = U[0]
    x, y = m.rollout(X0, U, p, steps=steps)
    xs, ys = [X0], []
    for k in range(steps):
        xn, yn = m.step(xs[-1], U[k] if sequence else U, p)
        xs.append(xn), ys.append(yn)
    np.testing.assert_allclose(x, np.array(xs), rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(y, np.array(ys), rtol=1e-13, atol=1e-15)
    # device tensors in, device tensors out
    dev = torch.device('cuda')
    xt, yt = m.rollout(torch.as_tensor(X0, device=dev), torch.as_tensor(U, device=dev), p, steps=steps)
    assert xt.is_cuda and yt.is_cuda
    np.testing.assert_array_equal(xt.cpu().numpy(), x)
    np.testing.assert_array_equal(yt.cpu().numpy(), y)


def test_dopri5_with_an_input_sequence():
    """Inputs that change at every sampling instant, against scipy integrating interval by interval."""
    steps, B, n = 10, 256, 16
    m = Model('pendulum4').setup(dt=.5, solver='dopri5', solver_options=OPTS)
    X0, _, P = _batch('pendulum4', B)
    U = np.random.default_rng(7).uniform(-1, 1, (steps, B, 1))
    x, y, st = m.rollout(X0, U, steps=steps, return_stats=True)
    assert not st['status'].any()
    ref, admissible, e45, e_tight = sr.bounds_batch('pendulum4', X0[:n], U[:, :n], P[:n], .5, steps, RTOL, ATOL)
    _check_against_bound('pendulum4, input sequence', x[:, :n], ref, admissible, e45, e_tight)
    # a sequence shared by the batch (batch axis 1) is the same as the sequence repeated
    xa, _ = m.rollout(X0, U[:, :1], steps=steps)
    xb, _ = m.rollout(X0, np.repeat(U[:, :1], B, axis=1), steps=steps)
    np.testing.assert_array_equal(xa, xb)


def _square_model():
    m = Model(name='square')
    x = m.set_dynamical_states(['x'])
    m.set_dynamical_equations([x[0] * x[0]])
    m.set_measurement_equations([x[0]])
    return m.setup(dt=.25, solver='dopri5', solver_options=OPTS)


def test_failure_is_contained():
    """dx/dt = x^2 over [0, 2]: from 1 the solution 1 / (1 - t) leaves at t = 1, from -1 it is -1 / (1 + t)."""
    m = _square_model()
    B, steps = 128, 8
    X0 = np.concatenate([np.ones((B // 2, 1)), -np.ones((B // 2, 1))])
    x, y, st = m.rollout(X0, steps=steps, return_stats=True)
    t = .25 * np.arange(steps + 1)
    bad, good = slice(0, B // 2), slice(B // 2, B)
    assert (st['status'][bad] != 0).all() and (st['status'][good] == 0).all()
    print("failed half: status", np.unique(st['status'][bad]), "attempted steps", (st['n_accepted'] + st['n_rejected'])[bad].max())
    # NaN after the escape time (the sampling instant t = 1 itself is the pole: whatever large number a last clipped step lands on)
    assert np.isnan(x[t > 1.][:, bad]).all() and np.isnan(y[t[1:] > 1.][:, bad]).all()
    np.testing.assert_allclose(x[t < 1.][:, bad, 0], np.tile(1. / (1. - t[t < 1.])[:, None], (1, B // 2)), rtol=1e-6)
    ref, admissible, e45, e_tight = sr.bounds_batch('square', X0[-1:], np.zeros((1, 0)), np.zeros((1, 0)), .25, steps, RTOL, ATOL)
    np.testing.assert_allclose(ref[:, 0, 0], -1. / (1. + t), rtol=1e-12)
    assert np.isfinite(x[:, good]).all()
    for i in (B // 2, B - 1):
        assert sr.rel_err(x[:, i], ref[:, 0], RTOL, ATOL) <= admissible[0]
        assert sr.rel_err(x[:, i, 0], -1. / (1. + t), RTOL, ATOL) <= admissible[0]
    # the call returned; the next one on the same handle works
    x2, _, st2 = m.rollout(-np.ones((4, 1)), steps=steps, return_stats=True)
    assert not st2['status'].any()
    np.testing.assert_array_equal(x2[:, 0], x[:, B - 1])


def test_an_instance_does_not_depend_on_its_wave():
    """Bitwise: alone, or among 4096 instances of all kinds (other states, other inputs, other numbers of steps)."""
    m = Model('pendulum4').setup(dt=.5, solver='dopri5', solver_options=OPTS)
    B, steps = 4096, 6
    rng = np.random.default_rng(13)
    X0 = rng.uniform(-1, 1, (B, 4)) * np.array([.5, .5, 3., 3.])
    U = rng.uniform(-5, 5, (B, 1))
    x, _, st = m.rollout(X0, U, steps=steps, return_stats=True)
    assert st['n_accepted'].max() > 1.5 * st['n_accepted'].min()           # the batch IS mixed
    for i in (0, 63, 64, 1000, 4095):
        xi, _, sti = m.rollout(X0[i:i + 1], U[i:i + 1], steps=steps, return_stats=True)
        np.testing.assert_array_equal(xi[:, 0], x[:, i])
        assert all(sti[k][0] == st[k][i] for k in st)


def test_closed_loop_with_an_error_controlled_plant():
    """SimpleControlLoop with the C2 controller, three steps: a chemostat plant integrated under error control (loop a) against the
    same plant discretised with the classic Runge-Kutta step (loop b).  Asserted, all with factor 1:
      - equal solver statuses;
      - loop a's plant follows the exact flow (scipy, tight) from its own (x_k, u_k) within the accuracy bound of test 4;
      - step 0, where both loops hold the same state and - the controller being a deterministic function of the state - the same
        input: the loops differ by no more than the discretisation error e = |oracle rk4 map - exact flow| on those inputs, plus
        what the accuracy bound admits for the integrator;
      - later steps, where the loops hold different (x_k, u_k): by the triangle inequality
          x_b+ - x_a+ = [rk4(x_b, u_b) - flow(x_b, u_b)] + [flow(x_b, u_b) - flow(x_a, u_a)] + [flow(x_a, u_a) - x_a+]
        the difference of the loops, less what the EXACT flow makes of their differing arguments (computed by scipy, not
        estimated), is no more than the rk4 map's discretisation error on loop b's own inputs plus the integrator's admissible error.
    Every quantity is elementwise and absolute.  The unreduced difference and the accumulated map error are printed."""
    from hilo_mpc_amd import SimpleControlLoop
    from oracle import models as omodels
    from tests.problems import C2, c2_x0, product_nmpc
    B, steps = 8, 3
    x0 = c2_x0(B)
    runs = {}
    for key, plant in (('rk4', Model('chemostat4').discretize('rk4').setup(dt=C2['dt'])),
                       ('dopri5', Model('chemostat4').setup(dt=C2['dt'], solver='dopri5', solver_options=OPTS))):
        runs[key] = SimpleControlLoop(plant, product_nmpc(C2)).run(steps, x0, p=C2['p'])
    a, b = runs['dopri5'], runs['rk4']
    for sa, sb in zip(a['status'], b['status']):
        np.testing.assert_array_equal(sa, sb)
    rk4 = omodels.get('chemostat4').discretize(4)
    P = np.tile(C2['p'], (B, 1))
    dt = C2['dt']
    np.testing.assert_array_equal(np.asarray(a['u'][0]), np.asarray(b['u'][0]))          # same state, same controller
    scale = np.abs(a['x']).max(axis=(0, 1)) + ATOL / RTOL
    acc = np.zeros(B)
    for k in range(steps):
        xa, ua, xan = (np.asarray(a[q][k + j]) for q, j in (('x', 0), ('u', 0), ('x', 1)))
        xb, ub, xbn = (np.asarray(b[q][k + j]) for q, j in (('x', 0), ('u', 0), ('x', 1)))
        flow_a, adm_a, _, _ = sr.bounds_batch('chemostat4', xa, ua, P, dt, 1, RTOL, ATOL)
        flow_b = sr.bounds_batch('chemostat4', xb, ub, P, dt, 1, RTOL, ATOL)[0] if k else flow_a
        flow_a, flow_b = flow_a[1], flow_b[1]
        for i in range(B):
            assert sr.rel_err(xan[i], flow_a[i], RTOL, ATOL) <= adm_a[i]
        adm_abs = adm_a[:, None] * (np.abs(flow_a) + ATOL / RTOL)        # the accuracy bound as an absolute error per component
        e_b = np.abs(rk4.f(xb, ub, P, dt) - flow_b)                        # discretisation error of the rk4 map on loop b's inputs
        reduced = np.abs((xbn - xan) - (flow_b - flow_a))
        acc += np.max(e_b / scale, axis=1)
        print(f"step {k}: loops differ by {np.max(np.abs(xbn - xan) / scale):.3e} of the states' range, accumulated rk4 map error "
              f"{acc.max():.3e}; reduced difference / (map error + admissible) at most {np.max(reduced / (e_b + adm_abs)):.3f}")
        assert (reduced <= e_b + adm_abs).all()


def test_the_library_refuses_what_the_integrator_is_not_built_for():
    """The refusals of hilo_model_rollout itself, which Python's own checks keep a user from reaching: method 1 on a discretised
    handle (HILO_ENOTSUP) and an unknown method, by calling the C entry directly.  (The width limit HILO_SIM_DOPRI5_MAX_NX = 12
    cannot be reached with a handle that exists today: the zoo's filter models have at most 4 states, and the filter unit of a
    run-time compiled model stops compiling at 10 states - the unscented filter's tile no longer fits the LDS - so no such handle
    is created)"""
    import ctypes as C
    from hilo_mpc_amd import _lib
    from hilo_mpc_amd._device import ptr, stream_ptr
    m = Model('chemostat4').discretize('rk4').setup(dt=1.)
    x, _ = m.rollout(np.array([[.1, 40., .5, .2]]), [.1, .2], P4, steps=2)          # method 0 on this handle works
    assert np.isfinite(x).all()
    h = m._plant_handle()
    dev = h._dev
    x0 = torch.tensor([[.1, 40., .5, .2]], dtype=torch.float64, device=dev)
    up = torch.tensor([[.1, .2] + P4], dtype=torch.float64, device=dev)
    X = torch.empty(3, 1, 4, dtype=torch.float64, device=dev)
    opts = _lib.SimOpts(1, 0, 0., 0., 0.)
    rc = _lib.lib().hilo_model_rollout(h._handle, C.byref(opts), 1, 2, ptr(x0), ptr(up), 6, 0, ptr(X), None, None, stream_ptr(dev))
    assert rc == -4 and b'HILO_SIM_DOPRI5 integrates a continuous model' in _lib.lib().hilo_last_error()
    opts.method = 7
    rc = _lib.lib().hilo_model_rollout(h._handle, C.byref(opts), 1, 2, ptr(x0), ptr(up), 6, 0, ptr(X), None, None, stream_ptr(dev))
    assert rc == -1 and b'unknown method 7' in _lib.lib().hilo_last_error()
