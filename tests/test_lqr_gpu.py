"""GPU: `LQR`, `Model.linearization` and the C entries behind them (csrc/hilo_lqr.hip) against the references of
tests/lqr_reference.py: the reference's two known gains, batches with per-instance parameters against the numpy recursion and
scipy.linalg.solve_discrete_are under `1e-10 max(1, max|P|)` (K: max|K|), failed instances next to healthy ones in one wave, device
Jacobians against `system_matrices` under `1e-11 max(1, max|J|)`, gain scheduling, LTI models through `hilo_lqr_gain`, the size
refusal and a closed loop."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from tests import lqr_reference as lr
from tests.test_pins import K_P0, K_P1

pytestmark = pytest.mark.gpu

B130 = 130                                              # two full waves and two lanes


def _controller(model, horizon, Q=None, R=None):
    from hilo_mpc_amd import LQR
    c = LQR(model)
    c.horizon = horizon
    c.setup()
    c.Q = np.ones(model.n_x) if Q is None else Q
    c.R = np.ones(model.n_u) if R is None else R
    return c


@pytest.fixture(scope='module')
def p130():
    return np.random.default_rng(130).uniform(.5, 2., (B130, 1))


@pytest.fixture(scope='module')
def stationary130(p130):
    """the stationary solve of the healthy batch, shared by the tests that compare with it (left unchanged)"""
    c = _controller(lr.reference_model(), None)
    X = np.random.default_rng(131).standard_normal((B130, 3))
    u = c.call(x=X, p=p130)
    return dict(X=X, u=u.copy(), K=c.K.copy(), P=c.P.copy(), status=c.status.copy(), iterations=c.iterations.copy())


@pytest.mark.parametrize('p,K_ref', [(1., K_P1), (0., K_P0)])
def test_the_reference_gains_through_the_public_class(p, K_ref):
    c = _controller(lr.reference_model(), 5)
    x = np.array([1., -2., .5])
    u = c.call(x=x, p=[p])
    np.testing.assert_allclose(c.K, K_ref, rtol=1e-7, atol=1e-9)         # tests/test_LQR.py:328,342 (printed to 8 digits)
    np.testing.assert_allclose(u, -c.K @ x, rtol=1e-14, atol=1e-15)
    assert c.status == 0 and c.iterations == 5 and c.K.shape == (2, 3) and c.P.shape == (3, 3)


def test_batch_finite_horizon_against_the_numpy_recursion(p130):
    c = _controller(lr.reference_model(), 5)
    X = np.random.default_rng(132).standard_normal((B130, 3))
    u = c.call(x=X, p=p130)
    assert c.K.shape == (B130, 2, 3) and np.all(c.status == 0) and np.all(c.iterations == 5)
    worst = 0.
    for b in range(B130):
        Kn, Pn = lr.riccati_finite(*lr.lqr_model(p130[b, 0]), np.eye(3), np.eye(2), 5)
        eP, eK = np.max(np.abs(c.P[b] - Pn)), np.max(np.abs(c.K[b] - Kn))
        worst = max(worst, eP / lr.bound(Pn), eK / lr.bound(Kn))
        assert eP <= lr.bound(Pn) and eK <= lr.bound(Kn), b
    print(f"worst error / bound: {worst:.2e}")
    np.testing.assert_allclose(u, -np.einsum('bij,bj->bi', c.K, X), rtol=1e-13, atol=1e-14)


def test_batch_stationary_against_scipy(p130, stationary130):
    s = stationary130
    assert np.all(s['status'] == 0) and np.all((s['iterations'] >= 4) & (s['iterations'] <= 14))
    worst = 0.
    for b in range(B130):
        Ks, Ps = lr.scipy_dare(*lr.lqr_model(p130[b, 0]), np.eye(3), np.eye(2))
        eP, eK = np.max(np.abs(s['P'][b] - Ps)), np.max(np.abs(s['K'][b] - Ks))
        worst = max(worst, eP / lr.bound(Ps), eK / lr.bound(Ks))
        assert eP <= lr.bound(Ps) and eK <= lr.bound(Ks), b
    print(f"worst error / bound: {worst:.2e}")
    np.testing.assert_allclose(s['u'], -np.einsum('bij,bj->bi', s['K'], s['X']), rtol=1e-13, atol=1e-14)


def test_failed_instances_do_not_disturb_their_neighbours(p130, stationary130):
    """Every fifth parameter 0: that instance cannot be stabilised (an ordinary input that the algorithm reports); its rows are NaN
    with a non-zero status, and every other row is bit for bit what the healthy batch gave."""
    p = p130.copy()
    p[::5] = 0.
    c = _controller(lr.reference_model(), None)
    with pytest.warns(RuntimeWarning, match=f"{len(p[::5])} of {B130} instance"):
        u = c.call(x=stationary130['X'], p=p)
    bad = np.zeros(B130, dtype=bool)
    bad[::5] = True
    assert np.all(c.status[bad] != 0) and np.all(np.isin(c.status[bad], (1, 2))) and np.all(c.status[~bad] == 0)
    assert np.all(np.isnan(c.K[bad])) and np.all(np.isnan(c.P[bad])) and np.all(np.isnan(u[bad]))
    np.testing.assert_array_equal(c.K[~bad], stationary130['K'][~bad])
    np.testing.assert_array_equal(c.P[~bad], stationary130['P'][~bad])
    np.testing.assert_array_equal(u[~bad], stationary130['u'][~bad])
    np.testing.assert_array_equal(c.iterations[~bad], stationary130['iterations'][~bad])


def _jacobian_check(m, X, U, P):
    """device Jacobians at the rows of (X, U, P) against system_matrices of the linearised copy, one call per point"""
    A, B, Cm = m.linearization(x=X, u=U, p=P)
    ml = m.linearize()
    worst = 0.
    for b in range(X.shape[0]):
        ml.set_equilibrium_point(x_eq=X[b], u_eq=U[b])
        As, Bs, Cs = ml.system_matrices(p=None if P is None else P[b])
        for got, ref in ((A[b], As), (B[b], Bs), (Cm[b], Cs)):
            tol = 1e-11 * max(1., np.max(np.abs(ref)))
            worst = max(worst, np.max(np.abs(got - ref)) / tol)
            assert np.max(np.abs(got - ref)) <= tol, b
    print(f"worst error / bound: {worst:.2e}")
    return A, B


def test_linearization_of_the_bicycle_at_67_operating_points():
    rng = np.random.default_rng(67)
    X = np.column_stack([rng.uniform(-2, 2, 67), rng.uniform(-2, 2, 67), rng.uniform(1, 3, 67), rng.uniform(-1, 1, 67)])
    U = np.column_stack([rng.uniform(-1, 1, 67), rng.uniform(-.4, .4, 67)])
    P = np.column_stack([rng.uniform(1.2, 1.6, 67), rng.uniform(1.6, 2., 67)])
    _jacobian_check(lr.bicycle(), X, U, P)


def test_linearization_of_the_pendulum_at_67_operating_points():
    from hilo_mpc_amd import Model
    rng = np.random.default_rng(68)
    X = rng.uniform(-1, 1, (67, 4))
    U = rng.uniform(-5, 5, (67, 1))
    A, B = _jacobian_check(lr.pendulum(), X, U, None)
    # the precompiled functor of the zoo (no expressions: no system_matrices) gives the same matrices
    Az, Bz, Cz = Model('pendulum4').discretize('rk4').setup(dt=.1).linearization(x=X, u=U)
    np.testing.assert_allclose(Az, A, rtol=0, atol=1e-11 * max(1., np.max(np.abs(A))))
    np.testing.assert_allclose(Bz, B, rtol=0, atol=1e-11)
    np.testing.assert_array_equal(Cz, np.tile(np.eye(4), (67, 1, 1)))


def _lqr_gain(A, B, Q, R, horizon):
    """hilo_lqr_gain called directly: per-instance A, B (strides n n, n m), shared Q, R"""
    from hilo_mpc_amd import _lib
    from hilo_mpc_amd._device import ptr
    n_b, n, m = B.shape
    dev = torch.device('cuda', torch.cuda.current_device())
    At, Bt = torch.as_tensor(A, device=dev).contiguous(), torch.as_tensor(B, device=dev).contiguous()
    Qt, Rt = torch.as_tensor(Q, device=dev).contiguous(), torch.as_tensor(R, device=dev).contiguous()
    K = torch.empty(n_b, m, n, dtype=torch.float64, device=dev)
    P = torch.empty(n_b, n, n, dtype=torch.float64, device=dev)
    st = torch.empty(n_b, 2, dtype=torch.int32, device=dev)
    o = _lib.LqrOpts()
    o.horizon = horizon
    _lib.check(_lib.lib().hilo_lqr_gain(n, m, n_b, ptr(At), n * n, ptr(Bt), n * m, ptr(Qt), 0, ptr(Rt), 0, None, 0, C.byref(o), ptr(K), ptr(P),
                                        ptr(st), torch.cuda.current_stream().cuda_stream))
    return K.cpu().numpy(), P.cpu().numpy(), st.cpu().numpy()


def test_gain_scheduling_equals_linearization_then_gain_then_feedback():
    m = lr.bicycle()
    rng = np.random.default_rng(69)
    nb = 70
    Xe = np.column_stack([rng.uniform(-2, 2, nb), rng.uniform(-2, 2, nb), rng.uniform(1, 3, nb), rng.uniform(-.5, .5, nb)])
    Ue = np.column_stack([np.zeros(nb), rng.uniform(-.2, .2, nb)])
    X = Xe + .1 * rng.standard_normal((nb, 4))
    p = [1.4, 1.8]
    c = _controller(m.linearize(), None, R=[1., 10.])
    u = c.call(x=X, p=p, x_eq=Xe, u_eq=Ue)
    assert np.all(c.status == 0) and c.K.shape == (nb, 2, 4)
    A, Bm, _ = m.linearization(x=Xe, u=Ue, p=p)
    K, P, st = _lqr_gain(A, Bm, np.eye(4), np.diag([1., 10.]), 0)
    assert np.all(st[:, 0] == 0)
    np.testing.assert_array_equal(st[:, 1], c.iterations)
    # the same Jacobians (the same statements in another kernel: rounding of a different contraction at most) and the same solver
    for b in range(nb):
        assert np.max(np.abs(c.K[b] - K[b])) <= lr.bound(K[b]) and np.max(np.abs(c.P[b] - P[b])) <= lr.bound(P[b]), b
    ref = Ue - np.einsum('bij,bj->bi', K, X - Xe)
    np.testing.assert_allclose(u, ref, rtol=0, atol=1e-10 * max(1., np.max(np.abs(K))) * np.max(np.abs(X - Xe)))
    # and against scipy on the device Jacobians
    for b in range(0, nb, 7):
        Ks, Ps = lr.scipy_dare(A[b], Bm[b], np.eye(4), np.diag([1., 10.]))
        assert np.max(np.abs(c.K[b] - Ks)) <= lr.bound(Ks) and np.max(np.abs(c.P[b] - Ps)) <= lr.bound(Ps), b


@pytest.mark.parametrize('name', ['cart_pendulum_0.1', 'cart_pendulum_0.01'])
def test_large_riccati_solutions_against_scipy(name):
    """The two cases with max|P| = 3e4 / 2.9e5, where the host-compiled header is 2.4e-12 / 9.9e-12 max|P| from scipy: the device's
    distance under the same bound, for 66 copies of the instance (every lane of a wave and two of the next give the same bits)."""
    A, B, Q, R, _ = lr.cases()[name]
    K, P, st = _lqr_gain(np.tile(A, (66, 1, 1)), np.tile(B, (66, 1, 1)), Q, R, 0)
    Ks, Ps = lr.scipy_dare(A, B, Q, R)
    eP, eK = np.max(np.abs(P[0] - Ps)), np.max(np.abs(K[0] - Ks))
    print(f"{name}: {st[0, 1]} steps, |P - scipy| / max|P| {eP / np.max(np.abs(Ps)):.2e}, |K - scipy| / max|K| {eK / np.max(np.abs(Ks)):.2e}")
    assert np.all(st[:, 0] == 0) and eP <= lr.bound(Ps) and eK <= lr.bound(Ks)
    assert np.all(P == P[0]) and np.all(K == K[0]) and np.all(st[:, 1] == st[0, 1])


@pytest.mark.parametrize('name', sorted(lr.wide_cases()))
def test_more_inputs_than_states(name):
    A, B = lr.wide_cases()[name]
    n, m = B.shape
    scale = np.linspace(.5, 1.5, 65)[:, None, None]                 # 65 different plants: a wave and a lane
    Ab, Bb = np.tile(A, (65, 1, 1)), scale * B
    for horizon in (3, 0):
        K, P, st = _lqr_gain(Ab, Bb, np.eye(n), np.eye(m), horizon)
        assert np.all(st[:, 0] == 0)
        for b in (0, 31, 64):
            Kr, Pr = lr.riccati_finite(A, Bb[b], np.eye(n), np.eye(m), horizon) if horizon else lr.scipy_dare(A, Bb[b], np.eye(n), np.eye(m))
            assert np.max(np.abs(P[b] - Pr)) <= lr.bound(Pr) and np.max(np.abs(K[b] - Kr)) <= lr.bound(Kr), (horizon, b)


def test_lti_model_with_set_points_per_instance():
    from hilo_mpc_amd import Model
    A, B, Q, R, _ = lr.cases()['random_6x2']
    rng = np.random.default_rng(71)
    X, Xe, Ue = rng.standard_normal((70, 6)), rng.standard_normal((70, 6)), rng.standard_normal((70, 2))
    c = _controller(Model('lti', A=A, B=B).setup(dt=1.), None)
    u = c.call(x=X, x_eq=Xe, u_eq=Ue)
    Ks, _ = lr.scipy_dare(A, B, Q, R)
    assert c.K.shape == (2, 6) and c.status == 0 and np.max(np.abs(c.K - Ks)) <= lr.bound(Ks)
    np.testing.assert_allclose(u, Ue - (X - Xe) @ c.K.T, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize('case', ['double_integrator_0.05', 'random_6x2'])
def test_lti_models_of_any_admitted_size(case):
    from hilo_mpc_amd import Model
    A, B, Q, R, _ = lr.cases()[case]
    X = np.random.default_rng(70).standard_normal((9, A.shape[0]))
    c = _controller(Model('lti', A=A, B=B).setup(dt=1.), None)
    u = c.call(x=X)
    Ks, Ps = lr.scipy_dare(A, B, Q, R)
    assert c.status == 0 and np.max(np.abs(c.K - Ks)) <= lr.bound(Ks) and np.max(np.abs(c.P - Ps)) <= lr.bound(Ps)
    np.testing.assert_allclose(u, -X @ c.K.T, rtol=1e-13, atol=1e-14)
    c.horizon = 20
    c.call(x=X)
    Kn, Pn = lr.riccati_finite(A, B, Q, R, 20)
    assert c.iterations == 20 and np.max(np.abs(c.K - Kn)) <= lr.bound(Kn) and np.max(np.abs(c.P - Pn)) <= lr.bound(Pn)


def test_widest_admitted_size_and_one_state_more():
    from hilo_mpc_amd import Model, _lib
    A, B, Q, R, _ = lr.cases()['random_8x4']                       # HILO_LQR_MAX_NX x HILO_LQR_MAX_NU
    c = _controller(Model('lti', A=A, B=B).setup(dt=1.), None)
    c.call(x=np.ones(8))
    Ks, Ps = lr.scipy_dare(A, B, Q, R)
    assert c.status == 0 and np.max(np.abs(c.K - Ks)) <= lr.bound(Ks) and np.max(np.abs(c.P - Ps)) <= lr.bound(Ps)
    A9 = np.eye(9) * .9
    c = _controller(Model('lti', A=A9, B=np.ones((9, 1))).setup(dt=1.), None)
    with pytest.raises(_lib.HiloError, match=r"8 states.*got 9 and 1") as e:
        c.call(x=np.ones(9))
    assert e.value.code == -4                                       # HILO_ENOTSUP


def test_a_continuous_handle_is_refused():
    from hilo_mpc_amd import Model, _lib
    from hilo_mpc_amd._device import ptr
    m = Model('pendulum4').setup(dt=.1)                            # not discretised
    h = m._plant_handle()
    z = torch.zeros(1, 16, dtype=torch.float64, device=h._dev)
    rc = _lib.lib().hilo_model_linearize(h._handle, 1, ptr(z), ptr(z), 1, ptr(z), ptr(z), None, None)
    assert rc == -4 and b'discretize' in _lib.lib().hilo_last_error()


def test_closed_loop_on_the_cart_pendulum():
    """Stationary gain at the upright origin (Q = I, R = .1; spectral radius of the closed loop .944), 200 steps of the NONLINEAR plant
    from theta0 = .2 and .5: |x| ends at 4.5e-5 and 1.3e-4 (in open loop it exceeds 3 after 30 steps)."""
    from hilo_mpc_amd import SimpleControlLoop
    plant = lr.pendulum()
    c = _controller(plant.linearize(), None, R=[.1])
    X0 = np.zeros((64, 4))
    X0[0::2, 2], X0[1::2, 2] = .2, .5
    sol = SimpleControlLoop(plant, c).run(200, X0)
    np.testing.assert_allclose(c.K.ravel(), lr.PENDULUM_GAIN, rtol=2e-6)      # (the figures are printed to 6 digits)
    A, B, _ = plant.linearization()
    assert abs(np.max(np.abs(np.linalg.eigvals(A - B @ c.K))) - .944) < 1e-3
    end = np.linalg.norm(sol['x'][-1], axis=1)
    print(f"|x_200|: {end[0]:.2e} (theta0 = .2), {end[1]:.2e} (theta0 = .5)")
    assert sol['x'].shape == (201, 64, 4) and np.all(end < 1e-3)
    open_loop = plant.rollout(X0[:2], np.zeros((1, 1)), steps=30)[0]
    assert np.all(np.linalg.norm(open_loop[-1], axis=1) > 3.)


def test_device_tensors_stay_on_the_device_and_the_gain_is_cached(p130):
    c = _controller(lr.reference_model(), None)
    dev = torch.device('cuda', torch.cuda.current_device())
    X = torch.randn(B130, 3, dtype=torch.float64, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    pt = torch.as_tensor(p130, device=dev)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        u = c.call(x=X, p=pt)
    assert isinstance(u, torch.Tensor) and u.device == X.device and u.shape == (B130, 2)
    assert isinstance(c.K, torch.Tensor) and c.K.device == X.device and isinstance(c.P, torch.Tensor) and isinstance(c.status, torch.Tensor)
    torch.testing.assert_close(u, -torch.einsum('bij,bj->bi', c.K, X), rtol=1e-13, atol=1e-14)
    # a second call with the same p launches the apply alone: the status buffer of a solve stays unwritten
    K0 = c.K.clone()
    c._stats.fill_(-7)
    u2 = c.call(x=2. * X, p=pt)
    torch.cuda.synchronize()
    assert torch.all(c._stats == -7) and torch.equal(c.K, K0)
    torch.testing.assert_close(u2, 2. * u, rtol=1e-13, atol=1e-14)
    pt[0, 0] = 1.                                                   # written in place: solved again
    c.call(x=X, p=pt)
    torch.cuda.synchronize()
    assert torch.all(c._stats[:, 0] == 0)
