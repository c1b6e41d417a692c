"""CPU: host-side contract of `LQR` (hilo_mpc_amd/lqr.py), `Model.linearization` and the `call` branch of `SimpleControlLoop`,
against a stand-in for the library that READS its pointer arguments the way include/hilo_hip.h declares them and answers with the
numpy references of tests/lqr_reference.py - messages, argument order, strides, shapes, the gain cache and the return types
without a GPU, in the manner of tests/test_rollout_host.py."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

from hilo_mpc_amd import LQR, LinearQuadraticRegulator, Model, SimpleControlLoop, _lib
from tests import lqr_reference as lr


def _arr(ptr, n, typ=C.c_double):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(typ)), shape=(n,))


def _reference_model(dt=1.):
    """tests/test_LQR.py:245-251 as expressions, the first input scaled by a parameter"""
    m = Model(discrete=True)
    x = m.set_dynamical_states(['x', 'y', 'z'])
    u = m.set_inputs(['u', 'w'])
    p = m.set_parameters(['p'])
    m.set_dynamical_equations([x[0] + dt * (2. * x[1] + p[0] * u[0]), x[1] - dt * x[0], x[2] + dt * u[1]])
    return m.setup(dt=dt)


def _stub(monkeypatch, log, fail=()):
    """The stand-in: hilo_lqr_call answers for the reference model (its A, B from the parameter row it is handed)."""
    class H:
        _dev, _handle, _n_p, _n_y = torch.device('cpu'), 4321, 1, 3
    monkeypatch.setattr(Model, '_linearization_handle', lambda self, device_index=None: H)
    monkeypatch.setattr('hilo_mpc_amd.lqr.stream_ptr', lambda dev: 0)
    monkeypatch.setattr('hilo_mpc_amd._device.stream_ptr', lambda dev: 0)
    monkeypatch.setattr('hilo_mpc_amd._device.device', lambda index=None: torch.device('cpu'))
    nx, nu = 3, 2

    def solve(A, B, Q, R, horizon):
        if horizon:
            return lr.riccati_finite(A, B, Q, R, horizon) + (0, horizon)
        return lr.dare_doubling(A, B, Q, R)

    class Lib:
        @staticmethod
        def hilo_lqr_call(h, opts, B, x, x_eq, u_eq, p, ps, Q, R, N, K, P, u, stats, stream):
            o = opts._obj
            log.append(dict(fn='call', h=h, B=B, ps=ps, x=x is not None, x_eq=x_eq is not None, u_eq=u_eq is not None, N=N, u=u is not None,
                            horizon=o.horizon, max_iter=o.max_iter, tol=o.tol))
            Qm, Rm = _arr(Q, nx * nx).reshape(nx, nx), _arr(R, nu * nu).reshape(nu, nu)
            prow = _arr(p, (B - 1) * ps + 1)
            Ko, Po, so = _arr(K, B * nu * nx).reshape(B, nu, nx), _arr(P, B * nx * nx).reshape(B, nx, nx), _arr(stats, B * 2, C.c_int32).reshape(B, 2)
            xe = _arr(x_eq, B * nx).reshape(B, nx) if x_eq is not None else np.zeros((B, nx))
            ue = _arr(u_eq, B * nu).reshape(B, nu) if u_eq is not None else np.zeros((B, nu))
            log[-1]['p'] = np.array([prow[b * ps] for b in range(B)])
            log[-1]['x_eq_rows'] = xe.copy()
            for b in range(B):
                A, Bm = lr.lqr_model(prow[b * ps])
                Ko[b], Po[b], so[b, 0], so[b, 1] = solve(A, Bm, Qm, Rm, o.horizon)
                if b in fail:
                    Ko[b], Po[b], so[b, 0] = np.nan, np.nan, 2
            if x is not None:
                xv = _arr(x, B * nx).reshape(B, nx)
                _arr(u, B * nu).reshape(B, nu)[:] = ue - np.einsum('bij,bj->bi', Ko, xv - xe)
            return 0

        @staticmethod
        def hilo_lqr_apply(n, m, B, K, ks, x, x_eq, u_eq, u, stream):
            log.append(dict(fn='apply', n=n, m=m, B=B, ks=ks, x_eq=x_eq is not None, u_eq=u_eq is not None))
            Kr = _arr(K, (B - 1) * ks + n * m)
            xv = _arr(x, B * n).reshape(B, n)
            xe = _arr(x_eq, B * n).reshape(B, n) if x_eq is not None else np.zeros((B, n))
            ue = _arr(u_eq, B * m).reshape(B, m) if u_eq is not None else np.zeros((B, m))
            uo = _arr(u, B * m).reshape(B, m)
            for b in range(B):
                uo[b] = ue[b] - Kr[b * ks:b * ks + n * m].reshape(m, n) @ (xv[b] - xe[b])
            return 0

        @staticmethod
        def hilo_lqr_gain(n, m, B, A, as_, Bm, bs, Q, qs, R, rs, N, ns, opts, K, P, stats, stream):
            o = opts._obj
            log.append(dict(fn='gain', n=n, m=m, B=B, strides=(as_, bs, qs, rs, ns), N=N, horizon=o.horizon))
            Am, Bv = _arr(A, n * n).reshape(n, n), _arr(Bm, n * m).reshape(n, m)
            Qm, Rm = _arr(Q, n * n).reshape(n, n), _arr(R, m * m).reshape(m, m)
            k, pm, st, it = solve(Am, Bv, Qm, Rm, o.horizon)
            _arr(K, m * n)[:] = k.ravel()
            _arr(P, n * n)[:] = pm.ravel()
            _arr(stats, 2, C.c_int32)[:] = [st, it]
            return 0

        @staticmethod
        def hilo_model_linearize(h, B, x, up, us, A, Bm, Cm, stream):
            log.append(dict(fn='linearize', h=h, B=B, us=us, x=_arr(x, B * nx).reshape(B, nx).copy(), up=_arr(up, B * us).reshape(B, us).copy()))
            for b in range(B):
                a, bb = lr.lqr_model(_arr(up, B * us).reshape(B, us)[b, nu])
                _arr(A, B * nx * nx).reshape(B, nx, nx)[b] = a
                _arr(Bm, B * nx * nu).reshape(B, nx, nu)[b] = bb
                _arr(Cm, B * 3 * nx).reshape(B, 3, nx)[b] = np.eye(3)
            return 0
    monkeypatch.setattr(_lib, 'lib', lambda: Lib)


def _lqr(monkeypatch, log, horizon=5, **kw):
    _stub(monkeypatch, log, **kw)
    c = LQR(_reference_model())
    c.horizon = horizon
    c.setup()
    c.Q, c.R = np.ones(3), np.ones(2)
    return c


# ---- constructor and setters: the reference's messages (lqr.py:60-73, :108-145, :270-285) ------------------------------------------
def test_constructor_checks_in_the_reference_order():
    assert LQR is LinearQuadraticRegulator
    with pytest.raises(TypeError, match="The model must be an object of the Model class."):
        LQR(object())
    m = Model(discrete=True)
    x = m.set_dynamical_states(['a'])
    u = m.set_inputs(['u'])
    m.set_dynamical_equations([x[0] * x[0] + u[0]])
    with pytest.raises(RuntimeError, match=r"Model is not set up. Run Model.setup\(\) before passing it to the controller."):
        LQR(m)
    m.setup(dt=1.)
    with pytest.raises(RuntimeError, match=r"needs to be linear. Use Model.linearize\(\) to obtain a linearized model."):
        LQR(m)
    LQR(m.linearize())                                              # a linearised copy counts as linear
    cont = Model('linear2').setup(dt=1.)                            # continuous and linear
    with pytest.raises(RuntimeError, match=r"needs to be discrete. Use Model.discretize\(\) to obtain a discrete model."):
        LQR(cont)
    with pytest.raises(RuntimeError, match="The model used for the LQR needs to be continuous."):
        LQR(_reference_model(), discrete=False)
    # not set up comes before continuous / discrete, nonlinear before autonomous
    with pytest.raises(RuntimeError, match="Model is not set up"):
        LQR(Model('linear2'))
    a = Model(discrete=True)
    xa = a.set_dynamical_states(['a'])
    a.set_dynamical_equations([.5 * xa[0]])
    a.setup(dt=1.)
    with pytest.raises(RuntimeError, match="The model used for the LQR is autonomous."):
        LQR(a)
    c = LQR(cont, discrete=False)                                   # passes the constructor ...
    with pytest.raises(NotImplementedError, match="only discrete formulations"):
        c.setup()                                                   # ... and stops here (lqr.py:217)


def test_setters_check_and_convert_like_the_reference(monkeypatch):
    log = []
    c = _lqr(monkeypatch, log)
    assert (c.n_x, c.n_u, c.n_p) == (3, 2, 1) and c.horizon == 5
    np.testing.assert_array_equal(c.N, np.zeros((3, 2)))
    c.Q = [1., 2., 3.]                                              # a vector becomes a diagonal
    np.testing.assert_array_equal(c.Q, np.diag([1., 2., 3.]))
    c.R = np.array([[2., .5], [.5, 1.]])
    np.testing.assert_array_equal(c.R, [[2., .5], [.5, 1.]])
    for name in ('Q', 'R'):
        with pytest.raises(ValueError, match=f"LQR matrix {name} needs to be real-valued"):
            setattr(c, name, np.array([1j, 1., 1.]))
    with pytest.raises(ValueError, match="Dimension mismatch. Supplied dimension is 2x2, but required dimension is 3x3"):
        c.Q = np.eye(2)
    with pytest.raises(ValueError, match="Dimension mismatch. Supplied dimension is 3x3, but required dimension is 2x2"):
        c.R = np.eye(3)
    with pytest.raises(ValueError, match="LQR matrix Q needs to be symmetric"):
        c.Q = np.array([[1., 1., 0.], [0., 1., 0.], [0., 0., 1.]])
    with pytest.raises(ValueError, match="LQR matrix R needs to be symmetric"):
        c.R = np.array([[1., 1.], [0., 1.]])
    with pytest.raises(ValueError, match="LQR matrix Q needs to be positive semidefinite"):
        c.Q = [1., -1., 1.]
    c.Q = [1., 0., 1.]                                              # semidefinite is enough for Q ...
    with pytest.raises(ValueError, match="LQR matrix R needs to be positive definite"):
        c.R = [1., 0.]                                              # ... not for R
    # a failed assignment leaves the old value
    np.testing.assert_array_equal(c.R, [[2., .5], [.5, 1.]])
    # before setup() the dimensions are zero, like the reference's
    c2 = LQR(_reference_model())
    with pytest.raises(ValueError, match="required dimension is 0x0"):
        c2.Q = np.eye(3)


def test_call_errors_and_reset(monkeypatch):
    log = []
    _stub(monkeypatch, log)
    c = LQR(_reference_model())
    c.horizon = 5
    with pytest.raises(RuntimeError, match=r"LQR is not set up. Run LQR.setup\(...\) before calling the LQR."):
        c.call(x=[1., 0., 0.])
    c.setup()
    with pytest.raises(RuntimeError, match="Matrix Q is not set properly."):
        c.call(x=[1., 0., 0.])
    c.Q = np.ones(3)
    with pytest.raises(RuntimeError, match="Matrix R is not set properly."):
        c.call(x=[1., 0., 0.])
    c.R = np.ones(2)
    with pytest.raises(ValueError, match="No state information was supplied to the LQR!"):
        c.call(p=[1.])
    assert c.K is None and c.P is None and c.status is None
    c.call(x=[1., 0., 0.], p=[1.])
    assert c.K is not None
    c.Q = 2. * np.ones(3)                                           # a new Q (or R, or horizon) resets K
    assert c.K is None
    c.call(x=[1., 0., 0.], p=[1.])
    c.R = np.ones(2)
    assert c.K is None
    c.call(x=[1., 0., 0.], p=[1.])
    c.horizon = None
    assert c.K is None and c.horizon is None
    c.call(x=[1., 0., 0.], p=[1.])
    c.setup()                                                       # setup() resets Q, R and K (lqr.py:255-258)
    assert c.Q is None and c.R is None and c.K is None
    with pytest.raises(ValueError, match="Dimension mismatch"):
        c.Q, c.R = np.ones(3), np.ones(2)
        c.call(x=[1., 0.], p=[1.])


# ---- packing, strides, cache, types ---------------------------------------------------------------------------------------
def test_shared_operating_data_one_gain_then_apply(monkeypatch):
    log = []
    c = _lqr(monkeypatch, log)
    K5, P5 = lr.riccati_finite(*lr.lqr_model(1.), np.eye(3), np.eye(2), 5)
    u = c.call(x=[1., 0., 1.], p=[1.])                              # one state, no batch axis anywhere
    assert isinstance(u, np.ndarray) and u.shape == (2,)
    np.testing.assert_allclose(u, -K5 @ [1., 0., 1.], rtol=1e-14)
    # B = 1 = the operating points: ONE launch does it all
    assert [e['fn'] for e in log] == ['call'] and log[0]['x'] and log[0]['u']
    assert (log[0]['h'], log[0]['B'], log[0]['ps'], log[0]['N'], log[0]['horizon'], log[0]['max_iter'], log[0]['tol']) == \
        (4321, 1, 0, None, 5, 50, 1e-12)
    assert c.K.shape == (2, 3) and c.P.shape == (3, 3) and isinstance(c.K, np.ndarray)
    np.testing.assert_allclose(c.K, K5, rtol=1e-14)
    np.testing.assert_allclose(c.feedback_gain, K5, rtol=1e-14)
    np.testing.assert_allclose(c.P, P5, rtol=1e-14)
    assert c.status == 0 and c.iterations == 5
    # a batch of states with the same shared parameter: the gain is kept, only the apply runs, with k_stride 0
    del log[:]
    X = np.random.default_rng(0).standard_normal((7, 3))
    u = c.call(x=X, p=[1.])
    assert u.shape == (7, 2)
    np.testing.assert_allclose(u, -X @ K5.T, rtol=1e-13, atol=1e-15)
    assert log == [dict(fn='apply', n=3, m=2, B=7, ks=0, x_eq=False, u_eq=False)]
    # other values: the gain for the ONE operating point alone (batch 1, no x), then the apply
    del log[:]
    u = c.call(x=X, p=[2.])
    K2, _ = lr.riccati_finite(*lr.lqr_model(2.), np.eye(3), np.eye(2), 5)
    np.testing.assert_allclose(u, -X @ K2.T, rtol=1e-13, atol=1e-15)
    assert [e['fn'] for e in log] == ['call', 'apply'] and (log[0]['B'], log[0]['x'], log[0]['u'], log[0]['ps']) == (1, False, False, 0)
    assert log[1]['ks'] == 0 and log[1]['B'] == 7
    # a missing p means zeros (lqr.py:291)
    del log[:]
    c.call(x=X)
    assert log[0]['fn'] == 'call' and log[0]['p'][0] == 0.


def test_per_instance_parameters_one_fused_call(monkeypatch):
    log = []
    c = _lqr(monkeypatch, log, horizon=None)
    rng = np.random.default_rng(1)
    B = 6
    X, Pp = rng.standard_normal((B, 3)), rng.uniform(.5, 2., (B, 1))
    u = c.call(x=X, p=Pp)
    assert [e['fn'] for e in log] == ['call']
    e = log[0]
    assert (e['B'], e['ps'], e['x'], e['u'], e['x_eq'], e['u_eq'], e['horizon']) == (B, 1, True, True, False, False, 0)
    np.testing.assert_array_equal(e['p'], Pp[:, 0])
    assert c.K.shape == (B, 2, 3) and c.P.shape == (B, 3, 3) and c.status.shape == (B,) and c.iterations.shape == (B,)
    for b in range(B):
        Ks, Ps = lr.scipy_dare(*lr.lqr_model(Pp[b, 0]), np.eye(3), np.eye(2))
        np.testing.assert_allclose(c.K[b], Ks, atol=lr.bound(Ks), rtol=0)
        np.testing.assert_allclose(u[b], -Ks @ X[b], atol=1e-9, rtol=0)
    # the same object and values again: the apply alone, per-instance gains (k_stride = n_u n_x)
    del log[:]
    c.call(x=X + 1., p=Pp)
    assert log == [dict(fn='apply', n=3, m=2, B=B, ks=6, x_eq=False, u_eq=False)]
    # equal values in another array are the same operating data; changed values are not
    del log[:]
    c.call(x=X, p=Pp.copy())
    assert [e['fn'] for e in log] == ['apply']
    Pp[2, 0] = 1.7
    c.call(x=X, p=Pp)
    assert [e['fn'] for e in log] == ['apply', 'call']
    # one state against B operating points: broadcast
    del log[:]
    u1 = c.call(x=X[0], p=Pp)
    assert u1.shape == (B, 2) and [e['fn'] for e in log] == ['apply'] and log[0]['B'] == B
    with pytest.raises(ValueError, match="does not match"):
        c.call(x=X[:4], p=Pp)
    with pytest.raises(ValueError, match="Dimension mismatch"):
        c.call(x=X, p=np.ones((B, 2)))


def test_operating_points_per_instance(monkeypatch):
    log = []
    c = _lqr(monkeypatch, log)
    rng = np.random.default_rng(2)
    B = 5
    X, Xe, Ue = rng.standard_normal((B, 3)), rng.standard_normal((B, 3)), rng.standard_normal((B, 2))
    u = c.call(x=X, p=[1.], x_eq=Xe, u_eq=Ue)
    K5, _ = lr.riccati_finite(*lr.lqr_model(1.), np.eye(3), np.eye(2), 5)
    e = log[0]
    assert [q['fn'] for q in log] == ['call'] and (e['B'], e['ps'], e['x_eq'], e['u_eq']) == (B, 0, True, True)
    np.testing.assert_array_equal(e['x_eq_rows'], Xe)
    np.testing.assert_allclose(u, Ue - (X - Xe) @ K5.T, rtol=1e-13, atol=1e-14)
    assert c.K.shape == (B, 2, 3)                                   # operating data with a batch axis: a gain per instance
    del log[:]
    u = c.call(x=2. * X, p=[1.], x_eq=Xe, u_eq=Ue)                  # cached: the apply with the offsets
    assert log == [dict(fn='apply', n=3, m=2, B=B, ks=6, x_eq=True, u_eq=True)]
    np.testing.assert_allclose(u, Ue - (2. * X - Xe) @ K5.T, rtol=1e-13, atol=1e-14)
    # the model's own equilibrium point: the Jacobians there, the feedback u = -K x
    del log[:]
    c.call(x=X, p=[1.])
    del log[:]
    c._model.set_equilibrium_point(x_eq=[.1, .2, .3], u_eq=[0., 1.])      # part of the operating data: the gain is solved again
    u = c.call(x=X, p=[1.])
    assert [q['fn'] for q in log] == ['call', 'apply'] and log[0]['x_eq'] and log[0]['u_eq'] and not log[0]['x'] and log[0]['B'] == 1
    np.testing.assert_array_equal(log[0]['x_eq_rows'], [[.1, .2, .3]])
    assert log[1] == dict(fn='apply', n=3, m=2, B=B, ks=0, x_eq=False, u_eq=False)
    np.testing.assert_allclose(u, -X @ K5.T, rtol=1e-13, atol=1e-14)


def test_tensors_in_tensors_out_and_their_cache(monkeypatch):
    log = []
    c = _lqr(monkeypatch, log)
    X, Pp = torch.randn(4, 3, dtype=torch.float64), torch.tensor([[1.], [1.5], [.5], [2.]], dtype=torch.float64)
    u = c.call(x=X, p=Pp)
    assert isinstance(u, torch.Tensor) and u.shape == (4, 2)
    assert isinstance(c.K, torch.Tensor) and c.K.shape == (4, 2, 3) and isinstance(c.P, torch.Tensor) and isinstance(c.status, torch.Tensor)
    del log[:]
    c.call(x=X, p=Pp)                                               # the same tensor object, not written since: cached
    assert [e['fn'] for e in log] == ['apply']
    Pp[1, 0] = 1.25                                                 # written in place: the version counter moves
    c.call(x=X, p=Pp)
    assert [e['fn'] for e in log] == ['apply', 'call'] and log[-1]['p'][1] == 1.25
    c.call(x=X, p=Pp.clone())                                       # another tensor object: solved again (no value comparison on the device)
    assert [e['fn'] for e in log] == ['apply', 'call', 'call']
    un = c.call(x=X.numpy(), p=Pp.numpy())
    assert isinstance(un, np.ndarray) and isinstance(c.K, np.ndarray)


def test_failed_instances_warn(monkeypatch):
    log = []
    c = _lqr(monkeypatch, log, horizon=None, fail=(1,))
    with pytest.warns(RuntimeWarning, match="1 of 3 instance"):
        u = c.call(x=np.ones((3, 3)), p=np.array([[1.], [1.], [2.]]))
    assert np.all(np.isnan(u[1])) and np.all(np.isfinite(u[[0, 2]]))
    np.testing.assert_array_equal(c.status, [0, 2, 0])
    # device tensors: no host copy inside call(); the warning comes when the status (or K, P) is read
    c.Q = np.ones(3)
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        c.call(x=torch.ones(3, 3, dtype=torch.float64), p=torch.tensor([[1.], [1.], [2.]], dtype=torch.float64))
    with pytest.warns(RuntimeWarning, match="status 2"):
        assert c.status.tolist() == [0, 2, 0]


def test_lti_model_goes_through_the_gain_entry(monkeypatch):
    log = []
    _stub(monkeypatch, log)
    A, B = lr.lqr_model(1.)
    c = LQR(Model('lti', A=A, B=B).setup(dt=1.))
    c.horizon = 5
    c.setup()
    c.Q, c.R = np.ones(3), np.ones(2)
    X = np.random.default_rng(3).standard_normal((4, 3))
    u = c.call(x=X)
    K5, _ = lr.riccati_finite(A, B, np.eye(3), np.eye(2), 5)
    np.testing.assert_allclose(u, -X @ K5.T, rtol=1e-13, atol=1e-15)
    assert log[0] == dict(fn='gain', n=3, m=2, B=1, strides=(0, 0, 0, 0, 0), N=None, horizon=5)
    assert log[1] == dict(fn='apply', n=3, m=2, B=4, ks=0, x_eq=False, u_eq=False)
    assert c.K.shape == (2, 3) and c.n_p == 9 + 6 + 9              # (the matrices are the model's parameters; call() needs none)


def test_lti_model_with_set_points_per_instance(monkeypatch):
    """A batch of identical plants with their own set-points: ONE gain (it does not depend on the operating point), applied with
    k_stride 0 and the offsets - no row of K, P or the status is left unwritten (every fresh tensor is poisoned here)."""
    log = []
    _stub(monkeypatch, log)
    real_empty = torch.empty

    def poisoned(*a, **k):
        t = real_empty(*a, **k)
        return t.fill_(777)
    monkeypatch.setattr(torch, 'empty', poisoned)
    A, B = lr.lqr_model(1.)
    c = LQR(Model('lti', A=A, B=B).setup(dt=1.))
    c.horizon = 5
    c.setup()
    c.Q, c.R = np.ones(3), np.ones(2)
    rng = np.random.default_rng(4)
    X, Xe, Ue = rng.standard_normal((4, 3)), rng.standard_normal((4, 3)), rng.standard_normal((4, 2))
    u = c.call(x=X, x_eq=Xe, u_eq=Ue)
    K5, P5 = lr.riccati_finite(A, B, np.eye(3), np.eye(2), 5)
    np.testing.assert_allclose(u, Ue - (X - Xe) @ K5.T, rtol=1e-13, atol=1e-14)
    assert log[0]['fn'] == 'gain' and log[0]['B'] == 1
    assert log[1] == dict(fn='apply', n=3, m=2, B=4, ks=0, x_eq=True, u_eq=True)
    assert c.K.shape == (2, 3) and c.P.shape == (3, 3) and c.status == 0 and c.iterations == 5
    np.testing.assert_allclose(c.K, K5, rtol=1e-14)
    np.testing.assert_allclose(c.P, P5, rtol=1e-14)
    del log[:]
    u = c.call(x=X[0], x_eq=Xe, u_eq=Ue)                             # cached; one state against four set-points
    assert [e['fn'] for e in log] == ['apply'] and log[0]['ks'] == 0 and u.shape == (4, 2)
    np.testing.assert_allclose(u, Ue - (X[0] - Xe) @ K5.T, rtol=1e-13, atol=1e-14)


def test_model_linearization_packs_rows_of_inputs_and_parameters(monkeypatch):
    log = []
    _stub(monkeypatch, log)
    m = _reference_model()
    A, B, Cm = m.linearization(p=[1.5])                              # the origin, no batch axis
    assert A.shape == (3, 3) and B.shape == (3, 2) and Cm.shape == (3, 3) and isinstance(A, np.ndarray)
    np.testing.assert_array_equal(B, lr.lqr_model(1.5)[1])
    assert (log[0]['h'], log[0]['B'], log[0]['us']) == (4321, 1, 3)
    np.testing.assert_array_equal(log[0]['up'], [[0., 0., 1.5]])
    X, Pp = np.arange(12.).reshape(4, 3), np.array([[.5], [1.], [1.5], [2.]])
    A, B, Cm = m.linearization(x=X, u=[.1, .2], p=Pp)
    assert A.shape == (4, 3, 3) and B.shape == (4, 3, 2)
    np.testing.assert_array_equal(log[1]['x'], X)
    np.testing.assert_array_equal(log[1]['up'], np.hstack([np.tile([.1, .2], (4, 1)), Pp]))
    np.testing.assert_array_equal(B[:, 0, 0], Pp[:, 0])
    At, _, _ = m.linearization(x=torch.as_tensor(X), p=torch.as_tensor(Pp))
    assert isinstance(At, torch.Tensor)
    with pytest.raises(ValueError, match="Their values are needed"):
        m.linearization()
    with pytest.raises(ValueError, match="does not match"):
        m.linearization(x=X, p=Pp[:3])
    with pytest.raises(NotImplementedError, match="discretize"):
        Model('linear2').setup(dt=1.).linearization()


# ---- the control loop ---------------------------------------------------------------------------------------------------------
def test_control_loop_accepts_a_controller_that_offers_call(monkeypatch):
    log = []
    c = _lqr(monkeypatch, log, horizon=None)
    A, B = lr.lqr_model(1.)
    loop = SimpleControlLoop(lambda x, u, p: x @ A.T + u @ B.T, c)
    X0 = np.array([[1., 0., 1.], [-.5, .5, 2.]])
    sol = loop.run(30, X0, p=[1.])
    assert sol['x'].shape == (31, 2, 3) and sol['u'].shape == (30, 2, 2)
    assert np.max(np.abs(sol['x'][-1])) < 1e-3 * np.max(np.abs(X0))   # the stationary gain stabilises the loop
    assert [e['fn'] for e in log].count('call') == 1                   # one solve, then 30 applies
    Ks, _ = lr.scipy_dare(A, B, np.eye(3), np.eye(2))
    np.testing.assert_allclose(sol['u'][0], -X0 @ Ks.T, atol=1e-9)

    class Neither:
        pass
    with pytest.raises(TypeError, match=r"the controller must offer optimize\(\) \(NMPC / LMPC\)"):
        SimpleControlLoop(lambda x, u, p: x, Neither())
