"""The 50-digit truth of tests/kf_reference.py: pinned to the reference's own known answers (the ones tests/test_oracle_kf.py quotes
from the reference's tests/test_KFs.py), then used to measure oracle/kf.py on every case of tests/test_kf_shapes_gpu.py.  That
oracle-vs-truth error per case is what the GPU tolerances are derived from (kf_reference.bound); it is printed (`pytest -s`).
No GPU.  Run time of this file: about 45 s on one core (the truth sets: 16 instances x 3 steps per case)."""
import numpy as np
import pytest

from oracle import models
from tests import kf_reference as ref, kf_shape_cases as S

P_BIO = S.P_BIO


def _f(a):
    return ref.to_float(a)


def _lin():
    return ref.TruthModel(models.get('linear2'), order=1)       # test_KFs.py:254 `discretize('erk', order=1)`


def test_kf_kats():
    tm = _lin()
    x, P = ref.ekf_predict(tm, [.8, 0.], [[1., 0.], [0., 1.]], [.8], [.5, .4], .01 * np.eye(2), 1.)          # test_KFs.py:488-503
    np.testing.assert_allclose(np.column_stack([_f(x), _f(P)]), [[1.2, .26, .25], [.4, .25, .62]], rtol=1e-15)
    x, P, yp = ref.ekf_update(tm, [1.2, .4], [[.26, .25], [.25, .62]], [.322052], [.8], [.5, .4], [[.064]], 1.)   # :505-522
    np.testing.assert_allclose(np.column_stack([_f(x), _f(P)]), [[1.17151023, .16862573, .023391813], [.32934538, .023391813, .0580117]],
                               rtol=1e-7)
    np.testing.assert_allclose(_f(yp), [.4], rtol=1e-15)
    x, _, _ = ref.ekf_step(tm, [.8, 0.], np.eye(2), [.3894626], [.8], [.5, .4], np.diag([.01, .01]), [[.064]], 1.)   # :298-316
    np.testing.assert_allclose(_f(x), [1.19614861, .39044856], rtol=1e-7)
    # the same step from the matrices: the plain LTI variant (Euler map of the chain: A = I + dt A_c)
    A, Bm, C = np.array([[.5, 0.], [.5, .6]]), np.array([[1.], [0.]]), np.array([[0., 1.]])
    xl, Pl, _ = ref.lti_step(A, Bm, C, [.8, 0.], np.eye(2), [.3894626], [.8], np.diag([.01, .01]), [[.064]])
    np.testing.assert_allclose(_f(xl), _f(x), rtol=1e-15)


def test_ekf_and_ukf_one_step_kats():
    tm = ref.TruthModel(models.get('toy1d'))
    x, _, _ = ref.ekf_step(tm, [9.], [[1.]], [2.59109], [], [], [[10.]], [[1.]], 1.)                          # test_KFs.py:548-566
    np.testing.assert_allclose(_f(x), [7.206059], rtol=1e-7)
    x, _, _ = ref.ukf_step(tm, [9.], [[1.]], [2.59109], [], [], [[10.]], [[1.]], 1.)                          # :606-624
    np.testing.assert_allclose(_f(x), [7.2739647], rtol=1e-7)


def test_ukf_sigma_point_tile_kats():
    """test_KFs.py:716-756 (alpha = 1, continuous model, dt = .1; the reference prints six digits and tests with atol 1e-3).  The truth
    propagates the points with classic RK4 in eight steps, like the product; the reference with CVODES."""
    tm = ref.TruthModel(models.get('bioreactor3'))
    x, P, X = ref.ukf_predict(tm, [299.876, .217108, 20.], np.eye(3), [.01], P_BIO, np.zeros((3, 3)), .1, alpha=1., continuous=True, n_sub=8)
    want = np.array([[299.925, 0.970453, 1.08254e-06, -2.11206e-05, 299.925, 301.631, 299.925, 299.925, 298.218, 299.925, 299.925],
                     [0.219433, 1.08254e-06, 1.02165, -0.0848792, 0.219446, 0.219451, 1.97011, 0.219537, 0.21944, -1.53128, 0.219345],
                     [19.9619, -2.11206e-05, -0.0848792, 1.00427, 19.9618, 19.9617, 19.8164, 21.6914, 19.9618, 20.1075, 18.2322]])
    np.testing.assert_allclose(np.column_stack([_f(x), _f(P), _f(X)]), want, atol=1e-3)
    P = np.array([[.970453, 1.08254e-06, -2.11206e-05], [1.08254e-06, 1.02165, -.0848792], [-2.11206e-05, -.0848792, 1.00427]])
    x, Pu, yp = ref.ukf_update(tm, [299.925, .219433, 19.9619], P, want[:, 4:], [300.941, .245805], [.01], P_BIO, np.diag([.25, .01]), .1,
                               alpha=1.)
    np.testing.assert_allclose(np.column_stack([_f(x), _f(Pu)]), [[300.733, 0.198539, -2.03814e-06, 1.56415e-06],
                                                                 [0.245549, -2.03814e-06, 0.00990874, -0.000819447],
                                                                 [19.9597, 1.56415e-06, -0.000819447, 0.997286]], atol=1e-3)
    np.testing.assert_allclose(_f(yp), [299.925, .219434], atol=1e-3)


def test_family_models_agree_between_product_expressions_and_oracle():
    """One definition, two symbol types: the product's expression tree evaluates to the oracle model's numbers."""
    import math
    for n_x, n_y, discrete in S.FAMILY.values():
        m = ref.family_product(n_x, n_y, discrete)
        assert (m.n_x, m.n_u, m.n_p, m.n_y) == (n_x, 1, 1, n_y) and not m.is_linear()
        om = ref.family_oracle(n_x, n_y, discrete)
        x0, u0, p0 = ref.family_point(n_x)
        f, h = ref.family_equations(list(x0), list(u0), list(p0), n_y, math.sin, discrete)
        np.testing.assert_allclose(om.f(x0, u0, p0, .1)[0], f, rtol=1e-14)
        np.testing.assert_allclose(om.h(x0, u0, p0, .1)[0], h, rtol=1e-14)
        F = om.fx(x0, u0, p0, .1)[0]
        assert np.all(F != 0) or n_x == 1
        assert len({tuple(r) for r in np.round(F, 12)}) == n_x and (n_x == 1 or not np.allclose(F, F.T))


@pytest.mark.parametrize('cid', S.MATRIX + list(S.ERK) + S.CONT)
def test_oracle_against_the_truth(cid):
    """oracle/kf.py on the inputs of the GPU tests (16 instances, 3 chained steps, Q and R per instance) against the truth.  The
    figures are the yardstick of the GPU tests; asserted here is only that the yardstick is rounding-limited and not degenerate:
    eps times the amplification of the chained problem.  Three steps through maps with |F| up to ~3 and the cancellation in
    P- - K Pyy K^T amplify a rounding error by up to 10^2 .. 10^3 (the scalar toy map is the worst: 6e-14 on P): 1e-12 for the
    EKF / KF and the UKF with alpha = 1.  With alpha = 1e-3 the weights 1 / (2 (n + lambda)), n + lambda = 1e-6 n, start from a
    relative rounding error of eps / 1e-6 = 2e-10: 1e-7 with the same amplification."""
    c = S.case(cid)
    d = c.data()
    args = (d['x'][S.TI], d['P'][S.TI], d['ys'][:, S.TI], d['us'][:, S.TI], d['p'][S.TI], d['Q'][S.TI], d['R'][S.TI])
    for kind in c.kinds:
        orc = S.oracle_steps(c, kind, *args, S.K)
        tru = S.truth(cid, kind, 'per')
        e = [ref.rel_err(o.reshape((-1,) + o.shape[2:]), t.reshape((-1,) + t.shape[2:])) for o, t in zip(orc, tru)]
        print(f'oracle vs truth  {cid:16s} {kind:8s} x {e[0]:.2e}  P {e[1]:.2e}  y {e[2]:.2e}')
        assert max(e) < (1e-7 if kind == 'ukf1e-3' else 1e-12), (cid, kind, e)
