"""CPU: the regulator of csrc/hilo_lqr.h compiled for the HOST and run there - the header is `__host__ __device__` up to the kernel
bodies and takes its storage as a view, so the statements the GPU runs (there on lane-strided LDS, here on a plain array) are
checked without one.

A small driver around `lqr_solve` and `lqr_linearize<M>` is built into tmp_path with `hipcc -x hip --cuda-host-only`, the way
tests/test_integrate_host.py builds its own.  Checked: the reference's two known gains (tests/test_pins.py K_P0, K_P1; horizon 5) and
the numpy recursion; the stationary gain on the cases of tests/lqr_reference.py against scipy.linalg.solve_discrete_are under
`1e-10 max(1, max|P|)` (K: max|K|); the Jacobians of Pendulum4 and of an Lti shape against central differences of the same host
code (one pass of all directions, and passes of four for robot6); more inputs than states; the unstabilisable instance.

Figures of the host-compiled header against scipy (printed by the test; measured where it was written):
    worst |P - P_scipy| / max|P| = 9.9e-12 (cart_pendulum_0.01, max|P| = 2.9e5, 14 steps), next 2.4e-12 (cart_pendulum_0.1,
    max|P| = 3.0e4); every other case below 2e-13.  The numpy restatement measures the same two figures (9.9e-12, 2.4e-12): the
    distance is between the doubling iteration and scipy's solver at these condition numbers, not between the two codes.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import lqr_reference as lr
from tests.test_pins import K_P0, K_P1

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'hilo_mpc_amd', 'csrc')

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "hilo_lqr.h"
using namespace hilo;
using HostVec = LaneVec<double*>;

static void print_row(const char* tag, const double* v, int n) {
  printf("%s", tag);
  for (int i = 0; i < n; ++i) printf(" %.17g", v[i]);
  printf("\n");
}

// gain n m horizon max_iter tol has_N  A B Q R [N]
static int gain(int argc, char** argv) {
  const int n = atoi(argv[2]), m = atoi(argv[3]);
  LqrParams o = {atoi(argv[4]), atoi(argv[5]), atof(argv[6])};
  const int has_n = atoi(argv[7]);
  if (n > LQR_MAX_NX || m > LQR_MAX_NU) { fprintf(stderr, "size\n"); return 3; }
  if (argc != 8 + 2 * n * n + n * m + m * m + (has_n ? n * m : 0)) { fprintf(stderr, "bad argument count %d\n", argc); return 2; }
  std::vector<double> work(lqr_work_doubles(n, m), 0.0), Q(n * n), R(m * m), N(n * m);
  const LqrWork<HostVec> w(HostVec{work.data(), 1}, n, m);
  int a = 8;
  for (int i = 0; i < n * n; ++i) w.A[i] = atof(argv[a++]);
  for (int i = 0; i < n * m; ++i) w.B[i] = atof(argv[a++]);
  for (int i = 0; i < n * n; ++i) Q[i] = atof(argv[a++]);
  for (int i = 0; i < m * m; ++i) R[i] = atof(argv[a++]);
  for (int i = 0; has_n && i < n * m; ++i) N[i] = atof(argv[a++]);
  int iters = 0;
  const int status = lqr_solve(n, m, o, w, Q.data(), R.data(), has_n ? N.data() : nullptr, &iters);
  printf("stats %d %d\n", status, iters);
  const double nan = __builtin_nan("");
  std::vector<double> K(m * n), P(n * n);
  for (int i = 0; i < m * n; ++i) K[i] = status == LQR_OK ? w.K[i] : nan;
  for (int i = 0; i < n * n; ++i) P[i] = status == LQR_OK ? w.P[i] : nan;
  print_row("K", K.data(), m * n);
  print_row("P", P.data(), n * n);
  // the feedback for x = (1, 2, ...), x_eq = .5 x, u_eq = (1, ...)
  std::vector<double> x(n), xe(n), ue(m, 1.0), u(m);
  for (int i = 0; i < n; ++i) { x[i] = i + 1.0; xe[i] = .5 * x[i]; }
  lqr_feedback(n, m, K.data(), x.data(), xe.data(), ue.data(), u.data());
  print_row("u", u.data(), m);
  return 0;
}

// lin / step  model order nsub dt  x u p
template <class M>
static int lin(int argc, char** argv) {
  constexpr int NX = M::NX, NU = M::NU, NP = M::NP, NY = M::NY;
  if (argc != 6 + NX + NU + NP) { fprintf(stderr, "bad argument count %d\n", argc); return 2; }
  const int order = atoi(argv[3]), nsub = atoi(argv[4]);
  const double dt = atof(argv[5]);
  double x[NX], u[NU], p[NP > 0 ? NP : 1];
  int a = 6;
  for (int i = 0; i < NX; ++i) x[i] = atof(argv[a++]);
  for (int i = 0; i < NU; ++i) u[i] = atof(argv[a++]);
  for (int i = 0; i < NP; ++i) p[i] = atof(argv[a++]);
  if (!strcmp(argv[1], "step")) {
    double xn[NX], y[NY];
    model_step<M>(order, nsub, x, u, p, dt, xn);
    M::meas(x, u, p, dt, y);
    print_row("x", xn, NX);
    print_row("y", y, NY);
    return 0;
  }
  double A[NX * NX], B[NX * NU], C[NY * NX];
  lqr_linearize<M, true>(order, nsub, x, u, p, dt, HostVec{A, 1}, HostVec{B, 1}, HostVec{C, 1});
  print_row("A", A, NX * NX);
  print_row("B", B, NX * NU);
  print_row("C", C, NY * NX);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 6) return 2;
  if (!strcmp(argv[1], "gain")) return gain(argc, argv);
  if (!strcmp(argv[2], "pendulum4")) return lin<Pendulum4>(argc, argv);
  if (!strcmp(argv[2], "chemostat4")) return lin<Chemostat4>(argc, argv);
  if (!strcmp(argv[2], "lti422")) return lin<Lti<4, 2, 2>>(argc, argv);
  if (!strcmp(argv[2], "robot6")) return lin<Robot6>(argc, argv);
  return 2;
}
"""


def _hipcc():
    for c in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', shutil.which('hipcc')):
        if c and os.path.exists(c):
            return c
    return None


def _rows(out):
    return {ln.split()[0]: np.array([float(v) for v in ln.split()[1:]]) for ln in out.strip().split('\n')}


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip('hipcc not available')
    d = tmp_path_factory.mktemp('lqr_host')
    src = d / 'driver.hip'
    src.write_text(DRIVER)
    exe = d / 'driver'
    subprocess.check_call([hipcc, '-x', 'hip', '--cuda-host-only', '-std=c++17', '-O2', '-I', CSRC, str(src), '-o', str(exe)])

    class D:
        @staticmethod
        def gain(A, B, Q, R, N=None, horizon=0, max_iter=50, tol=1e-12):
            n, m = B.shape
            args = [str(exe), 'gain', str(n), str(m), str(horizon), str(max_iter), repr(tol), str(int(N is not None))]
            for M in (A, B, Q, R) + ((N,) if N is not None else ()):
                args += [repr(float(v)) for v in np.asarray(M, dtype=float).ravel()]
            r = _rows(subprocess.check_output(args, text=True))
            return r['K'].reshape(m, n), r['P'].reshape(n, n), int(r['stats'][0]), int(r['stats'][1]), r['u']

        @staticmethod
        def model(mode, name, order, nsub, dt, x, u, p):
            args = [str(exe), mode, name, str(order), str(nsub), repr(float(dt))] + [repr(float(v)) for v in list(x) + list(u) + list(p)]
            return _rows(subprocess.check_output(args, text=True))
    return D


@pytest.mark.parametrize('p,K_ref', [(1., K_P1), (0., K_P0)])
def test_finite_horizon_reproduces_the_reference_gains(driver, p, K_ref):
    A, B = lr.lqr_model(p)
    K, P, status, iters, _ = driver.gain(A, B, np.eye(3), np.eye(2), horizon=5)
    assert (status, iters) == (0, 5)
    np.testing.assert_allclose(K, K_ref, rtol=1e-7, atol=1e-9)            # the reference's own tolerance (tests/test_LQR.py)
    Kn, Pn = lr.riccati_finite(A, B, np.eye(3), np.eye(2), 5)
    eP, eK = np.max(np.abs(P - Pn)), np.max(np.abs(K - Kn))
    print(f"p={p:g}: |P - recursion| {eP:.2e} (bound {lr.bound(Pn):.2e}), |K - recursion| {eK:.2e} (bound {lr.bound(Kn):.2e})")
    assert eP <= lr.bound(Pn) and eK <= lr.bound(Kn)


@pytest.mark.parametrize('name', ['lqr_p1_cross', 'random_6x2_cross', 'cart_pendulum_0.1'])
def test_finite_horizon_against_the_numpy_recursion(driver, name):
    A, B, Q, R, N = lr.cases()[name]
    for horizon in (1, 20):
        K, P, status, iters, _ = driver.gain(A, B, Q, R, N, horizon=horizon)
        Kn, Pn = lr.riccati_finite(A, B, Q, R, horizon, N)
        assert (status, iters) == (0, horizon)
        eP, eK = np.max(np.abs(P - Pn)), np.max(np.abs(K - Kn))
        print(f"{name} horizon {horizon}: |P - recursion| {eP:.2e} (bound {lr.bound(Pn):.2e}), |K - recursion| {eK:.2e}")
        assert eP <= lr.bound(Pn) and eK <= lr.bound(Kn)


@pytest.mark.parametrize('name', sorted(lr.cases()))
def test_stationary_gain_against_scipy(driver, name):
    A, B, Q, R, N = lr.cases()[name]
    K, P, status, iters, u = driver.gain(A, B, Q, R, N)
    Ks, Ps = lr.scipy_dare(A, B, Q, R, N)
    Kn, Pn, sn, itn = lr.dare_doubling(A, B, Q, R, N)
    eP, eK = np.max(np.abs(P - Ps)), np.max(np.abs(K - Ks))
    print(f"{name}: {iters} steps (numpy {itn}), max|P| {np.max(np.abs(Ps)):.3e}, |P - scipy| / max|P| {eP / max(1., np.max(np.abs(Ps))):.2e}, "
          f"|K - scipy| / max|K| {eK / max(1., np.max(np.abs(Ks))):.2e}; numpy restatement {np.max(np.abs(Pn - Ps)) / max(1., np.max(np.abs(Ps))):.2e}")
    assert status == 0 and sn == 0 and 5 <= iters <= 14 and abs(iters - itn) <= 1
    assert eP <= lr.bound(Ps) and eK <= lr.bound(Ks)
    assert np.max(np.abs(P - Pn)) <= lr.bound(Pn) and np.max(np.abs(K - Kn)) <= lr.bound(Kn)
    # the feedback the driver formed with that gain: u = u_eq - K (x - x_eq), x = (1, 2, ...), x_eq = x / 2, u_eq = 1
    x = np.arange(1., A.shape[0] + 1.)
    np.testing.assert_allclose(u, 1. - K @ (.5 * x), rtol=1e-13, atol=1e-13)


def test_doubling_replaces_hundreds_of_fixed_point_steps(driver):
    """What the doubling algorithm is for: the plain recursion needs hundreds to thousands of steps at small sampling intervals to
    reach what the host-compiled header reaches in at most 14 - and the two end at the same P."""
    for name, least in (('double_integrator_0.05', 200), ('double_integrator_0.005', 2000), ('cart_pendulum_0.01', 1000)):
        A, B, Q, R, _ = lr.cases()[name]
        Pf, n = lr.riccati_fixed_point(A, B, Q, R)
        _, P, status, it, _ = driver.gain(A, B, Q, R)
        print(f"{name}: fixed point {n} steps, doubling {it}; |P - P_fixed_point| / max|P| {np.max(np.abs(P - Pf)) / np.max(np.abs(Pf)):.2e}")
        assert n >= least and status == 0 and it <= 14
        # (the recursion stops when a STEP is below 1e-12 max|P|; at a contraction rate close to 1 its distance to the fixed point is
        # that step over (1 - rate): 1e-8 covers rates up to 1 - 1e-4)
        assert np.max(np.abs(P - Pf)) <= 1e-8 * np.max(np.abs(Pf))


@pytest.mark.parametrize('name', sorted(lr.wide_cases()))
def test_more_inputs_than_states(driver, name):
    """nu > nx: A'PB + N (n x m) is larger than the n x n matrices of the workspace; finite horizon (with and without N) against the
    numpy recursion and stationary against scipy."""
    A, B = lr.wide_cases()[name]
    n, m = B.shape
    Q, R = np.eye(n), np.eye(m)
    N = .1 * np.random.default_rng(n * 10 + m).standard_normal((n, m))
    for horizon in (1, 3, 20):
        for Nx in (None, N):
            K, P, status, iters, _ = driver.gain(A, B, Q, R, Nx, horizon=horizon)
            Kn, Pn = lr.riccati_finite(A, B, Q, R, horizon, Nx)
            assert (status, iters) == (0, horizon)
            assert np.max(np.abs(P - Pn)) <= lr.bound(Pn) and np.max(np.abs(K - Kn)) <= lr.bound(Kn), (horizon, Nx is not None)
    for Nx in (None, N):
        K, P, status, iters, _ = driver.gain(A, B, Q, R, Nx)
        Ks, Ps = lr.scipy_dare(A, B, Q, R, Nx)
        assert status == 0 and np.max(np.abs(P - Ps)) <= lr.bound(Ps) and np.max(np.abs(K - Ks)) <= lr.bound(Ks)


def test_unstabilisable_instance_is_reported(driver):
    """p = 0: the first input does nothing, and the block it would have to stabilise has spectral radius sqrt(3).  The doubling
    iterates grow until they overflow; with max_iter = 50 the status is 1 or 2 - never 0 - and the rows are NaN."""
    A, B = lr.lqr_model(0.)
    assert abs(np.max(np.abs(np.linalg.eigvals(A[:2, :2]))) - np.sqrt(3.)) < 1e-12
    K, P, status, iters, u = driver.gain(A, B, np.eye(3), np.eye(2))
    assert status in (1, 2) and 1 <= iters <= 50
    assert np.all(np.isnan(K)) and np.all(np.isnan(P)) and np.all(np.isnan(u))
    # R not positive definite: status 2 from the Cholesky factorisation, finite horizon and stationary
    A, B = lr.lqr_model(1.)
    for horizon in (0, 3):
        K, P, status, _, _ = driver.gain(A, B, np.eye(3), np.diag([1., -1.]), horizon=horizon)
        assert status == 2 and np.all(np.isnan(K))


def _central(driver, name, order, nsub, dt, x, u, p, h=1e-6):
    nx, nu = len(x), len(u)
    w = np.concatenate([x, u])
    cols_x, cols_y = [], []
    for j in range(nx + nu):
        e = np.zeros(nx + nu)
        e[j] = h
        a = driver.model('step', name, order, nsub, dt, (w + e)[:nx], (w + e)[nx:], p)
        b = driver.model('step', name, order, nsub, dt, (w - e)[:nx], (w - e)[nx:], p)
        cols_x.append((a['x'] - b['x']) / (2 * h))
        cols_y.append((a['y'] - b['y']) / (2 * h))
    return np.array(cols_x).T, np.array(cols_y).T


@pytest.mark.parametrize('order,nsub', [(4, 1), (2, 3)])
def test_linearisation_of_the_pendulum_against_central_differences(driver, order, nsub):
    x, u, dt = np.array([.3, -.4, .5, .8]), np.array([1.5]), .1
    r = driver.model('lin', 'pendulum4', order, nsub, dt, x, u, [])
    fd, fdy = _central(driver, 'pendulum4', order, nsub, dt, x, u, [])
    np.testing.assert_allclose(np.hstack([r['A'].reshape(4, 4), r['B'].reshape(4, 1)]), fd, rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(r['C'].reshape(4, 4), np.eye(4), atol=0)


def test_linearisation_with_parameters_and_a_measurement_map(driver):
    """chemostat4: 4 states + 2 inputs (one pass of six directions) with parameters; the measurement map picks two states."""
    x, u, p, dt = np.array([.1, 40., .5, .2]), np.array([.1, .05]), [100., 4., 1., 0.], .5
    r = driver.model('lin', 'chemostat4', 4, 1, dt, x, u, p)
    fd, fdy = _central(driver, 'chemostat4', 4, 1, dt, x, u, p, h=1e-5)
    np.testing.assert_allclose(np.hstack([r['A'].reshape(4, 4), r['B'].reshape(4, 2)]), fd, rtol=1e-7, atol=1e-9)
    np.testing.assert_allclose(r['C'].reshape(2, 4), fdy[:, :4], rtol=1e-7, atol=1e-9)


def test_linearisation_of_an_lti_shape_returns_its_matrices(driver):
    rng = np.random.default_rng(5)
    A, B, C = rng.standard_normal((4, 4)), rng.standard_normal((4, 2)), rng.standard_normal((2, 4))
    p = np.concatenate([A.ravel(), B.ravel(), C.ravel()])
    x, u = rng.standard_normal(4), rng.standard_normal(2)
    r = driver.model('lin', 'lti422', 4, 1, 1., x, u, p)
    np.testing.assert_allclose(r['A'].reshape(4, 4), A, rtol=1e-15)
    np.testing.assert_allclose(r['B'].reshape(4, 2), B, rtol=1e-15)
    np.testing.assert_allclose(r['C'].reshape(2, 4), C, rtol=1e-15)
    fd, _ = _central(driver, 'lti422', 4, 1, 1., x, u, p)
    np.testing.assert_allclose(np.hstack([r['A'].reshape(4, 4), r['B'].reshape(4, 2)]), fd, rtol=1e-7, atol=1e-9)


def test_linearisation_in_passes_of_four_directions(driver):
    """robot6: 6 states + 2 inputs = 8 directions, two passes of four - the second holds the last two states AND the inputs, and the
    measurement map (two of the states) is differentiated in the passes that hold state directions."""
    x, u, dt = np.array([.3, -.4, .5, .8, .6, -.2]), np.array([1.5, -.7]), .1
    for order, nsub in ((4, 1), (3, 2)):
        r = driver.model('lin', 'robot6', order, nsub, dt, x, u, [])
        fd, fdy = _central(driver, 'robot6', order, nsub, dt, x, u, [])
        np.testing.assert_allclose(np.hstack([r['A'].reshape(6, 6), r['B'].reshape(6, 2)]), fd, rtol=1e-7, atol=1e-9)
        C = np.zeros((2, 6))
        C[0, 0] = C[1, 2] = 1.
        np.testing.assert_array_equal(r['C'].reshape(2, 6), C)
