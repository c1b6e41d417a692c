"""CPU: time-variant models - the time-aware paths of csrc/hilo_integrate.h and csrc/hilo_models.h compiled for the HOST and run
there, the front end (`t` in equations, `Model.is_time_variant`, the emitted functor, the refusals) and the host plumbing of the
start time (`hilo_sim_opts.t0`).

The driver is built with `hipcc -x hip --cuda-host-only` like the ones of tests/test_integrate_host.py and tests/test_bdf_host.py.
It drives `dopri5_interval`, `bdf_interval` and `model_step` the way `rollout_body` / `rollout_bdf_body` do - the start time in the
carry structs, sampling interval k starting at t0 + k dt - with hand-written functors that declare TIME_VARIANT (the cases of
tests/timevar_reference.py), and carries the functors of the two existing drivers WITHOUT the declaration: they compile untouched
and give what their own tests expect."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from hilo_mpc_amd import Model, _lib
from tests import sim_reference as sr
from tests import stiff_reference as st
from tests import timevar_reference as tv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'hilo_mpc_amd', 'csrc')

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "hilo_integrate.h"
using namespace hilo;

// dx1/dt = x2, dx2/dt = -k x1 - c x2 + u sin(w t), y = x1 + cos t; p = (k, c, w)
struct Forced2 {
  static constexpr int NX = 2, NU = 1, NP = 3, NY = 1;
  static constexpr bool DISCRETE = false;
  static constexpr bool TIME_VARIANT = true;
  template <class T, class U, class P>
  HD static void ode_t(double t, const T* x, const U* u, const P* p, double, T* dx) {
    dx[0] = x[1];
    dx[1] = -1.0 * (p[0] * x[0]) - p[1] * x[1] + u[0] * sin(p[2] * t);
  }
  template <class T, class U, class P>
  HD static void meas_t(double t, const T* x, const U*, const P*, double, T* y) { y[0] = x[0] + cos(t); }
};
// dx/dt = -lam (x - cos t) - sin t; p = (lam)
struct Prothero1 {
  static constexpr int NX = 1, NU = 0, NP = 1, NY = 0;
  static constexpr bool DISCRETE = false;
  static constexpr bool TIME_VARIANT = true;
  template <class T, class U, class P>
  HD static void ode_t(double t, const T* x, const U*, const P* p, double, T* dx) {
    dx[0] = -1.0 * (p[0] * (x[0] - cos(t))) - sin(t);
  }
};
// dx/dt = t^M
template <int M>
struct Poly {
  static constexpr int NX = 1, NU = 0, NP = 0, NY = 0;
  static constexpr bool DISCRETE = false;
  static constexpr bool TIME_VARIANT = true;
  template <class T, class U, class P>
  HD static void ode_t(double t, const T*, const U*, const P*, double, T* dx) {
    double v = 1.0;
    for (int i = 0; i < M; ++i) v *= t;
    dx[0] = T(v);
  }
};
// x+ = a x + sin t, y = x + t: a discrete model; p = (a)
struct Disc1 {
  static constexpr int NX = 1, NU = 0, NP = 1, NY = 1;
  static constexpr bool DISCRETE = true;
  static constexpr bool TIME_VARIANT = true;
  template <class T, class U, class P>
  HD static void ode_t(double t, const T* x, const U*, const P* p, double, T* xn) { xn[0] = p[0] * x[0] + sin(t); }
  template <class T, class U, class P>
  HD static void meas_t(double t, const T* x, const U*, const P*, double, T* y) { y[0] = x[0] + t; }
};

// ---- the functors of the existing drivers, as they are there (no declaration: autonomous) ----
struct Blowup1 {
  static constexpr int NX = 1, NU = 0, NP = 0, NY = 0;
  static constexpr bool DISCRETE = false;
  template <class T, class U, class P>
  HD static void ode(const T* x, const U*, const P*, double, T* dx) { dx[0] = x[0] * x[0]; }
};
struct Robertson3 {
  static constexpr int NX = 3, NU = 0, NP = 3, NY = 0;
  static constexpr bool DISCRETE = false;
  template <class T, class U, class P>
  HD static void ode(const T* x, const U*, const P* p, double, T* dx) {
    dx[0] = -1.0 * (p[0] * x[0]) + p[2] * x[1] * x[2];
    dx[1] = p[0] * x[0] - p[2] * x[1] * x[2] - p[1] * x[1] * x[1];
    dx[2] = p[1] * x[1] * x[1];
  }
};
struct Vdp2 {
  static constexpr int NX = 2, NU = 0, NP = 1, NY = 0;
  static constexpr bool DISCRETE = false;
  template <class T, class U, class P>
  HD static void ode(const T* x, const U*, const P* p, double, T* dx) {
    dx[0] = x[1];
    dx[1] = p[0] * ((1.0 - x[0] * x[0]) * x[1]) - x[0];
  }
};
static_assert(model_time_variant<Forced2>::value && model_time_variant<Poly<3>>::value && !model_time_variant<Pendulum4>::value &&
              !model_time_variant<Blowup1>::value && !model_time_variant<Lti<2, 1, 1>>::value, "the trait");

// argv: method model t0 dt steps rtol atol max_steps per_step x0[NX] then rows of [u; p]
//   method dopri / bdf: the integrators, driven like rollout_body / rollout_bdf_body; map: model_step with rtol = order, atol = n_sub
template <class M>
int run(int argc, char** argv) {
  const char* method = argv[1];
  const double t0 = atof(argv[3]), dt = atof(argv[4]);
  const int steps = atoi(argv[5]);
  const double rtol = atof(argv[6]), atol = atof(argv[7]);
  const int max_steps = atoi(argv[8]), per_step = atoi(argv[9]);
  constexpr int NUP = M::NU + M::NP;
  constexpr bool TV = model_time_variant<M>::value;
  if (argc != 10 + M::NX + NUP * (per_step ? steps : 1)) { fprintf(stderr, "bad argument count %d\n", argc); return 2; }
  double x[M::NX], up[NUP > 0 ? NUP : 1];
  for (int i = 0; i < M::NX; ++i) x[i] = atof(argv[10 + i]);
  auto rows = [&](int k) {
    for (int i = 0; i < NUP; ++i) up[i] = atof(argv[10 + M::NX + (per_step ? k : 0) * NUP + i]);
  };
  auto out = [&](int k, bool ok) {
    printf("x");
    for (int i = 0; i < M::NX; ++i) printf(" %.17g", ok ? x[i] : __builtin_nan(""));
    printf("\n");
    if constexpr (M::NY > 0 && TV) {
      double y[M::NY];
      model_meas_at<M>(M::DISCRETE ? t0 + k * dt : t0 + k * dt + dt, x, up, up + M::NU, dt, y);
      printf("y");
      for (int i = 0; i < M::NY; ++i) printf(" %.17g", y[i]);
      printf("\n");
    }
  };
  if (!strcmp(method, "dopri")) {
    if constexpr (!M::DISCRETE) {
      Dopri5Carry<M::NX> c;
      dopri5_init(c, 0.0);
      if (TV) c.t0 = t0;
      for (int k = 0; k < steps; ++k) {
        if (k == 0 || per_step) { rows(k); c.have_k1 = false; }
        if (TV) c.t = k * dt;
        const int s = dopri5_interval<M>(c, x, up, up + M::NU, dt, rtol, atol, max_steps);
        out(k, s == SIM_OK);
      }
      printf("stats %d %d %d %d\n", c.status, c.n_acc, c.n_rej, c.n_rhs);
    }
  } else if (!strcmp(method, "bdf")) {
    if constexpr (!M::DISCRETE) {
      double* store = (double*)malloc(sizeof(double) * bdf_entries(M::NX));
      const BdfMem<M::NX, 1, double*> mem = {store};
      BdfCarry<M::NX> c;
      bdf_init(c, per_step ? dt : steps * dt);
      if (TV) c.t0 = t0;
      for (int k = 0; k < steps; ++k) {
        if (k == 0 || per_step) {
          rows(k);
          if (k > 0) { bdf_restart(c, dt); if (TV) c.t0 = t0 + k * dt; }
        }
        const int s = bdf_interval<M>(c, mem, x, up, up + M::NU, dt, per_step ? dt : (k + 1) * dt, rtol, atol, 0.0, max_steps);
        out(k, s == SIM_OK);
      }
      printf("stats %d %d %d %d %d %d\n", c.status, c.n_acc, c.n_rej, c.n_rhs, c.n_jac, c.n_lu);
      free(store);
    }
  } else {
    const int order = (int)rtol, n_sub = (int)atol;
    for (int k = 0; k < steps; ++k) {
      if (k == 0 || per_step) rows(k);
      double xo[M::NX];
      model_step<M>(order, n_sub, x, up, up + M::NU, dt, xo, NoExt(), t0 + k * dt);
      for (int i = 0; i < M::NX; ++i) x[i] = xo[i];
      out(k, true);
    }
    printf("stats 0\n");
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 10) return 2;
  const char* m = argv[2];
  if (!strcmp(m, "forced2")) return run<Forced2>(argc, argv);
  if (!strcmp(m, "prothero1")) return run<Prothero1>(argc, argv);
  if (!strcmp(m, "poly0")) return run<Poly<0>>(argc, argv);
  if (!strcmp(m, "poly1")) return run<Poly<1>>(argc, argv);
  if (!strcmp(m, "poly2")) return run<Poly<2>>(argc, argv);
  if (!strcmp(m, "poly3")) return run<Poly<3>>(argc, argv);
  if (!strcmp(m, "poly4")) return run<Poly<4>>(argc, argv);
  if (!strcmp(m, "disc1")) return run<Disc1>(argc, argv);
  if (!strcmp(m, "pendulum4")) return run<Pendulum4>(argc, argv);
  if (!strcmp(m, "chemostat4")) return run<Chemostat4>(argc, argv);
  if (!strcmp(m, "blowup1")) return run<Blowup1>(argc, argv);
  if (!strcmp(m, "robertson3")) return run<Robertson3>(argc, argv);
  if (!strcmp(m, "vdp2")) return run<Vdp2>(argc, argv);
  return 2;
}
"""


def _hipcc():
    for c in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', shutil.which('hipcc')):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip('hipcc not available')
    d = tmp_path_factory.mktemp('timevar_host')
    src = d / 'driver.hip'
    src.write_text(DRIVER)
    exe = d / 'driver'
    subprocess.check_call([hipcc, '-x', 'hip', '--cuda-host-only', '-std=c++17', '-O2', '-I', CSRC, str(src), '-o', str(exe)])

    def run(method, model, x0, up_rows, t0, dt, steps, a, b, max_steps=10000):
        up_rows = np.atleast_2d(np.asarray(up_rows, dtype=float))
        per_step = int(up_rows.shape[0] > 1)
        args = [str(exe), method, model, repr(float(t0)), repr(float(dt)), str(steps), repr(float(a)), repr(float(b)), str(max_steps),
                str(per_step)]
        args += [repr(float(v)) for v in x0] + [repr(float(v)) for v in up_rows.ravel()]
        out = subprocess.check_output(args, text=True).strip().split('\n')
        x = np.array([[float(v) for v in ln.split()[1:]] for ln in out if ln.startswith('x')])
        y = np.array([[float(v) for v in ln.split()[1:]] for ln in out if ln.startswith('y')])
        stats = [int(v) for v in out[-1].split()[1:]]
        return np.vstack([np.asarray(x0, dtype=float)[None], x]), y, stats
    return run


def _forced2_sequence(steps):
    return np.random.default_rng(5).uniform(-1., 1., (steps, 1))


def _prothero_sequence(p, steps):
    P = np.tile(p, (steps, 1))
    P[:, 0] *= np.random.default_rng(6).uniform(.5, 2., steps)        # lam jumps at every sampling instant
    return P


@pytest.fixture(scope='module')
def refs():
    """Every reference of this module, once, in worker processes."""
    jobs, keys = [], []
    for case in ('forced2', 'forced2_t0'):
        x0, u, p, dt, steps, t0 = tv.CASES[case]
        jobs.append(('explicit', case, x0, u, p, dt, steps, t0, tv.TOLS_EXPLICIT))
        keys.append((case, 'held'))
        jobs.append(('explicit', case, x0, _forced2_sequence(steps), p, dt, steps, t0, tv.TOLS_EXPLICIT))
        keys.append((case, 'seq'))
    x0, u, p, dt, steps, t0 = tv.CASES['prothero1']
    jobs.append(('stiff', 'prothero1', x0, u, p, dt, steps, t0, tv.TOLS_STIFF))
    keys.append(('prothero1', 'held'))
    jobs.append(('stiff', 'prothero1', x0, u, _prothero_sequence(p, steps), dt, steps, t0, tv.TOLS_STIFF))
    keys.append(('prothero1', 'seq'))
    return dict(zip(keys, tv.run_jobs(jobs)))


@pytest.mark.parametrize('i_tol', [0, 1])
@pytest.mark.parametrize('inputs', ['held', 'seq'])
@pytest.mark.parametrize('case', ['forced2', 'forced2_t0'])
def test_forced2_under_the_explicit_pair(driver, refs, case, inputs, i_tol):
    """t0 = 2.5 and t0 = 0, inputs held and a sequence: within the sim_reference bound, and the measurement is h at t_k + dt."""
    rtol, atol = tv.TOLS_EXPLICIT[i_tol]
    x0, u, p, dt, steps, t0 = tv.CASES[case]
    ref, admissible, e45, e_tight = refs[(case, inputs)][i_tol]
    U = np.tile(u, (1, 1)) if inputs == 'held' else _forced2_sequence(steps)
    rows = np.hstack([U, np.tile(p, (U.shape[0], 1))])
    x, y, (status, n_acc, n_rej, n_rhs) = driver('dopri', 'forced2', x0, rows, t0, dt, steps, rtol, atol)
    err = sr.rel_err(x, ref, rtol, atol)
    print(f"{case} {inputs} rtol={rtol:g}: error {err:.3e}, RK45 {e45:.3e}, DOP853 vs Radau {e_tight:.3e}; accepted {n_acc}, rejected "
          f"{n_rej}, rhs {n_rhs}")
    assert status == 0
    assert err <= admissible
    if inputs == 'held':
        assert n_rhs == 6 * (n_acc + n_rej) + 2        # the slope kept from an accepted step serves the next one across the instants
    tk = t0 + dt * np.arange(steps)
    np.testing.assert_allclose(y[:, 0], x[1:, 0] + np.cos(tk + dt), rtol=1e-15, atol=1e-15)


def test_forced2_tells_wrong_times_apart(refs):
    """What the bound rests on, on the references alone: the same problem with the time frozen at t_k over each interval, or with
    t0 ignored, is further from the tight solution than the admissible error by orders of magnitude."""
    rtol, atol = tv.TOLS_EXPLICIT[0]
    x0, u, p, dt, steps, t0 = tv.CASES['forced2']
    ref, admissible, e45, e_tight = refs[('forced2', 'held')][0]
    f, _ = tv.system('forced2')
    from scipy.integrate import solve_ivp
    frozen, x = [np.array(x0)], np.array(x0)
    for k in range(steps):
        tk = t0 + k * dt
        x = solve_ivp(lambda t, z: f(tk, z, u, p), (tk, tk + dt), x, method='DOP853', rtol=1e-12, atol=1e-14).y[:, -1]
        frozen.append(x)
    e_frozen = sr.rel_err(np.array(frozen), ref, rtol, atol)
    e_no_t0 = sr.rel_err(tv.integrate('forced2', x0, u, p, dt, steps, 0., 'DOP853', 1e-12, 1e-14), ref, rtol, atol)
    print(f"admissible {admissible:.3e}; time frozen {e_frozen:.3e}, t0 ignored {e_no_t0:.3e}; tight {e_tight:.3e}, RK45 {e45:.3e}")
    assert e_frozen > 1e4 * admissible and e_no_t0 > 1e4 * admissible
    assert e_tight <= e45 / 100.


@pytest.mark.parametrize('i_tol', [0, 1])
@pytest.mark.parametrize('inputs', ['held', 'seq'])
def test_prothero1_under_bdf(driver, refs, inputs, i_tol):
    rtol, atol = tv.TOLS_STIFF[i_tol]
    x0, u, p, dt, steps, t0 = tv.CASES['prothero1']
    ref, admissible, e_bdf, e_tight, counts = refs[('prothero1', inputs)][i_tol]
    rows = [p] if inputs == 'held' else _prothero_sequence(p, steps)
    x, _, (status, n_acc, n_rej, n_rhs, n_jac, n_lu) = driver('bdf', 'prothero1', x0, rows, t0, dt, steps, rtol, atol)
    err = sr.rel_err(x, ref, rtol, atol)
    print(f"prothero1 {inputs} rtol={rtol:g}: error {err:.3e}, scipy BDF {e_bdf:.3e}, tight solutions {e_tight:.3e}; accepted {n_acc}, "
          f"rejected {n_rej}, rhs {n_rhs}, Jacobians {n_jac}, factorisations {n_lu}; scipy steps {counts[0]}, nfev {counts[1]}")
    assert status == 0
    assert err <= admissible
    assert n_acc <= st.COST_MARGIN * counts[0] and n_rhs <= st.COST_MARGIN * counts[1]
    if inputs == 'held':
        t = t0 + dt * np.arange(steps + 1)
        exact = tv.prothero_exact(t, x0[0], p[0], t0)
        e_exact = float(np.max(np.abs(x[:, 0] - exact) / np.abs(exact)))
        print(f"   against the exact solution {e_exact:.3e}")
        assert e_exact <= 10. * sr.FACTOR * rtol


def test_preconditions(refs):
    """stiff_reference's precondition on the references alone: the two tight solutions of prothero1 agree at least ten times below
    the error of scipy's BDF at both tolerances, and Radau is within 1e-11 of the exact solution."""
    x0, u, p, dt, steps, t0 = tv.CASES['prothero1']
    for i_tol in (0, 1):
        ref, _, e_bdf, e_tight, _ = refs[('prothero1', 'held')][i_tol]
        print(f"rtol {tv.TOLS_STIFF[i_tol][0]:g}: BDF {e_bdf:.3e}, Radau vs LSODA {e_tight:.3e}")
        assert e_tight <= e_bdf / 10.
    exact = tv.prothero_exact(t0 + dt * np.arange(steps + 1), x0[0], p[0], t0)
    assert np.max(np.abs(ref[:, 0] - exact)) <= 1e-11


def _poly_exact(m, t0, t1):
    return (t1 ** (m + 1) - t0 ** (m + 1)) / (m + 1)


def test_poly_through_the_fixed_step_map(driver):
    """A Runge-Kutta method of order s integrates t^(s-1) exactly: only right stage times give the exact integral, to 4 ulp."""
    t0, dt, steps = 1.5, .25, 4
    for order in (1, 2, 3, 4):
        for n_sub in (1, 8) if order == 4 else (1,):
            m = order - 1
            x, _, _ = driver('map', f'poly{m}', [0.], [[]], t0, dt, steps, order, n_sub)
            exact = _poly_exact(m, t0, t0 + steps * dt)
            print(f"order {order} x {n_sub}, m = {m}: {x[-1, 0]!r} vs {exact!r}, {abs(x[-1, 0] - exact) / np.spacing(exact):.1f} ulp")
            assert abs(x[-1, 0] - exact) <= 4. * np.spacing(exact)
    # not trivially: t^4 is beyond order 4
    x, _, _ = driver('map', 'poly4', [0.], [[]], t0, dt, steps, 4, 1)
    exact = _poly_exact(4, t0, t0 + steps * dt)
    assert abs(x[-1, 0] - exact) > 1e3 * np.spacing(exact)


def test_discrete_map_and_measurement_see_the_time_of_the_call(driver):
    """x(k+1) = a x(k) + sin(t_k), y(k) = x(k+1) + t_k, t_k = t0 + k dt (modules/base.py:1785-1795: one time value per call of the
    discrete function)."""
    a, t0, dt, steps = .9, 2.5, .5, 5
    x, y, _ = driver('map', 'disc1', [1.], [[a]], t0, dt, steps, 1, 1)
    ref = [1.]
    for k in range(steps):
        ref.append(a * ref[-1] + np.sin(t0 + k * dt))
    np.testing.assert_allclose(x[:, 0], ref, rtol=1e-15)
    # the measurement of call k sees the new state and the SAME time t_k (modules/base.py:1882-1895)
    np.testing.assert_allclose(y[:, 0], np.array(ref[1:]) + (t0 + dt * np.arange(steps)), rtol=1e-15)


def test_functors_without_the_trait_give_what_their_tests_expect(driver):
    """pendulum4 at 1e-8 through the same driver: tests/test_integrate_host.py's and tests/test_bdf_host.py's checks."""
    x0, u, p, dt, steps = sr.CASES['pendulum4']
    rtol, atol = 1e-8, 1e-10
    om = sr.oracle_model('pendulum4')
    x, _, (status, n_acc, n_rej, n_rhs) = driver('dopri', 'pendulum4', x0, [list(u) + list(p)], 0., dt, steps, rtol, atol)
    ref, admissible, _, _ = sr.bound(om, x0, u, p, dt, steps, rtol, atol)
    assert status == 0 and n_rhs == 6 * (n_acc + n_rej) + 2 and sr.rel_err(x, ref, rtol, atol) <= admissible
    # the start time is not read by an autonomous functor
    x2, _, _ = driver('dopri', 'pendulum4', x0, [list(u) + list(p)], 7.25, dt, steps, rtol, atol)
    assert np.array_equal(x, x2)
    x, _, (status, n_acc, n_rej, n_rhs, n_jac, n_lu) = driver('bdf', 'pendulum4', x0, [list(u) + list(p)], 0., dt, steps, rtol, atol)
    ref, admissible, _, _, counts = st.bound('pendulum4', x0, u, p, dt, steps, rtol, atol)
    assert status == 0 and sr.rel_err(x, ref, rtol, atol) <= admissible
    assert n_acc <= st.COST_MARGIN * counts[0] and n_rhs <= st.COST_MARGIN * counts[1]
    x, _, stats = driver('dopri', 'blowup1', [1.], [[]], 0., .25, 8, 1e-8, 1e-10)
    assert stats[0] in (1, 2) and np.all(np.isnan(x[6:, 0]))


# ---- front end -------------------------------------------------------------------------------------------------------------------
FORCED2_TEXT = """
dx_1/dt = x_2(t)
dx_2/dt = -k*x_1(t) - c*x_2(t) + u(k)*sin(w*t)
y(k) = x_1(t) + cos(t)
"""

# what `Model.user_source()` returned for the model of `_autonomous()` before time-variant models existed
AUTONOMOUS_SOURCE = """struct UserModel {
  static constexpr int NX = 2, NU = 1, NP = 1, NY = 1;
  static constexpr bool DISCRETE = false;
  template <class T, class U, class P>
  __device__ __forceinline__ static void ode(const T* x, const U* u, const P* p, double dt, T* dx) {
    (void)x; (void)u; (void)p; (void)dt;
    const auto t0 = p[0] * x[0];
    const auto t1 = -1.0 * (t0);
    const auto t2 = sin(x[1]);
    const auto t3 = t1 + t2;
    const auto t4 = t3 + u[0];
    dx[0] = T(x[1]);
    dx[1] = T(t4);
  }
  template <class T, class U, class P>
  __device__ __forceinline__ static void meas(const T* x, const U* u, const P* p, double dt, T* y) {
    (void)x; (void)u; (void)p; (void)dt; (void)y;
    y[0] = T(x[0]);
  }
};
"""


def _autonomous():
    m = Model(name='auto2')
    x = m.set_dynamical_states(['a', 'b'])
    u = m.set_inputs(['u'])
    p = m.set_parameters(['k'])
    from hilo_mpc_amd.expr import sin
    m.set_dynamical_equations([x[1], -(p[0] * x[0]) + sin(x[1]) + u[0]])
    m.set_measurement_equations([x[0]])
    return m.setup(dt=.5)


def _forced2_model(**setup):
    m = Model(name='forced2')
    m.set_parameters(['k', 'c', 'w'])
    m.set_equations(FORCED2_TEXT)
    return m.setup(dt=.5, **setup)


def test_t_parses_in_text_and_expressions():
    m = _forced2_model()
    assert m.dynamical_state_names == ['x_1', 'x_2'] and m.input_names == ['u'] and m.parameter_names == ['k', 'c', 'w']
    assert m.measurement_names == ['y']
    assert m.is_time_variant() and not m.is_autonomous()
    assert m._ode[1].depends_on('t') and m._meas[0].depends_on('t') and not m._ode[0].depends_on('t')
    assert m.is_linear()                      # (linearity is about x and u; the check does not trip over the time)
    e = Model(name='expr')
    x = e.set_dynamical_states(['x'])
    from hilo_mpc_amd.expr import sin
    e.set_dynamical_equations([-x[0] + sin(e.t)])
    e.set_measurement_equations(['x + t^2'])
    assert e.is_time_variant() and e.is_autonomous()
    a = _autonomous()
    assert not a.is_time_variant() and not a.is_autonomous()
    assert not Model('pendulum4').is_time_variant()
    # differentiation with respect to x, u and p treats the time as a constant
    from hilo_mpc_amd.expr import jacobian
    J = jacobian([m._ode[1]], list(m.x) + list(m.u))
    assert repr(J[0][2]) == 'sin(mul(w, t))'
    d = Model(name='disc', discrete=True)
    d.set_equations("x(k+1) = a*x(k) + sin(t)\ny(k) = x(k) + t")
    assert d.is_time_variant() and d.discrete


def test_autonomous_source_is_unchanged():
    src = _autonomous().user_source()
    assert src.startswith(AUTONOMOUS_SOURCE)
    # ... followed by the symbolic derivative source, which names neither the trait nor the time-aware entry points
    assert 'TIME_VARIANT' not in src and 'ode_t' not in src and 't_abs' not in src
    from hilo_mpc_amd.symdiff import sym_source
    a = _autonomous()
    assert src == AUTONOMOUS_SOURCE + sym_source('UserModel', 2, 1, a._ode, a._meas)


def test_time_variant_source():
    src = _forced2_model().user_source()
    assert 'static constexpr bool TIME_VARIANT = true;' in src
    assert 'static void ode_t(double t_abs, const T* x, const U* u, const P* p, double dt, T* dx)' in src
    assert 'static void meas_t(double t_abs, const T* x, const U* u, const P* p, double dt, T* y)' in src
    assert 'p[2] * t_abs' in src and 'cos(t_abs)' in src
    assert 'ode_t(0.0, x, u, p, dt, dx);' in src and 'meas_t(0.0, x, u, p, dt, y);' in src
    assert 'ModelSym' not in src              # no symbolic derivative source: no consumer of it takes such a model


def _compile_only(model, monkeypatch):
    if _hipcc() is None or not os.path.exists(os.path.join(ROOT, 'hilo_mpc_amd', 'libhilo_hip.so')):
        pytest.skip('the library is not built')
    monkeypatch.setenv('HILO_JIT_COMPILE_ONLY', '1')
    from hilo_mpc_amd.estimator import ExtendedKalmanFilter
    ExtendedKalmanFilter(model, _as_plant=True).setup()          # what Model._plant_handle builds; raises on a compile error


def test_time_variant_source_compiles(monkeypatch):
    """Every kernel of the plant's handle builds for the time-aware functor (continuous and discrete)."""
    _compile_only(_forced2_model(), monkeypatch)
    d = Model(name='disc', discrete=True)
    d.set_equations("x(k+1) = a*x(k) + sin(t)\ny(k) = x(k) + t")
    _compile_only(d.setup(dt=.5), monkeypatch)


def test_learned_term_in_a_time_variant_model_compiles(monkeypatch):
    """`substitute_from` of a network into a time-variant model is allowed: the learned term is just another expression."""
    from hilo_mpc_amd import ANN, Layer
    m = Model(name='hybrid')
    m.set_equations("dx/dt = -x(t) + mu*sin(t) + u(k)\ny(k) = x(t)")
    ann = ANN(['x'], ['mu'])
    ann.add_layers(Layer.dense(3, activation='tanh'))
    rng = np.random.default_rng(0)
    ann.set_weights([rng.standard_normal((3, 1)), rng.standard_normal((1, 3))], [rng.standard_normal(3), rng.standard_normal(1)])
    m.substitute_from(ann)
    assert m.is_time_variant() and m.parameter_names == []
    _compile_only(m.setup(dt=.5), monkeypatch)


def test_refusals():
    from hilo_mpc_amd import EKF, KF, LMPC, LQR, MHE, NMPC, PF, SMPC, UKF
    m = _forced2_model()
    md = m.discretize('rk4')
    md.setup(dt=.5)
    what = "depends on time explicitly"
    for cls in (NMPC, MHE, EKF, UKF, PF, LMPC):
        with pytest.raises(NotImplementedError, match=f"model 'forced2' {what}"):
            cls(md)
    with pytest.raises(NotImplementedError, match=what):
        LQR(md)
    with pytest.raises(NotImplementedError, match=what):
        SMPC(md, md, np.eye(2))
    lin = Model(name='tvlin')                 # linear in x and u, time-variant: the Kalman filter's own check passes, ours refuses
    lin.set_equations("dx/dt = -x(t) + u(k) + sin(t)\ny(k) = x(t)")
    lin = lin.discretize('erk', 1).setup(dt=.1)
    assert lin.is_linear()
    with pytest.raises(NotImplementedError, match=what):
        KF(lin)
    with pytest.raises(NotImplementedError, match=what):
        LMPC(lin)
    with pytest.raises(NotImplementedError, match=what):
        m.linearize()
    with pytest.raises(NotImplementedError, match=what):
        md.linearization(np.zeros(2), np.zeros(1), [4., .4, 3.])
    with pytest.raises(NotImplementedError, match=what):
        lin.system_matrices()
    dae = Model(name='tvdae')
    x = dae.set_dynamical_states(['x'])
    z = dae.set_algebraic_states(['z'])
    dae.set_dynamical_equations([-x[0] + z[0] + dae.t])
    dae.set_algebraic_equations([z[0] - 2. * x[0]])
    with pytest.raises(NotImplementedError, match="algebraic states and depends on time explicitly"):
        dae.setup(dt=1.)


# ---- plumbing of the start time, against a stand-in for the library ------------------------------------------------------------------
def _stub(monkeypatch, m, n_p, n_y, log):
    """Returns the list that collects (proposals handed in, t0) of every `hilo_model_rollout_resume` call."""
    nx, resumed = m.n_x, []

    class H:
        _dev, _handle, _n_p, _n_y = torch.device('cpu'), 4321, n_p, n_y
    monkeypatch.setattr(m, '_plant_handle', lambda device_index=None: H)
    monkeypatch.setattr('hilo_mpc_amd._device.stream_ptr', lambda dev: 0)

    class Lib:
        @staticmethod
        def hilo_model_rollout(h, opts, B, steps, x0, up, us, ustep, X, Y, stats, stream, hc=None):
            o = opts._obj
            log.append(dict(fn='rollout', B=B, steps=steps, method=o.method, t0=o.t0))
            if hc is not None:                                          # (a stand-in: every call leaves its end time as the proposal)
                hv = np.ctypeslib.as_array(C.cast(hc, C.POINTER(C.c_double)), shape=(B,))
                resumed.append((hv.copy(), o.t0))
                hv[:] = o.t0 + steps * .5
            x = np.ctypeslib.as_array(C.cast(x0, C.POINTER(C.c_double)), shape=(B * nx,)).reshape(B, nx)
            Xo = np.ctypeslib.as_array(C.cast(X, C.POINTER(C.c_double)), shape=((steps + 1) * B * nx,)).reshape(steps + 1, B, nx)
            Yo = np.ctypeslib.as_array(C.cast(Y, C.POINTER(C.c_double)), shape=(steps * B * n_y,))
            Xo[:] = x[None] + np.arange(steps + 1)[:, None, None]       # (a stand-in: every interval adds one)
            Yo[:] = 0.
            if stats is not None:
                np.ctypeslib.as_array(C.cast(stats, C.POINTER(C.c_int32)), shape=(B * 4,))[:] = 0
            return 0

        @staticmethod
        def hilo_model_rollout_resume(h, opts, B, steps, x0, up, us, ustep, X, Y, stats, hc, stream):
            return Lib.hilo_model_rollout(h, opts, B, steps, x0, up, us, ustep, X, Y, stats, stream, hc)

        @staticmethod
        def hilo_pf_function(*a):
            log.append(dict(fn='pf'))
            raise AssertionError("a time-variant model must not be stepped through hilo_pf_function")
    monkeypatch.setattr(_lib, 'lib', lambda: Lib)
    return resumed


def test_sim_opts_mirror_has_t0_last():
    assert _lib.SimOpts._fields_[-1] == ('t0', C.c_double)
    assert _lib.SimOpts().t0 == 0.


@pytest.mark.parametrize('solver', [None, 'dopri5', 'bdf'])
def test_t0_reaches_the_library(monkeypatch, solver):
    m = _forced2_model(**({'solver': solver} if solver else {}))
    log = []
    resumed = _stub(monkeypatch, m, 3, 1, log)
    X0, p = np.zeros((3, 2)), [4., .4, 3.]
    m.rollout(X0, [1.], p, steps=4, t0=2.5)
    assert log[-1] == dict(fn='rollout', B=3, steps=4, method={None: 0, 'dopri5': 1, 'bdf': 2}[solver], t0=2.5)
    m.rollout(X0, [1.], p, steps=4)
    assert log[-1]['t0'] == 0.
    xn, y = m.step(X0, [1.], p, t0=1.25)                      # a one-interval roll-out whatever the solver, never hilo_pf_function
    assert log[-1] == dict(fn='rollout', B=3, steps=1, method={None: 0, 'dopri5': 1, 'bdf': 2}[solver], t0=1.25)
    assert xn.shape == (3, 2) and y.shape == (3, 1)
    m.set_initial_conditions(X0, t0=2.5)
    m.simulate(u=np.ones((3, 1)), p=p, steps=5)
    m.simulate(u=np.ones((3, 1)), p=p, steps=3)
    m.simulate(u=np.ones((3, 1)), p=p)
    assert [(q['steps'], q['t0']) for q in log[-3:]] == [(5, 2.5), (3, 5.), (1, 6.5)]     # each call starts where the last ended
    assert float(np.ravel(m.solution['t:f'])[0]) == 7. and m.solution['x'].shape == (10, 3, 2)
    # under 'dopri5' - and only there - `simulate` hands each call the step-size proposals the call before it left; `rollout` and
    # `step` stand alone
    if solver == 'dopri5':
        assert [t for _, t in resumed] == [2.5, 5., 6.5]
        assert [h.tolist() for h, _ in resumed] == [[0.] * 3, [5.] * 3, [6.5] * 3]
    else:
        assert not resumed
    c = m.copy()
    assert c._sim is None and m._sim['t'][-1] == 7.           # the copy simulates its own trajectory, from its own time
    if solver == 'dopri5':
        m.set_initial_conditions(X0, t0=1.)
        m.simulate(u=np.ones((3, 1)), p=p)
        assert resumed[-1][0].tolist() == [0.] * 3 and resumed[-1][1] == 1.          # new initial conditions: a fresh first step


def test_control_loop_plant_keeps_its_clock(monkeypatch):
    from hilo_mpc_amd import SimpleControlLoop
    m = _forced2_model()
    log = []
    _stub(monkeypatch, m, 3, 1, log)

    class Ctl:
        _model = None

        @staticmethod
        def optimize(x, cp=None, **kw):
            return np.ones((np.atleast_2d(x).shape[0], 1))
    m.set_initial_conditions(np.zeros((2, 2)), t0=2.5)
    loop = SimpleControlLoop(m, Ctl())
    sol = loop.run(3, np.zeros((2, 2)), p=[4., .4, 3.])
    assert [q for q in log] == [dict(fn='rollout', B=2, steps=1, method=0, t0=2.5 + .5 * k) for k in range(3)]
    assert sol['x'].shape == (4, 2, 2) and np.array_equal(sol['x'][-1], np.full((2, 2), 3.))
    loop.run(1, np.zeros((2, 2)), p=[4., .4, 3.])             # a second run goes on with the plant's clock
    assert log[-1]['t0'] == 4.
