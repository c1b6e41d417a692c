"""CPU: the DAE integrator of csrc/hilo_integrate.h (`idas_interval`, solver='idas') compiled for the HOST and run there, and the
host-side contract of `Model.setup(solver='idas')`.

A stand-alone driver around `idas_interval<M>` is built with `hipcc -x hip --cuda-host-only` like the one of
tests/test_bdf_host.py; its store is a heap array of exactly `bdf_entries(NX + NZ)` doubles.  The functors - lin1, Robertson's
kinetics with the conservation law as algebraic equation, alg_u - are hand-written in the driver.  Every sampling instant of x and
of z is compared with the tight solution of the reduced equation under the rule of tests/dae_reference.py."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from hilo_mpc_amd import Model, _lib
from tests import dae_reference as dr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'hilo_mpc_amd', 'csrc')
TOLS = [(1e-6, 1e-8), (1e-9, 1e-11)]
HOST_CASES = ['alg_u', 'lin1', 'robertson_dae', 'robertson_dae_long']

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "hilo_integrate.h"
using namespace hilo;

template <class M>
int run(int argc, char** argv) {
  // argv: model dt steps rtol atol max_steps per_step_inputs x0[NX] z0[NZ] then rows of [u; p]
  // per_step_inputs: 0 held, 1 one row per interval and a restart at every instant
  constexpr int NX = M::NX, NZ = M::NZ, N = NX + NZ, NUP = M::NU + M::NP;
  const double dt = atof(argv[2]);
  const int steps = atoi(argv[3]);
  const double rtol = atof(argv[4]), atol = atof(argv[5]);
  const int max_steps = atoi(argv[6]), per_step = atoi(argv[7]);
  if (argc != 8 + N + NUP * (per_step ? steps : 1)) { fprintf(stderr, "bad argument count %d\n", argc); return 2; }
  double w[N], up[NUP > 0 ? NUP : 1];
  for (int i = 0; i < N; ++i) w[i] = atof(argv[8 + i]);
  // exactly the doubles the integrator may touch, on the heap: an index outside them is the sanitizer's to find
  double* store = (double*)malloc(sizeof(double) * bdf_entries(N));
  const BdfMem<N, 1, double*> mem = {store};
  BdfCarry<N> c;
  bdf_init(c, per_step ? dt : steps * dt);
  for (int k = 0; k < steps; ++k) {
    if (k == 0 || per_step) {
      for (int i = 0; i < NUP; ++i) up[i] = atof(argv[8 + N + (per_step ? k : 0) * NUP + i]);
      if (k > 0) bdf_restart(c, dt);
    }
    if (k == 0) {
      const int s0 = idas_start<M>(c, mem, w, up, up + M::NU, rtol, atol, 0.0);
      printf("w");
      for (int i = 0; i < N; ++i) printf(" %.17g", s0 == SIM_OK || i < NX ? w[i] : __builtin_nan(""));
      printf("\n");
    }
    const int st = idas_interval<M>(c, mem, w, up, up + M::NU, per_step ? dt : (k + 1) * dt, rtol, atol, 0.0, max_steps);
    printf("w");
    for (int i = 0; i < N; ++i) printf(" %.17g", st == SIM_OK ? w[i] : __builtin_nan(""));
    printf("\n");
  }
  printf("stats %d %d %d %d %d %d\n", c.status, c.n_acc, c.n_rej, c.n_rhs, c.n_jac, c.n_lu);
  free(store);
  return 0;
}

#define DAE_FUN(name, out) template <class T, class P> HD static void name(const T* x, const T* z, const T* u, const P* p, T* out)

// x' = -x + z, 0 = z - 2 x
struct Lin1 {
  static constexpr int NX = 1, NZ = 1, NU = 0, NP = 0, NY = 0;
  static constexpr bool DISCRETE = false;
  DAE_FUN(ode_z, dx) { (void)u; (void)p; dx[0] = -1.0 * x[0] + z[0]; }
  DAE_FUN(alg, r) { (void)u; (void)p; r[0] = z[0] - 2.0 * x[0]; }
};
// Robertson's kinetics with the conservation law as algebraic equation, p = (k1, k2, k3)
struct RobertsonDae {
  static constexpr int NX = 2, NZ = 1, NU = 0, NP = 3, NY = 0;
  static constexpr bool DISCRETE = false;
  DAE_FUN(ode_z, dx) {
    (void)u;
    dx[0] = -1.0 * (p[0] * x[0]) + p[2] * x[1] * z[0];
    dx[1] = p[0] * x[0] - p[2] * x[1] * z[0] - p[1] * x[1] * x[1];
  }
  DAE_FUN(alg, r) { (void)u; (void)p; r[0] = x[0] + x[1] + z[0] - 1.0; }
};
// two coupled algebraic states, the first equation names the input
struct AlgU {
  static constexpr int NX = 2, NZ = 2, NU = 1, NP = 0, NY = 0;
  static constexpr bool DISCRETE = false;
  DAE_FUN(ode_z, dx) { (void)u; (void)p; dx[0] = -1.0 * x[0] + z[0]; dx[1] = z[1] - x[1]; }
  DAE_FUN(alg, r) { (void)p; r[0] = z[0] - x[0] * z[1] - u[0]; r[1] = z[1] + 0.5 * sin(z[0]) - x[1]; }
};
// 0 = z^2 - p: no root for p < 0
struct NoRoot {
  static constexpr int NX = 1, NZ = 1, NU = 0, NP = 1, NY = 0;
  static constexpr bool DISCRETE = false;
  DAE_FUN(ode_z, dx) { (void)u; (void)p; dx[0] = -1.0 * x[0] + z[0]; }
  DAE_FUN(alg, r) { (void)u; r[0] = z[0] * z[0] - p[0] + 0.0 * x[0]; }
};

int main(int argc, char** argv) {
  if (argc < 8) return 2;
  if (!strcmp(argv[1], "lin1")) return run<Lin1>(argc, argv);
  if (!strcmp(argv[1], "robertson_dae")) return run<RobertsonDae>(argc, argv);
  if (!strcmp(argv[1], "alg_u")) return run<AlgU>(argc, argv);
  if (!strcmp(argv[1], "noroot")) return run<NoRoot>(argc, argv);
  return 2;
}
"""


def _hipcc():
    for c in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', shutil.which('hipcc')):
        if c and os.path.exists(c):
            return c
    return None


def _runner(exe):
    def run(model, x0, z0, up_rows, dt, steps, rtol, atol, max_steps=10000):
        up_rows = np.atleast_2d(np.asarray(up_rows, dtype=float))
        per_step = int(up_rows.shape[0] > 1)
        args = [str(exe), model, repr(float(dt)), str(steps), repr(rtol), repr(atol), str(max_steps), str(per_step)]
        args += [repr(float(v)) for v in list(x0) + list(z0)] + [repr(float(v)) for v in up_rows.ravel()]
        out = subprocess.check_output(args, text=True, stderr=subprocess.STDOUT).strip().split('\n')
        w = np.array([[float(v) for v in ln.split()[1:]] for ln in out if ln.startswith('w')])
        stats = [int(v) for v in out[-1].split()[1:]]
        return w[:, :len(x0)], w[:, len(x0):], stats
    return run


@pytest.fixture(scope='module')
def build_dir(tmp_path_factory):
    if _hipcc() is None:
        pytest.skip('hipcc not available')
    d = tmp_path_factory.mktemp('idas_host')
    (d / 'driver.hip').write_text(DRIVER)
    return d


@pytest.fixture(scope='module')
def driver(build_dir):
    exe = build_dir / 'driver'
    subprocess.check_call([_hipcc(), '-x', 'hip', '--cuda-host-only', '-std=c++17', '-O2', '-I', CSRC, str(build_dir / 'driver.hip'),
                           '-o', str(exe)])
    return _runner(exe)


def _alg_u_sequence():
    x0, _, p, dt, steps = dr.CASES['alg_u']
    return x0, dr.sequence('alg_u', steps), p, dt, steps


@pytest.fixture(scope='module')
def refs():
    """Every reference of this module, once, in worker processes: the held cases (per tolerance) and the input sequence of alg_u."""
    jobs = [(case,) + tuple(dr.CASES[case]) + (TOLS,) for case in HOST_CASES]
    jobs.append(('alg_u',) + _alg_u_sequence() + (TOLS,))
    res = dr.run_jobs(jobs)
    return dict(zip(HOST_CASES, res[:-1])), res[-1]


def _name(case):
    return 'robertson_dae' if case.startswith('robertson_dae') else case


@pytest.mark.parametrize('i_tol', [0, 1])
@pytest.mark.parametrize('case', HOST_CASES)
def test_host_compiled_idas_against_the_tight_solution(driver, refs, case, i_tol):
    rtol, atol = TOLS[i_tol]
    x0, u, p, dt, steps = dr.CASES[case]
    b = refs[0][case][i_tol]
    x, z, (status, n_acc, n_rej, n_rhs, n_jac, n_lu) = driver(_name(case), x0, [0.] * dr.NZ[_name(case)], [list(u) + list(p)], dt, steps,
                                                             rtol, atol)
    ex, ez, ratio = dr.check(case, x, z, b, rtol, atol)
    res = dr.residual(case, x, z, u, p, steps)
    print(f"{case} rtol={rtol:g}: error x {ex:.3e} (BDF {b['e_bdf_x']:.3e}, tight {b['e_tight_x']:.3e}), z {ez:.3e} (BDF "
          f"{b['e_bdf_z']:.3e}, tight {b['e_tight_z']:.3e}), ratio {ratio:.3f}; residual {res:.1e}; accepted {n_acc}, rejected {n_rej}, "
          f"rhs {n_rhs}, Jacobians {n_jac}, factorisations {n_lu}; scipy steps {b['counts'][0]}, nfev {b['counts'][1]}")
    assert status == 0
    assert ex <= b['adm_x'] and ez <= b['adm_z']
    assert res <= 1e-10
    if case == 'lin1':      # the exact answer: x = e^t, z = 2 e^t
        t = dt * np.arange(steps + 1)
        assert np.max(np.abs(x[:, 0] - np.exp(t)) / np.exp(t)) <= 100. * rtol
        np.testing.assert_allclose(z, 2. * x, rtol=1e-12)


@pytest.mark.parametrize('i_tol', [0, 1])
def test_input_sequence_restarts_with_a_consistent_start(driver, refs, i_tol):
    """g names the input: z jumps at every sampling instant, and each interval starts from the z of the previous instant."""
    rtol, atol = TOLS[i_tol]
    x0, U, p, dt, steps = _alg_u_sequence()
    b = refs[1][i_tol]
    x, z, stats = driver('alg_u', x0, [0., 0.], U, dt, steps, rtol, atol)
    ex, ez, ratio = dr.check('alg_u', x, z, b, rtol, atol)
    res = dr.residual('alg_u', x, z, U, p, steps)
    print(f"alg_u sequence rtol={rtol:g}: error x {ex:.3e}, z {ez:.3e}, ratio {ratio:.3f}, residual {res:.1e}; steps {stats[1]} : "
          f"{b['counts'][0]}, rhs {stats[3]} : {b['counts'][1]}")
    assert stats[0] == 0 and ex <= b['adm_x'] and ez <= b['adm_z'] and res <= 1e-10


def test_failures_end_the_instance(driver):
    # no root of the algebraic equation: status 3 before the first step; x row 0 stands, everything else is NaN
    x, z, stats = driver('noroot', [1.], [1.], [[-1.]], .2, 3, 1e-6, 1e-8)
    assert stats[0] == 3 and stats[1] == 0
    assert x[0, 0] == 1. and np.isnan(x[1:]).all() and np.isnan(z).all()
    x, z, stats = driver('noroot', [1.], [1.], [[4.]], .2, 3, 1e-6, 1e-8)
    assert stats[0] == 0 and np.allclose(z, 2.)
    # max_steps binds between two sampling instants
    x0, u, p, dt, steps = dr.CASES['robertson_dae']
    x, z, stats = driver('robertson_dae', x0, [0.], [p], dt, steps, 1e-6, 1e-8, 3)
    assert stats[0] == 1 and stats[1] + stats[2] <= 3
    bad = np.isnan(x[:, 0])
    assert bad[-1] and not bad[0] and np.all(np.diff(bad.astype(int)) >= 0) and np.array_equal(bad, np.isnan(z[:, 0]))


def test_a_far_start_of_the_newton_iteration_still_converges(driver):
    x0, u, p, dt, steps = dr.CASES['lin1']
    a = driver('lin1', x0, [0.], [[]], dt, steps, 1e-6, 1e-8)
    b = driver('lin1', x0, [1e3], [[]], dt, steps, 1e-6, 1e-8)
    np.testing.assert_allclose(b[0], a[0], rtol=1e-12)


def test_driver_under_address_and_undefined_behaviour_sanitizers(build_dir, refs):
    """The same driver as a stand-alone program with -fsanitize=address,undefined on the host: the indexing of the difference
    table and of the pivot rows, on a store of exactly bdf_entries(NX + NZ) doubles."""
    exe = build_dir / 'driver_san'
    r = subprocess.run([_hipcc(), '-x', 'hip', '--cuda-host-only', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
                        '-fno-sanitize-recover=undefined', '-I', CSRC, str(build_dir / 'driver.hip'), '-o', str(exe)],
                       capture_output=True, text=True)
    if r.returncode != 0:
        # only a missing sanitizer runtime is a reason to skip (the `driver` fixture builds the same source without it): the linker
        # names the library it cannot find
        missing = any(w in r.stderr for w in ('clang_rt.asan', 'clang_rt.ubsan', 'libclang_rt', 'cannot find -lasan', 'cannot find -lubsan'))
        assert missing, r.stderr[-2000:]
        pytest.skip('the sanitizer runtime does not link with this toolchain: ' + r.stderr.strip().split('\n')[-1])
    run = _runner(exe)
    rtol, atol = TOLS[1]
    for case in ('robertson_dae', 'alg_u'):
        x0, u, p, dt, steps = dr.CASES[case]
        x, z, stats = run(case, x0, [0.] * dr.NZ[case], [list(u) + list(p)], dt, steps, rtol, atol)     # (a report ends the program)
        b = refs[0][case][1]
        ex, ez, _ = dr.check(case, x, z, b, rtol, atol)
        assert stats[0] == 0 and ex <= b['adm_x'] and ez <= b['adm_z']
    x0, U, p, dt, steps = _alg_u_sequence()
    x, z, stats = run('alg_u', x0, [0., 0.], U, dt, steps, rtol, atol)
    ex, ez, _ = dr.check('alg_u', x, z, refs[1][1], rtol, atol)
    assert stats[0] == 0 and ex <= refs[1][1]['adm_x'] and ez <= refs[1][1]['adm_z']


# ---- host logic, against a stand-in for hilo_model_rollout_dae that reads its pointer arguments as the header declares them -----------
def _arr(ptr, n, typ=C.c_double):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(typ)), shape=(n,))


def _lin1_model(**kw):
    m = Model(name='lin1')
    x = m.set_dynamical_states(['x'])
    z = m.set_algebraic_states(['z'])
    m.set_dynamical_equations([-x[0] + z[0]])
    m.set_algebraic_equations([z[0] - 2. * x[0]])
    m.set_measurement_equations([x[0] + z[0]])
    return m.setup(**kw) if kw else m


def _stub(monkeypatch, m, log):
    """x+ = x e^dt, z = 2 x (+ what the caller's z0 was off by, so that the start value shows in the result), y = x + z."""
    class H:
        _dev, _handle, _n_p, _n_y = torch.device('cpu'), 4321, 0, 1
    monkeypatch.setattr(m, '_plant_handle', lambda device_index=None: H)
    monkeypatch.setattr('hilo_mpc_amd._device.stream_ptr', lambda dev: 0)

    class Lib:
        @staticmethod
        def hilo_model_rollout(*a):
            pytest.fail("an 'idas' model goes through hilo_model_rollout_dae")

        @staticmethod
        def hilo_model_rollout_dae(h, opts, B, steps, x0, z0, up, us, ustep, X, Z, Y, stats, stream):
            o = opts._obj
            z0v = None if not z0 else _arr(z0, B).copy()
            log.append(dict(h=h, B=B, steps=steps, us=us, ustep=ustep, method=o.method, max_steps=o.max_steps, rtol=o.rtol,
                            atol=o.atol, h0=o.h0, stats=stats is not None, z0=z0v, Z=bool(Z), up=bool(up)))
            x = _arr(x0, B).copy()
            Xo, Yo = _arr(X, (steps + 1) * B).reshape(steps + 1, B, 1), _arr(Y, steps * B).reshape(steps, B, 1)
            for k in range(steps + 1):
                Xo[k, :, 0] = x * np.exp(m.dt * k)
            Yo[:] = 3. * Xo[1:]
            if Z:
                Zo = _arr(Z, (steps + 1) * B).reshape(steps + 1, B, 1)
                Zo[:] = 2. * Xo
            if stats is not None:
                _arr(stats, B * 4, C.c_int32).reshape(B, 4)[:] = [0, 7, 1, 50]
            return 0
    monkeypatch.setattr(_lib, 'lib', lambda: Lib)


def test_idas_reaches_the_library_as_method_3(monkeypatch):
    m = _lin1_model(dt=.2, solver='idas', solver_options={'reltol': 1e-8, 'abstol': 1e-10, 'max_num_steps': 500, 'first_step': 1e-3})
    log = []
    _stub(monkeypatch, m, log)
    X0 = np.array([[1.], [2.], [3.]])
    x, y, z, stats = m.rollout(X0, steps=3, z0=[[5.]], return_z=True, return_stats=True)
    q = log[-1]
    assert {k: q[k] for k in ('h', 'B', 'steps', 'us', 'ustep', 'method', 'max_steps', 'rtol', 'atol', 'h0', 'stats', 'Z', 'up')} == dict(
        h=4321, B=3, steps=3, us=0, ustep=0, method=3, max_steps=500, rtol=1e-8, atol=1e-10, h0=1e-3, stats=True, Z=True, up=False)
    np.testing.assert_array_equal(q['z0'], [5., 5., 5.])              # one row for the batch
    assert x.shape == (4, 3, 1) and y.shape == (3, 3, 1) and z.shape == (4, 3, 1) and isinstance(z, np.ndarray)
    np.testing.assert_allclose(z, 2. * x)
    assert sorted(stats) == ['n_accepted', 'n_rejected', 'n_rhs', 'status']
    x, y = m.rollout(X0, steps=2, z0=np.array([[1.], [2.], [3.]]))
    np.testing.assert_array_equal(log[-1]['z0'], [1., 2., 3.])
    assert not log[-1]['Z'] and not log[-1]['stats']
    m.rollout(X0, steps=2)
    assert log[-1]['z0'] is None
    xt, yt, zt = m.rollout(torch.as_tensor(X0), steps=2, return_z=True)
    assert all(isinstance(v, torch.Tensor) for v in (xt, yt, zt)) and zt.shape == (3, 3, 1)
    xn, yn = m.step(X0)                                                # a one-interval roll-out
    assert log[-1]['steps'] == 1 and log[-1]['method'] == 3 and xn.shape == (3, 1) and yn.shape == (3, 1)
    d = _lin1_model(dt=.5, solver='idas')
    assert d._solver_options == {'reltol': 1e-6, 'abstol': 1e-8, 'max_num_steps': 10000, 'first_step': 0.}
    assert d.setup(dt=.25)._solver == 'idas'
    with pytest.raises(ValueError, match="a z0 of 2 rows does not match 3 states"):
        m.rollout(X0, steps=2, z0=np.zeros((2, 1)))


@pytest.mark.parametrize('B', [1, 3])
def test_simulate_under_idas_fills_the_solution(monkeypatch, B):
    m = _lin1_model(dt=.2, solver='idas')
    log = []
    _stub(monkeypatch, m, log)
    X0 = np.arange(1., B + 1.)[:, None]
    m.set_initial_conditions(X0, 0., z0=np.full((B, 1), 7.))
    m.simulate(steps=4)
    np.testing.assert_array_equal(log[-1]['z0'], [7.] * B)            # the caller's start of the Newton iteration
    assert log[-1]['method'] == 3 and log[-1]['Z'] and log[-1]['stats'] and log[-1]['steps'] == 4
    m.simulate(tf=.4)
    np.testing.assert_allclose(log[-1]['z0'], 2. * X0[:, 0] * np.exp(.8))    # the second call starts from the stored z
    sol = m.solution
    if B == 1:
        assert sol['x'].shape == (1, 7) and sol['z'].shape == (1, 7) and sol['z:f'].shape == (1, 1) and sol['y'].shape == (1, 6)
    else:
        assert sol['x'].shape == (7, 3, 1) and sol['z'].shape == (7, 3, 1) and sol['z:f'].shape == (3, 1)
    np.testing.assert_allclose(sol['z'], 2. * sol['x'])
    assert sol['status'].shape == (2, B) and sol['t:f'] == pytest.approx(1.2)
    n = _lin1_model(dt=.2, solver='idas')
    _stub(monkeypatch, n, log)
    n.set_initial_conditions(X0)
    n.simulate(steps=1)
    assert log[-1]['z0'] is None                                        # no z0: the model's guess, chosen by the library


def test_control_loop_carries_the_algebraic_states(monkeypatch):
    """The plant of a SimpleControlLoop under 'idas': the first interval of a run starts the Newton iteration at the model's guess,
    every later one at the z the interval before it ended with."""
    from hilo_mpc_amd import SimpleControlLoop

    class Constant:
        def call(self, x=None, p=None):
            return None
    m = _lin1_model(dt=.2, solver='idas')
    log = []
    _stub(monkeypatch, m, log)
    loop = SimpleControlLoop(m, Constant())
    X0 = np.array([[1.], [2.]])
    sol = loop.run(3, X0)
    assert [q['steps'] for q in log] == [1, 1, 1] and all(q['Z'] for q in log) and log[0]['z0'] is None
    np.testing.assert_allclose(log[1]['z0'], 2. * sol['x'][1, :, 0])
    np.testing.assert_allclose(log[2]['z0'], 2. * sol['x'][2, :, 0])
    np.testing.assert_allclose(sol['x'][:, :, 0], X0[:, 0] * np.exp(.2 * np.arange(4))[:, None])
    loop.run(1, X0)
    assert log[-1]['z0'] is None                                        # a new run starts afresh


def test_idas_refusals():
    with pytest.raises(RuntimeError, match="Solver 'idas' integrates a model with algebraic states; model 'chemostat4' has none. Use 'bdf'"):
        Model('chemostat4').setup(dt=1., solver='idas')
    with pytest.raises(RuntimeError, match="Model is discrete. No solver is required."):
        Model('toy1d').setup(dt=1., solver='idas')
    wide = Model(name='wide9')
    x = wide.set_dynamical_states([f'x{i}' for i in range(6)])
    z = wide.set_algebraic_states(['a', 'b', 'c'])
    wide.set_dynamical_equations([-x[i] + z[i % 3] for i in range(6)])
    wide.set_algebraic_equations([z[i] - x[i] for i in range(3)])
    with pytest.raises(NotImplementedError, match="at most 8 differential and algebraic states together; model 'wide9' has 6 \\+ 3"):
        wide.setup(dt=1., solver='idas')
    wide.setup(dt=1.)                                                  # the fixed-step map has no such limit
    with pytest.raises(ValueError, match="Unknown option 'rtol' for solver 'idas'"):
        _lin1_model(dt=1., solver='idas', solver_options={'rtol': 1e-8})
    # the messages that point at 'idas' stay as they are
    with pytest.raises(RuntimeError, match="Solver 'bdf' is not suitable for DAE systems. Use 'idas' or 'collocation' instead"):
        _lin1_model(dt=1., solver='bdf')
    with pytest.raises(ValueError, match="Solver 'cvodes' is not available on your system. Use 'dopri5' instead, or 'bdf' for a stiff model"):
        _lin1_model(dt=1., solver='cvodes')
    for m in (Model('chemostat4').setup(dt=1., solver='bdf'), _lin1_model(dt=1.)):
        with pytest.raises(ValueError, match="z0 and return_z belong to solver='idas'"):
            m.rollout(np.zeros((1, m.n_x)), np.zeros(m.n_u), np.zeros(m.n_p), z0=[[0.]])
        with pytest.raises(ValueError, match="z0 and return_z belong to solver='idas'"):
            m.rollout(np.zeros((1, m.n_x)), np.zeros(m.n_u), np.zeros(m.n_p), return_z=True)


def test_dae_rollout_symbol_is_exported_and_checks_its_arguments():
    lib = _lib.lib()
    assert hasattr(lib, 'hilo_model_rollout_dae') and lib.hilo_abi_version() == 1
    rc = lib.hilo_model_rollout_dae(None, None, 1, 1, None, None, None, 0, 0, None, None, None, None, None)
    assert rc == -1 and b'hilo_model_rollout_dae: NULL handle' in lib.hilo_last_error()


def test_header_constants_match_the_host_table(tmp_path):
    if shutil.which('gcc') is None:
        pytest.skip('gcc not available')
    src = tmp_path / 'probe.c'
    src.write_text('#include <stdio.h>\n#include "hilo_hip.h"\nint main(void) {\n  printf("%d %d %d %d\\n", HILO_SIM_IDAS, '
                   'HILO_SIM_STATUS_IC_FAILED, HILO_SIM_BDF_MAX_NX, (int)sizeof(hilo_sim_opts));\n  return 0;\n}\n')
    exe = tmp_path / 'probe'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    idas, ic, width, size = (int(v) for v in subprocess.check_output([str(exe)], text=True).split())
    from hilo_mpc_amd.model import IDAS_MAX_STATES, SOLVERS
    assert idas == SOLVERS['idas'] == 3 and ic == 3 and width == IDAS_MAX_STATES and size == C.sizeof(_lib.SimOpts)
