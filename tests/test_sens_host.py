"""CPU: the interval function of the roll-out with forward sensitivities (csrc/hilo_integrate.h::dopri5_sens_interval) compiled for
the HOST and run there.  The device runs it with one column per lane on a team of lanes; here the same statements run with every
column in one "lane" and a team of one (`TeamOfOne`), built into tmp_path with `hipcc -x hip --cuda-host-only` like
tests/test_integrate_host.py.  Every sampling instant of the augmented trajectory [x; vec S] is compared with the tight scipy
solution under the bound of tests/sens_reference.py."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import sens_reference as sn
from tests import sim_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'hilo_mpc_amd', 'csrc')
WRT = {'x0': 1, 'u': 2, 'p': 4}

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "hilo_integrate.h"
using namespace hilo;

template <class M>
int run(int argc, char** argv) {
  // argv: model dt steps rtol atol max_steps per_step_inputs wrt x0[NX] then rows of [u; p]
  const double dt = atof(argv[2]);
  const int steps = atoi(argv[3]);
  const double rtol = atof(argv[4]), atol = atof(argv[5]);
  const int max_steps = atoi(argv[6]), per_step = atoi(argv[7]), wrt = atoi(argv[8]);
  constexpr int NX = M::NX, NUP = M::NU + M::NP, NC = NX + NUP;   // every column in the one lane; those behind ns are zero columns
  if (argc != 9 + NX + NUP * (per_step ? steps : 1)) { fprintf(stderr, "bad argument count %d\n", argc); return 2; }
  const int ns = sens_columns<M>(wrt);
  double xv[NX], up[NUP > 0 ? NUP : 1];
  for (int i = 0; i < NX; ++i) xv[i] = atof(argv[9 + i]);
  Dual<NC> x[NX], u[M::NU > 0 ? M::NU : 1], p[M::NP > 0 ? M::NP : 1];
  sens_seed_x<M>(wrt, 0, xv, x);
  SensCarry<NX, NC> c;
  sens_init(c, 0.0);
  const TeamOfOne team;
  for (int k = 0; k < steps; ++k) {
    if (k == 0 || per_step) {
      for (int i = 0; i < NUP; ++i) up[i] = atof(argv[9 + NX + (per_step ? k : 0) * NUP + i]);
      sens_seed_up<M>(wrt, 0, up, u, p);
      c.have_k1 = false;
    }
    const int st = dopri5_sens_interval<M>(c, team, ns, x, u, p, dt, rtol, atol, max_steps);
    printf("x");
    for (int i = 0; i < NX; ++i) printf(" %.17g", st == SIM_OK ? x[i].v : __builtin_nan(""));
    printf("\ns");
    for (int j = 0; j < ns; ++j)
      for (int i = 0; i < NX; ++i) printf(" %.17g", st == SIM_OK ? x[i].d[j] : __builtin_nan(""));
    printf("\n");
  }
  printf("stats %d %d %d %d\n", c.status, c.n_acc, c.n_rej, c.n_rhs);
  return 0;
}

// dx/dt = x^2: leaves every bound at t = 1 / x0
struct Blowup1 {
  static constexpr int NX = 1, NU = 0, NP = 0, NY = 0;
  static constexpr bool DISCRETE = false;
  template <class T, class U, class P>
  HD static void ode(const T* x, const U*, const P*, double, T* dx) { dx[0] = x[0] * x[0]; }
};

int main(int argc, char** argv) {
  if (argc < 9) return 2;
  if (!strcmp(argv[1], "pendulum4")) return run<Pendulum4>(argc, argv);
  if (!strcmp(argv[1], "chemostat4")) return run<Chemostat4>(argc, argv);
  if (!strcmp(argv[1], "blowup1")) return run<Blowup1>(argc, argv);
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
    d = tmp_path_factory.mktemp('sens_host')
    src = d / 'driver.hip'
    src.write_text(DRIVER)
    exe = d / 'driver'
    subprocess.check_call([hipcc, '-x', 'hip', '--cuda-host-only', '-std=c++17', '-O2', '-I', CSRC, str(src), '-o', str(exe)])

    def run(model, groups, x0, up_rows, dt, steps, rtol, atol, max_steps=10000):
        """augmented trajectory [steps + 1, nx (1 + ns)] (row 0: the seed) and (status, accepted, rejected, rhs)"""
        up_rows = np.atleast_2d(np.asarray(up_rows, dtype=float))
        per_step = int(up_rows.shape[0] > 1)
        wrt = sum(WRT[g] for g in groups)
        args = [str(exe), model, repr(float(dt)), str(steps), repr(rtol), repr(atol), str(max_steps), str(per_step), str(wrt)]
        args += [repr(float(v)) for v in x0] + [repr(float(v)) for v in up_rows.ravel()]
        out = subprocess.check_output(args, text=True).strip().split('\n')
        x = np.array([[float(v) for v in ln.split()[1:]] for ln in out if ln.startswith('x ')])
        s = np.array([[float(v) for v in ln.split()[1:]] for ln in out if ln.startswith('s ') or ln == 's'])
        stats = [int(v) for v in out[-1].split()[1:]]
        nx = len(x0)
        seed = np.zeros((s.shape[1] // nx, nx))
        if 'x0' in groups:
            seed[:nx] = np.eye(nx)
        w0 = np.concatenate([np.asarray(x0, dtype=float), seed.ravel()])
        return np.vstack([w0[None], np.hstack([x, s])]), stats
    return run


@pytest.mark.parametrize('rtol,atol', [(1e-6, 1e-8), (1e-8, 1e-10)])
@pytest.mark.parametrize('case', ['chemostat4', 'pendulum4'])
def test_host_compiled_sensitivities_against_tight_solution(driver, case, rtol, atol):
    """All columns (pendulum4: x0 and u, 5; chemostat4: x0, u and p, 10) in one lane."""
    x0, u, p, dt, steps = sr.CASES[case]
    groups = sn.groups_of(sr.oracle_model(case))
    w, (status, n_acc, n_rej, n_rhs) = driver(case, groups, x0, [list(u) + list(p)], dt, steps, rtol, atol)
    e_tight = sn.e_tight_nominal(case, groups, rtol, atol)
    ref, admissible, e45 = sn.bound(case, groups, x0, u, p, dt, steps, rtol, atol, e_tight)
    assert w.shape == ref.shape
    err = sr.rel_err(w, ref, rtol, atol)
    print(f"{case} {groups} rtol={rtol:g}: error {err:.3e}, RK45 {e45:.3e}, DOP853 vs Radau {e_tight:.3e}, "
          f"ratio {err / max(e45, e_tight):.2f}; accepted {n_acc}, rejected {n_rej}, rhs {n_rhs}")
    assert status == 0
    assert n_rhs == 6 * (n_acc + n_rej) + 2            # one augmented evaluation counts as one
    assert err <= admissible


@pytest.mark.parametrize('case', ['chemostat4', 'pendulum4'])
def test_preconditions_of_the_sensitivity_bound(case):
    """What the bound rests on, checked on the references alone: on the augmented system the two tight solutions agree at least 100
    times closer than scipy's RK45 at 1e-8 / 1e-10 is to them."""
    x0, u, p, dt, steps = sr.CASES[case]
    groups = sn.groups_of(sr.oracle_model(case))
    rtol, atol = 1e-8, 1e-10
    e_tight = sn.e_tight_nominal(case, groups, rtol, atol)
    _, _, e45 = sn.bound(case, groups, x0, u, p, dt, steps, rtol, atol, e_tight)
    print(f"{case}: RK45 {e45:.3e}, DOP853 vs Radau {e_tight:.3e}")
    assert e_tight <= e45 / 100.


def test_input_sequence_carries_the_x0_and_p_columns(driver):
    """Inputs that change at every sampling instant: the columns of x0 and p go on across the instants, the kept slope does not."""
    x0, _, p, dt, steps = sr.CASES['chemostat4']
    rng = np.random.default_rng(3)
    U = np.array([.1, .2]) * (1 + .5 * rng.uniform(-1., 1., (steps, 2)))
    groups = ('x0', 'p')
    rtol, atol = 1e-8, 1e-10
    w, stats = driver('chemostat4', groups, x0, np.hstack([U, np.tile(p, (steps, 1))]), dt, steps, rtol, atol)
    e_tight = sn.e_tight_nominal('chemostat4', groups, rtol, atol)
    ref, admissible, e45 = sn.bound('chemostat4', groups, x0, U, p, dt, steps, rtol, atol, e_tight)
    err = sr.rel_err(w, ref, rtol, atol)
    print(f"chemostat4, input sequence, {groups}: error {err:.3e}, RK45 {e45:.3e}, ratio {err / max(e45, e_tight):.2f}")
    assert stats[0] == 0 and stats[3] == 6 * (stats[1] + stats[2]) + steps + 1   # a first slope per interval, one first-step estimate
    assert err <= admissible


def test_failure_ends_the_instance_and_its_columns(driver):
    """dx/dt = x^2 from 1 over [0, 2] with at most 50 attempted steps per interval: the solution 1 / (1 - t) leaves at t = 1, and
    dx/dx0 = 1 / (1 - t)^2 with it.  A non-zero status, and NaN in S exactly where it is in x."""
    w, stats = driver('blowup1', ('x0',), [1.], [[]], .25, 8, 1e-8, 1e-10, 50)
    assert stats[0] != 0 and stats[1] + stats[2] <= 8 * 50
    t = .25 * np.arange(9)
    x, S = w[:, 0], w[:, 1]
    np.testing.assert_array_equal(np.isnan(S), np.isnan(x))
    assert np.all(np.isfinite(x[t < 1.])) and np.all(np.isnan(x[t > 1.]))
    np.testing.assert_allclose(x[t < 1.], 1. / (1. - t[t < 1.]), rtol=1e-6)
    np.testing.assert_allclose(S[t < 1.], 1. / (1. - t[t < 1.]) ** 2, rtol=1e-6)
