"""PID without a device wherever that is possible: the getters, setters and messages of the reference's tests/test_PID.py restated for
`hilo_mpc_amd.PID`; the law and the closed-loop body of csrc/hilo_pid.h compiled for the HOST (into tmp_path with
`hipcc -x hip --cuda-host-only`, like tests/test_sens_host.py) and compared with the numpy restatement of tests/pid_reference.py; the
refusals of `PID.closed_loop` that are decided before anything is launched.  `PID.call` itself runs a kernel, so the reference's two
known answers are checked twice: through the host build of `pid_update` here, and through `call` under the `gpu` mark."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from hilo_mpc_amd import PID, Model
from tests import pid_reference as pr
from tests import sim_reference as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'hilo_mpc_amd', 'csrc')
COUPLED = ("The number of set points is greater than 1, but the supplied matrix for {} is not a diagonal matrix. "
           "Coupled multi-variable control is not supported at the moment.")


# ---- the surface of the reference (tests/test_PID.py) ----------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2])
def test_initial_tuning_parameters_and_set_point(n):
    pid = PID(n_set_points=n, plot_backend='bokeh')
    np.testing.assert_equal(pid.k_p, np.eye(n))
    np.testing.assert_equal(pid.t_i, np.diag(np.inf * np.ones(n)))
    np.testing.assert_equal(pid.k_i, np.zeros((n, n)))
    np.testing.assert_equal(pid.t_d, np.zeros((n, n)))
    np.testing.assert_equal(pid.k_d, np.zeros((n, n)))
    np.testing.assert_allclose(pid.set_point, np.zeros((n, 1)))
    assert pid.type == 'PID'
    np.testing.assert_equal(pid.proportional_gain, pid.k_p)
    np.testing.assert_equal(pid.integral_time, pid.t_i)
    np.testing.assert_equal(pid.derivative_time, pid.t_d)


def test_is_set_up():
    pid = PID(plot_backend='bokeh')
    assert not pid.is_setup()
    pid.setup(dt=.01)
    assert pid.is_setup()


def test_setters_single_set_point():
    pid = PID(plot_backend='bokeh')
    pid.k_p = 2
    np.testing.assert_equal(pid.k_p, np.array([[2.]]))
    pid.k_p = 1
    pid.t_i = .1
    np.testing.assert_equal(pid.t_i, np.array([[.1]]))
    np.testing.assert_equal(pid.k_i, np.array([[10.]]))
    pid.t_d = 10.
    np.testing.assert_equal(pid.t_d, np.array([[10.]]))
    np.testing.assert_equal(pid.k_d, np.array([[10.]]))


@pytest.mark.parametrize('which,label,value', [('k_p', 'K_P', 2.), ('t_i', 'T_I', .1), ('t_d', 'T_D', 2.)])
def test_a_scalar_for_several_set_points_is_a_coupled_matrix(which, label, value):
    pid = PID(n_set_points=2, plot_backend='bokeh')
    with pytest.raises(ValueError) as e:
        setattr(pid, which, value)
    assert str(e.value) == COUPLED.format(label)


@pytest.mark.parametrize('which,value', [('k_p', 2.), ('t_i', .1), ('t_d', 10.)])
def test_setters_multiple_set_points(which, value):
    pid = PID(n_set_points=2, plot_backend='bokeh')
    setattr(pid, which, [value, value])
    np.testing.assert_equal(getattr(pid, which), value * np.eye(2))
    setattr(pid, which, value * np.eye(2))
    np.testing.assert_equal(getattr(pid, which), value * np.eye(2))


def test_set_point_setter():
    pid = PID(plot_backend='bokeh')
    pid.setup(dt=.01)
    pid.set_point = 1.
    np.testing.assert_allclose(pid.set_point, np.array([[1.]]))
    pid = PID(n_set_points=3, plot_backend='bokeh')
    pid.setup(dt=.01)
    pid.set_point = 1.
    np.testing.assert_allclose(pid.set_point, np.ones((3, 1)))
    pid = PID(n_set_points=2, plot_backend='bokeh')
    pid.setup(dt=.01)
    pid.set_point = [1., 1.]
    np.testing.assert_allclose(pid.s_p, np.ones((2, 1)))
    pid = PID(n_set_points=4, plot_backend='bokeh')
    pid.setup(dt=.01)
    with pytest.raises(ValueError) as e:
        pid.set_point = [1., 1., 1.]
    assert str(e.value) == "Dimension mismatch. Supplied dimension for the set point is 3x1, but required dimension is 4x1."


@pytest.mark.parametrize('kw,letters', [({}, 'P'), ({'t_i': .1}, 'PI'), ({'t_d': 10.}, 'PD'), ({'t_i': .1, 't_d': 10.}, 'PID')])
def test_call_before_setup(kw, letters):
    pid = PID(plot_backend='bokeh', **kw)
    with pytest.raises(RuntimeError) as e:
        pid.call()
    assert str(e.value) == f"{letters} controller is not set up. Run PID.setup() before calling the {letters} controller"


def test_per_instance_gains_and_set_points_are_kept_as_given():
    kp = np.linspace(1., 2., 6).reshape(3, 2)
    pid = PID(n_set_points=2, k_p=kp, t_i=2 * kp)
    np.testing.assert_equal(pid.k_p, kp)
    np.testing.assert_allclose(np.asarray(pid.k_i), np.full((3, 2), .5))
    pid.set_point = np.ones((3, 2))
    assert pid.set_point.shape == (3, 2)


def test_output_limits_are_checked():
    with pytest.raises(ValueError, match='must not exceed'):
        PID(output_limits=(1., 0.))
    with pytest.raises(ValueError, match='pair'):
        PID(output_limits=(1., 2., 3.))
    assert PID(n_set_points=2, output_limits=(0., [1., 2.])).output_limits[1].tolist() == [1., 2.]


@pytest.mark.gpu
@pytest.mark.parametrize('n', [1, 2])
def test_known_answers_of_the_reference_through_call(n):
    """tests/test_PID.py:272-298 of the reference: k_p 8, t_i 1, dt .01, set point 1."""
    pid = PID(n_set_points=n, k_p=n * [8.], t_i=n * [1.], plot_backend='bokeh')
    pid.setup(dt=.01)
    pid.set_point = 1.
    np.testing.assert_allclose(pid.call(), np.full((n, 1), 8.08))
    np.testing.assert_allclose(pid.call(pv=.1), np.full((n, 1), 7.352))
    pid.reset()
    np.testing.assert_allclose(pid.call(), np.full((n, 1), 8.08))


# ---- the refusals of closed_loop that need no device ------------------------------------------------------------------------------
def test_closed_loop_refusals():
    plant = Model('linear2')
    pid = PID(k_p=1., t_i=2.)
    x0, p = np.zeros((1, 2)), np.ones((1, 2))
    with pytest.raises(RuntimeError, match=r"PI controller is not set up. Run PID.setup\(\)"):
        pid.closed_loop(plant, x0, p=p)
    pid.setup(dt=.25)
    with pytest.raises(RuntimeError, match=r"Model is not set up. Run Model.setup\(\)"):
        pid.closed_loop(plant, x0, p=p)
    plant.setup(dt=.5)
    with pytest.raises(ValueError, match=r"Run PID.setup\(dt=0.5\)"):
        pid.closed_loop(plant, x0, p=p)
    for solver in ('bdf', 'idas'):
        stiff = Model('linear2')
        stiff.setup(dt=.25)
        stiff._solver = solver            # (what setup(solver=...) records; 'idas' itself wants a model with algebraic states)
        with pytest.raises(NotImplementedError, match=r"Model.setup\(solver='dopri5'\)"):
            pid.closed_loop(stiff, x0, p=p)
    plant.setup(dt=.25)
    with pytest.raises(ValueError, match="Use a PID with at most 1 set points"):
        PID(n_set_points=2).setup(dt=.25).closed_loop(plant, x0, p=p)
    with pytest.raises(ValueError, match=r"no measurement or state 'z'. Choose out of the measurements \['y'\] or the states \['x_1', 'x_2'\]"):
        pid.closed_loop(plant, x0, p=p, process_values=['z'])
    with pytest.raises(ValueError, match=r"no input 'v'. Choose out of \['u'\]"):
        pid.closed_loop(plant, x0, p=p, outputs=['v'])
    chem = Model('chemostat4')
    chem.setup(dt=1.)
    two = PID(n_set_points=2).setup(dt=1.)
    with pytest.raises(ValueError, match=r"\['X'\] used twice"):
        two.closed_loop(chem, np.zeros((1, 4)), p=np.ones((1, 4)), process_values=['X', 'X'])
    with pytest.raises(ValueError, match=r"\['DS'\] used twice"):
        two.closed_loop(chem, np.zeros((1, 4)), p=np.ones((1, 4)), outputs=['DS', 'DS'])
    one = PID().setup(dt=1.)
    with pytest.raises(ValueError, match=r"name the 1 controlled ones with process_values"):
        one.closed_loop(chem, np.zeros((1, 4)), p=np.ones((1, 4)), outputs=['DS'])
    with pytest.raises(ValueError, match=r"name the 1 driven ones with outputs"):
        one.closed_loop(chem, np.zeros((1, 4)), p=np.ones((1, 4)), process_values=['X'])
    with pytest.raises(ValueError, match=r"set-point schedule holds \[3, 1, 1\] values for 5 sampling intervals"):
        pid.closed_loop(plant, x0, p=p, steps=5, set_point=np.ones((3, 1, 1)))
    five = PID(n_set_points=5)
    with pytest.raises(ValueError, match="built for up to 4 loops"):
        five.setup(dt=.25).closed_loop(plant, x0, p=p)


# ---- csrc/hilo_pid.h compiled for the host -----------------------------------------------------------------------------------------
DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "hilo_pid.h"
#include "hilo_kf_params.h"
using namespace hilo;

static double next(FILE* f) {
  double v;
  if (fscanf(f, "%lf", &v) != 1) { fprintf(stderr, "short input\n"); exit(2); }
  return v;
}
static void dump(const char* tag, const std::vector<double>& v) {
  printf("%s", tag);
  for (double q : v) printf(" %.17g", q);
  printf("\n");
}

// input: flags use_limits B steps dt nsp sched, per loop pv_index pv_is_state out_index lo hi, then per instance x0, [u; p], the gains
// [3][nsp], mem [nsp][5], and the set points: [steps][B][nsp] with sched, else [B][nsp]
template <class M>
int loop(FILE* f) {
  constexpr int NX = M::NX, NUP = M::NU + M::NP, NY = M::NY;
  PidParams po;
  memset(&po, 0, sizeof(po));
  po.flags = (int)next(f);
  const int B = (int)next(f), steps = (int)next(f);
  KfParams kp;
  kp.kind = 0; kp.continuous = 1; kp.erk_order = 0; kp.n_sub = 8;
  kp.dt = next(f);
  po.nsp = (int)next(f);
  const int sched = (int)next(f), nsp = po.nsp;
  for (int j = 0; j < nsp; ++j) {
    po.pv_index[j] = (int)next(f); po.pv_is_state[j] = (int)next(f); po.out_index[j] = (int)next(f);
    po.lo[j] = next(f); po.hi[j] = next(f);
  }
  std::vector<double> x0(B * NX), up(B * NUP), g(B * 3 * nsp), mem(B * nsp * PID_MEM), sp((sched ? steps : 1) * B * nsp);
  for (int b = 0; b < B; ++b) {
    for (int i = 0; i < NX; ++i) x0[b * NX + i] = next(f);
    for (int i = 0; i < NUP; ++i) up[b * NUP + i] = next(f);
    for (int i = 0; i < 3 * nsp; ++i) g[b * 3 * nsp + i] = next(f);
    for (int i = 0; i < nsp * PID_MEM; ++i) mem[b * nsp * PID_MEM + i] = next(f);
  }
  for (auto& v : sp) v = next(f);
  std::vector<double> X((steps + 1) * B * NX), U(steps * B * nsp), Y(steps * B * NY), J(B * nsp * 4), xf(B * NX);
  std::vector<int> stats(B * 4);
  SimParams sim = {SIM_MAP, 10000, 1e-6, 1e-8, 0.0};
  for (int b = 0; b < B; ++b)
    pid_loop_instance<M, SIM_MAP>(kp, sim, po, b, B, steps, x0.data(), up.data(), NUP, sp.data(), nsp, sched ? B * nsp : 0, g.data(),
                                  3 * nsp, mem.data(), X.data(), U.data(), Y.data(), J.data(), xf.data(), stats.data(), 0.0, nullptr);
  dump("X", X); dump("U", U); dump("Y", Y); dump("J", J); dump("F", xf); dump("M", mem);
  return 0;
}

// input: flags lo hi dt k_p t_i t_d n, then n pairs (pv, sp): the law alone from a zero memory
static int law(FILE* f) {
  const int flags = (int)next(f);
  const double lo = next(f), hi = next(f), dt = next(f), k_p = next(f), t_i = next(f), t_d = next(f);
  const int n = (int)next(f);
  double m[PID_MEM] = {0, 0, 0, 0, 0}, e;
  std::vector<double> u;
  for (int i = 0; i < n; ++i) {
    const double pv = next(f), sp = next(f);
    u.push_back(pid_update(m, pv, sp, k_p, t_i, t_d, dt, flags, lo, hi, &e));
  }
  dump("U", u);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[2], "r");
  if (!f) return 2;
  if (!strcmp(argv[1], "law")) return law(f);
  if (!strcmp(argv[1], "linear2")) return loop<Linear2>(f);
  if (!strcmp(argv[1], "chemostat4")) return loop<Chemostat4>(f);
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
    d = tmp_path_factory.mktemp('pid_host')
    src = d / 'driver.hip'
    src.write_text(DRIVER)
    exe = d / 'driver'
    subprocess.check_call([hipcc, '-x', 'hip', '--cuda-host-only', '-std=c++17', '-O2', '-I', CSRC, str(src), '-o', str(exe)])
    count = [0]

    def run(what, numbers):
        count[0] += 1
        fin = d / f'in{count[0]}.txt'
        fin.write_text(' '.join(repr(float(v)) for v in numbers))
        out = subprocess.check_output([str(exe), what, str(fin)], text=True).strip().split('\n')
        return {ln.split()[0]: np.array([float(v) for v in ln.split()[1:]]) for ln in out}
    return run


def test_host_compiled_law_gives_the_known_answers(driver):
    out = driver('law', [0, 0., 0., .01, 8., 1., 0., 2, 0., 1., .1, 1.])
    np.testing.assert_allclose(out['U'], [8.08, 7.352])
    # t_i = inf adds nothing, and the clamped value is what is remembered: two steps of a P controller held at the limit
    out = driver('law', [4, -1., 1., .01, 8., np.inf, 0., 3, 0., 1., 0., 1., .5, 1.])
    np.testing.assert_array_equal(out['U'], [1., 1., -1.])


def _loop_on_host(driver, model, case, B, p_on_pv=False, d_on_pv=False, limits=None, schedule=None):
    nsp = case['k_p'].shape[1]
    steps, dt = case['steps'], case['dt']
    flags = (1 if p_on_pv else 0) | (2 if d_on_pv else 0) | (4 if limits is not None else 0)
    lo, hi = limits if limits is not None else (0., 0.)
    nums = [flags, B, steps, dt, nsp, int(schedule is not None)]
    for (kind, i), o in zip(case['pv_sel'], case['out_idx']):
        nums += [i, int(kind == 'x'), o, lo, hi]
    nu = 1 if model == 'linear2' else 2
    for b in range(B):
        nums += list(case['x0'][b]) + nu * [0.] + list(case['p'][b])
        nums += list(case['k_p'][b]) + list(case['t_i'][b]) + list(case['t_d'][b]) + nsp * pr.MEM * [0.]
    sp = np.tile(case['set_point'], (B, 1)) if schedule is None else schedule
    nums += list(np.asarray(sp, dtype=float).ravel())
    out = driver(model, nums)
    om = sr.oracle_model(model)
    ref = pr.batch(pr.oracle_plant(om), case['x0'][:B], np.zeros((B, nu)), case['p'][:B], case['k_p'][:B], case['t_i'][:B],
                   case['t_d'][:B], case['set_point'] if schedule is None else schedule, steps, dt, case['pv_sel'], case['out_idx'],
                   p_on_pv=p_on_pv, d_on_pv=d_on_pv, limits=limits)
    nx = case['x0'].shape[1]
    got = {'x': out['X'].reshape(steps + 1, B, nx), 'u': out['U'].reshape(steps, B, nsp), 'y': out['Y'].reshape(steps, B, -1),
           'mem': out['M'].reshape(B, nsp, pr.MEM), 'x_final': out['F'].reshape(B, nx)}
    J = out['J'].reshape(B, nsp, 4)
    worst = 0.
    pairs = [(got[k], ref[k]) for k in ('x', 'u', 'y', 'mem')] + [(got['x_final'], ref['x'][-1])] + \
            [(J[:, :, i], ref['indices'][k]) for i, k in enumerate(('ise', 'iae', 'itae', 'tvu'))]
    for a, r in pairs:
        assert a.shape == r.shape
        worst = max(worst, float(np.max(np.abs(a - r) / (1e-13 + 1e-11 * np.abs(r)))))
    return worst, got, ref


@pytest.mark.parametrize('p_on_pv', [False, True])
@pytest.mark.parametrize('d_on_pv', [False, True])
def test_host_compiled_loop_against_the_restatement(driver, p_on_pv, d_on_pv):
    """linear2, B = 3, 40 intervals of .25: X, U, Y, the indices, the final state and the memory at rtol 1e-11 / atol 1e-13."""
    worst, _, _ = _loop_on_host(driver, 'linear2', pr.linear2_case(3), 3, p_on_pv, d_on_pv)
    print(f"linear2 p_on_pv={p_on_pv} d_on_pv={d_on_pv}: worst |error| / (1e-13 + 1e-11 |ref|) = {worst:.3e}")
    assert worst <= 1.


def test_host_compiled_loop_with_limits_that_bind(driver):
    worst, got, _ = _loop_on_host(driver, 'linear2', pr.linear2_case(3), 3, limits=(0., 1.2))
    print(f"linear2 with limits (0, 1.2): worst ratio {worst:.3e}")
    assert worst <= 1.
    assert got['u'].max() == 1.2 and got['u'].min() >= 0. and np.any(got['u'] < 1.2)


def test_host_compiled_loop_with_a_set_point_schedule(driver):
    case = pr.linear2_case(3)
    k = np.arange(case['steps'])
    schedule = (1. + .5 * (k >= 15) - .8 * (k >= 30))[:, None, None] * np.array([1., .9, 1.1])[None, :, None]
    worst, _, _ = _loop_on_host(driver, 'linear2', case, 3, schedule=schedule)
    print(f"linear2 with a set-point schedule: worst ratio {worst:.3e}")
    assert worst <= 1.


def test_host_compiled_two_loops_on_states_with_limits(driver):
    """chemostat4 (two loops, state selectors, the lower limit binding) through the same body."""
    case = pr.chemostat4_case(3)
    worst, got, _ = _loop_on_host(driver, 'chemostat4', case, 3, limits=case['limits'])
    print(f"chemostat4, two loops: worst ratio {worst:.3e}")
    assert worst <= 1.
    assert got['u'].min() == 0. and got['u'].max() <= .5
