"""GPU: `PID.call` (hilo_pid_call) and the one-launch closed loop `PID.closed_loop` (hilo_pid_loop, csrc/hilo_pid.h).

The fused loop is compared with what a user could do before - `PID.call(pv=y)` + `Model.step`, alternating - with the numpy
restatement of tests/pid_reference.py, and under 'dopri5' with a tight scipy solution of the same closed loop under the bound of
tests/sim_reference.py.  The tolerances and where they come from are stated at each test; each test prints the figures it asserts
on."""
import ctypes

import numpy as np
import pytest
import torch

from hilo_mpc_amd import PID, Model, SimpleControlLoop, _lib
from tests import pid_reference as pr
from tests import sim_reference as sr

pytestmark = pytest.mark.gpu

B = 130                               # two waves and two lanes
RTOL, ATOL = 1e-8, 1e-10
OPTS = {'reltol': RTOL, 'abstol': ATOL}
ROWS = np.linspace(0, B - 1, 16).astype(int)


def _pid(case, **kw):
    nsp = case['k_p'].shape[1]
    pid = PID(n_set_points=nsp, k_p=case['k_p'], t_i=case['t_i'], t_d=case['t_d'], output_limits=case.get('limits'), **kw)
    pid.setup(dt=case['dt'])
    pid.set_point = case['set_point']
    return pid


def _loop(case, plant, pid=None, rows=slice(None), **kw):
    pid = pid or _pid(case)
    names = {k: case[k] for k in ('process_values', 'outputs') if k in case}
    if rows != slice(None):
        pid.k_p, pid.t_i, pid.t_d = case['k_p'][rows], case['t_i'][rows], case['t_d'][rows]
    return pid.closed_loop(plant, case['x0'][rows], p=case['p'][rows], steps=kw.pop('steps', case['steps']), **names, **kw)


def _worst(a, r, rtol, atol):
    return float(np.max(np.abs(a - r) / (atol + rtol * np.abs(r))))


@pytest.fixture(scope='module')
def linear2():
    case = pr.linear2_case(B)
    plant = Model('linear2').setup(dt=case['dt'])
    pid = _pid(case)
    return case, plant, pid, _loop(case, plant, pid, return_stats=True)


@pytest.fixture(scope='module')
def chemostat4():
    case = pr.chemostat4_case(B)
    plant = Model('chemostat4').setup(dt=case['dt'])
    pid = _pid(case)
    return case, plant, pid, _loop(case, plant, pid)


def _alternating(case, plant, pv_of):
    """What a user could do before: the law through PID.call, the plant through Model.step, `steps` rounds."""
    pid = _pid(case)
    x, y = case['x0'], None
    X, U, Y = [x], [], []
    for _ in range(case['steps']):
        u = pid.call(pv=pv_of(x, y))
        x, y = plant.step(x, u, case['p'])
        X.append(x), U.append(u), Y.append(y)
    return np.array(X), np.array(U), np.array(Y)


def test_fused_equals_alternating(linear2):
    """linear2, y = x_2 driven by u: one closed_loop against 40 rounds of PID.call(pv=y) + Model.step at rtol 1e-12 / atol 1e-14 -
    the project's 1e-13 / 1e-15 for one map compiled into two kernels (tests/test_rollout_gpu.py) times 10 for the loop's own
    conditioning (a 1e-12 relative perturbation of x0 moves no entry of x or u by more than 6.5e-12 in the numpy restatement).
    The same run against tests/pid_reference.py at 1e-11 / 1e-13."""
    case, plant, _, r = linear2
    assert r['x'].shape == (41, B, 2) and r['u'].shape == (40, B, 1) and r['y'].shape == (40, B, 1)
    assert not r['stats']['status'].any()
    X, U, Y = _alternating(case, plant, lambda x, y: x[:, 1:2] if y is None else y)
    print("fused vs alternating, worst |d| / (1e-14 + 1e-12 |ref|):", {k: f"{_worst(r[k], v, 1e-12, 1e-14):.3e}" for k, v in
                                                                        (('x', X), ('u', U), ('y', Y))})
    for k, v in (('x', X), ('u', U), ('y', Y)):
        np.testing.assert_allclose(r[k], v, rtol=1e-12, atol=1e-14)
    ref = pr.batch(pr.oracle_plant(sr.oracle_model('linear2')), case['x0'], np.zeros((B, 1)), case['p'], case['k_p'], case['t_i'],
                   case['t_d'], case['set_point'], case['steps'], case['dt'], case['pv_sel'], case['out_idx'])
    print("fused vs numpy restatement, worst |d| / (1e-13 + 1e-11 |ref|):", {k: f"{_worst(r[k], ref[k], 1e-11, 1e-13):.3e}"
                                                                              for k in ('x', 'u', 'y')})
    for k in ('x', 'u', 'y'):
        np.testing.assert_allclose(r[k], ref[k], rtol=1e-11, atol=1e-13)
    np.testing.assert_array_equal(r['x_final'], r['x'][-1])


def test_two_loops_selectors_and_clamp(chemostat4):
    """chemostat4: X by DS with k_p < 0 and P by DI, limits (0, .5).  Fused against alternating calls at rtol 1e-11: the two sides
    are the same statements in two kernels and can differ by roundings of 1e-16 relative, and in the numpy restatement of this case
    (initial states spread so that both limits are hit) a 1e-12 relative perturbation of x0 moves no entry of x by more than 2.5e-10
    and none of u by more than 1.5e-9 relative - an amplification of 1.5e3 at the most.  Both limits are hit and never exceeded; with
    the loops swapped and outputs=['DI', 'DS'] the result is the swapped one."""
    case, plant, _, r = chemostat4
    assert np.isfinite(r['x']).all()
    X, U, Y = _alternating(case, plant, lambda x, y: x[:, [0, 2]])
    print("two loops, fused vs alternating, worst relative difference:",
          {k: f"{np.max(np.abs(r[k] - v) / np.maximum(np.abs(v), 1e-300)):.3e}" for k, v in (('x', X), ('u', U), ('y', Y))})
    for k, v in (('x', X), ('u', U), ('y', Y)):
        np.testing.assert_allclose(r[k], v, rtol=1e-11)
    lo, hi = case['limits']
    assert r['u'].min() == lo and r['u'].max() == hi
    print("entries at the lower / upper limit:", int((r['u'] == lo).sum()), int((r['u'] == hi).sum()))
    swapped = dict(case, k_p=case['k_p'][:, ::-1].copy(), t_i=case['t_i'][:, ::-1].copy(), t_d=case['t_d'][:, ::-1].copy(),
                   set_point=case['set_point'][::-1].copy(), process_values=['P', 'X'], outputs=['DI', 'DS'])
    s = _loop(swapped, plant)
    np.testing.assert_array_equal(s['u'], r['u'][:, :, ::-1])
    np.testing.assert_array_equal(s['x'], r['x'])
    for k in r['indices']:
        np.testing.assert_array_equal(s['indices'][k], r['indices'][k][:, ::-1])
    # the measurements yX, yP select the same values as the states X, P
    by_y = _loop(dict(case, process_values=['yX', 'yP']), plant)
    np.testing.assert_array_equal(by_y['x'], r['x'])


def test_indices(linear2, chemostat4):
    """ise, iae, itae, tvu against the numpy sums over the returned 'u' and the errors sp - pv, at rtol 1e-12 (sums of 40
    non-negative terms: their rounding is 40 eps at the most)."""
    for (case, _, _, r), pv in ((linear2, lambda x: x[:, :, 1:2]), (chemostat4, lambda x: x[:, :, [0, 2]])):
        dt, steps = case['dt'], case['steps']
        e = case['set_point'] - pv(r['x'][:-1])
        k = np.arange(steps)[:, None, None]
        du = np.diff(np.concatenate([np.zeros((1,) + r['u'].shape[1:]), r['u']]), axis=0)
        sums = {'ise': (e * e * dt).sum(0), 'iae': (np.abs(e) * dt).sum(0), 'itae': (k * dt * np.abs(e) * dt).sum(0),
                'tvu': np.abs(du).sum(0)}
        for name, v in sums.items():
            assert r['indices'][name].shape == v.shape
            print(f"{name}: worst relative difference {np.max(np.abs(r['indices'][name] - v) / v):.3e}")
            np.testing.assert_allclose(r['indices'][name], v, rtol=1e-12)


def test_sweep_mode(linear2):
    case, plant, _, r = linear2
    s = _loop(case, plant, store=False)
    assert 'x' not in s and 'u' not in s and 'y' not in s
    np.testing.assert_array_equal(s['x_final'], r['x_final'])
    for k in r['indices']:
        np.testing.assert_array_equal(s['indices'][k], r['indices'][k])
    # device tensors in, device tensors out
    dev = torch.device('cuda')
    pid = PID(k_p=torch.as_tensor(case['k_p'], device=dev), t_i=torch.as_tensor(case['t_i'], device=dev),
              t_d=torch.as_tensor(case['t_d'], device=dev)).setup(dt=case['dt'])
    pid.set_point = 1.
    t = pid.closed_loop(plant, torch.as_tensor(case['x0'], device=dev), p=torch.as_tensor(case['p'], device=dev), steps=case['steps'])
    assert all(v.is_cuda for v in (t['x'], t['u'], t['y'], t['x_final'], t['indices']['ise']))
    np.testing.assert_array_equal(t['x'].cpu().numpy(), r['x'])


def test_continuation_and_reset(linear2):
    """Under the map 20 intervals equal two calls of 10, bit for bit, the memory included; reset() restores the first result."""
    case, plant, _, _ = linear2
    one = _pid(case)
    a = _loop(case, plant, one, steps=20)
    two = _pid(case)
    b1 = _loop(case, plant, two, steps=10)
    b2 = two.closed_loop(plant, b1['x_final'], p=case['p'], steps=10)
    np.testing.assert_array_equal(np.concatenate([b1['x'], b2['x'][1:]]), a['x'])
    np.testing.assert_array_equal(np.concatenate([b1['u'], b2['u']]), a['u'])
    np.testing.assert_array_equal(two._mem.cpu().numpy(), one._mem.cpu().numpy())
    assert np.any(b2['u'][0] != b1['u'][0])
    two.reset()
    c = _loop(case, plant, two, steps=10)
    for k in ('x', 'u', 'y'):
        np.testing.assert_array_equal(c[k], b1[k])


@pytest.mark.parametrize('solver', [None, 'dopri5'])
def test_an_instance_does_not_depend_on_its_wave(linear2, solver):
    case = linear2[0]
    plant = Model('linear2').setup(dt=case['dt'], **({'solver': solver, 'solver_options': OPTS} if solver else {}))
    r = _loop(case, plant, return_stats=True)
    alone = _loop(case, plant, _pid(case), rows=slice(77, 78), return_stats=True)
    for k in ('x', 'u', 'y'):
        np.testing.assert_array_equal(alone[k][:, 0], r[k][:, 77])
    for k in r['indices']:
        np.testing.assert_array_equal(alone['indices'][k][0], r['indices'][k][77])
    assert all(alone['stats'][k][0] == r['stats'][k][77] for k in r['stats'])


@pytest.mark.parametrize('name', ['linear2', 'chemostat4'])
def test_dopri5_closed_loop_against_tight_solution(name):
    """reltol 1e-8 / abstol 1e-10, 10 intervals: 16 instances against the tight closed-loop solution (DOP853 at 1e-13 per interval,
    the law in numpy) under the bound of tests/sim_reference.py - the error relative to |x| + abstol / reltol at most FACTOR = 10
    times the larger of scipy RK45's error in the same closed loop at the same tolerances and the DOP853-vs-Radau disagreement."""
    case = pr.CASES[name](B)
    steps = 10
    plant = Model(name).setup(dt=case['dt'], solver='dopri5', solver_options=OPTS)
    r = _loop(case, plant, steps=steps, return_stats=True)
    assert not r['stats']['status'].any()
    ref, admissible, e45, e_tight = pr.dopri5_bounds_batch(name, ROWS, steps, RTOL, ATOL)
    worst = 0.
    for i, row in enumerate(ROWS):
        err = sr.rel_err(r['x'][:, row], ref[:, i], RTOL, ATOL)
        worst = max(worst, err / max(e45[i], e_tight[i]))
        assert err <= admissible[i], (name, row, err, admissible[i])
    print(f"{name}: largest error / max(RK45's error, DOP853 vs Radau) over {len(ROWS)} instances: {worst:.2f} "
          f"(RK45 errors {e45.min():.2e} .. {e45.max():.2e}, DOP853 vs Radau up to {e_tight.max():.2e})")


def _square_plus_u():
    m = Model(name='square_u')
    x = m.set_dynamical_states(['x'])
    u = m.set_inputs(['u'])
    m.set_dynamical_equations([x[0] * x[0] + u[0]])
    m.set_measurement_equations([x[0]])
    return m.setup(dt=.25, solver='dopri5', solver_options=dict(OPTS, max_num_steps=40))


def test_failure_is_contained():
    """dx/dt = x^2 + u from .5 with the set point 0: k_p = 4 holds the state, k_p = -4 (positive feedback) drives it to its pole
    within a few intervals.  Bad and good instances alternate inside each wave.  The bad ones end with status 1, NaN rows from the
    instant they miss and NaN indices; the good ones equal their result in a batch without the bad ones."""
    m = _square_plus_u()
    n, steps = 128, 16
    bad = np.arange(n) % 2 == 0
    k_p = np.where(bad, -4., 4.)[:, None] * (1 + .1 * np.linspace(0., 1., n))[:, None]
    x0 = np.full((n, 1), .5)

    def run(rows):
        pid = PID(k_p=k_p[rows]).setup(dt=.25)
        return pid.closed_loop(m, x0[rows], steps=steps, return_stats=True)
    r = run(slice(None))
    st = r['stats']['status']
    print("status of the bad half:", np.unique(st[bad]), "of the good half:", np.unique(st[~bad]))
    assert (st[bad] == 1).all() and (st[~bad] == 0).all()
    assert np.isfinite(r['x'][:, ~bad]).all() and np.isfinite(r['indices']['ise'][~bad]).all()
    for i in np.flatnonzero(bad):
        miss = np.flatnonzero(np.isnan(r['x'][:, i, 0]))
        assert len(miss) and miss[0] >= 1 and np.isnan(r['x'][miss[0]:, i]).all() and np.isfinite(r['x'][:miss[0], i]).all()
        assert np.isnan(r['y'][miss[0] - 1:, i]).all() and np.isnan(r['u'][miss[0]:, i]).all() and np.isfinite(r['u'][:miss[0], i]).all()
        assert all(np.isnan(v[i]).all() for v in r['indices'].values()) and np.isnan(r['x_final'][i]).all()
    g = run(~bad)
    for k in ('x', 'u', 'y'):
        np.testing.assert_array_equal(g[k], r[k][:, ~bad])
    np.testing.assert_array_equal(g['indices']['ise'], r['indices']['ise'][~bad])


def _linear2_expressions(forced=False):
    m = Model(name='linear2_forced' if forced else 'linear2_expr')
    m.set_parameters(['k_1', 'k_2'] + (['w'] if forced else []))
    m.set_equations("dx_1/dt = -k_1*x_1(t) + u(k)" + (" + sin(w*t)" if forced else "") + "\ndx_2/dt = k_1*x_1(t) - k_2*x_2(t)\n"
                    "y(k) = x_2(t)")
    return m


def test_run_time_compiled_twin(linear2):
    """The linear2 equations written as expressions (hilo_user_pid_loop) against the zoo functor at rtol 1e-12; with + sin(w t) on
    the first state and t0 = 1.7 against tests/pid_reference.py at 1e-11 / 1e-13."""
    case, _, _, r = linear2
    m = _linear2_expressions().setup(dt=case['dt'])
    assert m.input_names == ['u'] and m.dynamical_state_names == ['x_1', 'x_2']
    e = _loop(case, m)
    print("expressions vs zoo functor:", {k: f"{_worst(e[k], r[k], 1e-12, 1e-14):.3e}" for k in ('x', 'u', 'y')})
    for k in ('x', 'u', 'y'):
        np.testing.assert_allclose(e[k], r[k], rtol=1e-12, atol=1e-14)
    f = _linear2_expressions(forced=True).setup(dt=case['dt'])
    assert f.is_time_variant()
    w = np.linspace(.5, 3., B)[:, None]
    P, t0 = np.hstack([case['p'], w]), 1.7
    t = _pid(case).closed_loop(f, case['x0'], p=P, steps=case['steps'], t0=t0)

    def rhs(t_, x, u, p):
        return np.stack([-p[:, 0] * x[:, 0] + u[:, 0] + np.sin(p[:, 2] * t_), p[:, 0] * x[:, 0] - p[:, 1] * x[:, 1]], axis=1)
    ref = pr.batch((rhs, lambda t_, x, u, p: x[:, 1:2]), case['x0'], np.zeros((B, 1)), P, case['k_p'], case['t_i'], case['t_d'],
                   case['set_point'], case['steps'], case['dt'], case['pv_sel'], case['out_idx'], t0=t0)
    print("time-variant twin vs numpy restatement:", {k: f"{_worst(t[k], ref[k], 1e-11, 1e-13):.3e}" for k in ('x', 'u', 'y')})
    for k in ('x', 'u', 'y'):
        np.testing.assert_allclose(t[k], ref[k], rtol=1e-11, atol=1e-13)
    assert np.max(np.abs(t['x'] - r['x'])) > 1e-2          # the forcing is felt


def test_simple_control_loop(linear2):
    """SimpleControlLoop(plant, pid).run is pid.closed_loop; with an observer attached it runs step by step (PID.call + Model.step)
    and agrees at the alternating tolerance."""
    from hilo_mpc_amd import EKF
    case, plant, _, r = linear2
    sol = SimpleControlLoop(plant, _pid(case)).run(case['steps'], case['x0'], p=case['p'])
    for k in ('x', 'u'):
        np.testing.assert_array_equal(sol[k], r[k])
    for k in r['indices']:
        np.testing.assert_array_equal(sol['indices'][k], r['indices'][k])
    assert set(sol) >= {'x', 'u', 'status', 'estimates', 'indices'}
    obs = EKF(Model('linear2').discretize('rk4').setup(dt=case['dt']))
    obs.setup()
    obs.Q, obs.R = 1e-4, 1e-2
    obs.set_initial_guess(case['x0'], P0=np.tile(np.eye(2), (B, 1, 1)))
    step = SimpleControlLoop(plant, _pid(case), observer=obs).run(case['steps'], case['x0'], p=case['p'], measure=lambda x: x[:, 1:2])
    assert len(step['estimates']) == case['steps'] and step['indices'] is None
    for k in ('x', 'u'):
        np.testing.assert_allclose(step[k], r[k], rtol=1e-12, atol=1e-14)


def test_library_refusals(linear2):
    """Through the C entries: SIM_BDF, five loops and a null x0 each return the error code and say why; none launches."""
    case, plant, _, _ = linear2
    h = plant._plant_handle()
    lib = _lib.lib()
    dev = torch.device('cuda')
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)
    x0, up, sp, mem, J, xf = z(1, 2), z(1, 3), z(1, 1), z(1, 1, 5), z(1, 1, 4), z(1, 2)
    g = torch.tensor([[1., float('inf'), 0.]], dtype=torch.float64, device=dev)      # k_p, t_i, t_d

    def call(sim, opts, x0_ptr):
        rc = lib.hilo_pid_loop(h._handle, ctypes.byref(sim), ctypes.byref(opts), 1, 1, x0_ptr, up.data_ptr(), 0, sp.data_ptr(), 0, 0,
                               g.data_ptr(), 0, mem.data_ptr(), None, None, None, J.data_ptr(), xf.data_ptr(), None, None, None)
        return rc, lib.hilo_last_error().decode()
    ok = _lib.PidOpts()
    ok.nsp = 1
    bdf = _lib.SimOpts()
    bdf.method = 2
    rc, msg = call(bdf, ok, x0.data_ptr())
    assert rc == -4 and 'HILO_SIM_MAP and HILO_SIM_DOPRI5' in msg
    five = _lib.PidOpts()
    five.nsp = 5
    rc, msg = call(_lib.SimOpts(), five, x0.data_ptr())
    assert rc == -1 and '5 loops' in msg
    rc, msg = call(_lib.SimOpts(), ok, None)
    assert rc == -1 and 'NULL argument' in msg
    rc, msg = call(_lib.SimOpts(), ok, x0.data_ptr())       # the same call with everything in place runs
    assert rc == 0
    torch.cuda.synchronize()
    assert float(J.abs().sum()) == 0. and float(mem.abs().sum()) == 0.     # all zeros in: no error, no output
