"""CPU: host-side contract of `Model.setup(solver=...)`, `Model.rollout` and the roll-out path of `Model.simulate`, against a
stand-in for `hilo_model_rollout` that READS its pointer arguments the way include/hilo_hip.h declares them (handle, opts, batch,
steps, x0, up, up_stride, up_step, X, Y, stats, stream) and answers with the oracle's model - argument order, strides and shapes of
the host call without a GPU, in the manner of tests/test_host_api.py::test_model_step_passes_the_arguments_of_the_c_signature."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

from hilo_mpc_amd import Model, _lib
from oracle import models as omodels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P4 = [100., 4., 1., 0.]


def _arr(ptr, n, typ=C.c_double):
    return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(typ)), shape=(n,))


def _stub(monkeypatch, m, om, n_p, n_y, log, fail_half=False):
    """Replaces the plant handle and the library: the stand-in walks the [u; p] rows with the strides it is handed."""
    nx, nu = m.n_x, m.n_u
    nup = nu + n_p

    class H:
        _dev, _handle, _n_p, _n_y = torch.device('cpu'), 4321, n_p, n_y
    monkeypatch.setattr(m, '_plant_handle', lambda device_index=None: H)
    monkeypatch.setattr('hilo_mpc_amd._device.stream_ptr', lambda dev: 0)

    class Lib:
        @staticmethod
        def hilo_model_rollout(h, opts, B, steps, x0, up, us, ustep, X, Y, stats, stream):
            o = opts._obj
            log.append(dict(h=h, B=B, steps=steps, us=us, ustep=ustep, method=o.method, max_steps=o.max_steps, rtol=o.rtol,
                            atol=o.atol, h0=o.h0, stats=stats is not None))
            assert us in (0, nup) and (ustep == 0 or ustep == (B * us if us else nup))
            x = _arr(x0, B * nx).reshape(B, nx).copy()
            Xo = _arr(X, (steps + 1) * B * nx).reshape(steps + 1, B, nx)
            Yo = _arr(Y, steps * B * n_y).reshape(steps, B, n_y)
            Xo[0] = x
            n_rows = (steps - 1) * ustep + (B - 1) * us + nup
            rows = _arr(up, n_rows) if nup else np.zeros(0)
            for k in range(steps):
                upk = np.array([rows[k * ustep + b * us:k * ustep + b * us + nup] for b in range(B)]).reshape(B, nup)
                x = om.f(x, upk[:, :nu], upk[:, nu:], m.dt)
                Xo[k + 1] = x
                Yo[k] = om.h(x, upk[:, :nu], upk[:, nu:], m.dt)
            if stats is not None:
                s = _arr(stats, B * 4, C.c_int32).reshape(B, 4)
                s[:] = [0, 7, 1, 50]
                if fail_half:
                    s[:B // 2, 0] = 2
                    Xo[-1, :B // 2] = np.nan
            return 0
    monkeypatch.setattr(_lib, 'lib', lambda: Lib)


def _oracle_rollout(om, X0, U, P, dt, steps):
    x, out = X0, [X0]
    for k in range(steps):
        u = U[k] if U.ndim == 3 else U
        x = om.f(x, np.broadcast_to(u, (X0.shape[0], u.shape[-1])), np.broadcast_to(P, (X0.shape[0], len(P))), dt)
        out.append(x)
    return np.array(out)


def test_rollout_passes_the_arguments_of_the_c_signature(monkeypatch):
    m = Model('chemostat4').discretize('rk4').setup(dt=.5)
    om = omodels.get('chemostat4').discretize(4)
    log = []
    _stub(monkeypatch, m, om, 4, 2, log)
    rng = np.random.default_rng(0)
    B, steps = 5, 6
    X0 = np.array([.1, 40., .5, .2]) * (1 + .1 * rng.standard_normal((B, 4)))
    # held inputs per instance, shared parameters: packed rows [B][6]
    U = rng.uniform(0, .3, (B, 2))
    x, y = m.rollout(X0, U, P4, steps=steps)
    ref = _oracle_rollout(om, X0, U, P4, .5, steps)
    assert x.shape == (steps + 1, B, 4) and y.shape == (steps, B, 2) and isinstance(x, np.ndarray)
    np.testing.assert_allclose(x, ref, rtol=1e-14)
    np.testing.assert_allclose(y, ref[1:][:, :, [0, 2]], rtol=1e-14)
    assert log[-1] == dict(h=4321, B=B, steps=steps, us=6, ustep=0, method=0, max_steps=0, rtol=0., atol=0., h0=0., stats=False)
    # a sequence of inputs, one row per sampling interval and instance: [steps][B][6]
    Us = rng.uniform(0, .3, (steps, B, 2))
    x, y = m.rollout(X0, Us, P4, steps=steps)
    np.testing.assert_allclose(x, _oracle_rollout(om, X0, Us, P4, .5, steps), rtol=1e-14)
    assert (log[-1]['us'], log[-1]['ustep']) == (6, B * 6)
    # a sequence shared by the batch (batch axis 1): [steps][1][6], stride 0 between instances
    U1 = rng.uniform(0, .3, (steps, 1, 2))
    x, y = m.rollout(X0, U1, P4, steps=steps)
    np.testing.assert_allclose(x, _oracle_rollout(om, X0, U1, P4, .5, steps), rtol=1e-14)
    assert (log[-1]['us'], log[-1]['ustep']) == (0, 6)
    # everything shared: one row
    x, y = m.rollout(X0, [.1, .2], P4, steps=steps)
    np.testing.assert_allclose(x, _oracle_rollout(om, X0, np.array([[.1, .2]]), P4, .5, steps), rtol=1e-14)
    assert (log[-1]['us'], log[-1]['ustep']) == (0, 0)
    # parameters per instance with a shared input sequence
    Pb = np.tile(P4, (B, 1)) * (1 + .01 * rng.standard_normal((B, 4)))
    x, y = m.rollout(X0, U1, Pb, steps=steps)
    refp = np.array([_oracle_rollout(om, X0[b:b + 1], U1, list(Pb[b]), .5, steps)[:, 0] for b in range(B)]).transpose(1, 0, 2)
    np.testing.assert_allclose(x, refp, rtol=1e-14)
    assert (log[-1]['us'], log[-1]['ustep']) == (6, B * 6)
    # device tensors in -> tensors out
    xt, yt = m.rollout(torch.as_tensor(X0), torch.as_tensor(U), torch.as_tensor(P4, dtype=torch.float64), steps=2)
    assert isinstance(xt, torch.Tensor) and isinstance(yt, torch.Tensor) and xt.shape == (3, B, 4)
    with pytest.raises(RuntimeError, match="The model has 2 inputs"):
        m.rollout(X0, None, P4)
    with pytest.raises(ValueError, match="does not match"):
        m.rollout(X0, U[:3], P4)
    with pytest.raises(ValueError, match="a sequence of 6 rows for 4 sampling intervals"):
        m.rollout(X0, Us, P4, steps=4)
    with pytest.raises(ValueError, match="steps must be at least 1"):
        m.rollout(X0, U, P4, steps=0)


def test_inputs_alone_travel_without_a_copy(monkeypatch):
    """A model without parameters: the caller's contiguous [steps, B, n_u] array IS the table of rows."""
    m = Model('pendulum4').discretize('rk4').setup(dt=.1)
    om = omodels.get('pendulum4').discretize(4)
    log = []
    _stub(monkeypatch, m, om, 0, 4, log)
    rng = np.random.default_rng(1)
    X0 = .1 * rng.standard_normal((3, 4))
    U = rng.uniform(-1, 1, (4, 3, 1))
    x, y = m.rollout(X0, U, steps=4)
    np.testing.assert_allclose(x, _oracle_rollout(om, X0, U, [], .1, 4), rtol=1e-14)
    np.testing.assert_allclose(y, x[1:], rtol=0)
    assert (log[-1]['us'], log[-1]['ustep']) == (1, 3) and not hasattr(m, '_rollout_up')


def test_solver_options_reach_the_library_and_stats_come_back(monkeypatch):
    m = Model('pendulum4').setup(dt=.5, solver='dopri5', solver_options={'reltol': 1e-8, 'abstol': 1e-10, 'max_num_steps': 500,
                                                                        'first_step': 1e-3})
    om = omodels.get('pendulum4').discretize(4)      # (the stand-in's dynamics: only the plumbing is under test)
    log = []
    _stub(monkeypatch, m, om, 0, 4, log, fail_half=True)
    X0 = np.zeros((4, 4))
    x, y, st = m.rollout(X0, [.5], steps=3, return_stats=True)
    assert log[-1] == dict(h=4321, B=4, steps=3, us=0, ustep=0, method=1, max_steps=500, rtol=1e-8, atol=1e-10, h0=1e-3, stats=True)
    assert sorted(st) == ['n_accepted', 'n_rejected', 'n_rhs', 'status']
    np.testing.assert_array_equal(st['status'], [2, 2, 0, 0])
    np.testing.assert_array_equal(st['n_accepted'], [7] * 4)
    assert np.isnan(x[-1, :2]).all() and np.isfinite(x[-1, 2:]).all()
    # step() with a solver is a one-interval roll-out
    xn, yn = m.step(X0, [.5])
    assert log[-1]['steps'] == 1 and log[-1]['method'] == 1 and xn.shape == (4, 4) and yn.shape == (4, 4)
    # defaults (CasADi's for CVODES)
    d = Model('pendulum4').setup(dt=.5, solver='dopri5')
    assert d._solver_options == {'reltol': 1e-6, 'abstol': 1e-8, 'max_num_steps': 10000, 'first_step': 0.}
    # a later setup() without a solver keeps it; the discretised copy is a map and has none
    assert d.setup(dt=.25)._solver == 'dopri5' and d.discretize('rk4')._solver is None and d._solver == 'dopri5'


def test_solver_refusals():
    """dynamic_model.py `check_solver` (:1958-1993): what the reference warns about before it fails is an error here."""
    with pytest.raises(RuntimeError, match="Model is discrete. No solver is required."):
        Model('chemostat4').discretize('rk4').setup(dt=1., solver='dopri5')
    with pytest.raises(RuntimeError, match="Model is discrete. No solver is required."):
        Model('toy1d').setup(dt=1., solver='dopri5')
    with pytest.raises(ValueError, match="Solver 'cvodes' is not available on your system. Use 'dopri5' instead"):
        Model('chemostat4').setup(dt=1., solver='cvodes')
    with pytest.raises(TypeError, match="Solver type must be a string"):
        Model('chemostat4').setup(dt=1., solver=5)
    with pytest.raises(ValueError, match="Unknown option 'rtol' for solver 'dopri5'"):
        Model('chemostat4').setup(dt=1., solver='dopri5', solver_options={'rtol': 1e-8})
    with pytest.raises(ValueError, match="reltol and abstol must be positive"):
        Model('chemostat4').setup(dt=1., solver='dopri5', solver_options={'reltol': 0.})
    with pytest.raises(ValueError, match="solver_options without a solver"):
        Model('chemostat4').setup(dt=1., solver_options={'reltol': 1e-8})
    dae = Model(name='dae')
    x = dae.set_dynamical_states(['x'])
    z = dae.set_algebraic_states(['z'])
    dae.set_dynamical_equations([-x[0] + z[0]])
    dae.set_algebraic_equations([z[0] - 2. * x[0]])
    with pytest.raises(RuntimeError, match="Solver 'dopri5' is not suitable for DAE systems. Use 'idas' or 'collocation' instead"):
        dae.setup(dt=1., solver='dopri5')
    m = Model('chemostat4')
    m.setup(dt=1.)                                        # solver=None: exactly as before
    assert m._solver is None and m._solver_options is None and m.dt == 1. and m._is_setup


def test_simulate_without_a_solver_is_the_loop_over_step(monkeypatch):
    m = Model('chemostat4').discretize('rk4').setup(dt=.5)
    m.set_initial_conditions([.1, 40., 0., 0.])
    calls = []

    def step(x, u=None, p=None, device_index=None):
        calls.append(np.array(x))
        return x + 1., x[:, [0, 2]]
    monkeypatch.setattr(m, 'step', step)
    monkeypatch.setattr(m, 'rollout', lambda *a, **k: pytest.fail("rollout must not be called"))
    m.simulate(u=[.1, .2], p=P4, steps=4)
    assert len(calls) == 4
    m.simulate(u=np.zeros((1, 2)), p=P4, tf=1.5)          # tf / dt = 3 further steps (dynamic_model.py:3937-3941)
    assert len(calls) == 7 and m.solution['t:f'] == 3.5
    assert m.solution['x'].shape == (4, 8)


def test_simulate_on_the_rollout_path_fills_the_solution(monkeypatch):
    om = omodels.get('chemostat4').discretize(4)
    # (a) a sequence of inputs on a model without a solver: one roll-out, `steps` from the sequence
    m = Model('chemostat4').discretize('rk4').setup(dt=.5)
    log = []
    _stub(monkeypatch, m, om, 4, 2, log)
    monkeypatch.setattr(m, 'step', lambda *a, **k: pytest.fail("step must not be called"))
    m.set_initial_conditions([.1, 40., .5, .2])
    U = np.random.default_rng(2).uniform(0, .3, (5, 1, 2))
    m.simulate(u=U, p=P4)
    assert len(log) == 1 and log[0]['steps'] == 5 and log[0]['method'] == 0
    sol = m.solution
    ref = _oracle_rollout(om, np.array([[.1, 40., .5, .2]]), U, P4, .5, 5)
    assert sol['x'].shape == (4, 6) and sol['y'].shape == (2, 5) and sol['u'].shape == (2, 5) and sol['t:f'] == 2.5
    np.testing.assert_allclose(sol['x'], ref[:, 0].T, rtol=1e-14)
    np.testing.assert_allclose(sol['x:f'], ref[-1].T, rtol=1e-14)
    assert sol['x:f'].shape == (4, 1)                                           # column vector like the reference's DM
    assert sol['status'].shape == (1, 1) and sol['n_accepted'].shape == (1, 1) and sol['n_rejected'].shape == (1, 1)
    # (b) a solver: one roll-out per simulate call, a batch of plants keeps the batch axis
    c = Model('chemostat4').setup(dt=.5, solver='dopri5')
    log2 = []
    _stub(monkeypatch, c, om, 4, 2, log2)
    c.set_initial_conditions(np.tile([.1, 40., .5, .2], (3, 1)))
    c.simulate(u=np.full((3, 2), .1), p=P4, steps=4)
    c.simulate(u=np.full((3, 2), .1), p=P4, tf=1.)
    assert [q['steps'] for q in log2] == [4, 2] and all(q['method'] == 1 and q['stats'] for q in log2)
    sol = c.solution
    assert sol['x'].shape == (7, 3, 4) and sol['y'].shape == (6, 3, 2) and sol['x:f'].shape == (3, 4)
    assert sol['status'].shape == (2, 3) and not sol['status'].any()
    np.testing.assert_array_equal(sol['n_accepted:f'], [7, 7, 7])
    np.testing.assert_array_equal(sol['n_rejected:f'], [1, 1, 1])


def test_simulate_up_to_a_time_below_the_sampling_interval_does_nothing(monkeypatch):
    """int(tf / dt) = 0 intervals (dynamic_model.py:3937-3941): a no-op on the loop path and on the roll-out path alike."""
    om = omodels.get('chemostat4').discretize(4)
    for m in (Model('chemostat4').discretize('rk4').setup(dt=.5), Model('chemostat4').setup(dt=.5, solver='dopri5')):
        log = []
        _stub(monkeypatch, m, om, 4, 2, log)
        monkeypatch.setattr(m, 'step', lambda *a, **k: pytest.fail("step must not be called"))
        m.set_initial_conditions([.1, 40., .5, .2])
        m.simulate(u=[.1, .2], p=P4, tf=.3)
        m.simulate(u=[.1, .2], p=P4, steps=0)
        assert not log and m.solution['t:f'] == 0. and m.solution['x'].shape == (4, 1)


def test_sim_opts_layout_matches_the_header(tmp_path):
    """The ctypes mirror of hilo_sim_opts against include/hilo_hip.h compiled by gcc."""
    if shutil.which('gcc') is None:
        pytest.skip('gcc not available')
    header = open(os.path.join(ROOT, 'include', 'hilo_hip.h')).read()
    body = re.search(r'typedef struct hilo_sim_opts \{(.*?)\} hilo_sim_opts;', header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = [part.split()[-1] for decl in body.split(';') if decl.strip() for part in decl.strip().split(',')]
    assert fields == [f[0] for f in _lib.SimOpts._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hilo_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(hilo_sim_opts));']
    lines += [f'  printf("{f} %zu\\n", offsetof(hilo_sim_opts, {f}));' for f in fields]
    lines += ['  printf("dopri5 %d\\n", HILO_SIM_DOPRI5);', '  return 0;', '}']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = dict(l.split() for l in subprocess.check_output([str(exe)], text=True).strip().split('\n'))
    assert int(got['size']) == C.sizeof(_lib.SimOpts)
    for f, _ in _lib.SimOpts._fields_:
        assert int(got[f]) == getattr(_lib.SimOpts, f).offset, f
    from hilo_mpc_amd.model import SOLVERS
    assert int(got['dopri5']) == SOLVERS['dopri5']


def test_rollout_symbol_is_exported_and_checks_its_arguments():
    lib = _lib.lib()
    assert hasattr(lib, 'hilo_model_rollout') and lib.hilo_abi_version() == 1
    rc = lib.hilo_model_rollout(None, None, 1, 1, None, None, 0, 0, None, None, None, None)
    assert rc == -1 and b'hilo_model_rollout: NULL handle' in lib.hilo_last_error()
