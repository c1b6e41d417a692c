"""CPU: host-side contract of `Model.rollout(..., sensitivities=)` / `Model.step(..., sensitivities=)` and of the C entry
`hilo_model_rollout_sens`, against a stand-in for the library that reads its pointer arguments the way include/hilo_hip.h declares
them (in the manner of tests/test_rollout_host.py): the return shapes, the column order, each refusal and its message, the exported
symbol and the ctypes signature against the header."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from hilo_mpc_amd import Model, _lib
from tests.test_rollout_host import _arr, _stub
from oracle import models as omodels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P4 = [100., 4., 1., 0.]
OPTS = {'reltol': 1e-8, 'abstol': 1e-10, 'max_num_steps': 500}


def _stub_sens(monkeypatch, m, n_p, n_y, log):
    """The stand-in writes a code into every entry of SX / SY that names its column and row: column j, state i at sampling instant k
    of instance b -> 1000 k + 100 b + 10 j + i (SY: negative)."""
    om = omodels.get(m.name).discretize(4)
    _stub(monkeypatch, m, om, n_p, n_y, [])
    nx = m.n_x
    lib = _lib.lib()

    def hilo_model_rollout_sens(h, opts, B, steps, x0, up, us, ustep, wrt, X, Y, SX, SY, stats, stream):
        ns = (nx if wrt & 1 else 0) + (m.n_u if wrt & 2 else 0) + (n_p if wrt & 4 else 0)
        log.append(dict(B=B, steps=steps, us=us, ustep=ustep, wrt=wrt, ns=ns, method=opts._obj.method, max_steps=opts._obj.max_steps,
                        rtol=opts._obj.rtol, SY=SY is not None, stats=stats is not None))
        _arr(X, (steps + 1) * B * nx)[:] = 0.
        _arr(Y, steps * B * n_y)[:] = 0.
        k, b, j, i = np.meshgrid(np.arange(steps + 1), np.arange(B), np.arange(ns), np.arange(nx), indexing='ij')
        _arr(SX, (steps + 1) * B * ns * nx)[:] = (1000 * k + 100 * b + 10 * j + i).ravel()
        if SY is not None:
            k, b, j, i = np.meshgrid(np.arange(steps), np.arange(B), np.arange(ns), np.arange(n_y), indexing='ij')
            _arr(SY, steps * B * ns * n_y)[:] = -(1000 * k + 100 * b + 10 * j + i).ravel()
        if stats is not None:
            _arr(stats, B * 4, C.c_int32)[:] = 0
        return 0
    lib.hilo_model_rollout_sens = staticmethod(hilo_model_rollout_sens)
    return lib


def test_without_sensitivities_the_return_value_is_unchanged(monkeypatch):
    m = Model('chemostat4').setup(dt=.5, solver='dopri5', solver_options=OPTS)
    log = []
    _stub_sens(monkeypatch, m, 4, 2, log)
    X0 = np.tile([.1, 40., .5, .2], (3, 1))
    out = m.rollout(X0, [.1, .2], P4, steps=2)
    assert len(out) == 2 and out[0].shape == (3, 3, 4) and out[1].shape == (2, 3, 2)
    out = m.rollout(X0, [.1, .2], P4, steps=2, sensitivities=None, return_stats=True)
    assert len(out) == 3 and sorted(out[2]) == ['n_accepted', 'n_rejected', 'n_rhs', 'status']
    out = m.step(X0, [.1, .2], P4)
    assert len(out) == 2 and out[0].shape == (3, 4) and out[1].shape == (3, 2)
    assert not log                                          # the sensitivity entry was never called


def test_shapes_and_column_order(monkeypatch):
    m = Model('chemostat4').setup(dt=.5, solver='dopri5', solver_options=OPTS)
    log = []
    _stub_sens(monkeypatch, m, 4, 2, log)
    B, steps = 3, 2
    X0 = np.tile([.1, 40., .5, .2], (B, 1))
    x, y, sens = m.rollout(X0, [.1, .2], P4, steps=steps, sensitivities=True)
    assert log[-1] == dict(B=B, steps=steps, us=0, ustep=0, wrt=7, ns=10, method=1, max_steps=500, rtol=1e-8, SY=True, stats=False)
    assert sorted(sens) == ['x', 'y'] and list(sens['x']) == ['x0', 'u', 'p'] and list(sens['y']) == ['x0', 'u', 'p']
    assert sens['x']['x0'].shape == (steps + 1, B, 4, 4) and sens['x']['u'].shape == (steps + 1, B, 4, 2)
    assert sens['x']['p'].shape == (steps + 1, B, 4, 4)
    assert sens['y']['x0'].shape == (steps, B, 2, 4) and sens['y']['u'].shape == (steps, B, 2, 2) and sens['y']['p'].shape == (steps, B, 2, 4)
    assert isinstance(sens['x']['p'], np.ndarray)
    # entry [k, b, i, j] of group g is column (offset of g) + j, state i: the columns run x0, u, p
    for g, off in (('x0', 0), ('u', 4), ('p', 6)):
        S = sens['x'][g]
        k, b, i, j = np.meshgrid(*[np.arange(n) for n in S.shape], indexing='ij')
        np.testing.assert_array_equal(S, 1000 * k + 100 * b + 10 * (off + j) + i)
        Sy = sens['y'][g]
        k, b, i, j = np.meshgrid(*[np.arange(n) for n in Sy.shape], indexing='ij')
        np.testing.assert_array_equal(Sy, -(1000 * k + 100 * b + 10 * (off + j) + i))
    # a subset, given in any order, keeps the kernel's order; with return_stats the dict stays in front of sens
    x, y, st, sens = m.rollout(X0, [.1, .2], P4, steps=steps, sensitivities=('p', 'x0'), return_stats=True)
    assert log[-1]['wrt'] == 5 and log[-1]['ns'] == 8 and log[-1]['stats'] and list(sens['x']) == ['x0', 'p'] and 'status' in st
    S = sens['x']['p']
    k, b, i, j = np.meshgrid(*[np.arange(n) for n in S.shape], indexing='ij')
    np.testing.assert_array_equal(S, 1000 * k + 100 * b + 10 * (4 + j) + i)
    x, y, sens = m.rollout(X0, [.1, .2], P4, steps=steps, sensitivities='u')
    assert log[-1]['wrt'] == 2 and list(sens['x']) == ['u'] and sens['x']['u'].shape == (steps + 1, B, 4, 2)
    # step: the end of the one interval, without the time axis
    xn, yn, sens = m.step(X0, [.1, .2], P4, sensitivities=True)
    assert log[-1]['steps'] == 1 and xn.shape == (B, 4) and sens['x']['p'].shape == (B, 4, 4) and sens['y']['u'].shape == (B, 2, 2)
    k, b, i, j = np.meshgrid(np.array([1]), np.arange(B), np.arange(4), np.arange(4), indexing='ij')
    np.testing.assert_array_equal(sens['x']['p'], (1000 * k + 100 * b + 10 * (6 + j) + i)[0])
    # tensors in, tensors out: permuted views of the kernel's layout
    xt, yt, sens = m.rollout(torch.as_tensor(X0), torch.tensor([.1, .2], dtype=torch.float64), torch.tensor(P4, dtype=torch.float64),
                             steps=steps, sensitivities=True)
    assert isinstance(sens['x']['u'], torch.Tensor) and sens['x']['u'].shape == (steps + 1, B, 4, 2)
    assert sens['x']['u'].stride() == (B * 40, 40, 1, 4)
    # an input sequence with the x0 and p columns
    U = np.full((steps, B, 2), .1)
    x, y, sens = m.rollout(X0, U, P4, steps=steps, sensitivities=('x0', 'p'))
    assert log[-1]['ustep'] == B * 6 and log[-1]['wrt'] == 5
    # a model without parameters: True selects x0 and u
    q = Model('pendulum4').setup(dt=.5, solver='dopri5', solver_options=OPTS)
    _stub_sens(monkeypatch, q, 0, 4, log)
    x, y, sens = q.rollout(np.zeros((2, 4)), [.5], steps=steps, sensitivities=True)
    assert log[-1]['wrt'] == 3 and log[-1]['ns'] == 5 and list(sens['x']) == ['x0', 'u'] and sens['y']['u'].shape == (steps, 2, 4, 1)


def test_refusals_say_what_to_do_instead(monkeypatch):
    X0 = np.tile([.1, 40., .5, .2], (2, 1))
    log = []
    m = Model('chemostat4').setup(dt=.5)                              # the fixed-step map
    _stub_sens(monkeypatch, m, 4, 2, log)
    with pytest.raises(NotImplementedError, match=r"Model.setup\(solver='dopri5'\)"):
        m.rollout(X0, [.1, .2], P4, sensitivities=True)
    with pytest.raises(NotImplementedError, match=r"Model.setup\(solver='dopri5'\)"):
        m.step(X0, [.1, .2], P4, sensitivities=True)
    b = Model('chemostat4').setup(dt=.5, solver='bdf')
    _stub_sens(monkeypatch, b, 4, 2, log)
    with pytest.raises(NotImplementedError, match=r"solver 'bdf' are not implemented.*Use Model.setup\(solver='dopri5'\), or central differences"):
        b.rollout(X0, [.1, .2], P4, sensitivities=True)
    m = Model('chemostat4').setup(dt=.5, solver='dopri5')
    _stub_sens(monkeypatch, m, 4, 2, log)
    U = np.full((3, 2, 2), .1)
    with pytest.raises(ValueError, match=r"input sequence.*Select \('x0', 'p'\), or hold the inputs"):
        m.rollout(X0, U, P4, steps=3, sensitivities=True)
    with pytest.raises(ValueError, match=r"input sequence"):
        m.rollout(X0, U, P4, steps=3, sensitivities=('u',))
    with pytest.raises(ValueError, match=r"parameter sequence.*hold the parameters"):
        m.rollout(X0, [.1, .2], np.tile(P4, (3, 1, 1)), steps=3, sensitivities=('p',))
    with pytest.raises(ValueError, match=r"unknown group 'x'. Choose out of \('x0', 'u', 'p'\)"):
        m.rollout(X0, [.1, .2], P4, sensitivities=('x',))
    with pytest.raises(ValueError, match=r"no group selected"):
        m.rollout(X0, [.1, .2], P4, sensitivities=())
    q = Model('pendulum4').setup(dt=.5, solver='dopri5')
    _stub_sens(monkeypatch, q, 0, 4, log)
    with pytest.raises(ValueError, match=r"the model has no parameters, so there is no group 'p'. Leave it out"):
        q.rollout(np.zeros((2, 4)), [.5], sensitivities=('x0', 'p'))
    assert not log                                                   # nothing reached the library
    r = Model('robot6').setup(dt=.1, solver='dopri5')
    _stub_sens(monkeypatch, r, 0, 2, log)
    with pytest.raises(NotImplementedError, match=r"built\s+for up to 4 states; the model has 6. Use central differences"):
        r.rollout(np.zeros((2, 6)), [.1, .1], sensitivities=True)


def test_the_symbol_is_exported_and_checks_its_arguments():
    lib = _lib.lib()
    assert hasattr(lib, 'hilo_model_rollout_sens')
    rc = lib.hilo_model_rollout_sens(None, None, 1, 1, None, None, 0, 0, 7, None, None, None, None, None, None)
    assert rc == -1 and b'hilo_model_rollout_sens: NULL handle' in lib.hilo_last_error()


def test_the_ctypes_signature_matches_the_header():
    """Argument by argument: pointers, int64_t, int / int32_t of the prototype in include/hilo_hip.h against _lib.py's table; and the
    HILO_SENS_* bits and the width limit against what model.py uses."""
    header = open(os.path.join(ROOT, 'include', 'hilo_hip.h')).read()
    proto = re.search(r'int hilo_model_rollout_sens\((.*?)\);', header, re.S).group(1)
    kinds = []
    for arg in re.sub(r'/\*.*?\*/', '', proto, flags=re.S).split(','):
        arg = ' '.join(arg.split())
        kinds.append('ptr' if '*' in arg else ('i64' if arg.startswith('int64_t') else ('i32' if re.match(r'(int32_t|int) ', arg) else arg)))
    names = [a.split()[-1].lstrip('*') for a in re.sub(r'/\*.*?\*/', '', proto, flags=re.S).split(',')]
    assert names == ['kf', 'opts', 'batch', 'steps', 'x0', 'up', 'up_stride', 'up_step', 'wrt', 'X', 'Y', 'SX', 'SY', 'stats', 'stream']
    fn = _lib.lib().hilo_model_rollout_sens
    assert fn.restype is C.c_int and len(fn.argtypes) == len(kinds)
    for k, t in zip(kinds, fn.argtypes):
        if k == 'ptr':
            assert t is C.c_void_p or issubclass(t, C._Pointer), (k, t)
        else:
            assert t is {'i64': C.c_int64, 'i32': C.c_int}[k], (k, t)
    defs = dict(re.findall(r'#define (HILO_SENS_\w+|HILO_SIM_SENS_MAX_NX) (\d+)', header))
    assert (defs['HILO_SENS_X0'], defs['HILO_SENS_U'], defs['HILO_SENS_P']) == ('1', '2', '4')
    from hilo_mpc_amd.model import SENS_MAX_NX
    assert int(defs['HILO_SIM_SENS_MAX_NX']) == SENS_MAX_NX
