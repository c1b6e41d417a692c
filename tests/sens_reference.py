"""Reference solutions for the tests of the roll-out with forward sensitivities (not a test module): scipy on the AUGMENTED system

    dx/dt = f(x, u, p),   dS/dt = f_x S + f_theta,   theta = [x0; u; p] restricted to the selected groups,   S(0) = [I | 0 | 0]

built with sympy from the right-hand sides of oracle/models.py, integrated like tests/sim_reference.py: sampling interval by
sampling interval with the inputs held, every solver started afresh at each sampling instant.  The augmented vector is
[x; column 0 of S; column 1; ...] - the kernel's layout of SX, [NS][n_x].

The bound is sim_reference's with the augmented vector in place of the state: the error of an augmented trajectory against the tight
solution (DOP853 at 1e-13 / 1e-15), measured with `rel_err` over all components, is at most FACTOR (the 10 of sim_reference, for the
reasons given there) times the larger of
  - the error scipy's RK45 makes on the same augmented instance at the same tolerances, and
  - the disagreement of DOP853 and Radau (1e-12) on the augmented system.
Radau is slow here (finite-difference Jacobians of 24 to 44 components), so that second term is computed at the NOMINAL instance of a
case only and used for the whole batch; it lies four to five orders below RK45's error (tests/test_sens_host.py asserts so)."""
import functools

import numpy as np
import sympy as sp
from scipy.integrate import solve_ivp

from tests import sim_reference as sr

FACTOR = sr.FACTOR
GROUPS = ('x0', 'u', 'p')


def groups_of(om, groups=None):
    """The selected groups in the order x0, u, p; None: every group the model has."""
    have = {'x0': om.nx, 'u': om.nu, 'p': om.np_}
    if groups is None:
        return tuple(g for g in GROUPS if have[g])
    return tuple(g for g in GROUPS if g in groups)


def n_columns(om, groups):
    have = {'x0': om.nx, 'u': om.nu, 'p': om.np_}
    return sum(have[g] for g in groups)


@functools.lru_cache(maxsize=None)
def _augmented(name, groups):
    om = sr.oracle_model(name)
    nx, ns = om.nx, n_columns(om, groups)
    f = sp.Matrix(om.ode)
    S = sp.Matrix(nx, ns, lambda i, j: sp.Symbol(f's_{i}_{j}'))
    cols = []
    for g in groups:
        if g == 'x0':
            cols += [sp.zeros(nx, 1)] * nx
        else:
            cols += [f.diff(s) for s in (om.u if g == 'u' else om.p)]
    F_theta = sp.Matrix.hstack(*cols) if cols else sp.zeros(nx, 0)
    dS = f.jacobian(om.x) * S + F_theta
    exprs = list(f) + [dS[i, j] for j in range(ns) for i in range(nx)]
    args = list(om.x) + [S[i, j] for j in range(ns) for i in range(nx)] + list(om.u) + list(om.p)
    fn = sp.lambdify(args, exprs, modules='numpy', cse=True)
    return fn, nx, ns


def seed(om, groups, x0):
    """[x0; vec S(0)]"""
    nx, ns = om.nx, n_columns(om, groups)
    S0 = np.zeros((ns, nx))
    if 'x0' in groups:
        S0[:nx] = np.eye(nx)
    return np.concatenate([np.asarray(x0, dtype=float), S0.ravel()])


def integrate(name, groups, x0, u, p, dt, steps, method, rtol, atol):
    """The augmented vector [steps + 1, nx (1 + ns)] at the sampling instants; u [nu] held or [steps, nu] (then without 'u')."""
    om = sr.oracle_model(name)
    fn, nx, ns = _augmented(name, tuple(groups))
    u, p = np.asarray(u, dtype=float), [float(v) for v in np.asarray(p, dtype=float).ravel()]
    assert u.ndim == 1 or 'u' not in groups
    w = [seed(om, groups, x0)]
    for k in range(steps):
        uk = [float(v) for v in (u[k] if u.ndim == 2 else u)]
        s = solve_ivp(lambda t, y: np.array(fn(*y, *uk, *p), dtype=float), (0., dt), w[-1], method=method, rtol=rtol, atol=atol)
        assert s.success, s.message
        w.append(s.y[:, -1])
    return np.array(w)


def split(w, nx):
    """augmented [..., nx (1 + ns)] -> x [..., nx], S [..., ns, nx]"""
    w = np.asarray(w)
    return w[..., :nx], w[..., nx:].reshape(w.shape[:-1] + (-1, nx))


def join(x, S):
    """x [..., nx], S [..., ns, nx] (the kernel's layout) -> augmented [..., nx (1 + ns)]"""
    x, S = np.asarray(x), np.asarray(S)
    return np.concatenate([x, S.reshape(S.shape[:-2] + (-1,))], axis=-1)


def tight(name, groups, x0, u, p, dt, steps):
    return integrate(name, groups, x0, u, p, dt, steps, 'DOP853', 1e-13, 1e-15)


@functools.lru_cache(maxsize=None)
def _nominal_pair(case, groups, steps):
    """(DOP853, Radau) on the nominal instance of a case of sim_reference.CASES: the slow term, once per process."""
    x0, u, p, dt, n = sr.CASES[case]
    steps = n if steps is None else steps
    name = case.split('_')[0]
    return (tight(name, groups, x0, u, p, dt, steps), integrate(name, groups, x0, u, p, dt, steps, 'Radau', 1e-12, 1e-15))


def e_tight_nominal(case, groups, rtol, atol, steps=None):
    a, b = _nominal_pair(case, tuple(groups), steps)
    return sr.rel_err(b, a, rtol, atol)


def bound(name, groups, x0, u, p, dt, steps, rtol, atol, e_tight):
    """(tight augmented solution, admissible error, RK45's error) of one instance; e_tight: e_tight_nominal of its case."""
    ref = tight(name, groups, x0, u, p, dt, steps)
    e45 = sr.rel_err(integrate(name, groups, x0, u, p, dt, steps, 'RK45', rtol, atol), ref, rtol, atol)
    return ref, FACTOR * max(e45, e_tight), e45


def meas_sens(name, groups, x, S, u, p):
    """h_x S + h_theta [ns, ny] (the kernel's layout of SY) at one state x [nx] with S [ns, nx]."""
    om = sr.oracle_model(name)
    h = sp.Matrix(om.meas)
    key = ('meas', name, tuple(groups))
    if key not in _MEAS:
        theta = []
        for g in groups:
            theta += [None] * om.nx if g == 'x0' else list(om.u if g == 'u' else om.p)
        H_theta = sp.Matrix.hstack(*[sp.zeros(len(om.meas), 1) if s is None else h.diff(s) for s in theta])
        args = list(om.x) + list(om.u) + list(om.p)
        _MEAS[key] = (sp.lambdify(args, h.jacobian(om.x), modules='numpy'), sp.lambdify(args, H_theta, modules='numpy'))
    hx, ht = _MEAS[key]
    vals = [float(v) for v in np.concatenate([np.ravel(x), np.ravel(u), np.ravel(p)])]
    return (np.asarray(hx(*vals), dtype=float) @ np.asarray(S).T + np.asarray(ht(*vals), dtype=float)).T


_MEAS = {}


def _one(job):
    if job[0] == 'nominal':
        _, case, groups, rtol, atol, steps = job
        return e_tight_nominal(case, groups, rtol, atol, steps)
    name, groups, x0, u, p, dt, steps, rtol, atol = job
    ref = tight(name, groups, x0, u, p, dt, steps)
    return ref, sr.rel_err(integrate(name, groups, x0, u, p, dt, steps, 'RK45', rtol, atol), ref, rtol, atol)


def bounds_batch(name, groups, X0, U, P, dt, steps, rtol, atol, nominal_case=None, e_tight=0.):
    """`bound` for every row of X0 [n, nx] with U [n, nu] held or [steps, n, nu], P [n, np]: (tight augmented solutions
    [steps + 1, n, nx (1 + ns)], admissible errors [n], RK45's errors [n], the DOP853-vs-Radau term).  nominal_case: the case of
    sim_reference.CASES whose nominal instance gives that term, over `steps` intervals (None: the value passed as e_tight).  The jobs
    are spread over worker processes of a fresh interpreter that never opens the GPU, as in sim_reference.bounds_batch."""
    import os
    import subprocess
    import sys
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, 'in.npz'), os.path.join(d, 'out.npz')
        np.savez(fin, name=name, groups=np.array(list(groups)), X0=X0, U=U, P=P, dt=dt, steps=steps, rtol=rtol, atol=atol,
                 nominal_case=nominal_case or '')
        subprocess.check_call([sys.executable, '-m', 'tests.sens_reference', fin, fout], cwd=root)
        with np.load(fout) as z:
            ref, e45 = z['ref'], z['e45']
            e_tight = float(z['e_tight']) if nominal_case else e_tight
    return ref, FACTOR * np.maximum(e45, e_tight), e45, e_tight


def _main(fin, fout):
    import multiprocessing
    import os
    with np.load(fin) as z:
        name, groups, X0, U, P = str(z['name']), tuple(str(g) for g in z['groups']), z['X0'], z['U'], z['P']
        dt, steps, rtol, atol = float(z['dt']), int(z['steps']), float(z['rtol']), float(z['atol'])
        nominal_case = str(z['nominal_case'])
    jobs = [('nominal', nominal_case, groups, rtol, atol, steps)] if nominal_case else []   # the slowest job first
    jobs += [(name, groups, X0[i], U[:, i] if U.ndim == 3 else U[i], P[i], dt, steps, rtol, atol) for i in range(X0.shape[0])]
    with multiprocessing.Pool(min(16, os.cpu_count() or 1, len(jobs))) as pool:
        res = pool.map(_one, jobs, chunksize=1)
    e_tight = res.pop(0) if nominal_case else 0.
    np.savez(fout, ref=np.stack([r[0] for r in res], axis=1), e45=np.array([r[1] for r in res]), e_tight=e_tight)


if __name__ == '__main__':
    import sys
    _main(sys.argv[1], sys.argv[2])
