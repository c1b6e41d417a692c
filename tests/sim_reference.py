"""Reference solutions for the error-controlled integrator's tests (not a test module): scipy on the continuous right-hand sides
of oracle/models.py, sampling interval by sampling interval with the inputs held (zero-order hold), every solver started afresh
at each sampling instant.

The bound of the accuracy tests: the error of a trajectory against the tight solution (DOP853 at rtol 1e-13), measured relative to
|x| + abstol / reltol, is at most 10 times the larger of
  - the error scipy's RK45 makes on the same instance at the same tolerances, and
  - the disagreement of two tight solutions (DOP853 at 1e-13 against Radau at 1e-12).
The factor 10 covers what separates two implementations of one controller (the step size carried across sampling instants,
fused arithmetic); it is not tuned to any result."""
import numpy as np
from scipy.integrate import solve_ivp

FACTOR = 10.

# name -> (x0, u, p, dt, intervals): the cases of the accuracy tests.  The two cstr3 cases: the heated reactor (Q = 5e4) and the
# reactor left alone (Q = 0), both from the notebook's initial state.
CASES = {
    'pendulum4': ([0., 0., .3, 0.], [.5], [], .5, 10),
    'chemostat4': ([.1, 40., .5, .2], [.1, .2], [100., 4., 1., 0.], 4., 10),
    'cstr3_heated': ([1., 0., 400.], [5e4], [], 10., 10),
    'cstr3_idle': ([1., 0., 400.], [0.], [], 10., 10),
}


def oracle_model(case):
    from oracle import models as omodels
    return omodels.get(case.split('_')[0])


def rhs(om, u, p):
    u, p = np.asarray(u, dtype=float).reshape(1, -1), np.asarray(p, dtype=float).reshape(1, -1)
    return lambda t, x: om.f(x[None, :], u, p, 1.)[0]


def integrate(om, x0, u, p, dt, steps, method, rtol, atol):
    """x [steps + 1, nx] at the sampling instants; u [nu] held or [steps, nu]."""
    u = np.asarray(u, dtype=float)
    x = [np.asarray(x0, dtype=float)]
    for k in range(steps):
        uk = u[k] if u.ndim == 2 else u
        s = solve_ivp(rhs(om, uk, p), (0., dt), x[-1], method=method, rtol=rtol, atol=atol)
        assert s.success, s.message
        x.append(s.y[:, -1])
    return np.array(x)


def tight(om, x0, u, p, dt, steps):
    return integrate(om, x0, u, p, dt, steps, 'DOP853', 1e-13, 1e-15)


def tight_radau(om, x0, u, p, dt, steps):
    return integrate(om, x0, u, p, dt, steps, 'Radau', 1e-12, 1e-15)


def rel_err(x, ref, rtol, atol):
    """Largest error over the trajectory relative to |x| + abstol / reltol."""
    return float(np.max(np.abs(x - ref) / (np.abs(ref) + atol / rtol)))


def rk4_substeps(om, x0, u, p, dt, steps, n_sub=8):
    """The fixed-step map without error control: n_sub classic Runge-Kutta steps per sampling interval."""
    f = rhs(om, u, p)
    x = [np.asarray(x0, dtype=float)]
    h = dt / n_sub
    for _ in range(steps):
        z = x[-1]
        for _ in range(n_sub):
            k1 = f(0., z)
            k2 = f(0., z + .5 * h * k1)
            k3 = f(0., z + .5 * h * k2)
            k4 = f(0., z + h * k3)
            z = z + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
        x.append(z)
    return np.array(x)


def bound(om, x0, u, p, dt, steps, rtol, atol, ref=None):
    """(tight solution, admissible error): FACTOR x max(RK45's error at these tolerances, DOP853 vs Radau)."""
    ref = tight(om, x0, u, p, dt, steps) if ref is None else ref
    e45 = rel_err(integrate(om, x0, u, p, dt, steps, 'RK45', rtol, atol), ref, rtol, atol)
    e_tight = rel_err(tight_radau(om, x0, u, p, dt, steps), ref, rtol, atol)
    return ref, FACTOR * max(e45, e_tight), e45, e_tight


class _Square:
    """dx/dt = x^2 (leaves every bound at t = 1 / x0): not a model of the oracle's zoo."""
    @staticmethod
    def f(x, u, p, dt):
        return np.asarray(x, dtype=float) ** 2


def _model(name):
    return _Square if name == 'square' else oracle_model(name)


def _one(job):
    name, x0, u, p, dt, steps, rtol, atol = job
    ref, admissible, e45, e_tight = bound(_model(name), x0, u, p, dt, steps, rtol, atol)
    return ref, admissible, e45, e_tight


def bounds_batch(name, X0, U, P, dt, steps, rtol, atol):
    """`bound` for every row of X0 [n, nx] with U [n, nu] held or [steps, n, nu], P [n, np]: (tight solutions [steps + 1, n, nx],
    admissible errors [n], RK45's errors [n], DOP853-vs-Radau [n]).  The instances are independent and Radau at 1e-12 takes seconds
    each, so they are spread over worker processes - of a fresh interpreter that never opens the GPU, not forks of the test
    process."""
    import os
    import subprocess
    import sys
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, 'in.npz'), os.path.join(d, 'out.npz')
        np.savez(fin, name=name, X0=X0, U=U, P=P, dt=dt, steps=steps, rtol=rtol, atol=atol)
        subprocess.check_call([sys.executable, '-m', 'tests.sim_reference', fin, fout], cwd=root)
        with np.load(fout) as z:
            return z['ref'], z['admissible'], z['e45'], z['e_tight']


def _main(fin, fout):
    import multiprocessing
    import os
    with np.load(fin) as z:
        name, X0, U, P = str(z['name']), z['X0'], z['U'], z['P']
        dt, steps, rtol, atol = float(z['dt']), int(z['steps']), float(z['rtol']), float(z['atol'])
    jobs = [(name, X0[i], U[:, i] if U.ndim == 3 else U[i], P[i], dt, steps, rtol, atol) for i in range(X0.shape[0])]
    with multiprocessing.Pool(min(16, os.cpu_count() or 1, len(jobs))) as pool:
        res = pool.map(_one, jobs)
    np.savez(fout, ref=np.stack([r[0] for r in res], axis=1), admissible=np.array([r[1] for r in res]),
             e45=np.array([r[2] for r in res]), e_tight=np.array([r[3] for r in res]))


if __name__ == '__main__':
    import sys
    _main(sys.argv[1], sys.argv[2])
