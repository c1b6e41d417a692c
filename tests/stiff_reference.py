"""Reference solutions for the tests of the implicit integrator `solver='bdf'` (not a test module): scipy on numpy right-hand
sides with their exact Jacobians.

The cases: Robertson's kinetics and van der Pol's oscillator (stiff; right-hand sides and analytic Jacobians below) and the cases
of tests/sim_reference.py through the oracle's right-hand sides and symbolic Jacobians (not stiff).  All run 10 sampling intervals.

The comparator is scipy's `BDF` on the same instance at the same tolerances, given the exact Jacobian, driven the way `solve_ivp`
drives it:
  inputs held     ONE integration over [0, steps dt]; the sampling instants are read off the dense output (`t_eval`), only the
                  end clips a step
  input sequence  one integration per sampling interval, started afresh at every instant
The bound of the accuracy tests is the rule of tests/sim_reference.py with the comparator exchanged: the error against the tight
solution, relative to |x| + abstol / reltol, is at most `sim_reference.FACTOR` times the larger of BDF's error and the
disagreement of two tight solutions - Radau at 1e-12 / 1e-15 against LSODA at 1e-11 / 1e-14 (both given the Jacobian) for the stiff
cases, `sim_reference.tight` against `tight_radau` for the others.  The cost bound: accepted steps and right-hand-side evaluations
at most a quarter above the comparator's."""
import numpy as np
from scipy.integrate import BDF, solve_ivp

from tests import sim_reference as sr

COST_MARGIN = 1.25

# name -> (x0, u, p, dt, intervals)
STIFF_CASES = {
    'robertson3': ([1., 0., 0.], [], [.04, 3e7, 1e4], 4., 10),
    'robertson3_long': ([1., 0., 0.], [], [.04, 3e7, 1e4], 100., 10),
    'vdp2': ([2., 0.], [], [100.], 20., 10),
    'vdp2_stiffer': ([2., 0.], [], [1000.], 200., 10),
}
CASES = dict(STIFF_CASES, **sr.CASES)


def _robertson(x, u, p):
    k1, k2, k3 = p
    return np.array([-k1 * x[0] + k3 * x[1] * x[2], k1 * x[0] - k3 * x[1] * x[2] - k2 * x[1] * x[1], k2 * x[1] * x[1]])


def _robertson_jac(x, u, p):
    k1, k2, k3 = p
    return np.array([[-k1, k3 * x[2], k3 * x[1]], [k1, -k3 * x[2] - 2. * k2 * x[1], -k3 * x[1]], [0., 2. * k2 * x[1], 0.]])


def _vdp(x, u, p):
    return np.array([x[1], p[0] * (1. - x[0] * x[0]) * x[1] - x[0]])


def _vdp_jac(x, u, p):
    return np.array([[0., 1.], [-2. * p[0] * x[0] * x[1] - 1., p[0] * (1. - x[0] * x[0])]])


def _square(x, u, p):
    return x * x


def _square_jac(x, u, p):
    return np.array([[2. * x[0]]])


_SYSTEMS = {'robertson3': (_robertson, _robertson_jac), 'vdp2': (_vdp, _vdp_jac), 'square': (_square, _square_jac)}


def is_stiff(case):
    return case.split('_')[0] in ('robertson3', 'vdp2')


def system(case):
    """(f(x, u, p), jac(x, u, p)) of a case's model, on 1-D arrays."""
    name = case.split('_')[0]
    if name in _SYSTEMS:
        return _SYSTEMS[name]
    om = sr.oracle_model(name)

    def f(x, u, p):
        return om.f(x[None, :], u[None, :], p[None, :], 1.)[0]

    def jac(x, u, p):
        if 'fx' not in om._cache:     # (OracleModel.fx differentiates the expressions anew at every call before it looks here)
            om.fx(x[None, :], u[None, :], p[None, :], 1.)
        return om._cache['fx'](x[None, :], u[None, :], p[None, :], 1.)[0]
    return f, jac


def _rows(v, steps):
    """(rows [steps, n], held) of an input or parameter vector given once or per interval."""
    v = np.asarray(v, dtype=float)
    if v.ndim == 2:
        return v, False
    return np.broadcast_to(v, (steps, v.size)), True


def _drive(fun, jac, x0, t_bound, t_eval, rtol, atol):
    """solve_ivp(method='BDF', jac=jac, t_eval=t_eval), with the accepted steps counted."""
    s = BDF(fun, 0., np.asarray(x0, dtype=float), t_bound, rtol=rtol, atol=atol, jac=jac)
    out, i, n_acc = [], 0, 0
    while s.status == 'running':
        msg = s.step()
        assert s.status != 'failed', msg
        n_acc += 1
        dense = s.dense_output()
        while i < len(t_eval) and t_eval[i] <= s.t:
            out.append(dense(t_eval[i]))
            i += 1
    assert i == len(t_eval)
    return np.array(out), np.array([n_acc, s.nfev, s.njev, s.nlu])


def bdf(case, x0, u, p, dt, steps, rtol, atol):
    """(x [steps + 1, nx] at the sampling instants, [accepted steps, nfev, njev, nlu]) of the comparator."""
    f, jac = system(case)
    U, held_u = _rows(u, steps)
    P, held_p = _rows(p, steps)
    x0 = np.asarray(x0, dtype=float)
    if held_u and held_p:
        x, counts = _drive(lambda t, x: f(x, U[0], P[0]), lambda t, x: jac(x, U[0], P[0]), x0, steps * dt,
                           dt * np.arange(1, steps + 1), rtol, atol)
        return np.vstack([x0[None], x]), counts
    x, counts = [x0], np.zeros(4, dtype=int)
    for k in range(steps):
        xk, ck = _drive(lambda t, x: f(x, U[k], P[k]), lambda t, x: jac(x, U[k], P[k]), x[-1], dt, np.array([dt]), rtol, atol)
        x.append(xk[0])
        counts += ck
    return np.array(x), counts


def _restarted(case, x0, u, p, dt, steps, method, rtol, atol):
    f, jac = system(case)
    U, _ = _rows(u, steps)
    P, _ = _rows(p, steps)
    x = [np.asarray(x0, dtype=float)]
    for k in range(steps):
        s = solve_ivp(lambda t, x: f(x, U[k], P[k]), (0., dt), x[-1], method=method, rtol=rtol, atol=atol,
                      jac=lambda t, x: jac(x, U[k], P[k]))
        assert s.success, s.message
        x.append(s.y[:, -1])
    return np.array(x)


def tight_pair(case, x0, u, p, dt, steps):
    """Two tight solutions by different methods."""
    if is_stiff(case):
        return (_restarted(case, x0, u, p, dt, steps, 'Radau', 1e-12, 1e-15),
                _restarted(case, x0, u, p, dt, steps, 'LSODA', 1e-11, 1e-14))
    om = sr._model(case.split('_')[0])
    return sr.tight(om, x0, u, p, dt, steps), sr.tight_radau(om, x0, u, p, dt, steps)


def bound(case, x0, u, p, dt, steps, rtol, atol, tight=None):
    """(tight solution, admissible error, BDF's error, disagreement of the tight solutions, BDF's counts)."""
    ref, other = tight_pair(case, x0, u, p, dt, steps) if tight is None else tight
    xb, counts = bdf(case, x0, u, p, dt, steps, rtol, atol)
    e_bdf, e_tight = sr.rel_err(xb, ref, rtol, atol), sr.rel_err(other, ref, rtol, atol)
    return ref, sr.FACTOR * max(e_bdf, e_tight), e_bdf, e_tight, counts


def _one(job):
    case, x0, u, p, dt, steps, tols = job
    tight = tight_pair(case, x0, u, p, dt, steps)
    return [bound(case, x0, u, p, dt, steps, rtol, atol, tight) for rtol, atol in tols]


def run_jobs(jobs):
    """`bound` for every job (case, x0, u, p, dt, steps, [(rtol, atol), ...]) - one list of results per job, the tight solutions
    computed once per job.  The jobs are spread over worker processes of a fresh interpreter that never opens the GPU, as
    `sim_reference.bounds_batch` does."""
    import os
    import pickle
    import subprocess
    import sys
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, 'in.pkl'), os.path.join(d, 'out.pkl')
        with open(fin, 'wb') as f:
            pickle.dump(jobs, f)
        subprocess.check_call([sys.executable, '-m', 'tests.stiff_reference', fin, fout], cwd=root)
        with open(fout, 'rb') as f:
            return pickle.load(f)


def bounds_batch(case, X0, U, P, dt, steps, rtol, atol):
    """`bound` for every row of X0 [n, nx] with U [n, nu] and P [n, np] held or [steps, n, .]: (tight solutions [steps + 1, n, nx],
    admissible errors [n], BDF's errors [n], tight-solution disagreements [n], BDF's counts [n, 4])."""
    X0, U, P = np.asarray(X0, dtype=float), np.asarray(U, dtype=float), np.asarray(P, dtype=float)
    jobs = [(case, X0[i], U[:, i] if U.ndim == 3 else U[i], P[:, i] if P.ndim == 3 else P[i], dt, steps, [(rtol, atol)])
            for i in range(X0.shape[0])]
    res = [r[0] for r in run_jobs(jobs)]
    return (np.stack([r[0] for r in res], axis=1), np.array([r[1] for r in res]), np.array([r[2] for r in res]),
            np.array([r[3] for r in res]), np.array([r[4] for r in res]))


def _main(fin, fout):
    import multiprocessing
    import os
    import pickle
    with open(fin, 'rb') as f:
        jobs = pickle.load(f)
    with multiprocessing.Pool(min(16, os.cpu_count() or 1, len(jobs))) as pool:
        res = pool.map(_one, jobs)
    with open(fout, 'wb') as f:
        pickle.dump(res, f)


if __name__ == '__main__':
    import sys
    _main(sys.argv[1], sys.argv[2])
