"""Reference solutions for the tests of time-variant models (not a test module): scipy with t in the right-hand side.

The cases
  forced2    dx1/dt = x2, dx2/dt = -k x1 - c x2 + u sin(w t), y = x1 + cos(t); p = (k, c, w)
  prothero1  dx/dt = -lam (x - cos t) - sin t (Prothero and Robinson's problem: stiff for a large lam), p = (lam);
             exact solution cos t + (x0 - cos t0) exp(-lam (t - t0))
  poly       dx/dt = t^m: a Runge-Kutta method of order s integrates it exactly for m < s
Sampling interval k starts at t_k = t0 + k dt; the inputs are held over it, time is not.

The bounds are the rules of tests/sim_reference.py (explicit pair: FACTOR x the larger of RK45's error at the same tolerances and
the disagreement of DOP853 at 1e-13 with Radau at 1e-12) and tests/stiff_reference.py (implicit method: FACTOR x the larger of the
error of scipy's BDF, given the exact Jacobian and driven like solve_ivp, and the disagreement of Radau at 1e-12 with LSODA at
1e-11; cost at most COST_MARGIN above BDF's), with their constants, error measure and BDF driver imported from there.  scipy's
BDF is handed the right-hand side on the clock of its own integration, s -> f(t_start + s, x): the same instance, and the clock the
device method keeps.

Tolerances.  forced2 runs at (1e-8, 1e-10) and (1e-10, 1e-12) like the other explicit cases.  prothero1 runs at (1e-6, 1e-8) and
(1e-8, 1e-10), the pairs of tests/stiff_reference.py: its rule asks the two tight solutions to agree ten times below the
comparator's error, and they agree to about 3e-12 - below a tenth of BDF's error at 1e-8 (about 6e-10), not of what BDF reaches at
1e-10.  `test_preconditions` of tests/test_timevar_host.py checks this on the references alone."""
import numpy as np
from scipy.integrate import solve_ivp

from tests import sim_reference as sr
from tests import stiff_reference as st

TOLS_EXPLICIT = [(1e-8, 1e-10), (1e-10, 1e-12)]
TOLS_STIFF = [(1e-6, 1e-8), (1e-8, 1e-10)]

# name -> (x0, u, p, dt, intervals, t0)
CASES = {
    'forced2': ([1., 0.], [1.], [4., .4, 3.], .5, 10, 2.5),
    'forced2_t0': ([1., 0.], [1.], [4., .4, 3.], .5, 10, 0.),
    'prothero1': ([np.cos(1.) + .1], [], [1e4], 1., 10, 1.),
}


def _forced2(t, x, u, p):
    return np.array([x[1], -p[0] * x[0] - p[1] * x[1] + u[0] * np.sin(p[2] * t)])


def _forced2_jac(t, x, u, p):
    return np.array([[0., 1.], [-p[0], -p[1]]])


def forced2_meas(t, x, u, p):
    """y = x1 + cos(t) for x [..., 2] and t broadcast against its leading axes."""
    return x[..., :1] + np.cos(t)[..., None]


def _prothero(t, x, u, p):
    return np.array([-p[0] * (x[0] - np.cos(t)) - np.sin(t)])


def _prothero_jac(t, x, u, p):
    return np.array([[-p[0]]])


SYSTEMS = {'forced2': (_forced2, _forced2_jac), 'prothero1': (_prothero, _prothero_jac)}


def system(case):
    return SYSTEMS[case.split('_')[0]]


def prothero_exact(t, x0, lam, t0):
    return np.cos(t) + (x0 - np.cos(t0)) * np.exp(-lam * (t - t0))


def integrate(case, x0, u, p, dt, steps, t0, method, rtol, atol):
    """x [steps + 1, nx] at the sampling instants, every solver started afresh at each of them over [t_k, t_k + dt]; u and p held
    ([n]) or one row per interval ([steps, n])."""
    f, jac = system(case)
    U, _ = st._rows(u, steps)
    P, _ = st._rows(p, steps)
    x = [np.asarray(x0, dtype=float)]
    for k in range(steps):
        tk = t0 + k * dt
        kw = {} if method in ('RK45', 'DOP853') else {'jac': lambda t, y: jac(t, y, U[k], P[k])}
        s = solve_ivp(lambda t, y: f(t, y, U[k], P[k]), (tk, tk + dt), x[-1], method=method, rtol=rtol, atol=atol, **kw)
        assert s.success, s.message
        x.append(s.y[:, -1])
    return np.array(x)


def tight_explicit(case, x0, u, p, dt, steps, t0):
    return (integrate(case, x0, u, p, dt, steps, t0, 'DOP853', 1e-13, 1e-15),
            integrate(case, x0, u, p, dt, steps, t0, 'Radau', 1e-12, 1e-15))


def tight_stiff(case, x0, u, p, dt, steps, t0):
    return (integrate(case, x0, u, p, dt, steps, t0, 'Radau', 1e-12, 1e-15),
            integrate(case, x0, u, p, dt, steps, t0, 'LSODA', 1e-11, 1e-14))


def bound_explicit(case, x0, u, p, dt, steps, t0, rtol, atol, tight=None):
    """sim_reference's rule: (tight solution, admissible error, RK45's error, disagreement of the tight solutions)."""
    ref, other = tight_explicit(case, x0, u, p, dt, steps, t0) if tight is None else tight
    e45 = sr.rel_err(integrate(case, x0, u, p, dt, steps, t0, 'RK45', rtol, atol), ref, rtol, atol)
    e_tight = sr.rel_err(other, ref, rtol, atol)
    return ref, sr.FACTOR * max(e45, e_tight), e45, e_tight


def bdf(case, x0, u, p, dt, steps, t0, rtol, atol):
    """stiff_reference.bdf with the time: (x [steps + 1, nx], [accepted steps, nfev, njev, nlu]) of scipy's BDF - inputs held: one
    integration over [t0, t0 + steps dt] read off its dense output; a sequence: one integration per interval from t_k."""
    f, jac = system(case)
    U, held_u = st._rows(u, steps)
    P, held_p = st._rows(p, steps)
    x0 = np.asarray(x0, dtype=float)
    if held_u and held_p:
        x, counts = st._drive(lambda s, y: f(t0 + s, y, U[0], P[0]), lambda s, y: jac(t0 + s, y, U[0], P[0]), x0, steps * dt,
                              dt * np.arange(1, steps + 1), rtol, atol)
        return np.vstack([x0[None], x]), counts
    x, counts = [x0], np.zeros(4, dtype=int)
    for k in range(steps):
        tk = t0 + k * dt
        xk, ck = st._drive(lambda s, y: f(tk + s, y, U[k], P[k]), lambda s, y: jac(tk + s, y, U[k], P[k]), x[-1], dt, np.array([dt]),
                           rtol, atol)
        x.append(xk[0])
        counts += ck
    return np.array(x), counts


def bound_stiff(case, x0, u, p, dt, steps, t0, rtol, atol, tight=None):
    """stiff_reference's rule: (tight solution, admissible error, BDF's error, disagreement of the tight solutions, BDF's counts)."""
    ref, other = tight_stiff(case, x0, u, p, dt, steps, t0) if tight is None else tight
    xb, counts = bdf(case, x0, u, p, dt, steps, t0, rtol, atol)
    e_bdf, e_tight = sr.rel_err(xb, ref, rtol, atol), sr.rel_err(other, ref, rtol, atol)
    return ref, sr.FACTOR * max(e_bdf, e_tight), e_bdf, e_tight, counts


# ---- the fixed-step recipe with stage times, restated in numpy for batches (f(t, X, U, P) on [B, .] arrays) -----------------------
ERK_C = {1: [0.], 2: [0., .5], 3: [0., .5, 1.], 4: [0., .5, .5, 1.]}
ERK_A = {1: [[]], 2: [[], [.5]], 3: [[], [.5], [-1., 2.]], 4: [[], [.5], [0., .5], [0., 0., 1.]]}
ERK_B = {1: [1.], 2: [0., 1.], 3: [1. / 6, 2. / 3, 1. / 6], 4: [1. / 6, 1. / 3, 1. / 3, 1. / 6]}


def erk_rollout(f, X0, U, P, dt, steps, t0, order, n_sub):
    """[steps + 1, B, nx]: `n_sub` explicit Runge-Kutta sub-steps of `order` per sampling interval; stage i of a sub-step of length
    h that starts at s is evaluated at s + c_i h; interval k starts at t0 + k dt, sub-step j of it at that + j h."""
    X = [np.asarray(X0, dtype=float)]
    h = dt / n_sub
    for k in range(steps):
        Uk = U[k] if np.ndim(U) == 3 else U
        Pk = P[k] if np.ndim(P) == 3 else P
        z = X[-1]
        for j in range(n_sub):
            s = (t0 + k * dt) + j * h
            ks = []
            for i in range(order):
                zi = z
                for q, a in enumerate(ERK_A[order][i]):
                    if a != 0.:
                        zi = zi + (h * a) * ks[q]
                ks.append(f(s + ERK_C[order][i] * h, zi, Uk, Pk))
            z = z + sum((h * b) * kq for b, kq in zip(ERK_B[order], ks) if b != 0.)
        X.append(z)
    return np.array(X)


def forced2_batch(t, X, U, P):
    return np.stack([X[:, 1], -P[:, 0] * X[:, 0] - P[:, 1] * X[:, 1] + U[:, 0] * np.sin(P[:, 2] * t)], axis=1)


# ---- batches of bounds in worker processes of a fresh interpreter that never opens the GPU (as sim_reference.bounds_batch) ---------
def _one(job):
    kind, case, x0, u, p, dt, steps, t0, tols = job
    if kind == 'explicit':
        tight = tight_explicit(case, x0, u, p, dt, steps, t0)
        return [bound_explicit(case, x0, u, p, dt, steps, t0, rtol, atol, tight) for rtol, atol in tols]
    tight = tight_stiff(case, x0, u, p, dt, steps, t0)
    return [bound_stiff(case, x0, u, p, dt, steps, t0, rtol, atol, tight) for rtol, atol in tols]


def run_jobs(jobs):
    """One list of results (one per tolerance pair) per job (kind, case, x0, u, p, dt, steps, t0, [(rtol, atol), ...]); the tight
    solutions are computed once per job."""
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
        subprocess.check_call([sys.executable, '-m', 'tests.timevar_reference', fin, fout], cwd=root)
        with open(fout, 'rb') as f:
            return pickle.load(f)


def bounds_batch(kind, case, X0, U, P, dt, steps, t0, tols):
    """Per tolerance pair: (tight solutions [steps + 1, n, nx], admissible errors [n], the comparator's errors [n], tight-solution
    disagreements [n], and for kind 'stiff' BDF's counts [n, 4]) for every row of X0 [n, nx], U and P [n, .] or [steps, n, .]."""
    X0, U, P = np.asarray(X0, dtype=float), np.asarray(U, dtype=float), np.asarray(P, dtype=float)
    jobs = [(kind, case, X0[i], U[:, i] if U.ndim == 3 else U[i], P[:, i] if P.ndim == 3 else P[i], dt, steps, t0, list(tols))
            for i in range(X0.shape[0])]
    res = run_jobs(jobs)
    out = []
    for q in range(len(tols)):
        rows = [r[q] for r in res]
        out.append((np.stack([r[0] for r in rows], axis=1),) + tuple(np.array([r[c] for r in rows]) for c in range(1, len(rows[0]))))
    return out


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
