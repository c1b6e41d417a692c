"""Reference solutions for the tests of `solver='idas'` (not a test module): scipy on the REDUCED ordinary differential equation
dx/dt = f(x, zeta(x, u, p), u, p) of each semi-explicit index-1 DAE  dx/dt = f(x, z, u, p),  0 = g(x, z, u, p).

zeta is in closed form, or found by `scipy.optimize.brentq` on a monotone scalar equation to 1e-15 and polished by Newton sweeps
on g with the analytic dg/dz.  The Jacobian of the reduced right-hand side is exact, by the implicit-function theorem:
f_x - f_z g_z^-1 g_x.  The comparator is scipy's `BDF` on the reduced equation, driven as tests/stiff_reference.py drives it (inputs
held: one integration, the sampling instants off the dense output; an input sequence: one integration per interval).  The tight
pair is Radau at 1e-12 / 1e-15 against LSODA at 1e-11 / 1e-14, restarted at every sampling instant.  The reference of z is
zeta(x_tight).

The bound, for x and for z separately: the error against the tight solution, relative to |.| + abstol / reltol
(`sim_reference.rel_err`), is at most `sim_reference.FACTOR` times the larger of the error of scipy's BDF at the same tolerances and
the disagreement of the two tight solutions."""
import numpy as np
from scipy.integrate import solve_ivp
from scipy.optimize import brentq

from tests import sim_reference as sr
from tests import stiff_reference as st

ROB = [.04, 3e7, 1e4]
# name -> (x0, u, p, dt, intervals); all of 10 sampling intervals or fewer
CASES = {
    'lin1': ([1.], [], [], .2, 10),
    'robertson_dae': ([1., 0.], [], ROB, 4., 10),
    'robertson_dae_long': ([1., 0.], [], ROB, 100., 10),
    'cubic': ([2.], [.5], [], .5, 10),
    'alg_u': ([.5, 1.], [.3], [], .5, 10),
    'meas_only': ([0., 0., .3, 0.], [.5], [], .5, 10),
    'wide8': ([.5, 1., .2, -.1, .3], [.3], [], .5, 10),
}
NZ = {'lin1': 1, 'robertson_dae': 1, 'cubic': 1, 'alg_u': 2, 'meas_only': 1, 'wide8': 3}
SEQUENCE_CASES = ('cubic', 'alg_u')


def sequence(case, steps, seed=5):
    """The input sequence [steps, nu] of a case."""
    return np.random.default_rng(seed).uniform(-.5, .8, (steps, 1))


def _alg_u_z(x1, x2, u):
    # z2 = x2 - .5 sin z1 in the first equation: z1 + .5 x1 sin z1 = x1 x2 + u, monotone in z1 for |x1| < 2
    assert abs(x1) < 2.
    rhs = x1 * x2 + u
    span = abs(rhs) + abs(x1) + 1.
    z1 = brentq(lambda s: s + .5 * x1 * np.sin(s) - rhs, -span, span, xtol=1e-15, rtol=4 * np.finfo(float).eps)
    return z1, x2 - .5 * np.sin(z1)


class _Sys:
    """One DAE: parts(x, z, u, p) -> (f, g, f_x, f_z, g_x, g_z) on 1-D arrays, guess(x, u, p) -> z close to the root."""
    def __init__(self, parts, guess):
        self.parts, self.guess = parts, guess

    def zeta(self, x, u, p):
        z = np.asarray(self.guess(x, u, p), dtype=float)
        for _ in range(3):                                   # the start is at round-off of the root already
            _, g, _, _, _, gz = self.parts(x, z, u, p)
            z = z - np.linalg.solve(gz, g)
        return z

    def f(self, x, u, p):
        return self.parts(x, self.zeta(x, u, p), u, p)[0]

    def jac(self, x, u, p):
        _, _, fx, fz, gx, gz = self.parts(x, self.zeta(x, u, p), u, p)
        return fx - fz @ np.linalg.solve(gz, gx)

    def g(self, x, z, u, p):
        return self.parts(x, z, u, p)[1]


def _lin1(x, z, u, p):
    return (np.array([-x[0] + z[0]]), np.array([z[0] - 2. * x[0]]), np.array([[-1.]]), np.array([[1.]]), np.array([[-2.]]),
            np.array([[1.]]))


def _robertson(x, z, u, p):
    k1, k2, k3 = p
    r = k3 * x[1] * z[0]
    return (np.array([-k1 * x[0] + r, k1 * x[0] - r - k2 * x[1] * x[1]]), np.array([x[0] + x[1] + z[0] - 1.]),
            np.array([[-k1, k3 * z[0]], [k1, -k3 * z[0] - 2. * k2 * x[1]]]), np.array([[k3 * x[1]], [-k3 * x[1]]]),
            np.array([[1., 1.]]), np.array([[1.]]))


def _cubic(x, z, u, p):
    return (np.array([-z[0] + u[0]]), np.array([z[0] ** 3 + z[0] - x[0]]), np.array([[0.]]), np.array([[-1.]]), np.array([[-1.]]),
            np.array([[3. * z[0] ** 2 + 1.]]))


def _cubic_guess(x, u, p):
    s = np.sqrt(x[0] * x[0] / 4. + 1. / 27.)
    return [np.cbrt(x[0] / 2. + s) + np.cbrt(x[0] / 2. - s)]


def _alg_u(x, z, u, p):
    return (np.array([-x[0] + z[0], z[1] - x[1]]), np.array([z[0] - x[0] * z[1] - u[0], z[1] + .5 * np.sin(z[0]) - x[1]]),
            -np.eye(2), np.eye(2), np.array([[-z[1], 0.], [0., -1.]]), np.array([[1., -x[0]], [.5 * np.cos(z[0]), 1.]]))


def _wide8(x, z, u, p):
    f2, g2, fx2, fz2, gx2, gz2 = _alg_u(x[:2], z[:2], u, p)
    f = np.concatenate([f2, [-2. * x[2] + x[0], -3. * x[3] + x[2] + z[2], -x[4] + x[3]]])
    g = np.concatenate([g2, [z[2] - .5 * x[4] - z[1]]])
    fx, fz, gx, gz = np.zeros((5, 5)), np.zeros((5, 3)), np.zeros((3, 5)), np.zeros((3, 3))
    fx[:2, :2], fz[:2, :2], gx[:2, :2], gz[:2, :2] = fx2, fz2, gx2, gz2
    fx[2, 2], fx[2, 0] = -2., 1.
    fx[3, 3], fx[3, 2], fz[3, 2] = -3., 1., 1.
    fx[4, 4], fx[4, 3] = -1., 1.
    gx[2, 4], gz[2, 1], gz[2, 2] = -.5, -1., 1.
    return f, g, fx, fz, gx, gz


def _wide8_guess(x, u, p):
    z1, z2 = _alg_u_z(x[0], x[1], u[0])
    return [z1, z2, .5 * x[4] + z2]


class _MeasOnly:
    """pendulum4_dae of tests/problems.py: the oracle's pendulum4 with the height of the tip, 0 = h + l cos(theta) - z, as an
    algebraic state that only the measurement names."""
    def __init__(self):
        self.f, self.jac = st.system('pendulum4')

    @staticmethod
    def zeta(x, u, p):
        return np.array([.5 + np.cos(x[2])])

    @staticmethod
    def g(x, z, u, p):
        return np.array([.5 + np.cos(x[2]) - z[0]])


def system(case):
    name = 'robertson_dae' if case.startswith('robertson_dae') else case
    if name == 'meas_only':
        return _MeasOnly()
    return {'lin1': _Sys(_lin1, lambda x, u, p: [2. * x[0]]),
            'robertson_dae': _Sys(_robertson, lambda x, u, p: [1. - x[0] - x[1]]),
            'cubic': _Sys(_cubic, _cubic_guess),
            'alg_u': _Sys(_alg_u, lambda x, u, p: _alg_u_z(x[0], x[1], u[0])),
            'wide8': _Sys(_wide8, _wide8_guess)}[name]


def symbolic_model(case):
    """The case as a `hilo_mpc_amd.Model` written as expressions (not set up).  Every model measures its states' first entry and all
    of its algebraic states, so that y is checked against the recorded pair."""
    from hilo_mpc_amd import Model
    from hilo_mpc_amd.expr import cos, sin
    name = 'robertson_dae' if case.startswith('robertson_dae') else case
    m = Model(name=name)
    if name == 'lin1':
        x, z = m.set_dynamical_states(['x']), m.set_algebraic_states(['z'])
        m.set_dynamical_equations([-x[0] + z[0]])
        m.set_algebraic_equations([z[0] - 2. * x[0]])
    elif name == 'robertson_dae':
        x, z, k = m.set_dynamical_states(['a', 'b']), m.set_algebraic_states(['c']), m.set_parameters(['k1', 'k2', 'k3'])
        m.set_dynamical_equations([-k[0] * x[0] + k[2] * x[1] * z[0], k[0] * x[0] - k[2] * x[1] * z[0] - k[1] * x[1] * x[1]])
        m.set_algebraic_equations([x[0] + x[1] + z[0] - 1.])
    elif name == 'cubic':
        x, z, u = m.set_dynamical_states(['x']), m.set_algebraic_states(['z']), m.set_inputs(['u'])
        m.set_dynamical_equations([-z[0] + u[0]])
        m.set_algebraic_equations([z[0] * z[0] * z[0] + z[0] - x[0]])
    elif name in ('alg_u', 'wide8'):
        wide = name == 'wide8'
        x = m.set_dynamical_states(['x1', 'x2'] + (['x3', 'x4', 'x5'] if wide else []))
        z = m.set_algebraic_states(['z1', 'z2'] + (['z3'] if wide else []))
        u = m.set_inputs(['u'])
        ode = [-x[0] + z[0], z[1] - x[1]]
        alg = [z[0] - x[0] * z[1] - u[0], z[1] + .5 * sin(z[0]) - x[1]]
        if wide:
            ode += [-2. * x[2] + x[0], -3. * x[3] + x[2] + z[2], -x[4] + x[3]]
            alg += [z[2] - .5 * x[4] - z[1]]
        m.set_dynamical_equations(ode)
        m.set_algebraic_equations(alg)
    elif name == 'meas_only':
        x, z, u = m.set_dynamical_states(['x', 'v', 'theta', 'omega']), m.set_algebraic_states(['y']), m.set_inputs(['F'])
        M, mm, l, g, h = 5.0, 1.0, 1.0, 9.81, .5
        s, c = sin(x[2]), cos(x[2])
        dv = 1.0 / (M + mm - mm * c) * (mm * g * s - mm * l * s * x[3] * x[3] + u[0])
        m.set_dynamical_equations([x[1], dv, x[3], 1.0 / l * (dv * c + g * s)])
        m.set_algebraic_equations([h + l * c - z[0]])
    else:
        raise KeyError(case)
    m.set_measurement_equations([x[0]] + [z[i] for i in range(NZ[name])])
    return m


def zetas(case, x, u, p, steps):
    """z [steps + 1, nz] = zeta(x[k]) with the inputs under which instant k was REACHED (row 0: those of the first interval) - what
    the roll-out records."""
    s = system(case)
    U, _ = st._rows(u, steps)
    P, _ = st._rows(p, steps)
    return np.array([s.zeta(x[k], U[max(k - 1, 0)], P[max(k - 1, 0)]) for k in range(steps + 1)])


def residual(case, x, z, u, p, steps):
    """|g(x[k], z[k])| / (1 + |z[k]|), largest over the trajectory, with the inputs of `zetas`."""
    s = system(case)
    U, _ = st._rows(u, steps)
    P, _ = st._rows(p, steps)
    return max(float(np.max(np.abs(s.g(x[k], z[k], U[max(k - 1, 0)], P[max(k - 1, 0)])) / (1. + np.max(np.abs(z[k])))))
               for k in range(steps + 1))


def bdf(case, x0, u, p, dt, steps, rtol, atol):
    """scipy's BDF on the reduced equation: (x [steps + 1, nx], [accepted steps, nfev, njev, nlu])."""
    s = system(case)
    U, held_u = st._rows(u, steps)
    P, held_p = st._rows(p, steps)
    x0 = np.asarray(x0, dtype=float)
    if held_u and held_p:
        x, counts = st._drive(lambda t, x: s.f(x, U[0], P[0]), lambda t, x: s.jac(x, U[0], P[0]), x0, steps * dt,
                              dt * np.arange(1, steps + 1), rtol, atol)
        return np.vstack([x0[None], x]), counts
    x, counts = [x0], np.zeros(4, dtype=int)
    for k in range(steps):
        xk, ck = st._drive(lambda t, x: s.f(x, U[k], P[k]), lambda t, x: s.jac(x, U[k], P[k]), x[-1], dt, np.array([dt]), rtol, atol)
        x.append(xk[0])
        counts += ck
    return np.array(x), counts


def _restarted(case, x0, u, p, dt, steps, method, rtol, atol):
    s = system(case)
    U, _ = st._rows(u, steps)
    P, _ = st._rows(p, steps)
    x = [np.asarray(x0, dtype=float)]
    for k in range(steps):
        r = solve_ivp(lambda t, x: s.f(x, U[k], P[k]), (0., dt), x[-1], method=method, rtol=rtol, atol=atol,
                      jac=lambda t, x: s.jac(x, U[k], P[k]))
        assert r.success, r.message
        x.append(r.y[:, -1])
    return np.array(x)


def tight_pair(case, x0, u, p, dt, steps):
    return (_restarted(case, x0, u, p, dt, steps, 'Radau', 1e-12, 1e-15), _restarted(case, x0, u, p, dt, steps, 'LSODA', 1e-11, 1e-14))


def bound(case, x0, u, p, dt, steps, rtol, atol, tight=None):
    """dict: x, z (tight), adm_x, adm_z (admissible errors), e_bdf_x, e_bdf_z, e_tight_x, e_tight_z, counts (BDF's)."""
    ref, other = tight_pair(case, x0, u, p, dt, steps) if tight is None else tight
    xb, counts = bdf(case, x0, u, p, dt, steps, rtol, atol)
    zr, zo, zb = (zetas(case, v, u, p, steps) for v in (ref, other, xb))
    ebx, etx = sr.rel_err(xb, ref, rtol, atol), sr.rel_err(other, ref, rtol, atol)
    ebz, etz = sr.rel_err(zb, zr, rtol, atol), sr.rel_err(zo, zr, rtol, atol)
    return dict(x=ref, z=zr, adm_x=sr.FACTOR * max(ebx, etx), adm_z=sr.FACTOR * max(ebz, etz), e_bdf_x=ebx, e_bdf_z=ebz,
                e_tight_x=etx, e_tight_z=etz, counts=counts)


def _one(job):
    case, x0, u, p, dt, steps, tols = job
    tight = tight_pair(case, x0, u, p, dt, steps)
    return [bound(case, x0, u, p, dt, steps, rtol, atol, tight) for rtol, atol in tols]


def run_jobs(jobs):
    """`bound` for every job (case, x0, u, p, dt, steps, [(rtol, atol), ...]): one list of results per job, in worker processes of a
    fresh interpreter that never opens the GPU (as `stiff_reference.run_jobs`)."""
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
        subprocess.check_call([sys.executable, '-m', 'tests.dae_reference', fin, fout], cwd=root)
        with open(fout, 'rb') as f:
            return pickle.load(f)


def check(case, x, z, b, rtol, atol):
    """(error of x, error of z, ratio to the larger of BDF's error and the tight disagreement - the rule admits FACTOR)."""
    ex, ez = sr.rel_err(x, b['x'], rtol, atol), sr.rel_err(z, b['z'], rtol, atol)
    return ex, ez, max(ex / (b['adm_x'] / sr.FACTOR), ez / (b['adm_z'] / sr.FACTOR))


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
