"""Three models as expressions, their sympy statements, and the 50-digit reference of values, Jacobians and Hessians (sympy ->
mpmath) for the model-level derivative tests (tests/test_model_probe_gpu.py, tests/test_model_masks.py, tests/test_table_api_gpu.py).

Tolerance.  tests/test_symdiff.py applies to the same table expressions on the host: values rtol 1e-14; first derivatives rtol 1e-12,
atol 1e-14; contracted second derivatives rtol 1e-11, atol 1e-13.  The device's math library is measured against the host's in
tests/ad_reference_ulp.py; the largest device-over-host ratio of the per-function ulp figures is FACTOR = 2.4 (atan2: 1.199 over
0.500), and the bounds here are exactly those numbers times FACTOR: 2.4e-14 | 2.4e-12, 2.4e-14 | 2.4e-11, 2.4e-13 per ENTRY.  A sum
of entries (J d, d'H d, sum_m kb_m H_m, a polarised difference) inherits the sum of its entries' bounds times the magnitudes of
their coefficients."""
import functools

import mpmath
import numpy as np
import sympy as sp

FACTOR = 2.4
V_RTOL = 1e-14 * FACTOR
J_RTOL, J_ATOL = 1e-12 * FACTOR, 1e-14 * FACTOR
H_RTOL, H_ATOL = 1e-11 * FACTOR, 1e-13 * FACTOR

MP = mpmath.mp.clone()
MP.dps = 50

TABLE_TEXT = '''
    da/dt = -a(t) + log10(2 + a(t)^2) + arcsin(a(t)/30) * arccos(b(t)/40) + arctan(a(t)*b(t)) + abs(a(t) - b(t)) * sign(c(k))
    db/dt = -b(t) + arctan2(a(t), 1 + c(k)^2) + arsinh(b(t)*c(k)) + arcosh(2 + a(t)^2) + artanh(b(t)/50) ...
            + min(a(t)*c(k), b(t)) + max(a(t), b(t)^2) + tanh(a(t)) + sqrt(1 + exp(-b(t)))
    y(k) = a(t) + abs(b(t))
    '''


def _smin(p, q):
    return (p + q - sp.Abs(p - q)) / 2          # the active branch, the mean at a tie (CasADi's convention, expr.py::fmin)


def _smax(p, q):
    return (p + q + sp.Abs(p - q)) / 2


def _table_sympy():
    a, b, c = sp.symbols('a b c', real=True)
    f = [-a + sp.log(2 + a * a, 10) + sp.asin(a / 30) * sp.acos(b / 40) + sp.atan(a * b) + sp.Abs(a - b) * sp.sign(c),
         -b + sp.atan2(a, 1 + c * c) + sp.asinh(b * c) + sp.acosh(2 + a * a) + sp.atanh(b / 50) + _smin(a * c, b) + _smax(a, b * b)
         + sp.tanh(a) + sp.sqrt(1 + sp.exp(-b))]
    return [a, b], [c], [], f, [a + sp.Abs(b)]


def table_model(discrete=False):
    """The table model of tests/test_jit_cpu.py as text; discrete: the same right-hand sides as a discrete model x+ = f(x, u)
    written with the expression functions - its linearisation is A = df/dx, B = df/du exactly."""
    from hilo_mpc_amd import Model, expr as ex
    if not discrete:
        m = Model(name='table')
        m.set_equations(equations=TABLE_TEXT)
        return m
    m = Model(name='table_d', discrete=True)
    x, u = m.set_dynamical_states(['a', 'b']), m.set_inputs(['c'])
    a, b, c = x[0], x[1], u[0]
    m.set_dynamical_equations([
        -a + ex.log10(2.0 + a ** 2) + ex.asin(a / 30.0) * ex.acos(b / 40.0) + ex.atan(a * b) + ex.fabs(a - b) * ex.sign(c),
        -b + ex.atan2(a, 1.0 + c ** 2) + ex.asinh(b * c) + ex.acosh(2.0 + a ** 2) + ex.atanh(b / 50.0) + ex.fmin(a * c, b)
        + ex.fmax(a, b ** 2) + ex.tanh(a) + ex.sqrt(1.0 + ex.exp(-b))])
    m.set_measurement_equations([a + ex.fabs(b)])
    return m


def edges_model():
    """tan sinh cosh tanh min max, a^-3, a nested quotient, tanh(k a) with k a reaching +-1000 (k = p[0] = 1000, |a| up to 1).  sinh
    and cosh see |a| <= 1 here; their whole range up to the overflow at 709.78 is in tests/ad_reference.py (COMPOSED)."""
    from hilo_mpc_amd import Model, expr as ex
    m = Model(name='edges')
    x, u, p = m.set_dynamical_states(['a', 'b']), m.set_inputs(['c']), m.set_parameters(['k'])
    a, b, c, k = x[0], x[1], u[0], p[0]
    m.set_dynamical_equations([ex.tan(a) + ex.sinh(b) * ex.cosh(a) + ex.tanh(k * a) + ex.fmin(a, b * c),
                               ex.fmax(a * a, b) + a ** -3 + (a / (1.0 + b * b)) / (2.0 + c / (1.0 + a * a)) + ex.tanh(k * b * c)])
    m.set_measurement_equations([ex.tanh(k * a) * b])
    return m


def _edges_sympy():
    a, b, c, k = sp.symbols('a b c k', real=True)
    f = [sp.tan(a) + sp.sinh(b) * sp.cosh(a) + sp.tanh(k * a) + _smin(a, b * c),
         _smax(a * a, b) + a ** -3 + (a / (1 + b * b)) / (2 + c / (1 + a * a)) + sp.tanh(k * b * c)]
    return [a, b], [c], [k], f, [sp.tanh(k * a) * b]


def _pendulum_sympy():
    from oracle import models
    m = models.get('pendulum4')
    return list(m.x), list(m.u), [], list(m.ode), list(m.meas)


def pendulum_model():
    from tests.problems import symbolic_model
    return symbolic_model('pendulum4')


MODELS = {'table': (table_model, _table_sympy), 'edges': (edges_model, _edges_sympy), 'pendulum4': (pendulum_model, _pendulum_sympy)}
# the three points of tests/test_symdiff.py (x, u), then random ones
BASE_POINTS = {'table': [(.7, -.4, 1.3), (-1.1, .9, -.6), (.2, .3, .8)],
               # the last three: k a = 0.1, -3, 20 and k b c = 1.4, 5.4, 330 - tanh between its linear part and saturation, where
               # sech2 and tanh sech2 in the generated derivative code are neither 1 nor 0 (everywhere else |k a| >= 150)
               'edges': [(.7, -.4, 1.3), (-1.0, .9, -.6), (.2, .3, .8), (1e-4, 2e-3, .7), (-3e-3, -.9, -6e-3), (2e-2, .3, 1.1)],
               'pendulum4': [(.4, -.3, .7, 1.2, 2.), (-.2, .5, -2.9, -.8, -1.), (0., 0., 3.1, .1, .5)]}
PARAMS = {'table': [], 'edges': [1000.], 'pendulum4': []}


def points(name, n=64, seed=5):
    """(X [n][nx], U [n][nu], p): the base points, then random ones of the same size."""
    rng = np.random.default_rng(seed)
    base = np.array(BASE_POINTS[name])
    nz = base.shape[1]
    Z = np.concatenate([base, rng.uniform(.15, 1., (n - len(base), nz)) * rng.choice([-1., 1.], (n - len(base), nz))])
    nx = 4 if name == 'pendulum4' else 2
    if name == 'pendulum4':
        Z[len(base):, 2] *= 3.                   # the angle over the whole circle
    return Z[:, :nx].copy(), Z[:, nx:].copy(), np.array(PARAMS[name])


def _no_delta(e):
    return e.replace(sp.DiracDelta, lambda *a: sp.Integer(0))      # d sign = 0, d2 |a| = 0 away from the kink (CasADi: everywhere)


@functools.lru_cache(maxsize=None)
def symbolic(name):
    """(xs, us, ps, f, h, Jf, Jh, Hf, Hh): sympy; J over w = (x, u), H[m] the Hessian of row m over w."""
    xs, us, ps, f, h = MODELS[name][1]()
    w = xs + us
    Jf = [[_no_delta(sp.diff(e, v)) for v in w] for e in f]
    Jh = [[_no_delta(sp.diff(e, v)) for v in w] for e in h]
    Hf = [[[_no_delta(sp.diff(Jf[m][i], v)) for v in w] for i in range(len(w))] for m in range(len(f))]
    Hh = [[[_no_delta(sp.diff(Jh[m][i], v)) for v in w] for i in range(len(w))] for m in range(len(h))]
    return xs, us, ps, f, h, Jf, Jh, Hf, Hh


@functools.lru_cache(maxsize=None)
def _evaluator(name):
    xs, us, ps, f, h, Jf, Jh, Hf, Hh = symbolic(name)
    flat = (list(f) + list(h) + [e for r in Jf for e in r] + [e for r in Jh for e in r] + [e for M_ in Hf for r in M_ for e in r] +
            [e for M_ in Hh for r in M_ for e in r])
    mods = [{'Abs': lambda v: abs(v), 'sign': lambda v: MP.sign(v), 'log': MP.log, 'sqrt': MP.sqrt, 'exp': MP.exp, 'sin': MP.sin,
             'cos': MP.cos, 'tan': MP.tan, 'asin': MP.asin, 'acos': MP.acos, 'atan': MP.atan, 'atan2': MP.atan2, 'sinh': MP.sinh,
             'cosh': MP.cosh, 'tanh': MP.tanh, 'asinh': MP.asinh, 'acosh': MP.acosh, 'atanh': MP.atanh, 'sech': MP.sech,
             'pi': MP.pi}]
    return sp.lambdify(xs + us + ps, flat, modules=mods, cse=True)


def reference(name, X, U, p):
    """dict of float arrays at the points: f [n][nx], y [n][ny], Jf [n][nx][nz], Jy [n][ny][nz], Hf [n][nx][nz][nz], Hy [n][ny][nz][nz]."""
    xs, us, ps, f, h = symbolic(name)[:5]
    nx, nu, ny = len(xs), len(us), len(h)
    nz = nx + nu
    fn = _evaluator(name)
    rows = []
    for x, u in zip(X, U):
        args = [MP.mpf(float(v)) for v in list(x) + list(u) + list(p)]
        rows.append([float(MP.mpf(v)) for v in fn(*args)])
    R = np.array(rows)
    n = len(R)
    o = np.cumsum([0, nx, ny, nx * nz, ny * nz, nx * nz * nz, ny * nz * nz])
    return {'f': R[:, o[0]:o[1]], 'y': R[:, o[1]:o[2]], 'Jf': R[:, o[2]:o[3]].reshape(n, nx, nz), 'Jy': R[:, o[3]:o[4]].reshape(n, ny, nz),
            'Hf': R[:, o[4]:o[5]].reshape(n, nx, nz, nz), 'Hy': R[:, o[5]:o[6]].reshape(n, ny, nz, nz)}
