"""References for the regulator of csrc/hilo_lqr.h: the plain finite-horizon Riccati recursion of the reference
(hilo_mpc/modules/controller/lqr.py:236-245), a numpy restatement of the structure-preserving doubling algorithm for the stationary
equation, the cases both are measured on, and the bound the tests hold the device (and host-compiled) code to.

The bound: `1e-10 * max(1, max|P|)` for P against scipy.linalg.solve_discrete_are and against the numpy recursion, the same with
max|K| for K.  Measured here for the doubling restatement against scipy on the cases below (Q = I, R = I; `measure()` prints them,
`python -m tests.lqr_reference`): 5 to 14 steps; error below 2e-13 max|P| on every case but the two cart-pendulums, whose P is
large (max|P| = 3.0e4 at dt = .1: 2.4e-12 max|P|; 2.9e5 at dt = .01: 9.9e-12 max|P|).  The bound leaves a factor of 10 on the worst
of these and of 400 and more on the others for another summation order and contraction on the device; the device measures the same
two figures on the two cart-pendulums (tests/test_lqr_gpu.py::test_large_riccati_solutions_against_scipy: 2.35e-12, 9.91e-12).
"""
import numpy as np

TOL = 1e-10


def bound(ref):
    return TOL * max(1., float(np.max(np.abs(ref))))


def riccati_finite(A, B, Q, R, horizon, N=None):
    """lqr.py:236-245: from P = Q, `horizon` backward steps, then the gain.  Returns (K, P)."""
    N = np.zeros((A.shape[0], B.shape[1])) if N is None else N
    P = Q.copy()
    for _ in range(horizon):
        APBN = A.T @ P @ B + N
        RBPB = R + B.T @ P @ B
        P = A.T @ P @ A - np.linalg.solve(RBPB.T, APBN.T).T @ (B.T @ P @ A + N.T) + Q
    return np.linalg.solve(R + B.T @ P @ B, B.T @ P @ A + N.T), P


def riccati_fixed_point(A, B, Q, R, tol=1e-12, max_iter=100000):
    """The plain recursion run to a fixed point: what the doubling algorithm replaces (iteration count for the record)."""
    P = Q.copy()
    for it in range(max_iter):
        Pn = A.T @ P @ A - (A.T @ P @ B) @ np.linalg.solve(R + B.T @ P @ B, B.T @ P @ A) + Q
        if np.max(np.abs(Pn - P)) <= tol * max(1., np.max(np.abs(Pn))):
            return Pn, it + 1
        P = Pn
    return P, max_iter


def dare_doubling(A, B, Q, R, N=None, tol=1e-12, max_iter=50):
    """Structure-preserving doubling (the statements of csrc/hilo_lqr.h::lqr_solve).  Returns (K, P, status, iterations)."""
    n = A.shape[0]
    N = np.zeros((n, B.shape[1])) if N is None else N
    RiNt, RiBt = np.linalg.solve(R, N.T), np.linalg.solve(R, B.T)
    Ad, G, H = A - B @ RiNt, B @ RiBt, Q - N @ RiNt
    G, H = .5 * (G + G.T), .5 * (H + H.T)
    status, it = 1, 0
    with np.errstate(all='ignore'):
        for it in range(1, max_iter + 1):
            W = np.eye(n) + G @ H
            if not np.all(np.isfinite(W)):
                status = 2
                break
            try:
                V1, V2 = np.linalg.solve(W, Ad), np.linalg.solve(W, G)
            except np.linalg.LinAlgError:
                status = 2
                break
            G = G + Ad @ V2 @ Ad.T
            G = .5 * (G + G.T)
            Hn = H + Ad.T @ H @ V1
            Hn = .5 * (Hn + Hn.T)
            delta, H = np.max(np.abs(Hn - H)), Hn
            Ad = Ad @ V1
            if not (np.all(np.isfinite(H)) and np.all(np.isfinite(G)) and np.all(np.isfinite(Ad))):
                status = 2
                break
            if delta <= tol * max(1., np.max(np.abs(H))):
                status = 0
                break
    if status:
        return np.full((B.shape[1], n), np.nan), np.full((n, n), np.nan), status, it
    return np.linalg.solve(R + B.T @ H @ B, B.T @ H @ A + N.T), H, 0, it


# ---- the cases ------------------------------------------------------------------------------------------------------------
def lqr_model(p, dt=1.):
    """The reference's LQR test model (tests/test_LQR.py:245-251): x+ = x + dt (2 y + p u), y+ = y - dt x, z+ = z + dt w."""
    A = np.array([[1., 2. * dt, 0.], [-dt, 1., 0.], [0., 0., 1.]])
    B = np.array([[p * dt, 0.], [0., 0.], [0., dt]])
    return A, B


def double_integrator(dt):
    return np.array([[1., dt], [0., 1.]]), np.array([[dt * dt / 2.], [dt]])


def cart_pendulum(dt):
    """The cart-pendulum of the zoo (csrc/hilo_models.h::Pendulum4) linearised at the upright origin, forward-Euler plus the
    second-order term of the matrix exponential (any discretisation serves a Riccati test; this one needs no integrator)."""
    M, m, l, g = 5., 1., 1., 9.81
    Ac = np.zeros((4, 4))
    Ac[0, 1] = Ac[2, 3] = 1.
    Ac[1, 2] = m * g / M
    Ac[3, 2] = (m * g / M + g) / l
    Bc = np.array([[0.], [1. / M], [0.], [1. / (M * l)]])
    A = np.eye(4) + dt * Ac + dt * dt / 2. * Ac @ Ac
    return A, (dt * np.eye(4) + dt * dt / 2. * Ac) @ Bc


def random_system(n, m, seed, radius=1.2):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal((n, n))
    A *= radius / np.max(np.abs(np.linalg.eigvals(A)))
    return A, rng.standard_normal((n, m))


def cases():
    """name -> (A, B, Q, R, N or None)"""
    out = {'lqr_p1': lqr_model(1.)}
    for dt in (.5, .05, .005):
        out[f'double_integrator_{dt:g}'] = double_integrator(dt)
    for dt in (.1, .01):
        out[f'cart_pendulum_{dt:g}'] = cart_pendulum(dt)
    out['random_6x2'] = random_system(6, 2, 11)
    out['random_8x4'] = random_system(8, 4, 12)
    full = {k: (A, B, np.eye(A.shape[0]), np.eye(B.shape[1]), None) for k, (A, B) in out.items()}
    # a cross weight: Q - N R^-1 N' stays positive definite (|N| small against Q = I, R = I)
    A, B = random_system(6, 2, 11)
    full['random_6x2_cross'] = (A, B, np.eye(6), np.eye(2), .2 * np.random.default_rng(13).standard_normal((6, 2)))
    A, B = lqr_model(1.)
    full['lqr_p1_cross'] = (A, B, np.eye(3), np.eye(2), np.array([[.1, 0.], [0., .2], [-.1, .1]]))
    return full


def wide_cases():
    """More inputs than states (the n x m products of the finite-horizon step are then larger than the n x n ones): name -> (A, B)"""
    return {'wide_2x3': random_system(2, 3, 21), 'wide_1x2': random_system(1, 2, 22), 'wide_3x4': random_system(3, 4, 23),
            'wide_1x4': random_system(1, 4, 24)}


def scipy_dare(A, B, Q, R, N=None):
    from scipy.linalg import solve_discrete_are
    P = solve_discrete_are(A, B, Q, R, s=N)
    Nt = np.zeros((B.shape[1], A.shape[0])) if N is None else N.T
    return np.linalg.solve(R + B.T @ P @ B, B.T @ P @ A + Nt), P


def measure():
    for name, (A, B, Q, R, N) in cases().items():
        K, P, status, it = dare_doubling(A, B, Q, R, N)
        Ks, Ps = scipy_dare(A, B, Q, R, N)
        print(f"{name:24s} steps {it:3d} status {status}  max|P| {np.max(np.abs(Ps)):9.3e}  err P {np.max(np.abs(P - Ps)) / max(1., np.max(np.abs(Ps))):8.2e}"
              f"  err K {np.max(np.abs(K - Ks)) / max(1., np.max(np.abs(Ks))):8.2e}")


# ---- the models of the GPU tests, through the public front-end --------------------------------------------------------------------
def reference_model(dt=1.):
    """`lqr_model` as expressions, p a parameter (run-time compiled)."""
    from hilo_mpc_amd import Model
    m = Model(discrete=True)
    x = m.set_dynamical_states(['x', 'y', 'z'])
    u = m.set_inputs(['u', 'w'])
    p = m.set_parameters(['p'])
    m.set_dynamical_equations([x[0] + dt * (2. * x[1] + p[0] * u[0]), x[1] - dt * x[0], x[2] + dt * u[1]])
    return m.setup(dt=dt)


def bicycle(dt=.05):
    """The kinematic bicycle of tests/test_linearize.py with the two lengths as parameters, RK4."""
    from hilo_mpc_amd import Model, expr
    m = Model()
    s = m.set_dynamical_states(['px', 'py', 'v', 'phi'])
    i = m.set_inputs(['a', 'delta'])
    q = m.set_parameters(['lr', 'lf'])
    beta = expr.atan(q[0] / (q[0] + q[1]) * expr.tan(i[1]))
    m.set_dynamical_equations([s[2] * expr.cos(s[3] + beta), s[2] * expr.sin(s[3] + beta), i[0], s[2] / q[0] * expr.sin(beta)])
    m.discretize('rk4', inplace=True)
    return m.setup(dt=dt)


def pendulum(dt=.1):
    """pendulum4 as hilo_mpc_amd/zoo_expr.py writes it, RK4."""
    from hilo_mpc_amd import Model, zoo_expr
    m = zoo_expr.define(Model(), 'pendulum4')
    m.discretize('rk4', inplace=True)
    return m.setup(dt=dt)


PENDULUM_GAIN = np.array([-2.11318, -6.00619, 132.22857, 39.49195])   # stationary, Q = I, R = .1, at the origin (6 digits)


if __name__ == '__main__':
    measure()
