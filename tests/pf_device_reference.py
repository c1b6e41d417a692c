"""Plain-numpy restatement of the particle filter's device mode (`ParticleFilter(generator='device')`,
include/hilo_hip.h::hilo_pf_run): the counter-based generator, the maps from its words to uniforms and normals, the tolerant
Cholesky factor, and one step of the filter in the kernel's order, on the oracle's models (oracle/models.py).

A draw is a pure function of (seed, filter, step, particle, purpose), so this file reproduces a device run draw by draw.  What a
correct kernel may do differently is the order of its sums: a resampling draw whose target u * cdf[-1] lies within 1e-9 * cdf[-1]
(the tolerance asked of the weights) of a cdf entry is `frail` - it may land one index off.  A replay therefore checks its own
indices against the device's and then ADOPTS the device's for that step, so that one tie does not turn the rest of the chain into
noise."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
STREAM_INITIAL, STREAM_PROCESS, STREAM_MEASUREMENT, STREAM_RESAMPLING, STREAM_ROUGHENING = range(5)
FRAIL_TOL = 1e-9
FRAIL_CAP = .005


def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw: Parallel random numbers: as easy as 1, 2, 3; SC'11).  counter: four words or arrays
    of words, key: two words.  Returns four uint64 arrays holding 32-bit words."""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & MASK for v in np.broadcast_arrays(*counter)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]                      # 32 x 32 -> 64 bits: no overflow
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c


def uniform(a, b):
    """53 bits of two words, centred in their cell: (((a >> 5) << 26 | b >> 6) + 0.5) 2^-53 in IEEE double arithmetic."""
    a, b = np.asarray(a, dtype=np.uint64), np.asarray(b, dtype=np.uint64)
    m = ((a >> np.uint64(5)) << np.uint64(26)) | (b >> np.uint64(6))
    return (m.astype(np.float64) + .5) * 2. ** -53


def words(seed, j, k, b, stream, d=0):
    return philox4x32_10((j, k, b, (stream << 16) | d), (seed & 0xFFFFFFFF, seed >> 32))


def normals(seed, j, k, b, stream, dim):
    """[len(j), dim] standard normals: block d gives components 2d and 2d+1 by Box-Muller."""
    j = np.atleast_1d(j)
    z = np.empty((j.size, (dim + 1) // 2 * 2))
    for d in range((dim + 1) // 2):
        r = words(seed, j, k, b, stream, d)
        rad, ang = np.sqrt(-2. * np.log(uniform(r[0], r[1]))), 6.283185307179586 * uniform(r[2], r[3])
        z[:, 2 * d], z[:, 2 * d + 1] = rad * np.cos(ang), rad * np.sin(ang)
    return z[:, :dim]


def cholesky_tolerant(A):
    """Lower Cholesky factor; a non-positive pivot zeroes its column (a covariance with unexcited states)."""
    A = np.atleast_2d(np.asarray(A, dtype=float))
    n = A.shape[0]
    L = np.zeros((n, n))
    for j in range(n):
        s = A[j, j] - L[j, :j] @ L[j, :j]
        if s > 0.:
            L[j, j] = np.sqrt(s)
            for i in range(j + 1, n):
                L[i, j] = (A[i, j] - L[i, :j] @ L[j, :j]) / L[j, j]
    return L


def resample(q, u):
    """numpy's `choice` for given uniforms: index = first i with cdf[i] > u cdf[-1]; and the frail draws."""
    cdf = np.cumsum(q)
    last = cdf[-1]
    t = u * last
    idx = np.minimum(cdf.searchsorted(t, side='right'), q.size - 1)
    near = np.minimum(np.abs(cdf[idx] - t), np.abs(cdf[np.maximum(idx - 1, 0)] - t))
    return idx, near <= FRAIL_TOL * last


class Filter:
    """One filter of the batch: `number` is its global number (position in the batch + filter_offset)."""

    def __init__(self, model, dt, n_samples, seed=0, resampling='multinomial', roughening=False, K=.2, number=0):
        self.model, self.dt, self.N, self.seed, self.number = model, dt, int(n_samples), int(seed), int(number)
        self.resampling, self.roughening, self.K = resampling, roughening, K
        self.k = 0
        self.status = (0, 0)
        self.j = np.arange(self.N)

    def set_initial_guess(self, x0, P0):
        x0 = np.asarray(x0, dtype=float).reshape(-1)
        self.nx = x0.size
        z = normals(self.seed, self.j, 0, self.number, STREAM_INITIAL, self.nx)
        self.X = x0[None, :] + z @ cholesky_tolerant(P0).T
        self.k = 0
        self.status = (0, 0)

    def step(self, y, u, p, Q, R, device_index=None):
        """One step.  device_index: the indices a device run chose - checked (exact but for the frail draws, those one off at the most,
        at most FRAIL_CAP of them) and adopted."""
        N, nx, k = self.N, self.nx, self.k
        y = np.asarray(y, dtype=float).reshape(-1)
        U = np.tile(np.asarray(u, dtype=float).reshape(1, -1), (N, 1))
        Pm = np.tile(np.asarray(p, dtype=float).reshape(1, -1), (N, 1))
        sig = np.sqrt(np.diag(np.atleast_2d(np.asarray(R, dtype=float))))
        Xp = self.model.f(self.X, U, Pm, self.dt) + normals(self.seed, self.j, k, self.number, STREAM_PROCESS, nx) @ cholesky_tolerant(Q).T
        Y = self.model.h(Xp, U, Pm, self.dt) + sig[None, :] * normals(self.seed, self.j, k, self.number, STREAM_MEASUREMENT, y.size)
        with np.errstate(invalid='ignore', over='ignore'):
            l = -.5 * np.sum(((Y - y[None, :]) / sig[None, :]) ** 2, axis=1)
        m = np.inf if np.any(np.isnan(l)) else l.max()
        out = dict(X_prop=Xp, Y=Y)
        if np.isfinite(m):
            e = np.exp(l - m)
            q = e / e.sum()
            ess = e.sum() ** 2 / np.sum(e * e)
            if self.resampling == 'systematic':
                r = words(self.seed, 0, k, self.number, STREAM_RESAMPLING)
                uni = (self.j + uniform(r[0], r[1])[0]) / N
            else:
                r = words(self.seed, self.j, k, self.number, STREAM_RESAMPLING)
                uni = uniform(r[0], r[1])
            index, frail = resample(q, uni)
        else:
            q, ess = np.full(N, np.nan), np.nan
            index, frail = self.j.copy(), np.zeros(N, dtype=bool)
            if self.status[0] == 0:
                self.status = (1, k)
        out.update(q=q, ess=ess, own_index=index, frail=frail)
        if device_index is not None:
            device_index = np.asarray(device_index)
            assert frail.mean() <= FRAIL_CAP, (k, frail.mean())
            np.testing.assert_array_equal(device_index[~frail], index[~frail], err_msg=f'step {k}')
            assert np.all(np.abs(device_index[frail] - index[frail]) <= 1), k
            index = device_index
        X, Yr = Xp[index], Y[index]
        if self.roughening:
            spread = X.max(axis=0) - X.min(axis=0)
            X = X + np.sqrt(self.K * spread * N ** (-1. / nx))[None, :] * normals(self.seed, self.j, k, self.number, STREAM_ROUGHENING, nx)
        self.X = X
        self.k += 1
        out.update(index=index, X=X, x=X.mean(axis=0), P=np.atleast_2d(np.cov(X.T)), y=Yr.mean(axis=0))
        return out


def covariance_atol(X):
    """A deviation x - mean carries eps |x| of rounding, so an entry of the covariance eps (|x_i| s_j + |x_j| s_i) with s the
    standard deviations (the bound of tests/test_pf_gpu.py::test_particle_count_edges_vs_numpy, from the sample itself)."""
    a, s = np.abs(X).max(axis=0), X.std(axis=0)
    return 16 * np.finfo(float).eps * (np.outer(a, s) + np.outer(s, a))


def double_integrator():
    """`Lti<2, 1, 1>`: position and velocity, the position measured (tests/test_kf_gpu.py::test_lti_kf_and_shared_inputs); the
    sampling interval is the `dt` handed to f and h."""
    import sympy as sp
    from oracle.models import OracleModel
    x0, x1, u, dt = sp.symbols('x0 x1 u dt')
    return OracleModel('lti211', -1, [x0, x1], [u], [], [x0 + dt * x1 + dt ** 2 / 2 * u, x1 + dt * u], [x0], discrete=True)
