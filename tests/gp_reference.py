"""Extended-precision reference of exact GP inference for tests/test_gp_paths_gpu.py and tests/test_gp_reference_cpu.py.

What is under test there is the LINEAR ALGEBRA of csrc/hilo_gp.hip (Cholesky, the two triangular solves, L^-1 K*, the trace
formula of the LML gradient), not the covariance functions - those are pinned by the known-answer tests of
tests/test_gp_gpu.py.  So the covariance matrix and the mean vector are evaluated in float64 by `oracle.gp.kernel` / `oracle.gp.mean`
(what the float64 oracle `oracle.gp.Posterior` starts from as well) and everything after that is restated here in `np.longdouble`,
in plain numpy loops over rows: no LAPACK, no BLAS (numpy has neither for longdouble).

  inference.py:197-217   L L^T = K + sn2 I;  alpha = L^-T L^-1 (y - m);  LML = -1/2 (y-m) alpha - sum log diag L - n/2 log 2 pi
  inference.py:212-217   mean* = m(x*) + k*^T alpha;  var* = k** - |L^-1 k*|^2   (+ sn2 unless noise free, gp.py:699-718)
  Rasmussen & Williams eq. 5.9   d LML / d theta_j = 1/2 tr((alpha alpha^T - K_y^-1) dK_y / d theta_j)

Also here: the data set and the two kernel / mean pairs of the case matrix, so that the CPU module and the GPU module build the
same inputs.
"""
import functools

import numpy as np

from oracle import gp as ogp

LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)
# x87 80-bit extended precision (eps = 2^-63 = 1.08e-19).  Where numpy's longdouble is float64 (eps = 2.2e-16) this module is
# of no use as a reference and must not pretend otherwise: the import fails, and with it every test that needs the reference.
assert EPS_LD < 1e-18, (f"np.longdouble has eps = {EPS_LD:.3g} on this host (no extended precision): the GP reference of "
                        f"tests/gp_reference.py cannot be computed here, and it does NOT fall back to float64")
EPS64 = float(np.finfo(np.float64).eps)
PI = 4 * np.arctan(LD(1))


class NotPositiveDefinite(ArithmeticError):
    def __init__(self, pivot):
        super().__init__(f"not positive definite (pivot {pivot})")
        self.pivot = pivot


def cholesky(A):
    """Lower factor of a symmetric positive definite matrix, column by column (left looking): column j of L from column j of
    A minus the rows of L to its left times row j of L.  The pivot reported on failure counts from 1, like the device's."""
    A = np.asarray(A, dtype=LD)
    n = A.shape[0]
    L = np.zeros((n, n), dtype=LD)
    for j in range(n):
        col = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not col[0] > 0:
            raise NotPositiveDefinite(j + 1)
        d = np.sqrt(col[0])
        L[j, j] = d
        L[j + 1:, j] = col[1:] / d
    return L


def solve_lower(L, B):
    """L^-1 B by forward substitution (B a vector or a matrix of columns)."""
    X = np.array(B, dtype=LD)
    for i in range(L.shape[0]):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def solve_lower_transposed(L, B):
    """L^-T B by backward substitution."""
    X = np.array(B, dtype=LD)
    for i in range(L.shape[0] - 1, -1, -1):
        X[i] = (X[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


class Reference:
    """`oracle.gp.Posterior` in longdouble: same arguments, same attributes (L instead of R = L^T)."""

    def __init__(self, kernel_spec, mean_spec, X, y, noise_variance):
        X = np.atleast_2d(np.asarray(X, dtype=float))
        y = np.asarray(y, dtype=float).reshape(-1)
        n = X.shape[1]
        self.sn2 = float(np.exp(2 * ogp._log_param(noise_variance, True)))   # the float64 number the device adds to the diagonal
        K = ogp.kernel(kernel_spec, X, X).astype(LD)
        K[np.diag_indices(n)] += LD(self.sn2)
        self.Ky = K
        self.L = cholesky(K)
        self.ym = y.astype(LD) - ogp.mean(mean_spec, X)[0].astype(LD)
        self.alpha = solve_lower_transposed(self.L, solve_lower(self.L, self.ym))
        self.lml = -self.ym @ self.alpha / 2 - np.sum(np.log(np.diag(self.L))) - LD(n) / 2 * np.log(2 * PI)
        self.X, self.kernel_spec, self.mean_spec = X, kernel_spec, mean_spec
        self._linv = None

    def l_inv_kstar(self, Xq):
        """V = L^-1 K* (n x m): the matrix whose column sums of squares the predictive variance subtracts."""
        return solve_lower(self.L, ogp.kernel(self.kernel_spec, self.X, np.atleast_2d(Xq)).astype(LD))

    def predict(self, Xq, noise_free=False):
        """(mean (m,), var (m,)) in longdouble."""
        Xq = np.atleast_2d(np.asarray(Xq, dtype=float))
        Ks = ogp.kernel(self.kernel_spec, self.X, Xq).astype(LD)
        mu = ogp.mean(self.mean_spec, Xq)[0].astype(LD) + Ks.T @ self.alpha
        V = solve_lower(self.L, Ks)
        kss = np.array([ogp.kernel(self.kernel_spec, Xq[:, [i]], Xq[:, [i]])[0, 0] for i in range(Xq.shape[1])]).astype(LD)
        var = kss - np.sum(V * V, axis=0)
        if not noise_free:
            var = var + LD(self.sn2)
        return mu, var

    @property
    def L_inv(self):
        if self._linv is None:
            self._linv = solve_lower(self.L, np.eye(self.L.shape[0], dtype=LD))
        return self._linv

    def trace_weights(self):
        """alpha alpha^T - K_y^-1 with K_y^-1 = L^-T L^-1."""
        return np.outer(self.alpha, self.alpha) - self.L_inv.T @ self.L_inv

    def lml_gradient(self, dKy):
        """1/2 tr((alpha alpha^T - K_y^-1) dK_y) for each matrix of the list `dKy` (both factors symmetric)."""
        A = self.trace_weights()
        return np.array([np.sum(A * np.asarray(d, dtype=LD)) / 2 for d in dKy], dtype=LD)


def oracle_lml_gradient(post, dKy):
    """The same trace formula with the float64 oracle's factor (`oracle.gp_fit.lml_gradient` takes scalar hyper-parameters by
    name only; the ARD length scales of the case matrix need the derivative matrices handed in)."""
    from scipy.linalg import cho_solve
    A = np.outer(post.alpha, post.alpha) - cho_solve((post.R, False), np.eye(post.R.shape[0]))
    return np.array([.5 * np.sum(A * d) for d in dKy])


# =================================================================================================
# the inputs of the case matrix
# =================================================================================================
NF = 3
NOISE_VARIANCE = 1e-2
FEATURES = ['a', 'b', 'c']

# (a) one squared-exponential node over features 0 and 2 - the inline shortcut of the register and matrix-core predict kernels,
#     with an inactive feature between the two active ones;  (b) five nodes (Matern, constant, squared exponential, product,
#     sum) and a two-node mean - the interpreter.  0.3 k_SE is written as the product with a constant kernel of bias^2 = 0.3.
KERNELS = {
    'se_ard02': ({'type': 'squared_exponential', 'kwargs': {'active_dims': [0, 2], 'length_scales': [1.3, .8], 'ard': True}},
                 {'type': 'zero'}),
    'm52+se': ({'type': 'sum', 'children': [
        {'type': 'matern_52', 'kwargs': {'active_dims': [0, 2]}},
        {'type': 'product', 'children': [{'type': 'constant', 'kwargs': {'bias': float(np.sqrt(.3))}},
                                         {'type': 'squared_exponential', 'kwargs': {'active_dims': [1]}}]}]},
               {'type': 'sum', 'children': [{'type': 'linear'}, {'type': 'one'}]}),
}
# k(x, x): the scale of the predictive variance
SIGNAL_VARIANCE = {'se_ard02': 1., 'm52+se': 1. + float(np.exp(2 * np.log(np.sqrt(.3))))}


@functools.lru_cache(maxsize=None)
def training_data(n):
    """n points uniform in [0, 10]^3; y a smooth function of features 0 and 2 plus noise of standard deviation 1e-2."""
    rng = np.random.default_rng(20261019 + n)
    X = rng.uniform(0., 10., (NF, n))
    y = np.sin(.7 * X[0]) * np.cos(.4 * X[2]) + .05 * X[0] + 1e-2 * rng.standard_normal(n)
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y[None, :]


@functools.lru_cache(maxsize=None)
def queries(m):
    """m query points, a little beyond the box of the training inputs on either side."""
    Xq = np.random.default_rng(77000 + m).uniform(-.5, 10.5, (NF, m))
    Xq.setflags(write=False)
    return Xq


@functools.lru_cache(maxsize=None)
def reference(n, kern):
    X, y = training_data(n)
    return Reference(*KERNELS[kern], X, y, NOISE_VARIANCE)


@functools.lru_cache(maxsize=None)
def oracle(n, kern):
    X, y = training_data(n)
    return ogp.Posterior(*KERNELS[kern], X, y, NOISE_VARIANCE)


@functools.lru_cache(maxsize=None)
def predictions(n, kern, m):
    """{'ref': (mean, var noise free), 'orc': (mean, var noise free)} at `queries(m)`; the noisy variance adds `sn2` to either."""
    r = reference(n, kern).predict(queries(m), noise_free=True)
    o = oracle(n, kern).predict(queries(m), noise_free=True)
    return {'ref': r, 'orc': (o[0][0], o[1][0])}


def bound(oracle_value, reference_value, scale):
    """max(max|o - r|, 4 eps64 scale): what float64 in another summation order legitimately costs on this problem, with the
    resolution of the number format as its floor.  The device result is held to C times this."""
    o = np.asarray(oracle_value, dtype=LD)
    r = np.asarray(reference_value, dtype=LD)
    return max(float(np.max(np.abs(o - r))), 4 * EPS64 * float(scale))


def error(device_value, reference_value):
    return float(np.max(np.abs(np.asarray(device_value, dtype=LD) - np.asarray(reference_value, dtype=LD))))
