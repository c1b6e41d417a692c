"""Numpy restatement of the on-device hyper-parameter fit (csrc/hilo_gp.hip::gp_fit_batch_kernel) on the oracle's functions.

TEST INFRASTRUCTURE ONLY.  The objective is `oracle.gp.Posterior.lml`, the gradient the trace formula
1/2 tr((alpha alpha^T - K_y^-1) dK_y/dtheta_j) with dK_y/dtheta_j by central differences (h = 1e-5) of the kernel matrix -
`oracle.gp_fit.lml_gradient` for a single kernel, restated below for kernel trees (sums, products), which that function does not
take.  The optimiser follows the kernel rule for rule:

* variables theta = log of [noise variance | free kernel hyper-parameters]; f = -LML, g = -d LML / d theta
* direction d = -H g; H = I (and "fresh" again) when g.d >= 0
* first step length min(1, 1 / |g|_2), afterwards 1; Armijo f(theta + t d) <= f + 1e-4 t g.d, halving, at most 40 halvings;
  a trial point that is not positive definite or whose LML is not finite is a rejected trial; a step t whose first-order change
  t g.d no longer changes f in floating point (f + t g.d == f) is not tried: no trial point can show a decrease any more
* update of H only if s.y > 1e-12 |s| |y|; H = (s.y / y.y) I before the first update after a (re)start
* status 0: max |g| <= gtol; 1: maxiter; 2: no decrease within the 41 trial points, or none can be shown; 3: the start point is
  not positive definite
"""
import numpy as np
from scipy.linalg import cho_solve

from oracle import gp as ogp
from oracle import gp_fit

H_STEP, C1, MAX_HALVINGS = 1e-5, 1e-4, 40

# the eleven kernels of tests/test_gp_gpu.py::test_fit_model_reference_kats (reference tests/test_GPs.py:846-904):
# id, oracle type, free hyper-parameter names in the order of `hyperparameter_values`, fixed keyword arguments, shift of y,
# expected fitted values [noise variance | names], tolerance
KATS = [
    ('SE', 'squared_exponential', ['length_scales', 'signal_variance'], {}, 0., [.0085251, .5298217, .8114553], 1e-5),
    ('Const', 'constant', ['bias'], {}, 3., [.7009480, 3.0498634], 1e-5),
    ('M32', 'matern_32', ['length_scales', 'signal_variance'], {}, 0., [.0088262, .8329355, .9398366], 1e-5),
    ('NN', 'neural_network', ['signal_variance', 'weight_variance'], {}, 0., [.0095177, 5.7756069, .1554265], 1e-5),
    ('M52', 'matern_52', ['length_scales', 'signal_variance'], {}, 0., [.0086694, .7180206, .9571137], 1e-5),
    ('PP1', 'piecewise_polynomial', ['length_scales', 'signal_variance'], {'degree': 1}, 0., [.0088391, 1.6079331, .6545336], 1e-5),
    ('PP2', 'piecewise_polynomial', ['length_scales', 'signal_variance'], {'degree': 2}, 0., [.0088244, 2.0883167, .852502], 1e-5),
    ('PP3', 'piecewise_polynomial', ['length_scales', 'signal_variance'], {'degree': 3}, 0., [.0086766, 2.247363, .7873581], 1e-5),
    ('Poly', 'polynomial', ['signal_variance', 'offset'], {'degree': 3}, 0., [.0980796, 1.3112287, .5083423], 1e-5),
    ('Lin', 'linear', ['signal_variance'], {}, 0., [.6627861, .008198], 1e-4),
    ('Periodic', 'periodic', ['signal_variance', 'length_scales', 'period'], {}, 0., [.4975112, .159969, .5905631, .8941061], 1e-3),
]


def kat_data():
    """The data set of the reference's fit tests (tests/test_GPs.py:835-838): x [20, 1], y [20, 1] without the shift."""
    x = ogp.park_miller_randn(.8, (20, 1))
    return x, np.sin(3 * x) + .1 * ogp.park_miller_randn(.9, (20, 1))


def kat_kernel(K, kid):
    """The product kernel of a KATS row (`K` = hilo_mpc_amd.Kernel)."""
    return {'SE': lambda: K.squared_exponential(), 'Const': lambda: K.constant(), 'M32': lambda: K.matern_32(),
            'NN': lambda: K.neural_network(), 'M52': lambda: K.matern_52(), 'PP1': lambda: K.piecewise_polynomial(1),
            'PP2': lambda: K.piecewise_polynomial(2), 'PP3': lambda: K.piecewise_polynomial(3), 'Poly': lambda: K.polynomial(3),
            'Lin': lambda: K.linear(), 'Periodic': lambda: K.periodic()}[kid]()


def single(kernel_type, names, fixed=None):
    """theta -> kernel spec of one kernel whose hyper-parameters `names` are exp(theta[1:])."""
    def spec_of(theta):
        kw = dict(fixed or {})
        kw.update({n: float(np.exp(t)) for n, t in zip(names, theta[1:])})
        return {'type': kernel_type, 'kwargs': kw}
    return spec_of


def lml(spec_of, theta, X, y, mean_spec=None):
    """Log marginal likelihood at theta; None where K + sn2 I is not positive definite or the value is not finite."""
    try:
        post = ogp.Posterior(spec_of(theta), mean_spec or {'type': 'zero'}, X, y, float(np.exp(theta[0])))
    except np.linalg.LinAlgError:
        return None
    return float(post.lml) if np.isfinite(post.lml) else None


def lml_gradient(spec_of, theta, X, y, mean_spec=None, h=H_STEP):
    """`oracle.gp_fit.lml_gradient` for any kernel spec (the same statements; that function takes one kernel type only)."""
    theta = np.asarray(theta, dtype=float)
    Xa = np.atleast_2d(np.asarray(X, dtype=float))

    def K_of(th):
        return ogp.kernel(spec_of(th), Xa, Xa) + np.exp(th[0]) * np.eye(Xa.shape[1])
    post = ogp.Posterior(spec_of(theta), mean_spec or {'type': 'zero'}, X, y, float(np.exp(theta[0])))
    n = post.R.shape[0]
    A = np.outer(post.alpha, post.alpha) - cho_solve((post.R, False), np.eye(n))
    g = np.zeros_like(theta)
    for i in range(theta.size):
        e = np.zeros_like(theta)
        e[i] = h
        g[i] = 0.5 * np.sum(A * ((K_of(theta + e) - K_of(theta - e)) / (2 * h)))
    return g


def fit(spec_of, theta0, X, y, mean_spec=None, gtol=1e-6, maxiter=200, oracle_single=None):
    """The device algorithm.  oracle_single = (kernel_type, names, fixed): objective and gradient are then literally
    `oracle.gp_fit.negative_lml` / `oracle.gp_fit.lml_gradient(h=1e-5)`.  Returns a dict like a row of `GPArray.fit_stats`."""
    if oracle_single is not None:
        kt, names, fixed = oracle_single

        def f_of(th):
            v = gp_fit.negative_lml(kt, names, th, X, y, fixed, mean_spec)
            return v if np.isfinite(v) else None

        def g_of(th):
            return -gp_fit.lml_gradient(kt, names, th, X, y, fixed, mean_spec, h=H_STEP)
    else:
        def f_of(th):
            v = lml(spec_of, th, X, y, mean_spec)
            return None if v is None else -v

        def g_of(th):
            return -lml_gradient(spec_of, th, X, y, mean_spec)
    th = np.array(theta0, dtype=float)
    nth = th.size
    f = f_of(th)
    nfev, it = 1, 0
    if f is None:
        return {'status': 3, 'theta': None, 'lml': np.nan, 'grad': None, 'iterations': 0, 'evaluations': nfev}
    g = g_of(th)
    H, fresh = np.eye(nth), True
    while True:
        if not np.max(np.abs(g)) > gtol:
            status = 0
            break
        if it >= maxiter:
            status = 1
            break
        d = -H @ g
        gd = float(g @ d)
        if not gd < 0.:
            H, fresh = np.eye(nth), True
            d = -g
            gd = -float(g @ g)
        step = min(1., 1. / np.sqrt(float(g @ g))) if it == 0 else 1.
        accepted = False
        for ls in range(MAX_HALVINGS + 1):
            if f + step * gd == f:
                break
            tht = th + step * d
            ft = f_of(tht)
            nfev += 1
            if ft is not None and ft <= f + C1 * step * gd:
                accepted = True
                break
            step *= .5
        if not accepted:
            status = 2
            break
        gn = g_of(tht)
        s, yv = tht - th, gn - g
        sy = float(s @ yv)
        if sy > 1e-12 * np.sqrt(float(s @ s)) * np.sqrt(float(yv @ yv)):
            if fresh:
                H, fresh = np.eye(nth) * (sy / float(yv @ yv)), False
            rho = 1. / sy
            Hy = H @ yv
            H = H - rho * (np.outer(s, Hy) + np.outer(Hy, s)) + (rho * rho * float(yv @ Hy) + rho) * np.outer(s, s)
        th, f, g = tht, ft, gn
        it += 1
    return {'status': status, 'theta': th, 'lml': -f, 'grad': -g, 'iterations': it, 'evaluations': nfev}
