"""Every factor / predict / gradient kernel of csrc/hilo_gp.hip at the edges of the sizes it serves, against the longdouble
reference of tests/gp_reference.py.

The host code chooses a kernel by the training-set size n, by the LDS its tiles need and by three environment switches.
`factor_path` and `predict_path` below restate that arithmetic (`gp_factorize`, `hilo_gp_predict`); the sizes of the case matrix
are derived from them for the actual program length of each kernel and nf = 3, and the test ids name the paths a case takes:
`<factor path>-<predict path>-n<n>-<kernel>[+switch]`.

  path           kernel                              n (nf = 3, klen = 10 and 30)      sizes in the matrix
  reg<NT>        gp_predict_reg_kernel<NT>           16 NT - 15 .. 16 NT, NT = 1..16   16 NT - 3 for every NT; 16, 32, 256; 1, 17, 241;
                                                                                       15, 33, 240 (from the factor list)
  mfma2          gp_predict_mfma_kernel<2>           257 .. 352                        257, 272, 352
  mfma1          gp_predict_mfma_kernel<1>           353 .. 528                        353, 400 (nk no multiple of 32), 528
  mfma4          gp_predict_mfma_kernel<4>           <= 208, HILO_GP_PREDICT_LDS only  37, 200, 208
  generic16      gp_predict_kernel, Q = 16           529 ..                            529, 560, 561, 600
  generic32      gp_predict_kernel, Q = 32           <= 504, HILO_GP_PREDICT_VALU only 37, 200, 500
  blocked        gp_factor_blocked_kernel            1 .. 240                          1, 15, 16, 17, 32, 33, 240 and the reg sizes
  blocked_optin  the same, dynamic LDS > 64 KiB      241 .. 560                        241, 256, 257, 560 and the mfma sizes
  unblocked      gp_factor_kernel                    561 .., or the switch             561, 600; 17, 200 (HILO_GP_FACTOR_UNBLOCKED)
  (kmat_kernel, mean_kernel run in every case; gp_linv_kernel in every case, gp_linv_swizzle_kernel's output is read by the
   reg cases; gp_amat_kernel and gp_grad_kernel in the gradient cases, one block column of the grid at n = 20, the grid-stride
   loop and all 64 blocks at n = 129 and 200.)

Tolerance.  For every number there are the reference r (longdouble), the float64 oracle o (`oracle.gp.Posterior`, LAPACK) and
the device result d; the assertion is  max|d - r| <= C max(max|o - r|, 4 eps64 scale)  with scale = max|r| for the mean and the
LML and k(x, x) for the variance: max|o - r| is what float64 in another summation order costs on this very problem.  For the
gradient the floor needs its own scale: dK/dtheta is a central difference (step h = 1e-5 in log theta) of float64 kernel values,
each good to a relative eps64 at best, so an error of eps64 (|K+| + |K-|) / (2 h) per entry reaches the trace; to first order the
gradient moves by at most  eps64 scale_j,  scale_j = 1/2 sum_ab |A_ab| (|K+_ab| + |K-_ab|) / (2 h)  with A = alpha alpha^T - K_y^-1.
The oracle and the reference share their kernel matrices, so max|o - r| cannot see this; the device evaluates its own.

The three results of a case are taken over ALL its query counts together (the concatenation of the four predictions): one
query alone makes max|o - r| a single sample - 7e-17 was seen at m = 1 next to device errors of 4e-15, no larger than at the other
counts of the same handle - while the figures per query count are still printed.

Largest ratio  max|d - r| / max(max|o - r|, 4 eps64 scale)  of each path on an MI355X (both kernels, every size of the matrix;
every test prints its own as `RATIO <path> <quantity> <ratio> ...`):

  path        quantity    largest ratio   where
  reg         mean         2.30           n = 173, se_ard02
              variance     1.78           n = 93, se_ard02
  mfma1       mean         1.31           n = 353, se_ard02
              variance     1.61           n = 400, se_ard02
  mfma2       mean         1.60           n = 352, se_ard02
              variance     2.35           n = 272 after the refit, se_ard02
  mfma4       mean         1.18           n = 37, se_ard02
              variance     1.63           n = 208, se_ard02
  generic     mean         1.31           n = 600, se_ard02 (Q = 16)
              variance     1.66           n = 200, se_ard02 (Q = 32)
  blocked     LML          8.76           n = 109, se_ard02: |d - r| = 6.7e-14 where three terms of size 100 cancel to an LML of
                                          8.65; the oracle happens to be within 1.9e-16 there, so the floor 4 eps64 |LML| is the bound
  unblocked   LML          0.93           n = 561, se_ard02
  gradient    d LML/d theta  0.04         n = 20, Matern 5/2
  (blocked against unblocked factor, and the three predict kernels on one handle, against each other: at most 0.83 of the bound)

C = 64: the next power of two at or above four times the largest of them (4 x 8.76 = 35).
"""
import collections

import numpy as np
import pytest

from tests import gp_reference as R
from tests.util import kernel_from_spec, mean_from_spec

pytestmark = pytest.mark.gpu

C = 64.0

SWITCHES = ('HILO_GP_PREDICT_LDS', 'HILO_GP_PREDICT_VALU', 'HILO_GP_FACTOR_UNBLOCKED')
LDS, VALU, UNBLOCKED = SWITCHES


# =================================================================================================
# the dispatch arithmetic of csrc/hilo_gp.hip, restated
# =================================================================================================
def factor_path(n, env=()):
    """gp_factorize: the blocked kernel while its dynamic LDS (diagonal block, T inverses, panel, right-hand side) fits 150 KiB."""
    T = (n + 15) // 16
    lds = 8 * (16 * 17 + T * 256 + T * 16 * 16 + T * 16)
    if lds <= 150 * 1024 and UNBLOCKED not in env:
        return 'blocked_optin' if lds > 64 * 1024 else 'blocked'          # above 64 KiB the launch needs hipFuncSetAttribute
    return 'unblocked'


def predict_path(n, klen, env=(), nf=R.NF):
    """hilo_gp_predict: register kernel up to n_pad = 256; matrix-core kernel with the widest tile W in {4, 2, 1} whose LDS fits
    150 KiB; else the LDS / VALU kernel with Q in {32, 16, ...} queries per workgroup (tile within 128 KiB)."""
    n_pad = (n + 15) & ~15
    if n_pad <= 256 and VALU not in env and LDS not in env:
        return f'reg{n_pad // 16}'

    def lds_of(w):
        return 8 * ((n_pad + 16) * (16 * w + 16) + 64 * w + klen + nf * (n_pad + 16 * w))
    W = 4
    while W > 1 and lds_of(W) > 150 * 1024:
        W >>= 1
    if lds_of(W) <= 150 * 1024 and VALU not in env:
        return f'mfma{W}'
    Q = 32
    while Q > 1 and 8 * (n * Q + 256) > 128 * 1024:
        Q >>= 1
    return f'generic{Q}'


def program_length(kern):
    return len(kernel_from_spec(R.KERNELS[kern][0]).program(R.NF))


def _sizes_of(path_of, label, upto=700):
    ns = [n for n in range(1, upto + 1) if path_of(n) == label]
    return ns[0], ns[-1]


# query counts that leave partial tiles in each kernel's own tile width: 64 per workgroup (16 per wave) in the register kernel,
# Q = 16 W in the matrix-core kernel, Q = 16 or 32 in the generic one
QUERY_COUNTS = {'reg': (1, 63, 65, 130), 'mfma': (1, 17, 33, 70), 'generic': (1, 31, 33, 50)}

Case = collections.namedtuple('Case', 'n kern env factor predict')


def _family(path):
    return path.rstrip('0123456789')


def case_id(c):
    return f"{c.factor}-{c.predict}-n{c.n}-{c.kern}" + ''.join('+' + s[len('HILO_GP_'):].lower() for s in c.env)


def build_cases():
    cases = []
    for kern in R.KERNELS:
        klen = program_length(kern)

        def pp(n, env=()):
            return predict_path(n, klen, env)
        reg_last = _sizes_of(pp, 'reg16')[1]
        w2, w1 = _sizes_of(pp, 'mfma2'), _sizes_of(pp, 'mfma1')
        assert w2[0] == reg_last + 1 and w1[0] == w2[1] + 1
        optin_first, blocked_last = _sizes_of(factor_path, 'blocked_optin')
        w4_last = _sizes_of(lambda n: pp(n, (LDS,)), 'mfma4')[1]
        natural = {16 * NT - 3 for NT in range(1, 17)} | {16, 32, reg_last} | {1, 17, 16 * 15 + 1}        # register kernel
        natural |= {w2[0], 272, w2[1]} | {w1[0], 400, w1[1]}                                               # matrix cores, W = 2, 1
        natural |= {w1[1] + 1, 600}                                                                        # generic, Q = 16
        natural |= {1, 15, 16, 17, 32, 33, optin_first - 1, optin_first, 256, 257, blocked_last}           # blocked factor
        natural |= {blocked_last + 1, 600}                                                                 # unblocked factor
        for n in sorted(natural):
            cases.append(Case(n, kern, (), factor_path(n), pp(n)))
        for env, sizes in (((LDS,), (37, 200, w4_last)), ((VALU,), (37, 200, 500)), ((UNBLOCKED,), (17, 200))):
            for n in sizes:
                cases.append(Case(n, kern, env, factor_path(n, env), pp(n, env)))
    return cases


CASES = build_cases()


# =================================================================================================
# helpers
# =================================================================================================
def make_gp(n, kern):
    from hilo_mpc_amd import GP
    ks, ms = R.KERNELS[kern]
    gp = GP(R.FEATURES, 'y', kernel=kernel_from_spec(ks), mean=mean_from_spec(ms), noise_variance=R.NOISE_VARIANCE)
    gp.set_training_data(*R.training_data(n))
    gp.setup()
    return gp


def set_switches(monkeypatch, env):
    """The library reads the switches with getenv on every call."""
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for s in env:
        monkeypatch.setenv(s, '1')


class Checks:
    """Prints every figure before anything is asserted; `done()` then fails with the list of those beyond C times the bound."""

    def __init__(self, label):
        self.label, self.failed = label, []

    def __call__(self, path, quantity, d, r, o, scale, factor=1.0):
        err, bnd = R.error(d, r), R.bound(o, r, scale)
        print(f"RATIO {path:<14s} {quantity:<12s} {err / bnd:9.3f}   |d-r| = {err:.3e}  bound = {bnd:.3e}  [{self.label}]")
        if not err <= factor * C * bnd:
            self.failed.append(f"{path} {quantity}: |d - r| = {err:.3e} > {factor * C:g} x {bnd:.3e}")

    def pair(self, what, a, b, o, r, scale, factor):
        diff, bnd = R.error(a, b), R.bound(o, r, scale)
        print(f"PAIR  {what:<27s} {diff / bnd:9.3f}   |a-b| = {diff:.3e}  bound = {bnd:.3e}  [{self.label}]")
        if not diff <= factor * C * bnd:
            self.failed.append(f"{what}: |a - b| = {diff:.3e} > {factor * C:g} x {bnd:.3e}")

    def done(self):
        assert not self.failed, f"{self.label}: " + '; '.join(self.failed)


def predict_all(gp, n, kern, counts):
    """Predictions at `queries(m)` for every m of `counts`, with and without noise; the mean-only call and a device-tensor
    query must repeat the first call bit for bit.  Returns {'mean' | 'var' | 'var_nf': (device, reference, oracle)}, each the
    concatenation over the query counts - the three results of one case."""
    import torch
    sn2 = R.reference(n, kern).sn2
    cat = {k: ([], [], []) for k in ('mean', 'var', 'var_nf')}
    for m in counts:
        Xq, p = R.queries(m).copy(), R.predictions(n, kern, m)      # (the shared array is read-only; torch wants a writable one)
        (rm, rv), (om, ov) = p['ref'], p['orc']
        mean, var = gp.predict(Xq)
        mean_nf, var_nf = gp.predict(Xq, noise_free=True)
        assert mean.shape == var.shape == var_nf.shape == (1, m)
        np.testing.assert_array_equal(mean_nf, mean)
        mean_only, none = gp.predict(Xq, return_var=False)
        assert none is None
        np.testing.assert_array_equal(mean_only, mean)
        md, vd = gp.predict(torch.as_tensor(Xq, device='cuda'))
        assert isinstance(md, torch.Tensor) and isinstance(vd, torch.Tensor) and md.is_cuda and vd.is_cuda
        np.testing.assert_array_equal(md.cpu().numpy(), mean)
        np.testing.assert_array_equal(vd.cpu().numpy(), var)
        for key, d, r, o in (('mean', mean[0], rm, om), ('var', var[0], rv + R.LD(sn2), ov + sn2), ('var_nf', var_nf[0], rv, ov)):
            print(f"      m = {m:<4d}{key:<7s} max|d-r| = {R.error(d, r):.3e}  max|o-r| = {R.error(o, r):.3e}")
            for dst, src in zip(cat[key], (d, r, o)):
                dst.append(np.asarray(src, dtype=R.LD))
    return {k: tuple(np.concatenate(x) for x in v) for k, v in cat.items()}


def check_predictions(chk, out, kern, path, factor=1.0):
    row = path if path.startswith('mfma') else _family(path)
    for key, (d, r, o) in out.items():
        chk(row, key, d, r, o, np.max(np.abs(r)) if key == 'mean' else R.SIGNAL_VARIANCE[kern], factor)


# =================================================================================================
# the case matrix
# =================================================================================================
@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_path(case, monkeypatch):
    """One GP per (n, kernel): LML of the factorisation, then predictions at every query count of the predict path."""
    set_switches(monkeypatch, case.env)
    n, kern = case.n, case.kern
    gp = make_gp(n, kern)
    ref, orc = R.reference(n, kern), R.oracle(n, kern)
    chk = Checks(case_id(case))
    chk(case.factor.replace('_optin', ''), 'lml', gp.log_marginal_likelihood(), ref.lml, orc.lml, abs(float(ref.lml)))
    check_predictions(chk, predict_all(gp, n, kern, QUERY_COUNTS[_family(case.predict)]), kern, case.predict)
    chk.done()


@pytest.mark.parametrize('kern', list(R.KERNELS))
@pytest.mark.parametrize('n', [17, 200])
def test_forced_unblocked_factor_agrees_with_blocked(n, kern, monkeypatch):
    """The two factor kernels on the same matrix: LML and predictions agree within the tolerance either is held to."""
    set_switches(monkeypatch, ())
    blocked = make_gp(n, kern)
    set_switches(monkeypatch, (UNBLOCKED,))
    unblocked = make_gp(n, kern)
    set_switches(monkeypatch, ())
    ref, orc = R.reference(n, kern), R.oracle(n, kern)
    chk = Checks(f"blocked ~ unblocked n={n} {kern}")
    chk.pair('lml', blocked.log_marginal_likelihood(), unblocked.log_marginal_likelihood(), orc.lml, ref.lml, abs(float(ref.lml)), 1.0)
    b, u = predict_all(blocked, n, kern, QUERY_COUNTS['reg']), predict_all(unblocked, n, kern, QUERY_COUNTS['reg'])
    for key in b:
        _, r, o = b[key]
        chk.pair(key, b[key][0], u[key][0], o, r, np.max(np.abs(r)) if key == 'mean' else R.SIGNAL_VARIANCE[kern], 1.0)
    chk.done()


@pytest.mark.parametrize('kern', list(R.KERNELS))
def test_three_predict_kernels_on_one_handle(kern, monkeypatch):
    """n = 200: the register kernel, the matrix-core kernel (W = 4) and the generic kernel (Q = 32) read the same alpha and
    L^-1 of one handle; each matches the reference, and each other within twice the tolerance."""
    n, counts, klen = 200, (33, 70), program_length(kern)
    set_switches(monkeypatch, ())
    gp = make_gp(n, kern)
    chk = Checks(f"one handle n={n} {kern}")
    out = {}
    for env, path in (((), 'reg13'), ((LDS,), 'mfma4'), ((VALU,), 'generic32')):
        assert predict_path(n, klen, env) == path
        set_switches(monkeypatch, env)
        out[path] = predict_all(gp, n, kern, counts)
        check_predictions(chk, out[path], kern, path)
    for a, b in (('reg13', 'mfma4'), ('reg13', 'generic32'), ('mfma4', 'generic32')):
        for key in ('mean', 'var', 'var_nf'):
            _, r, o = out[a][key]
            chk.pair(f'{key} {a} ~ {b}', out[a][key][0], out[b][key][0], o, r,
                     np.max(np.abs(r)) if key == 'mean' else R.SIGNAL_VARIANCE[kern], 2.0)
    chk.done()


# =================================================================================================
# gradient of the log marginal likelihood
# =================================================================================================
def _se_spec(v):
    return {'type': 'squared_exponential', 'kwargs': {'active_dims': [0, 2], 'length_scales': [float(v[0]), float(v[1])],
                                                      'signal_variance': float(v[2]), 'ard': True}}


def _m52_spec(v):
    return {'type': 'matern_52', 'kwargs': {'active_dims': [0, 2], 'length_scales': float(v[0]), 'signal_variance': float(v[1])}}


GRADIENT_KERNELS = {'se_ard02': (_se_spec, [1.3, .8, 1.]), 'm52': (_m52_spec, [.9, .8])}


@pytest.mark.parametrize('kern', list(GRADIENT_KERNELS))
@pytest.mark.parametrize('n', [20, 128, 129, 200])
def test_lml_gradient(n, kern):
    """hilo_gp_lml_gradient with the +- programs of test_gp_gpu.py::test_device_lml_gradient_vs_oracle_trace_formula.  n * n > 64 * 256
    (n > 128) is where gp_grad_kernel's grid stops growing and every thread loops."""
    from hilo_mpc_amd import GP, _lib
    from oracle import gp as ogp
    spec_of, values = GRADIENT_KERNELS[kern]
    X, y = R.training_data(n)
    g = GP(R.FEATURES, 'y', kernel=kernel_from_spec(spec_of(values)), noise_variance=R.NOISE_VARIANCE)
    g.set_training_data(X, y)
    g.setup()
    th = np.log(np.asarray(g.hyperparameter_values))
    h = 1e-5
    progs, noise, dKy, Kabs = [], [], [], []
    for i in range(th.size):
        Kpm = []
        for sgn in (1., -1.):
            e = np.zeros_like(th)
            e[i] = sgn * h
            v = np.exp(th + e)
            g._set_hyperparameters(v)
            progs.append(np.asarray(g.kernel.program(R.NF), dtype=np.float64))
            noise.append(float(g.noise_variance))
            Kpm.append(ogp.kernel(spec_of(v[1:]), X, X) + float(v[0]) * np.eye(n))
        dKy.append((Kpm[0].astype(R.LD) - Kpm[1].astype(R.LD)) / (2 * R.LD(h)))
        Kabs.append(np.abs(Kpm[0]) + np.abs(Kpm[1]))
    g._set_hyperparameters(np.exp(th))
    progs, noise, hh = np.ascontiguousarray(np.stack(progs)), np.array(noise), np.full(th.size, h)
    out = np.zeros(th.size)
    _lib.check(_lib.lib().hilo_gp_lml_gradient(g._handle, th.size, progs.ctypes.data, noise.ctypes.data, hh.ctypes.data,
                                               out.ctypes.data))
    ref = R.Reference(spec_of(values), {'type': 'zero'}, X, y, R.NOISE_VARIANCE)
    orc = ogp.Posterior(spec_of(values), {'type': 'zero'}, X, y, R.NOISE_VARIANCE)
    r = ref.lml_gradient(dKy)
    o = R.oracle_lml_gradient(orc, [np.asarray(d, dtype=np.float64) for d in dKy])
    A = np.abs(ref.trace_weights())
    chk = Checks(f"gradient n={n} {kern}")
    for j in range(th.size):
        scale = float(np.sum(A * Kabs[j])) / 2 / (2 * h)
        chk('gradient', f'theta_{j}', out[j], r[j], o[j], scale)
    assert np.max(np.abs(r)) > 1.                    # a gradient worth the name: the point is no optimum
    chk.done()


# =================================================================================================
# refit, and a matrix that is not positive definite
# =================================================================================================
def test_refit_rebuilds_l_inverse_on_the_matrix_core_path(monkeypatch):
    """New hyper-parameters into an n = 272 handle whose L^-1 is already built: the variance afterwards is that of a fresh GP
    at the new values (to the bit: same kernels on the same inputs), and that of the reference."""
    set_switches(monkeypatch, ())
    from hilo_mpc_amd import GP
    n, m, kern = 272, 33, 'se_ard02'
    assert predict_path(n, program_length(kern)) == 'mfma2'
    X, y = R.training_data(n)
    Xq = R.queries(m).copy()
    gp = make_gp(n, kern)
    _, var_old = gp.predict(Xq)                                            # builds L^-1 of the old factor
    new = [2e-2, 1.6, .7, 1.2]
    gp._set_hyperparameters(new)
    assert gp._device_refit()
    mean, var = gp.predict(Xq)
    fresh = GP(R.FEATURES, 'y', kernel=kernel_from_spec(_se_spec(new[1:])), noise_variance=new[0])
    fresh.set_training_data(X, y)
    fresh.setup()
    mean_f, var_f = fresh.predict(Xq)
    assert gp.log_marginal_likelihood() == fresh.log_marginal_likelihood()
    np.testing.assert_array_equal(mean, mean_f)
    np.testing.assert_array_equal(var, var_f)
    assert np.max(np.abs(var - var_old)) > 1e-3                            # the new values are another posterior
    ref = R.Reference(_se_spec(new[1:]), {'type': 'zero'}, X, y, new[0])
    from oracle import gp as ogp
    orc = ogp.Posterior(_se_spec(new[1:]), {'type': 'zero'}, X, y, new[0])
    rm, rv = ref.predict(Xq)
    om, ov = orc.predict(Xq)
    chk = Checks(f"refit n={n} {kern}")
    chk('blocked', 'lml', gp.log_marginal_likelihood(), ref.lml, orc.lml, abs(float(ref.lml)))
    chk('mfma2', 'mean', mean[0], rm, om[0], np.max(np.abs(rm)))
    chk('mfma2', 'var', var[0], rv, ov[0], new[3])
    chk.done()


@pytest.mark.parametrize('env', [(), (UNBLOCKED,)], ids=['blocked', 'unblocked'])
def test_not_positive_definite_reports_the_first_bad_pivot(env, monkeypatch):
    """A constant kernel without noise: K is all ones, the second pivot is exactly 1 - 1 = 0 in any arithmetic."""
    from hilo_mpc_amd import GP, Kernel
    set_switches(monkeypatch, env)
    n = 40
    assert factor_path(n, env) == ('unblocked' if env else 'blocked')
    gp = GP(['x'], 'y', kernel=Kernel.constant(), noise_variance=0.)
    gp.set_training_data(np.arange(n, dtype=float)[None, :], np.arange(n, dtype=float)[None, :])
    with pytest.raises(ValueError, match=r"not positive definite \(pivot 2\)"):
        gp.setup()
