"""CPU: host side of `GPArray` (hilo_mpc_amd/gp.py) - the slot maps that let the device rebuild a kernel program from the
optimisation variables, the container protocol, shapes, refusals and restart start points - and the numpy restatement of the
device optimiser (tests/gp_fit_batch_reference.py) against the reference's fitted-value known answers."""
import warnings

import numpy as np
import pytest

from tests import gp_fit_batch_reference as ref


def _kernels():
    from hilo_mpc_amd import Kernel as K
    ard = dict(active_dims=[0, 2], ard=True, length_scales=[.7, 1.9])
    iso = dict(length_scales=1.3, signal_variance=.6)
    out = {'Const': (K.constant(bias=1.7), 3)}
    for name, make in (('SE', K.squared_exponential), ('E', K.exponential), ('M32', K.matern_32), ('M52', K.matern_52),
                       ('RQ', K.rational_quadratic), ('PP0', lambda **kw: K.piecewise_polynomial(0, **kw)),
                       ('PP3', lambda **kw: K.piecewise_polynomial(3, **kw))):
        out[name + '-iso'] = (make(**iso), 3)
        out[name + '-ard'] = (make(**ard), 3)
    from hilo_mpc_amd.gp import GammaExponentialKernel
    out['GE-iso'] = (GammaExponentialKernel(gamma=1.2, **iso), 2)
    out['GE-ard'] = (GammaExponentialKernel(gamma=.8, **ard), 3)
    out['Poly'] = (K.polynomial(3, active_dims=[1, 2], offset=.4), 3)
    out['Lin'] = (K.linear(signal_variance=2.), 2)
    out['NN'] = (K.neural_network(weight_variance=.3), 2)
    out['Periodic'] = (K.periodic(active_dims=[1], length_scales=.8, period=2.5), 3)
    out['Sum'] = (K.squared_exponential(**ard) + K.linear(active_dims=[1]), 3)
    out['Product'] = (K.matern_32(**iso) * K.periodic(active_dims=[0], period=1.5), 3)
    out['Power'] = (K.rational_quadratic(alpha=2., **ard) ** 2, 3)
    out['Tree'] = ((K.squared_exponential(**ard) * K.constant(.5) + K.matern_52(**iso) ** 3) * K.polynomial(2), 3)
    return out


KERNELS = _kernels()


@pytest.mark.parametrize('name', list(KERNELS))
def test_program_rebuilt_from_the_slot_map(name):
    """exp(coef * theta) / coef * theta at the mapped slots of any program of the kernel = `program(nf)` at exp(theta)."""
    from hilo_mpc_amd import GP
    from hilo_mpc_amd.gp import MAP_EXP
    kernel, nf = KERNELS[name]
    g = GP([f'x{i}' for i in range(nf)], 'y', kernel=kernel, noise_variance=.1)
    base = np.array(kernel.program(nf))
    pmap = kernel.program_map(nf)
    assert len(pmap) == len(kernel.hyperparameter_handles()) == len(g.hyperparameter_values) - 1
    assert all(len(entry) >= 1 for entry in pmap)
    slots = [s for entry in pmap for s, _, _ in entry]
    assert len(set(slots)) == len(slots)
    rng = np.random.default_rng(len(name))
    for _ in range(3):
        theta = rng.normal(size=1 + len(pmap))
        g._set_hyperparameters(np.exp(theta))
        want = np.array(kernel.program(nf))
        got = base.copy()
        for j, entry in enumerate(pmap):
            for slot, kind, c in entry:
                got[slot] = np.exp(c * theta[1 + j]) if kind == MAP_EXP else c * theta[1 + j]
        np.testing.assert_allclose(got, want, rtol=1e-14, atol=0)
        assert np.any(want != base)


def test_power_is_not_a_hyperparameter():
    from hilo_mpc_amd import Kernel as K
    k = K.squared_exponential() ** 3
    prog = k.program(1)
    assert prog[-1] == 3. and len(prog) - 1 not in [s for e in k.program_map(1) for s, _, _ in e]


@pytest.mark.parametrize('row', ref.KATS, ids=[r[0] for r in ref.KATS])
def test_restated_optimiser_reaches_the_reference_known_answers(row):
    """The optimiser the device runs, in numpy on the oracle's objective and gradient, from the reference's start (noise
    variance e^-2, every kernel hyper-parameter 1), within the tolerances of tests/test_gp_gpu.py::test_fit_model_reference_kats."""
    kid, ktype, names, fixed, shift, expected, rtol = row
    x, y = ref.kat_data()
    th0 = np.log([np.exp(-2)] + [1.] * len(names))
    res = ref.fit(None, th0, x.T, (y + shift).T, oracle_single=(ktype, names, fixed))
    assert res['status'] == 0 and np.max(np.abs(res['grad'])) <= 1e-6
    assert 1 <= res['iterations'] <= 60 and res['evaluations'] >= res['iterations'] + 1
    np.testing.assert_allclose(np.exp(res['theta']), expected, rtol=max(rtol, 2e-6))
    # the general (tree) objective and gradient are the same functions
    sp = ref.single(ktype, names, fixed)
    np.testing.assert_allclose(ref.lml(sp, res['theta'], x.T, (y + shift).T), res['lml'], rtol=1e-13)
    np.testing.assert_allclose(ref.lml_gradient(sp, th0, x.T, (y + shift).T),
                               __import__('oracle.gp_fit').gp_fit.lml_gradient(ktype, names, th0, x.T, (y + shift).T, fixed, h=1e-5),
                               rtol=1e-12, atol=1e-14)


def test_restated_optimiser_two_optima_and_statuses():
    x, y = ref.kat_data()
    sp = ref.single('squared_exponential', ['length_scales', 'signal_variance'])
    bad = ref.fit(sp, np.log([1., 10., 1.]), x.T, y.T)
    good = ref.fit(sp, np.log([np.exp(-2), 1., 1.]), x.T, y.T)
    assert bad['status'] == 0 and good['status'] == 0
    np.testing.assert_allclose(bad['lml'], -24.35894, rtol=1e-6)
    np.testing.assert_allclose(np.exp(bad['theta'][0]), .668992, rtol=1e-5)
    np.testing.assert_allclose(good['lml'], 2.78213, rtol=1e-6)
    assert ref.fit(sp, np.log([np.exp(-2), 1., 1.]), x.T, y.T, maxiter=3)['status'] == 1
    ev = ref.fit(sp, np.log([np.exp(-2), 1., 1.]), x.T, y.T, maxiter=0)
    assert ev['status'] == 1 and ev['iterations'] == 0 and ev['evaluations'] == 1
    # a constant kernel on duplicate inputs with the smallest positive noise variance: the oracle's Cholesky fails at the start
    xd = np.array([[.5, .5, 1.]])
    with pytest.raises(np.linalg.LinAlgError):
        from oracle import gp as ogp
        ogp.Posterior({'type': 'constant', 'kwargs': {'bias': 1.}}, {'type': 'zero'}, xd, np.array([1., 2., 3.]), 5e-324)
    assert ref.fit(ref.single('constant', ['bias']), np.log([5e-324, 1.]), xd, np.array([1., 2., 3.]))['status'] == 3


# ---- container ------------------------------------------------------------------------------------------------------------
def test_container_protocol():
    from hilo_mpc_amd import GP, GPArray, GaussianProcess, Kernel
    arr = GPArray(3)
    assert len(arr) == 3 and arr[0] is None and arr[2] is None
    filled = list(arr)                                        # iteration fills the empty slots with uninitialised objects
    assert len(filled) == 3 and all(type(g) is GaussianProcess for g in filled) and arr[1] is filled[1]
    assert not filled[0].is_setup()
    with pytest.raises(RuntimeError, match="empty members"):
        arr.setup()
    g = GP(['a'], 'b')
    arr[1] = g
    assert arr[1] is g and list(arr)[1] is g
    with pytest.raises(TypeError):
        arr[0] = 'gp'
    with pytest.raises(IndexError):
        arr[3]
    fl = GPArray.from_labels(['S', 'I'], ['mu', 'Rs', 'Rfp'], kernel=Kernel.matern_52(length_scales=2.), noise_variance=[.1, .2, .3])
    assert len(fl) == 3 and [m.labels for m in fl] == [['mu'], ['Rs'], ['Rfp']] and all(m.features == ['S', 'I'] for m in fl)
    assert fl[0].kernel is not fl[1].kernel and fl[1].kernel.length_scales == 2. and [m.noise_variance for m in fl] == [.1, .2, .3]
    ks = [Kernel.constant(), Kernel.linear()]
    two = GPArray.from_labels(['x'], ['a', 'b'], kernel=ks)
    assert two[0].kernel is ks[0] and two[1].kernel is ks[1]
    assert GPArray.from_labels(['x'], ['a'])[0].kernel.acronym == 'SE'
    with pytest.raises(ValueError, match="Dimension mismatch"):
        GPArray.from_labels(['x'], ['a', 'b'], kernel=[Kernel.constant()])


def test_training_data_shapes():
    from hilo_mpc_amd import GPArray
    arr = GPArray.from_labels(['S', 'I'], ['mu', 'Rs'])
    X, Y = np.arange(10.).reshape(2, 5), np.arange(10.).reshape(2, 5) + 1.
    arr.set_training_data(X, Y)
    np.testing.assert_array_equal(arr[1].y_train, Y[1:2])
    np.testing.assert_array_equal(arr[0].X_train, X)
    with pytest.raises(ValueError, match="dimension for the labels is 3"):
        arr.set_training_data(X, np.zeros((3, 5)))
    with pytest.raises(ValueError, match="dimension for the features is 3"):
        arr.set_training_data(np.zeros((3, 5)), Y)
    with pytest.raises(ValueError, match="do not match"):
        arr.set_training_data(X, np.zeros((2, 4)))
    arr[1].set_training_data(X[:, :3], Y[1:2, :3])             # a member may have its own data
    assert arr[1].X_train.shape == (2, 3) and arr[0].X_train.shape == (2, 5)
    with pytest.raises(RuntimeError, match="has not been set up"):
        arr.predict(X)
    with pytest.raises(RuntimeError, match="has not been set up"):
        arr.log_marginal_likelihood()


def _stub_array(n=2, **kw):
    """Members that claim to be set up (no device here): what `_fit_problem` and `_start_points` look at."""
    from hilo_mpc_amd import GPArray, GaussianProcess

    class Stub(GaussianProcess):
        def is_setup(self):
            return True
    arr = GPArray(n)
    for k in range(n):
        arr[k] = Stub(['x'], [f'y{k}'], **kw)
        arr[k].set_training_data(np.linspace(0., 1., 6)[None], np.linspace(0., 1., 6)[None] ** 2)
    return arr


def test_refusals_name_the_single_gp_route():
    from hilo_mpc_amd import GPArray, Kernel, Mean
    arr = GPArray.from_labels(['x'], ['a', 'b'])
    arr.set_training_data(np.zeros((1, 4)), np.zeros((2, 4)))
    with pytest.raises(NotImplementedError, match=r"member 0 .*not set up.*GaussianProcess.fit_model of member 0"):
        arr.fit_model()
    arr = _stub_array()
    arr[1].set_hyperprior('SE.length_scales', 'Gaussian')
    with pytest.raises(NotImplementedError, match=r"hyper-priors.*GaussianProcess.fit_model of member 1"):
        arr.fit_model()
    arr = _stub_array(kernel=Kernel.squared_exponential(bounds={'length_scales': (.1, 10.)}))
    with pytest.raises(NotImplementedError, match=r"boxed bounds.*GaussianProcess.fit_model of member 0"):
        arr.fit_model()
    arr = _stub_array(mean=Mean.constant(.3))
    with pytest.raises(NotImplementedError, match=r"mean function.*GaussianProcess.fit_model of member 0"):
        arr.fit_model()
    # 'fixed' is supported: the hyper-parameter is simply absent from the variables and from the map
    arr = _stub_array(kernel=Kernel.squared_exponential(signal_variance=.5, bounds={'signal_variance': 'fixed'}),
                      mean=Mean.constant(.3, bounds={'bias': 'fixed'}))
    pb = arr._fit_problem(0, arr[0])
    assert pb['free'] == [0, 1] and list(pb['theta']) == [1] and pb['kprog'][5] == .5
    # more free hyper-parameters than the device's inverse Hessian holds
    big = _stub_array(1)
    big[0].features = [f'x{i}' for i in range(16)]
    big[0].kernel = Kernel.squared_exponential(active_dims=list(range(16)), ard=True, length_scales=[1.] * 16)
    big[0].set_training_data(np.zeros((16, 4)), np.zeros((1, 4)))
    with pytest.raises(NotImplementedError, match=r"18 free hyper-parameters.*GaussianProcess.fit_model of member 0"):
        big.fit_model()
    many = _stub_array(1)
    many[0].set_training_data(np.zeros((1, 257)), np.zeros((1, 257)))
    with pytest.raises(NotImplementedError, match=r"257 training points.*n <= 256"):
        many.fit_model()


def test_restart_start_points():
    arr = _stub_array(2, noise_variance=.2)
    arr[1].kernel.length_scales = 3.
    pbs = [arr._fit_problem(g, m) for g, m in enumerate(arr)]
    one = arr._start_points(pbs)
    assert [t.shape for t in one] == [(1, 3), (1, 3)]
    np.testing.assert_array_equal(one[1][0], np.log([.2, 3., 1.]))
    a = arr._start_points(pbs, n_restarts=4, seed=1)
    b = arr._start_points(pbs, n_restarts=4, seed=1)
    c = arr._start_points(pbs, n_restarts=4, seed=2)
    d = arr._start_points(pbs, n_restarts=6, seed=1, spread=1.)
    for g in range(2):
        assert a[g].shape == (4, 3)
        np.testing.assert_array_equal(a[g], b[g])                                   # a function of the seed alone
        np.testing.assert_array_equal(a[g][0], one[g][0])                           # row 0: the current hyper-parameters
        assert not np.array_equal(a[g][1:], c[g][1:])
        np.testing.assert_array_equal(d[g][:4], a[g])
    assert not np.array_equal(a[0][1:] - a[0][0], a[1][1:] - a[1][0])               # members draw their own deviates
    wide = arr._start_points(pbs, n_restarts=4, seed=1, spread=3.)
    np.testing.assert_allclose(wide[0][1:] - wide[0][0], 3. * (a[0][1:] - a[0][0]), rtol=1e-12)
    # explicit starts are values, for all members, per member, or for some
    v = [[1., 10., 1.], [np.exp(-2), 1., 1.]]
    for given in (v, [v, v], {0: v, 1: v}):
        e = arr._start_points(pbs, starts=given)
        np.testing.assert_array_equal(e[0], np.log(v))
        np.testing.assert_array_equal(e[1], np.log(v))
    e = arr._start_points(pbs, n_restarts=2, starts={1: v[:1]}, seed=1)
    np.testing.assert_array_equal(e[0], a[0][:2])
    np.testing.assert_array_equal(e[1], np.log(v[:1]))
    with pytest.raises(ValueError, match="Dimension mismatch"):
        arr._start_points(pbs, starts=[[1., 2.]])
    with pytest.raises(ValueError, match="positive"):
        arr._start_points(pbs, starts=[[1., 0., 1.]])
    with pytest.raises(KeyError):
        arr._start_points(pbs, starts={2: v})
    with pytest.raises(ValueError, match="n_restarts"):
        arr._start_points(pbs, n_restarts=0)


def test_descriptor_mirrors_match_the_header(tmp_path):
    """`_lib.GpFitProblem` / `_lib.GpFitOpts` against include/hilo_hip.h compiled by the C compiler: sizes and offsets."""
    import ctypes as C
    import os
    import shutil
    import subprocess
    from hilo_mpc_amd import _lib
    if shutil.which('gcc') is None:
        pytest.skip('gcc not available')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    pairs = [('hilo_gp_fit_problem', _lib.GpFitProblem), ('hilo_gp_fit_opts', _lib.GpFitOpts)]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hilo_hip.h"', 'int main(void) {']
    for cname, cls in pairs:
        lines.append(f'  printf("{cname} %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname}.{f} %zu\\n", offsetof({cname}, {f}));' for f, _ in cls._fields_]
    lines += ['  printf("limits %d %d %d %d\\n", HILO_GPFIT_MAX_N, HILO_GPFIT_MAX_THETA, HILO_GPFIT_MAX_PROG, HILO_GPFIT_MAX_MAP);',
              '  printf("kinds %d %d\\n", HILO_GPFIT_EXP, HILO_GPFIT_LIN);', '  return 0;', '}']
    (tmp_path / 'layout.c').write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-I', os.path.join(root, 'include'), str(tmp_path / 'layout.c'), '-o', str(tmp_path / 'layout')])
    got = [l.split() for l in subprocess.check_output([str(tmp_path / 'layout')], text=True).strip().split('\n')]
    table = {l[0]: l[1:] for l in got}
    for cname, cls in pairs:
        assert int(table[cname][0]) == C.sizeof(cls)
        for f, _ in cls._fields_:
            assert int(table[f'{cname}.{f}'][0]) == getattr(cls, f).offset, (cname, f)
    from hilo_mpc_amd import gp
    assert [int(v) for v in table['limits']] == [_lib.GPFIT_MAX_N, _lib.GPFIT_MAX_THETA, _lib.GPFIT_MAX_PROG, _lib.GPFIT_MAX_MAP]
    assert [int(v) for v in table['kinds']] == [gp.MAP_EXP, gp.MAP_LIN]


def test_model_substitute_from_takes_the_array_like_the_list_of_its_members():
    """Without a device: the members are handed on one by one, in order (an array with an empty slot is an error)."""
    from hilo_mpc_amd import GPArray, Model
    seen = []

    class M(Model):
        def substitute_from(self, obj):
            if not isinstance(obj, (list, tuple, set, GPArray)):
                seen.append(obj)
                return self
            return Model.substitute_from(self, obj)
    arr = _stub_array(3)
    M('chemostat4').substitute_from(arr)
    assert seen == [arr[0], arr[1], arr[2]]
    with pytest.raises(RuntimeError, match="empty members"):
        M('chemostat4').substitute_from(GPArray(2))
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        assert len(GPArray(0)) == 0
