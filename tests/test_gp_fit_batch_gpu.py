"""GPU: `GPArray.fit_model` - the hyper-parameter fits of many GPs in one launch (csrc/hilo_gp.hip::gp_fit_batch_kernel) - against
the oracle (LML, trace-formula gradient), the reference's fitted-value known answers, the numpy restatement of the device
optimiser (tests/gp_fit_batch_reference.py) and the existing single-GP path."""
import warnings

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import gp as ogp                                  # noqa: E402
from oracle import gp_fit                                     # noqa: E402
from tests import gp_fit_batch_reference as ref               # noqa: E402

E2 = float(np.exp(-2))


def _member(kernel, X, y, noise, features=None):
    from hilo_mpc_amd import GP
    X = np.atleast_2d(X)
    g = GP(features or [f'x{i}' for i in range(X.shape[0])], ['y'], kernel=kernel, noise_variance=noise)
    g.set_training_data(X, np.atleast_2d(y))
    g.setup()
    return g


def _array(members):
    from hilo_mpc_amd import GPArray
    arr = GPArray(len(members))
    for k, m in enumerate(members):
        arr[k] = m
    return arr


# ---- 1. evaluate only -------------------------------------------------------------------------------------------------------
def _eval_cases():
    """(id, product kernel, theta -> oracle spec, oracle (type, names) or None, X, y, noise variance)"""
    from hilo_mpc_amd import Kernel as K
    x, y = ref.kat_data()
    X20, y20 = x.T, y.T
    rng = np.random.default_rng(20261021)
    cases = [('SE', K.squared_exponential(length_scales=.7, signal_variance=1.3),
              ('squared_exponential', ['length_scales', 'signal_variance']), None, X20, y20, .05),
             ('M52', K.matern_52(length_scales=.9, signal_variance=.8), ('matern_52', ['length_scales', 'signal_variance']), None,
              X20, y20, .05)]

    def sum_spec(th):
        return {'type': 'sum', 'children': [
            {'type': 'squared_exponential', 'kwargs': {'length_scales': np.exp(th[1]), 'signal_variance': np.exp(th[2])}},
            {'type': 'linear', 'kwargs': {'signal_variance': np.exp(th[3])}}]}
    cases.append(('Sum', K.squared_exponential(length_scales=.6, signal_variance=.9) + K.linear(signal_variance=.5), None, sum_spec,
                  X20, y20, .1))

    def prod_spec(th):
        return {'type': 'product', 'children': [
            {'type': 'matern_32', 'kwargs': {'length_scales': np.exp(th[1]), 'signal_variance': np.exp(th[2])}},
            {'type': 'periodic', 'kwargs': {'signal_variance': np.exp(th[3]), 'length_scales': np.exp(th[4]), 'period': np.exp(th[5])}}]}
    cases.append(('Product', K.matern_32(length_scales=.8, signal_variance=1.1) * K.periodic(signal_variance=.7, length_scales=1.2, period=2.),
                  None, prod_spec, X20, y20, .08))
    X3 = rng.uniform(-2, 2, (3, 40))

    def ard_spec(th):
        return {'type': 'squared_exponential', 'kwargs': {'active_dims': [0, 1, 2], 'ard': True, 'length_scales': list(np.exp(th[1:4])),
                                                          'signal_variance': np.exp(th[4])}}
    cases.append(('ARD3', K.squared_exponential(active_dims=[0, 1, 2], ard=True, length_scales=[.7, 1.3, 2.], signal_variance=1.2), None,
                  ard_spec, X3, (np.sin(X3[0]) + .3 * X3[1] * X3[2] + .1 * rng.normal(size=40))[None], .02))
    for n in (1, 15, 16, 17, 33):                                  # the edges of the 16-wide blocks
        Xn = rng.uniform(-2, 2, (1, n))
        cases.append((f'n{n}', K.matern_32(length_scales=.8, signal_variance=1.4), ('matern_32', ['length_scales', 'signal_variance']), None,
                      Xn, np.sin(2 * Xn) + .1 * rng.normal(size=(1, n)), .03))
    X2 = rng.uniform(-3, 3, (2, 256))

    def se2_spec(th):
        return {'type': 'squared_exponential', 'kwargs': {'active_dims': [0, 1], 'ard': True, 'length_scales': list(np.exp(th[1:3])),
                                                          'signal_variance': np.exp(th[3])}}
    cases.append(('n256', K.squared_exponential(active_dims=[0, 1], ard=True, length_scales=[1.1, .8], signal_variance=.9), None, se2_spec,
                  X2, (np.sin(X2[0]) * np.cos(X2[1]) + .2 * rng.normal(size=256))[None], .05))
    return cases


def test_evaluate_only_lml_and_gradient_in_one_heterogeneous_launch():
    cases = _eval_cases()
    arr = _array([_member(k, X, y, nv) for _, k, _, _, X, y, nv in cases])
    lml, grads = arr.lml_and_gradient()
    for g, (cid, kernel, single, spec_of, X, y, nv) in enumerate(cases):
        th = np.log(np.asarray(arr[g].hyperparameter_values))
        sp = ref.single(*single) if single else spec_of
        post = ogp.Posterior(sp(th), {'type': 'zero'}, X, y, nv)
        print(cid, 'lml', lml[g], post.lml, 'grad', grads[g])
        np.testing.assert_allclose(lml[g], post.lml, rtol=1e-9, err_msg=cid)
        want = gp_fit.lml_gradient(single[0], single[1], th, X, y, h=1e-5) if single else ref.lml_gradient(sp, th, X, y)
        np.testing.assert_allclose(grads[g], want, rtol=1e-7, atol=1e-9, err_msg=cid)
    for g in (0, 1):                                               # and against the single-GP gradient of the member's own handle
        th = np.log(np.asarray(arr[g].hyperparameter_values))
        np.testing.assert_allclose(grads[g], arr[g]._device_lml_gradient(th, 1e-5), rtol=1e-7, atol=1e-9)
    # evaluate only through fit_model: nothing moves, status = maximum number of iterations (0) reached
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        before = [list(m.hyperparameter_values) for m in arr]
        arr.fit_model(maxiter=0)
    assert [list(m.hyperparameter_values) for m in arr] == before
    assert all(s[0] == 1 and i[0] == 0 and e[0] == 1 for s, i, e in zip(arr.fit_stats['status'], arr.fit_stats['iterations'],
                                                                        arr.fit_stats['evaluations']))
    np.testing.assert_array_equal(np.concatenate(arr.fit_stats['lml']), lml)


# ---- 2., 3. the known answers, and independence of the batch ----------------------------------------------------------------
def _kat_array(rows):
    from hilo_mpc_amd import GPArray, Kernel
    x, y = ref.kat_data()
    arr = GPArray.from_labels(['x'], [f'y_{r[0]}' for r in rows], kernel=[ref.kat_kernel(Kernel, r[0]) for r in rows], noise_variance=E2)
    arr.set_training_data(x.T, np.vstack([(y + r[4]).T for r in rows]))
    arr.setup()
    return arr


@pytest.fixture(scope='module')
def kat_fit():
    arr = _kat_array(ref.KATS)
    lml0 = arr.log_marginal_likelihood()
    with warnings.catch_warnings():
        warnings.simplefilter('error')                             # a successful fit does not warn
        arr.fit_model()
    return arr, lml0


def test_known_answers_of_eleven_kernels_in_one_launch(kat_fit):
    arr, lml0 = kat_fit
    x, y = ref.kat_data()
    st = arr.fit_stats
    print('iterations', [int(v[0]) for v in st['iterations']], 'evaluations', [int(v[0]) for v in st['evaluations']],
          'max|g|', [float(v[0]) for v in st['max_gradient']])
    assert [int(s[0]) for s in st['status']] == [0] * 11 and list(st['chosen']) == [0] * 11
    xs = np.linspace(-3, 3, 61).reshape(1, -1)
    mean, var = arr.predict(xs)
    assert mean.shape == (11, 61) and var.shape == (11, 61)
    for g, (kid, ktype, names, fixed, shift, expected, rtol) in enumerate(ref.KATS):
        np.testing.assert_allclose(arr[g].hyperparameter_values, expected, rtol=max(rtol, 2e-6), err_msg=kid)
        assert arr[g].log_marginal_likelihood() > lml0[g] and arr[g]._optimization_stats['success']
        np.testing.assert_allclose(arr[g].log_marginal_likelihood(), st['lml'][g][0], rtol=1e-10)
        assert st['max_gradient'][g][0] <= 1e-6
        # the numpy restatement of the optimiser stops the same way (the iterates differ in the last bits: counts are not compared)
        r = ref.fit(None, np.log([E2] + [1.] * len(names)), x.T, (y + shift).T, oracle_single=(ktype, names, fixed))
        assert r['status'] == st['status'][g][0]
        np.testing.assert_allclose(st['lml'][g][0], r['lml'], rtol=1e-8, err_msg=kid)
        vals = arr[g].hyperparameter_values
        post = ogp.Posterior(ref.single(ktype, names, fixed)(np.log(vals)), {'type': 'zero'}, x.T, (y + shift).T, vals[0])
        mo, vo = post.predict(xs)
        np.testing.assert_allclose(mean[g:g + 1], mo, rtol=1e-6, atol=1e-8, err_msg=kid)
        np.testing.assert_allclose(var[g:g + 1], vo, rtol=1e-5, atol=1e-9, err_msg=kid)


def _rows(arr):
    st = arr.fit_stats
    return [(st['theta'][g][0].tobytes(), st['lml'][g][0].tobytes(), int(st['iterations'][g][0]), int(st['evaluations'][g][0]),
             int(st['status'][g][0]), tuple(arr[g].hyperparameter_values)) for g in range(len(arr))]


def test_a_result_does_not_depend_on_the_batch_or_the_position(kat_fit):
    batch = _rows(kat_fit[0])
    rev = _kat_array(ref.KATS[::-1])
    rev.fit_model()
    assert _rows(rev)[::-1] == batch
    for g, row in enumerate(ref.KATS):
        alone = _kat_array([row])
        alone.fit_model()
        assert _rows(alone)[0] == batch[g], row[0]


# ---- 4. restarts ------------------------------------------------------------------------------------------------------------
def _se_member(noise=1., ls=10., sv=1.):
    from hilo_mpc_amd import Kernel
    x, y = ref.kat_data()
    return _member(Kernel.squared_exponential(length_scales=ls, signal_variance=sv), x.T, y.T, noise)


def test_restarts_pick_the_better_of_two_optima():
    arr = _array([_se_member()])
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        arr.fit_model(starts=[[1., 10., 1.], [E2, 1., 1.]])
    st = arr.fit_stats
    print('lml', st['lml'][0], 'status', st['status'][0], 'iterations', st['iterations'][0])
    np.testing.assert_allclose(st['lml'][0], [-24.35894, 2.78213], rtol=1e-6)
    assert st['chosen'][0] == 1 and list(st['status'][0]) == [0, 0]
    np.testing.assert_allclose(arr[0].hyperparameter_values, [.0085251, .5298217, .8114553], rtol=1e-5)
    np.testing.assert_allclose(arr[0].log_marginal_likelihood(), 2.78213, rtol=1e-6)
    one = _array([_se_member()])
    one.fit_model()                                                # from (1, 10, 1) alone: the all-noise optimum
    np.testing.assert_allclose(one[0].noise_variance, .668992, rtol=1e-5)
    four = _array([_se_member()])
    four.fit_model(n_restarts=4, seed=1)
    s1, s4 = one.fit_stats, four.fit_stats
    assert s4['lml'][0].shape == (4,)
    for k in ('theta', 'lml', 'iterations', 'evaluations', 'status', 'max_gradient'):
        assert np.asarray(s4[k][0][0]).tobytes() == np.asarray(s1[k][0][0]).tobytes(), k
    ok = (s4['status'][0] == 0) | (s4['max_gradient'][0] < 1e-4)
    assert ok[0] and s4['lml'][0][s4['chosen'][0]] == np.max(s4['lml'][0][ok])
    np.testing.assert_allclose(four[0].log_marginal_likelihood(), s4['lml'][0][s4['chosen'][0]], rtol=1e-10)


# ---- 5. a bad start ---------------------------------------------------------------------------------------------------------
def test_a_start_that_is_not_positive_definite_is_a_status():
    from hilo_mpc_amd import Kernel
    xd, yd = np.array([[.5, .5, 1., 1., -.3]]), np.array([[1., 2., 3., 2., 1.]])
    tiny = 5e-324                                                  # the smallest positive double
    with pytest.raises(np.linalg.LinAlgError):                     # the oracle's Cholesky fails at this start
        ogp.Posterior({'type': 'constant', 'kwargs': {'bias': 1.}}, {'type': 'zero'}, xd, yd, tiny)

    def healthy():
        return [_se_member(E2, 1., 1.), _member(Kernel.matern_52(), *[a.T for a in ref.kat_data()], E2)]
    good = _array(healthy())
    good.fit_model()
    h = healthy()
    bad = _member(Kernel.constant(bias=1.), xd, yd, .7)
    mixed = _array([h[0], bad, h[1]])
    with pytest.warns(UserWarning, match="Fitting of GP didn't terminate successfully") as rec:
        mixed.fit_model(starts={1: [[tiny, 1.]]})
    assert len(rec) == 1
    st = mixed.fit_stats
    assert int(st['status'][1][0]) == 3 and st['chosen'][1] == -1 and np.isnan(st['lml'][1][0])
    assert bad.hyperparameter_values == [.7, 1.] and not bad._optimization_stats['success']
    np.testing.assert_allclose(bad.predict(np.array([[0.]]))[0], bad.predict(np.array([[5.]]))[0])       # still a factorised object
    a, b = _rows(good), _rows(mixed)
    assert b[0] == a[0] and b[2] == a[1] and a[0][4] == 0 and a[1][4] == 0


# ---- 6. against the existing path at size -----------------------------------------------------------------------------------
def test_against_gaussian_process_fit_model_at_n_200():
    from hilo_mpc_amd import Kernel
    X = ogp.park_miller_randn(.3, (2, 200))
    y = (np.sin(2 * X[0]) + .5 * np.cos(X[1]) + .1 * ogp.park_miller_randn(.15, (200,)))[None]

    def make():
        return _member(Kernel.squared_exponential(active_dims=[0, 1], ard=True, length_scales=[1., 1.]), X, y, .1)
    single = make()
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        single.fit_model()
        arr = _array([make()])
        arr.fit_model()
    print('batched', arr[0].hyperparameter_values, 'single', single.hyperparameter_values, 'iterations', arr.fit_stats['iterations'][0],
          'evaluations', arr.fit_stats['evaluations'][0])
    assert arr.fit_stats['status'][0][0] == 0
    np.testing.assert_allclose(arr[0].hyperparameter_values, single.hyperparameter_values, rtol=2e-5)


# ---- 7. in a model ----------------------------------------------------------------------------------------------------------
def test_substitute_from_an_array_is_substitute_from_its_members():
    from tests.problems import c4_training_data, product_gp, symbolic_model
    X, y = c4_training_data()
    arr = _array([product_gp(X, y)])
    outs = []
    for learned in (arr, [arr[0]]):
        m = symbolic_model('chemostat4_mu')
        m.substitute_from(learned)
        assert m.parameter_names == ['Sf', 'If', 'ISF', 'IRF']
        m = m.discretize('erk', order=4).setup(dt=1.)
        rng = np.random.default_rng(3)
        x0 = np.array([.1, 30., .5, .4]) * (1 + .2 * rng.uniform(-1, 1, (5, 4)))
        xs, ys = m.rollout(x0, u=rng.uniform(0, .3, (5, 2)), p=np.tile([100., 4., 1., 0.], (5, 1)), steps=4)
        outs.append((np.asarray(xs), np.asarray(ys)))
    assert np.all(np.isfinite(outs[0][0])) and not np.array_equal(outs[0][0][0], outs[0][0][-1])
    assert outs[0][0].tobytes() == outs[1][0].tobytes() and outs[0][1].tobytes() == outs[1][1].tobytes()
