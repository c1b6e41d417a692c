"""The inputs and the yardstick of tests/test_gp_paths_gpu.py, pinned without a GPU: the longdouble reference
(tests/gp_reference.py) is checked against its own defining equations, the float64 oracle (`oracle.gp.Posterior`) agrees with it to
the conditioning-scaled float64 level on EVERY case of the GPU matrix (that difference is the unit the device results are measured
in, printed here per case), and the restated dispatch arithmetic sends the matrix through every kernel path it names."""
import numpy as np
import pytest

from tests import gp_reference as R
from tests import test_gp_paths_gpu as P

POINTS = sorted({(c.n, c.kern) for c in P.CASES})


def test_longdouble_is_extended_precision():
    assert R.EPS_LD < 1e-18 and np.finfo(R.LD).eps == R.LD(2) ** -63
    assert abs(float(R.PI) - np.pi) <= np.spacing(np.pi) and R.PI != R.LD(np.pi)
    one_third = R.LD(1) / 3
    assert one_third != R.LD(float(one_third))                    # a longdouble that float64 cannot hold


@pytest.mark.parametrize('kern', list(R.KERNELS))
@pytest.mark.parametrize('n', [1, 17, 200])
def test_reference_satisfies_its_own_equations(n, kern):
    """L is lower triangular with L L^T = K_y, K_y alpha = y - m, and V = L^-1 K* solves L V = K*, all at the longdouble level."""
    ref = R.reference(n, kern)
    L, Ky = ref.L, ref.Ky
    tiny = 64 * n * R.EPS_LD
    assert np.all(np.triu(L, 1) == 0) and np.all(np.diag(L) > 0)
    assert np.max(np.abs(L @ L.T - Ky)) <= tiny * float(np.max(np.abs(Ky)))
    cond = np.linalg.cond(Ky.astype(np.float64))
    assert np.max(np.abs(Ky @ ref.alpha - ref.ym)) <= tiny * cond * float(np.max(np.abs(ref.ym)))
    Xq = R.queries(33)
    V = ref.l_inv_kstar(Xq)
    from oracle import gp as ogp
    Ks = ogp.kernel(ref.kernel_spec, ref.X, Xq)
    assert np.max(np.abs(L @ V - Ks.astype(R.LD))) <= tiny * float(np.max(np.abs(L)))
    mean, var = ref.predict(Xq, noise_free=True)
    _, var_noisy = ref.predict(Xq)
    np.testing.assert_array_equal(var_noisy, var + R.LD(ref.sn2))
    assert np.all(var > 0) and np.all(var <= R.SIGNAL_VARIANCE[kern])
    if n > 1:
        assert np.max(np.abs(ref.L_inv @ L - np.eye(n))) <= tiny * cond


def test_reference_lml_of_a_hand_made_problem():
    """n = 1, zero mean, k = 1, sn2 = 1/4: LML = -1/2 y^2 / 1.25 - 1/2 log 1.25 - 1/2 log 2 pi; variance at the point itself."""
    ref = R.Reference({'type': 'constant'}, {'type': 'zero'}, np.array([[2.]]), np.array([[3.]]), .25)
    assert float(ref.alpha[0]) == 3. / 1.25
    want = -.5 * 9. / 1.25 - .5 * np.log(1.25) - .5 * np.log(2 * np.pi)
    assert abs(float(ref.lml) - want) < 4e-16 * abs(want)
    mean, var = ref.predict(np.array([[7.]]), noise_free=True)
    assert abs(float(mean[0]) - 2.4) < 1e-15 and abs(float(var[0]) - .2) < 1e-16


def test_reference_reports_the_first_bad_pivot():
    with pytest.raises(R.NotPositiveDefinite, match=r"pivot 2") as info:
        R.cholesky(np.ones((40, 40)))
    assert info.value.pivot == 2


@pytest.mark.parametrize('n,kern', POINTS, ids=[f"n{n}-{k}" for n, k in POINTS])
def test_oracle_agrees_with_reference(n, kern):
    """|o - r| <= 8 cond(K_y) eps64 scale for the LML, the mean and both variances at every query count the GPU cases of this
    (n, kernel) use: backward-stable float64 solves lose cond * eps and no more.  The figures printed are the units of the GPU
    module's tolerance."""
    ref, orc = R.reference(n, kern), R.oracle(n, kern)
    cond = float(np.linalg.cond(ref.Ky.astype(np.float64)))
    level = 8 * max(cond, 1.) * R.EPS64
    e_lml = R.error(orc.lml, ref.lml)
    print(f"n={n} {kern}: cond {cond:.2e}; oracle error: lml {e_lml:.2e} (|lml| {abs(float(ref.lml)):.3g})", end='')
    assert e_lml <= level * abs(float(ref.lml))
    counts = sorted({m for c in P.CASES if (c.n, c.kern) == (n, kern) for m in P.QUERY_COUNTS[P._family(c.predict)]})
    assert counts
    for m in counts:
        p = R.predictions(n, kern, m)
        (rm, rv), (om, ov) = p['ref'], p['orc']
        e_mean, e_var = R.error(om, rm), R.error(ov, rv)
        print(f"; m={m}: mean {e_mean:.2e} var {e_var:.2e}", end='')
        assert rm.dtype == rv.dtype == R.LD and rm.shape == rv.shape == (m,)
        assert e_mean <= level * max(float(np.max(np.abs(rm))), float(np.max(np.abs(ref.ym))))
        assert e_var <= level * R.SIGNAL_VARIANCE[kern]
    print()


def test_problem_is_well_conditioned():
    """Unit signal variance over noise variance 1e-2: cond(K_y) stays in the thousands up to the largest size, so the GPU
    module's tolerances are tight ones."""
    for kern in R.KERNELS:
        cond = np.linalg.cond(R.reference(600, kern).Ky.astype(np.float64))
        print(f"n=600 {kern}: cond(K + sn2 I) = {cond:.3g}")
        assert cond < 2e4


@pytest.mark.parametrize('kern', list(P.GRADIENT_KERNELS))
def test_reference_trace_formula_is_the_derivative_of_the_reference_lml(kern):
    """1/2 tr((alpha alpha^T - K_y^-1) dK_y) with central-difference dK_y against central differences of the longdouble LML
    itself (both O(h^2) approximations of the same derivative), and the float64 oracle's trace formula against it."""
    from oracle import gp as ogp
    spec_of, values = P.GRADIENT_KERNELS[kern]
    n, h = 20, 1e-5
    X, y = R.training_data(n)
    th = np.log([R.NOISE_VARIANCE] + values)
    ref = R.Reference(spec_of(values), {'type': 'zero'}, X, y, R.NOISE_VARIANCE)
    dKy, fd = [], []
    for i in range(th.size):
        K, lml = [], []
        for sgn in (1., -1.):
            e = np.zeros_like(th)
            e[i] = sgn * h
            v = np.exp(th + e)
            K.append(ogp.kernel(spec_of(v[1:]), X, X) + float(v[0]) * np.eye(n))
            lml.append(R.Reference(spec_of(v[1:]), {'type': 'zero'}, X, y, float(v[0])).lml)
        dKy.append((K[0].astype(R.LD) - K[1].astype(R.LD)) / (2 * R.LD(h)))
        fd.append((lml[0] - lml[1]) / (2 * R.LD(h)))
    g = ref.lml_gradient(dKy)
    assert g.dtype == R.LD and np.max(np.abs(g)) > 1.
    np.testing.assert_allclose(g.astype(float), np.array(fd, dtype=float), rtol=1e-7)
    o = R.oracle_lml_gradient(ogp.Posterior(spec_of(values), {'type': 'zero'}, X, y, R.NOISE_VARIANCE),
                              [d.astype(np.float64) for d in dKy])
    np.testing.assert_allclose(o, g.astype(float), rtol=1e-10)


def test_case_matrix_reaches_every_path():
    """The restated dispatch: its boundaries for the inputs of the matrix (nf = 3), for the two-feature example the host code
    was sized with, and the set of paths the cases take."""
    for kern in R.KERNELS:
        klen = P.program_length(kern)
        assert klen == {'se_ard02': 10, 'm52+se': 30}[kern]
        path = [None] + [P.predict_path(n, klen) for n in range(1, 701)]
        assert all(path[n] == f'reg{(n + 15) // 16}' for n in range(1, 257))
        assert set(path[257:353]) == {'mfma2'} and set(path[353:529]) == {'mfma1'} and set(path[529:]) == {'generic16'}
        forced = [None] + [P.predict_path(n, klen, (P.LDS,)) for n in range(1, 701)]
        assert set(forced[1:209]) == {'mfma4'} and forced[209] == 'mfma2' and forced[353:] == path[353:]
        valu = [None] + [P.predict_path(n, klen, (P.VALU,)) for n in range(1, 701)]
        assert set(valu[1:505]) == {'generic32'} and set(valu[505:]) == {'generic16'}
    two = [None] + [P.predict_path(n, 10, nf=2) for n in range(1, 701)]
    assert two[256] == 'reg16' and two[257] == 'mfma2' and two[352] == 'mfma2' and two[353] == 'mfma1'
    assert two[544] == 'mfma1' and two[545] == 'generic16'
    fac = [None] + [P.factor_path(n) for n in range(1, 701)]
    assert set(fac[1:241]) == {'blocked'} and set(fac[241:561]) == {'blocked_optin'} and set(fac[561:]) == {'unblocked'}
    assert P.factor_path(17, (P.UNBLOCKED,)) == 'unblocked'
    for kern in R.KERNELS:
        mine = [c for c in P.CASES if c.kern == kern]
        assert {c.predict for c in mine} == {f'reg{nt}' for nt in range(1, 17)} | {'mfma1', 'mfma2', 'mfma4', 'generic16', 'generic32'}
        assert {c.factor for c in mine} == {'blocked', 'blocked_optin', 'unblocked'}
        natural = {c.n for c in mine if not c.env}
        assert {16 * nt - 3 for nt in range(1, 17)} | {1, 15, 16, 17, 32, 33, 240, 241, 256} <= natural
        assert {257, 272, 352, 353, 400, 528, 529, 560, 561, 600} <= natural
        assert {(c.n, c.env) for c in mine if c.env} == {(37, (P.LDS,)), (200, (P.LDS,)), (208, (P.LDS,)), (37, (P.VALU,)),
                                                         (200, (P.VALU,)), (500, (P.VALU,)), (17, (P.UNBLOCKED,)),
                                                         (200, (P.UNBLOCKED,))}
    assert len({P.case_id(c) for c in P.CASES}) == len(P.CASES)
    assert max(c.n for c in P.CASES) == 600 and max(max(v) for v in P.QUERY_COUNTS.values()) == 130


def test_inputs_are_deterministic_and_read_only():
    X, y = R.training_data(37)
    assert X.shape == (3, 37) and y.shape == (1, 37) and X.min() >= 0. and X.max() <= 10.
    assert R.training_data(37)[0] is X
    with pytest.raises(ValueError):
        X[0, 0] = 1.
    # y depends on features 0 and 2 only: the same draws with another middle feature give the same labels
    rng = np.random.default_rng(20261019 + 37)
    X2 = rng.uniform(0., 10., (3, 37))
    np.testing.assert_array_equal(X2, X)
    assert R.queries(65).shape == (3, 65)
