"""GPU: `ANN.predict` (csrc/hilo_ann.hip, chained f64 matrix-core products) against the numpy oracle of tests/ann_reference.py,
and neural terms inside models (`Model.substitute_from(ann)`) through step / rollout / linearization / EKF / NMPC.

Tolerance of the predict tests (ann_reference.tolerance): 32 x the largest difference between the oracle in float64 and in
extended precision on the test's own data, floor 4 ulp of max|y|; the margin covers the device's summation order (k-blocks of 4,
bias first, fused multiply-adds) and its 1-2 ulp exp / log.  The resulting bounds for the networks and data below (m = 1 ... 1000;
max|y| between 0.75 and 10): no-hidden 2.2e-16 ... 2.6e-15, reference 2-10-3 1.4e-14 ... 2.3e-14, 5-16-5 tanh 2.4e-15 ... 2.2e-14,
8-17-16 relu 2.1e-14 ... 7.8e-14, 2-40-1 softplus 1.8e-15 ... 2.5e-14, 5-10-17-40-3 1.7e-14 ... 5.3e-14, 8-16-16-16-5
9.7e-15 ... 3.1e-14, 20-10-2 1.1e-14 ... 2.4e-14, 32-64-64-16 1.9e-14 ... 1.6e-13,
8-64-64-64-4 softplus 1.1e-14 ... 5.1e-14, 8-64x4-2 1.9e-14 ... 5.3e-14; each test prints its error next to its bound."""
import numpy as np
import pytest
import torch

from tests import ann_reference as ar

pytestmark = pytest.mark.gpu

MS = (1, 15, 16, 17, 1000)
# (nf, hidden widths, activations, nl, scaling)
NETS = {
    'no-hidden': (1, [], [], 1, False),
    'reference-2-10-3': (2, [10], ['sigmoid'], 3, True),
    '5-16-5-tanh': (5, [16], ['tanh'], 5, False),
    '8-17-16-relu': (8, [17], ['relu'], 16, True),
    '2-40-1-softplus': (2, [40], ['softplus'], 1, False),
    '5-10-17-40-3': (5, [10, 17, 40], ['tanh', 'sigmoid', 'softplus'], 3, True),
    '8-16-16-16-5': (8, [16, 16, 16], ['linear', 'relu', 'tanh'], 5, False),
    '20-10-2-wide-input': (20, [10], ['sigmoid'], 2, True),
    '32-64-64-16-limits': (32, [64, 64], ['tanh', 'softplus'], 16, True),
    # staged blocks above 64 KiB (82.5 and 115 KiB of the 128 KiB the kernel may request): the launch that first raises the kernel's
    # dynamic LDS limit
    '8-64-64-64-4-softplus': (8, [64, 64, 64], ['softplus'] * 3, 4, False),
    '8-64x4-2-largest-lds': (8, [64] * 4, ['tanh', 'sigmoid', 'relu', 'softplus'], 2, True),
}


def _net(key, seed=0):
    nf, widths, acts, nl, scaled = NETS[key]
    W, b = ar.random_net(nf, widths, nl, seed=seed)
    rng = np.random.default_rng(seed + 100)
    xs = (rng.normal(size=nf), rng.uniform(.5, 2., nf)) if scaled else None
    ys = (rng.normal(size=nl), rng.uniform(.5, 2., nl)) if scaled else None
    ann = ar.make_ann([f'f{i}' for i in range(nf)], [f'l{i}' for i in range(nl)], widths, acts, W, b, xs, ys).setup()
    return ann, (W, b, acts, xs, ys)


@pytest.mark.parametrize('key', list(NETS))
def test_predict_against_the_oracle(key):
    ann, net = _net(key)
    rng = np.random.default_rng(7)
    for m in MS:
        X = rng.normal(size=(ann.n_features, m)) * 1.5
        ref, atol = ar.tolerance(X, *net)
        got = ann.predict(X)
        assert got.shape == (ann.n_labels, m) and isinstance(got, np.ndarray)
        err = np.max(np.abs(got - ref))
        print(f"{key} m={m}: max error {err:.3e}, bound {atol:.3e}")
        assert err <= atol, (key, m, err, atol)


def test_integer_network_is_exact():
    """Small integers through linear layers: every product and sum is exact, so any slip in the fragment maps (weights
    A[n][k], activations B[k][q], accumulator row = 4 reg + lane / 16) shows as a wrong integer."""
    rng = np.random.default_rng(3)
    nf, widths, nl = 7, [40, 33], 16
    dims = [nf] + widths + [nl]
    W = [rng.integers(-3, 4, size=(dims[k + 1], dims[k])).astype(float) for k in range(3)]
    b = [rng.integers(-5, 6, size=dims[k + 1]).astype(float) for k in range(3)]
    ann = ar.make_ann([f'f{i}' for i in range(nf)], [f'l{i}' for i in range(nl)], widths, ['linear', 'linear'], W, b).setup()
    X = rng.integers(-4, 5, size=(nf, 53)).astype(float)
    assert np.array_equal(ann.predict(X), ar.forward(X, W, b, ['linear', 'linear']))


def test_device_tensors_and_views():
    ann, net = _net('5-10-17-40-3')
    dev = ann._dev
    rng = np.random.default_rng(2)
    m = 37
    X = rng.normal(size=(5, m))
    ref, atol = ar.tolerance(X, *net)
    Xd = torch.as_tensor(X, device=dev)
    y = ann.predict(Xd)
    assert isinstance(y, torch.Tensor) and y.device == dev and y.shape == (3, m)
    assert np.max(np.abs(y.cpu().numpy() - ref)) <= atol
    big = torch.full((5, 101), float('nan'), dtype=torch.float64, device=dev)
    big[:, 11:11 + m] = Xd
    out = torch.full((3, 64), -7., dtype=torch.float64, device=dev)
    r = ann.predict(big[:, 11:11 + m], out=out[:, 20:20 + m])           # ldx = 101, ldy = 64, unaligned starts
    assert r.data_ptr() == out[:, 20:20 + m].data_ptr()
    assert torch.equal(out[:, 20:20 + m], y)                              # bit-identical to the contiguous call
    assert torch.all(out[:, :20] == -7.) and torch.all(out[:, 20 + m:] == -7.)


def test_containment_and_reproducibility():
    for key in ('reference-2-10-3', '5-10-17-40-3', '8-17-16-relu'):
        ann, _ = _net(key)
        rng = np.random.default_rng(5)
        X = rng.normal(size=(ann.n_features, 50))
        clean = ann.predict(X)
        for bad in (np.nan, np.inf):
            Xb = X.copy()
            Xb[:, 21] = bad
            got = ann.predict(Xb)
            keep = np.arange(50) != 21
            assert np.array_equal(got[:, keep], clean[:, keep]), (key, bad)      # bit-identical neighbours
        # a query's bits depend neither on m nor on its position in the batch
        for i in (0, 15, 16, 33, 49):
            assert np.array_equal(ann.predict(X[:, i:i + 1]), clean[:, i:i + 1]), (key, i)
        assert np.array_equal(ann.predict(X[:, 16:35]), clean[:, 16:35])


@pytest.mark.parametrize('act', ['sigmoid', 'tanh', 'relu', 'softplus'])
def test_large_pre_activations_stay_finite(act):
    ann = ar.make_ann(['a'], ['y'], [3], [act], [np.array([[1.], [-1.], [.5]]), np.array([[1., 1., 1.]])],
                      [np.zeros(3), np.zeros(1)]).setup()
    X = np.array([[800., -800., 0., 1600.]])
    got = ann.predict(X)
    ref = ar.forward(X, ann._weights, ann._bias, [act])
    assert np.all(np.isfinite(got))
    np.testing.assert_allclose(got, ref, rtol=1e-14, atol=1e-15)


def test_limits_are_refused_with_their_message():
    from hilo_mpc_amd import _lib

    def build(nf, widths, nl):
        W, b = ar.random_net(nf, widths, nl)
        return ar.make_ann([f'f{i}' for i in range(nf)], [f'l{i}' for i in range(nl)], widths, ['tanh'] * len(widths), W, b)
    for args, msg in (((2, [65], 1), "hidden layer 0 has 65 neurons, at most 64"), ((33, [8], 1), "33 features, at most 32"),
                      ((2, [8], 17), "17 labels, at most 16"), ((2, [4] * 9, 1), "9 hidden layers, at most 8"),
                      ((2, [64] * 8, 1), "bytes of staged weights")):
        ann = build(*args)
        with pytest.raises(_lib.HiloError, match=msg) as ei:
            ann.setup()
        assert ei.value.code == -4 and not ann.is_setup()


# ---- the hybrid model on the device ---------------------------------------------------------------------------------------------------
def _hybrid(widths=(10,), acts=('sigmoid',), dt=.5):
    W, b, acts, xs, ys = ar.bio_net(widths, acts)
    ann = ar.make_ann(ar.FEATURES, ar.LABELS, widths, acts, W, b, xs, ys)
    m = ar.bioreactor()
    m.substitute_from(ann)
    twin = ar.bioreactor(rates=ar.hand_rates(W, b, acts, xs, ys))
    return m, twin, (W, b, acts, xs, ys)


def _batch(B, seed=1):
    rng = np.random.default_rng(seed)
    x = ar.X0 + rng.uniform(0., 1., (B, 4)) * [.5, 10., 1., 2.]
    u = rng.uniform(0., .3, (B, 2))
    return x, u


def _rk4(x, u, net, dt):
    f = lambda xx: ar.bio_rhs(xx, u, *net)
    k1 = f(x)
    k2 = f(x + .5 * dt * k1)
    k3 = f(x + .5 * dt * k2)
    k4 = f(x + dt * k3)
    return x + dt / 6. * (k1 + 2. * k2 + 2. * k3 + k4)


@pytest.mark.parametrize('widths,acts', [((10,), ('sigmoid',)), ((8, 8), ('tanh', 'tanh'))])
def test_step_and_rollout_against_numpy_rk4(widths, acts):
    dt = .5
    m, _, net = _hybrid(widths, acts)
    m = m.discretize('rk4').setup(dt=dt)
    x, u = _batch(33)
    xn, y = m.step(x, u, ar.P_REST)
    ref = _rk4(x, u, net, dt)
    np.testing.assert_allclose(xn, ref, rtol=1e-11, atol=1e-13)
    np.testing.assert_allclose(y, ref[:, :3], rtol=1e-11, atol=1e-13)
    X, Y = m.rollout(x, u, ar.P_REST, steps=4)
    xr = x
    for k in range(4):
        xr = _rk4(xr, u, net, dt)
        np.testing.assert_allclose(X[k + 1], xr, rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(Y[k], xr[:, :3], rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize('widths,acts', [((10,), ('sigmoid',)), ((8, 8), ('tanh', 'tanh'))])
def test_linearization_against_torch_autograd(widths, acts):
    dt = .5
    m, _, (W, b, acts, xs, ys) = _hybrid(widths, acts)
    m = m.discretize('rk4').setup(dt=dt)
    x, u = _batch(5, seed=4)
    A, Bm, Cm = m.linearization(x, u, ar.P_REST)
    seq = ar.torch_sequential(W, b, acts)
    p = torch.as_tensor(ar.P_REST)

    def rhs(xx, uu):
        r = seq((torch.stack([xx[1], xx[3]]) - torch.as_tensor(xs[0])) / torch.as_tensor(xs[1])) * torch.as_tensor(ys[1]) + \
            torch.as_tensor(ys[0])
        D = uu[0] + uu[1]
        return torch.stack([r[0] * xx[0] - D * xx[0], -r[1] * xx[0] - D * xx[1] + uu[0] * p[0], r[2] * xx[0] - D * xx[2],
                            -D * xx[3] + uu[1] * p[1]])

    def phi(w):
        xx, uu = w[:4], w[4:]
        k1 = rhs(xx, uu)
        k2 = rhs(xx + .5 * dt * k1, uu)
        k3 = rhs(xx + .5 * dt * k2, uu)
        k4 = rhs(xx + dt * k3, uu)
        return xx + dt / 6. * (k1 + 2. * k2 + 2. * k3 + k4)
    for i in range(5):
        J = torch.autograd.functional.jacobian(phi, torch.as_tensor(np.concatenate([x[i], u[i]]))).numpy()
        np.testing.assert_allclose(A[i], J[:, :4], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(Bm[i], J[:, 4:], rtol=1e-10, atol=1e-12)
        np.testing.assert_allclose(Cm[i], np.eye(4)[:3], rtol=0, atol=0)


def test_ekf_step_against_the_hand_written_twin():
    from hilo_mpc_amd import EKF
    m, twin, _ = _hybrid()
    x, u = _batch(16, seed=6)
    rng = np.random.default_rng(9)
    y = x[:, :3] * (1. + .01 * rng.normal(size=(16, 3)))
    P0 = np.tile(np.eye(4) * .1, (16, 1, 1))
    res = []
    for mod in (m, twin):
        f = EKF(mod.discretize('rk4').setup(dt=.5))
        f.setup()
        f.Q, f.R = 1e-4, 1e-2
        f.set_initial_guess(x, P0=P0)
        f.estimate(y=y, u=u, p=np.tile(ar.P_REST, (16, 1)))
        res.append((f.x.cpu().numpy(), f.P.cpu().numpy()))
    np.testing.assert_allclose(res[0][0], res[1][0], rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(res[0][1], res[1][1], rtol=1e-9, atol=1e-13)


def _nmpc_pair(ma, mb, B=8):
    """NMPC (N = 5) on two models that are the same function: same statuses, and the solution within the tolerance tests/test_jit_gpu.py
    uses for a compiled problem against its reference (u0: rtol 5e-5 / atol 1e-6, objective: rtol 1e-8) - its bit-for-bit comparison
    is between two emissions of the SAME operation sequence, which a network written by hand in textbook forms is not."""
    from tests.problems import C2, product_nmpc
    spec = dict(C2, N=5, p=list(ar.P_REST))
    rng = np.random.default_rng(12)
    x0 = np.array([.1, 40., 0., 0.]) * (1 + .1 * rng.uniform(-1, 1, (B, 4)))
    sol = []
    for mod in (ma, mb):
        nmpc = product_nmpc(spec, model=mod)
        u0 = nmpc.optimize(x0, cp=spec['p'])
        sol.append((u0, nmpc._nlp_solution['f'].cpu().numpy(), np.array(nmpc.solver_status_code)))
    assert np.array_equal(sol[0][2], sol[1][2])
    assert np.all(np.isin(sol[0][2], (1, 2)))
    np.testing.assert_allclose(sol[0][0], sol[1][0], rtol=5e-5, atol=1e-6)
    np.testing.assert_allclose(sol[0][1], sol[1][1], rtol=1e-8)


@pytest.mark.parametrize('widths,acts', [((10,), ('sigmoid',)), ((8, 8), ('tanh', 'tanh'))])
def test_nmpc_on_the_hybrid_model_against_the_twin(widths, acts):
    m, twin, _ = _hybrid(widths, acts)
    _nmpc_pair(m, twin)


def test_linear_network_equals_the_affine_term():
    """A network of `linear` layers only is an affine map: the NMPC solution equals that of the model with the map written out."""
    W, b = ar.random_net(2, [4], 3, seed=21, scale=.05)
    b = [0.1 * b[0], np.array([.3, .5, .1])]
    ann = ar.make_ann(ar.FEATURES, ar.LABELS, [4], ['linear'], W, b, (np.array([20., 2.]), np.array([15., 2.])))
    m = ar.bioreactor()
    m.substitute_from(ann)
    Wa = W[1] @ W[0] / np.array([15., 2.])
    ba = W[1] @ (b[0] - W[0] @ (np.array([20., 2.]) / np.array([15., 2.]))) + b[1]

    def rates(S, I):
        return [float(Wa[i, 0]) * S + float(Wa[i, 1]) * I + float(ba[i]) for i in range(3)]
    _nmpc_pair(m, ar.bioreactor(rates=rates))
