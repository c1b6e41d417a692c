"""GPU: `DataGenerator` / `Model.generate_data` (hilo_datagen_run, csrc/hilo_datagen.h) against the numpy restatement of
tests/datagen_reference.py - the comparisons and their tolerances are `datagen_reference.check`, shared with the host build of
tests/test_datagen_host.py - and against `Model.rollout` fed with the inputs the run returned."""
import ctypes
import warnings

import numpy as np
import pytest
import torch

from hilo_mpc_amd import DataGenerator, GaussianProcess, Model, _lib
from tests import datagen_reference as dr

pytestmark = pytest.mark.gpu

TPB = 64                                   # ROLLOUT_TPB: one wave per workgroup
T = dr.T
OPTS = {'reltol': 1e-8, 'abstol': 1e-10}
# (signal, noise) pairs a parametrised test walks through: every signal kind and every noise kind
PAIRS = [('random_uniform', 'uniform'), ('random_normal', 'normal'), ('chirp', 'per_state'), ('random_uniform', 'none')]
_MODELS = {}


def _model(name, solver=None):
    key = (name, solver)
    if key not in _MODELS:
        dt = dr.case(name, 1)['dt']
        _MODELS[key] = Model(name).setup(dt=dt) if solver is None else Model(name).setup(dt=dt, solver=solver, solver_options=OPTS)
    return _MODELS[key]


def _signal(gen, case, signal, seed):
    if signal == 'chirp':
        col = lambda key, default=None: [[s.get(key, default) for s in segs] for segs in case['chirps']]
        gen.chirp(col('type'), col('amplitude'), col('length'), col('mean'), col('chirp_rate'), initial_phase=col('initial_phase'),
                  initial_frequency=col('initial_frequency'), initial_frequency_ratio=col('initial_frequency_ratio'))
        gen.seed = seed                     # (a chirp draws nothing; the noise takes the generator's seed)
    else:
        a, b = case[signal.split('_')[-1]]
        getattr(gen, signal)(T // dr.HOLD, dr.HOLD, a, b, seed=seed)


def _add_noise(m, noise):
    spec = dr.NOISES[noise]
    if not spec:
        return None
    if 'all' in spec:
        return dict(spec['all'])
    return {m.dynamical_state_names[-1]: dict(spec['last'])}


def _run(m, case, signal, noise, shift, output, skip, offset=0, seed=dr.SEED, rows=slice(None), tensors=False, t0=0.):
    x0, p = case['x0'][rows], case['p'][rows]
    if tensors:
        x0, p = torch.as_tensor(x0, device='cuda'), torch.as_tensor(p, device='cuda')
    gen = DataGenerator(m, x0=x0, p0=p, instance_offset=offset)
    _signal(gen, case, signal, seed)
    with warnings.catch_warnings():
        warnings.simplefilter('error', UserWarning)   # every distribution parameter is given: no default is assumed, no instance fails
        ds = gen.run(output, skip=skip or None, shift=shift, add_noise=_add_noise(m, noise), t0=t0)
    return gen, ds


def _got(ds):
    return dict(F=ds._F, L=ds._L, X=ds.x, U=ds.u)


@pytest.mark.parametrize('solver', [None, 'dopri5'])
@pytest.mark.parametrize('name', ['chemostat4', 'linear2'])
def test_against_the_restatement_and_the_rollout(name, solver):
    """B = 1 and 65 (one lane; one past a wave, ROLLOUT_TPB + 1), T = 6, shift 0 and 2, both outputs, states skipped in every other
    run, each signal and noise kind; once shift = T - 1 (a single row).  Under the map the states are compared with the restatement's
    classic Runge-Kutta steps; under 'dopri5' - as under the map - `Model.rollout(x0, u=ds.u, p)` must equal ds.x bit for bit (the
    roll-out's own accuracy is the subject of tests/test_rollout_gpu.py)."""
    m = _model(name, solver)
    run = 0
    for B in (1, TPB + 1):
        case = dr.case(name, B)
        for shift, output in ((0, 'absolute'), (0, 'difference'), (2, 'absolute'), (2, 'difference'), (T - 1, 'absolute')):
            signal, noise = PAIRS[run % len(PAIRS)]
            skip = case['skip'] if run % 2 else []
            run += 1
            if shift == T - 1 and B == 1:
                continue
            _, ds = _run(m, case, signal, noise, shift, output, skip, offset=3)
            keep = [k for k in range(case['nx']) if k not in skip]
            got = _got(ds)
            tag = f"{name} {solver} B={B} {signal} noise={noise} shift={shift} {output} skip={skip}"
            X_ref = dr.plant_reference(name, case, got['U']) if solver is None else None
            dr.check(tag, case, signal, noise, shift, output, keep, got, X_ref, 3)
            xs, _ = m.rollout(case['x0'], u=ds.u, p=case['p'], steps=T)
            np.testing.assert_array_equal(xs, ds.x, err_msg=tag)
            assert not ds.status.any() and ds.finite_rows().tolist() == list(range(len(ds)))
            # the reference's orientation and names
            f, l = ds.raw_data
            N = T - shift
            assert f.shape == (len(ds.features), N * B) and l.shape == (len(ds.labels), N * B) and len(ds) == N * B
            np.testing.assert_array_equal(f[:, (N - 1) * B + B // 2], got['F'][N - 1, B // 2])
            assert (ds.features, ds.labels) == dr.names(m.dynamical_state_names, m.input_names, keep, output, shift)
            np.testing.assert_allclose(ds.time, (np.arange(N) + shift + 1) * m.dt, rtol=1e-15)
            if shift == T - 1:
                assert N == 1 and f.shape[0] == T * len(keep) + case['nu']


def test_batch_independence_and_seeds():
    """Instance b of a batch of 5 with instance_offset = 60 is instance 60 + b of a batch of 65, bit for bit, noise included; the same
    seed repeats; another seed gives other inputs and other noise."""
    m = _model('chemostat4', 'dopri5')
    case = dr.case('chemostat4', 65)
    for signal, noise in PAIRS[:3]:
        _, big = _run(m, case, signal, noise, 1, 'difference', [1])
        _, small = _run(m, case, signal, noise, 1, 'difference', [1], offset=60, rows=slice(60, 65))
        for a, b in ((small._F, big._F[:, 60:]), (small._L, big._L[:, 60:]), (small.x, big.x[:, 60:]), (small.u, big.u[:, 60:])):
            np.testing.assert_array_equal(a, b)
        _, again = _run(m, case, signal, noise, 1, 'difference', [1])
        np.testing.assert_array_equal(again._F, big._F)
        np.testing.assert_array_equal(again._L, big._L)
        if signal != 'chirp':
            _, other = _run(m, case, signal, noise, 1, 'difference', [1], seed=dr.SEED + 1)
            assert not np.any(other.u[::2] == big.u[::2])
            assert not np.any(other._L == big._L)
    # neighbours in the batch and in time draw other numbers
    _, ds = _run(m, case, 'random_uniform', 'uniform', 0, 'absolute', [])
    assert not np.any(ds.u[:, 1:] == ds.u[:, :-1]) and not np.any(ds.u[2:] == ds.u[:-2])
    n = ds._F[:, :, :4] - ds.x[:-1]
    assert not np.any(n[:, 1:] == n[:, :-1]) and not np.any(n[1:] == n[:-1]) and not np.any(n[:, :, 1:] == n[:, :, :-1])


def _linear2_expressions(forced=False):
    m = Model(name='linear2_forced' if forced else 'linear2_expr')
    m.set_parameters(['k_1', 'k_2'] + (['w'] if forced else []))
    m.set_equations("dx_1/dt = -k_1*x_1(t) + u(k)" + (" + sin(w*t)" if forced else "") + "\ndx_2/dt = k_1*x_1(t) - k_2*x_2(t)\n"
                    "y(k) = x_2(t)")
    return m


def test_run_time_compiled_twin():
    """linear2 written as expressions (hilo_user_datagen) against the zoo functor at rtol 1e-12 (tests/test_pid_gpu.py: one map
    compiled into two kernels, times 10), under the map and under 'dopri5'; with + sin(w t) on the first state and t0 = 1.7 against the
    restatement (classic Runge-Kutta steps that see the time)."""
    B = TPB + 1
    case = dr.case('linear2', B)
    for solver in (None, 'dopri5'):
        kw = {} if solver is None else dict(solver=solver, solver_options=OPTS)
        e = _linear2_expressions().setup(dt=case['dt'], **kw)
        _, z = _run(_model('linear2', solver), case, 'random_normal', 'normal', 1, 'difference', [])
        _, r = _run(e, case, 'random_normal', 'normal', 1, 'difference', [])
        for a, b in ((r.u, z.u), (r.x, z.x), (r._F, z._F)):
            np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-14)
        np.testing.assert_allclose(r._L, z._L, rtol=0., atol=1e-12 * np.abs(z.x).max())     # differences: absolute in the states' size
    f = _linear2_expressions(forced=True).setup(dt=case['dt'])
    assert f.is_time_variant()
    forced = dict(case, p=np.hstack([case['p'], np.linspace(.5, 3., B)[:, None]]))
    t0 = 1.7
    _, t = _run(f, forced, 'random_uniform', 'uniform', 2, 'absolute', [0], t0=t0)

    def rhs(t_, x, u, p):
        return np.stack([-p[:, 0] * x[:, 0] + u[:, 0] + np.sin(p[:, 2] * t_), p[:, 0] * x[:, 0] - p[:, 1] * x[:, 1]], axis=1)
    x, X, hs = forced['x0'].copy(), [forced['x0'].copy()], case['dt'] / 8
    for k in range(T):
        for i in range(8):
            ts = t0 + k * case['dt'] + i * hs
            k1 = rhs(ts, x, t.u[k], forced['p'])
            k2 = rhs(ts + .5 * hs, x + .5 * hs * k1, t.u[k], forced['p'])
            k3 = rhs(ts + .5 * hs, x + .5 * hs * k2, t.u[k], forced['p'])
            k4 = rhs(ts + hs, x + hs * k3, t.u[k], forced['p'])
            x = x + hs / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
        X.append(x.copy())
    dr.check('time-variant twin', forced, 'random_uniform', 'uniform', 2, 'absolute', [1], _got(t), np.array(X), 0)
    np.testing.assert_allclose(t.time, t0 + (np.arange(T - 2) + 3) * case['dt'], rtol=1e-15)
    _, r = _run(_model('linear2'), case, 'random_uniform', 'uniform', 2, 'absolute', [0])
    assert np.max(np.abs(t.x - r.x)) > 1e-2          # the forcing is felt


def _square_plus_u():
    m = Model(name='square_u')
    x = m.set_dynamical_states(['x'])
    u = m.set_inputs(['u'])
    m.set_dynamical_equations([x[0] * x[0] + u[0]])
    m.set_measurement_equations([x[0]])
    return m.setup(dt=.25, solver='dopri5', solver_options=dict(OPTS, max_num_steps=40))


def test_a_failing_instance_is_contained():
    """dx/dt = x^2 + u, u in [0, .1]: from .2 the pole lies beyond the run's 1.5 time units, from 2 it is reached by the end of the
    second interval at the latest - 40 steps do not get there.  The middle instance of three ends with status 1 and NaN from the first
    row that needs the state it did not reach; its neighbours equal their runs alone; finite_rows() leaves out exactly its rows; the
    warning is raised."""
    m = _square_plus_u()
    x0 = np.array([[.2], [2.], [.25]])
    shift = 1

    def run(rows, offset):
        gen = DataGenerator(m, x0=x0[rows], instance_offset=offset)
        gen.random_uniform(3, 2, 0., .1, seed=4)
        return gen.run('absolute', shift=shift, add_noise={'distribution': 'random_uniform', 'lb': -.01, 'ub': .01})
    with pytest.warns(UserWarning, match='1 of 3 instances did not reach the end'):
        ds = run(slice(None), 0)
    assert ds.status.tolist() == [0, 1, 0]
    miss = np.flatnonzero(np.isnan(ds.x[:, 1, 0]))
    print("first state not reached:", miss[:1], "integrator statistics:", {k: v.tolist() for k, v in ds.stats.items()})
    assert len(miss) and miss[0] >= 1 and np.isnan(ds.x[miss[0]:, 1]).all() and np.isfinite(ds.x[:miss[0], 1]).all()
    first = max(0, miss[0] - shift - 1)               # row r holds the states r .. r + shift and, as its label, r + shift + 1
    N, B = T - shift, 3
    bad_row = np.isnan(ds._F[:, 1]).any(axis=1) | np.isnan(ds._L[:, 1]).any(axis=1)
    assert bad_row.tolist() == [r >= first for r in range(N)]
    assert np.isnan(ds._L[first:, 1]).all() and np.isfinite(ds.u).all()
    assert np.isfinite(ds._F[:, [0, 2]]).all() and np.isfinite(ds._L[:, [0, 2]]).all() and np.isfinite(ds.x[:, [0, 2]]).all()
    assert ds.finite_rows().tolist() == [c for c in range(N * B) if not (c % B == 1 and c // B >= first)]
    for b in (0, 2):
        with warnings.catch_warnings():
            warnings.simplefilter('error')
            alone = run(slice(b, b + 1), b)
        np.testing.assert_array_equal(alone._F[:, 0], ds._F[:, b])
        np.testing.assert_array_equal(alone._L[:, 0], ds._L[:, b])
        np.testing.assert_array_equal(alone.x[:, 0], ds.x[:, b])


def test_hand_over_to_a_gaussian_process():
    """Device tensors in, device tensors out: raw_data are views of the kernel's buffers, and a GaussianProcess given `train_data`
    predicts the same bits as one given host copies of them.  `Model.generate_data` is the same run."""
    m = _model('chemostat4')
    case = dr.case('chemostat4', 5)
    gen, ds = _run(m, case, 'random_uniform', 'uniform', 0, 'difference', [1, 3], tensors=True)
    f, l = ds.raw_data
    F, L = gen._buffers
    assert isinstance(f, torch.Tensor) and f.is_cuda and isinstance(ds.x, torch.Tensor) and isinstance(ds.u, torch.Tensor)
    assert f.shape == (4, 30) and l.shape == (2, 30)
    for v, buf in ((f, F), (l, L)):
        assert buf.data_ptr() <= v.data_ptr() < buf.data_ptr() + buf.numel() * 8 and not v.is_contiguous()
    _, host = _run(m, case, 'random_uniform', 'uniform', 0, 'difference', [1, 3])
    np.testing.assert_array_equal(f.cpu().numpy(), host.raw_data[0])
    np.testing.assert_array_equal(ds.time.cpu().numpy(), host.time)
    ds.select_train_data('downsample', downsample_factor=2)
    ds.select_test_data('downsample', downsample_factor=7)
    Xt, yt = ds.train_data
    assert Xt.is_cuda and Xt.shape == (4, 15) and ds.test_data[0].shape == (4, 5)
    preds = []
    for X, y in ((Xt, yt[:1]), (Xt.cpu().numpy().copy(), yt[:1].cpu().numpy().copy())):
        gp = GaussianProcess(ds.features, ds.labels[0], noise_variance=1e-4)
        gp.set_training_data(X, y)
        gp.setup()
        preds.append(gp.predict(ds.test_data[0].cpu().numpy()))
    np.testing.assert_array_equal(preds[0][0], preds[1][0])
    np.testing.assert_array_equal(preds[0][1], preds[1][1])
    # Model.generate_data: the same launch behind the reference's one call
    uni = case['uniform']
    bounds = {n: {'lb': uni[0][i], 'ub': uni[1][i]} for i, n in enumerate(m.input_names)}
    gd = m.generate_data('random_uniform', output='difference', n_samples=T // dr.HOLD, steps=dr.HOLD, bounds=bounds, seed=dr.SEED,
                         add_noise=dict(dr.NOISES['uniform']['all']), skip=['S', 'I'], x0=case['x0'], p0=case['p'])
    np.testing.assert_array_equal(gd.raw_data[0], host.raw_data[0])
    np.testing.assert_array_equal(gd.raw_data[1], host.raw_data[1])
    assert gd.features == ['X', 'P', 'DS', 'DI'] and gd.labels == ['delta_X', 'delta_P'] and gd.sampling_time == 1.


def test_library_refusals():
    """Through the C entry: HILO_SIM_BDF, a model with algebraic states and a model of five inputs return HILO_ENOTSUP, a null F
    HILO_EINVAL, each with its reason and without a launch; the same call with everything in place runs."""
    lib = _lib.lib()
    dev = torch.device('cuda')
    z = lambda *s: torch.zeros(*s, dtype=torch.float64, device=dev)

    def call(h, nx, nup, sim, F=True):
        x0, up, Fb, Lb = z(1, nx), z(1, nup), z(64), z(64)          # (room for two rows of any model here, should a refusal fail)
        opts = _lib.DatagenOpts()
        opts.kind, opts.hold, opts.seed = 0, 1, 1
        for i in range(4):
            opts.b[i] = 1.
        rc = lib.hilo_datagen_run(h._handle, ctypes.byref(sim), ctypes.byref(opts), None, 1, 2, x0.data_ptr(), up.data_ptr(), 0,
                                  Fb.data_ptr() if F else None, Lb.data_ptr(), None, None, None, None)
        torch.cuda.synchronize()
        return rc, lib.hilo_last_error().decode(), Fb
    plant = _model('linear2')
    h = plant._plant_handle()
    bdf = _lib.SimOpts()
    bdf.method = 2
    rc, msg, _ = call(h, 2, 3, bdf)
    assert rc == -4 and 'HILO_SIM_MAP and HILO_SIM_DOPRI5' in msg
    rc, msg, _ = call(h, 2, 3, _lib.SimOpts(), F=False)
    assert rc == -1 and 'NULL argument' in msg
    dae = Model(name='noroot')
    x, zz, p = dae.set_dynamical_states(['x']), dae.set_algebraic_states(['z']), dae.set_parameters(['p'])
    dae.set_dynamical_equations([-x[0] + zz[0]])
    dae.set_algebraic_equations([zz[0] * zz[0] - p[0] + 0. * x[0]])
    dae.set_measurement_equations([x[0] + zz[0]])
    dae.setup(dt=.2, solver='idas')
    rc, msg, _ = call(dae._plant_handle(), 1, 1, _lib.SimOpts())
    assert rc == -4 and 'algebraic states' in msg
    five = Model(name='five_inputs')
    x, u = five.set_dynamical_states(['x']), five.set_inputs(['a', 'b', 'c', 'd', 'e'])
    five.set_dynamical_equations([-x[0] + u[0] + u[1] + u[2] + u[3] + u[4]])
    five.set_measurement_equations([x[0]])
    five.setup(dt=.2)
    rc, msg, _ = call(five._plant_handle(), 1, 5, _lib.SimOpts())
    assert rc == -4 and 'up to 4 inputs; the model has 5' in msg
    rc, msg, Fb = call(h, 2, 3, _lib.SimOpts())
    assert rc == 0
    rows = Fb[:6].reshape(2, 3).cpu().numpy()                        # [x_1, x_2, u] of rows 0 and 1: x0 = 0, u uniform in (0, 1)
    assert rows[0, :2].tolist() == [0., 0.] and np.all(rows[:, 2] > 0.) and np.all(rows[:, 2] < 1.) and rows[1, 0] > 0.
    assert float(Fb[6:].abs().sum()) == 0.
