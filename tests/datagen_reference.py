"""Plain-numpy restatement of the data generator (`DataGenerator`, include/hilo_hip.h::hilo_datagen_run) - not a test module.

Three parts, each the reference's own statements (hilo_mpc/util/data.py) with the draws replaced by the counter-based generator of
tests/pf_device_reference.py:
  - the excitation signals: `random_uniform` / `random_normal` staircases (data.py:806-854) and the three chirps (data.py:687-755,
    856-993);
  - the measurement noise (data.py:757-796) as ONE array n [T + 1, B, n_x], a pure function of (seed of the state, time index,
    instance number);
  - the slicing algebra of `run` (data.py:1048-1141) for use_input_as_label=False, instance by instance in the reference's
    orientation [quantity, time].
A draw: Philox4x32-10 on the counter (0, index, instance, stream << 16 | d) with block d supplying values 2d and 2d+1; streams 8 / 9
input uniforms / normals (index: the sample number), 10 / 11 noise uniforms / normals (index: the time index, value i: state i)."""
from fractions import Fraction

import numpy as np

from tests import pf_device_reference as pfr

STREAM_INPUT_UNIFORM, STREAM_INPUT_NORMAL, STREAM_NOISE_UNIFORM, STREAM_NOISE_NORMAL = 8, 9, 10, 11


def fma(a, b, c):
    """a * b + c rounded once (the kernel's explicit fma): exact rational arithmetic, then one correctly rounded conversion."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=float), np.asarray(b, dtype=float), np.asarray(c, dtype=float))
    out = np.empty(a.shape)
    for idx in np.ndindex(a.shape):
        out[idx] = float(Fraction(float(a[idx])) * Fraction(float(b[idx])) + Fraction(float(c[idx])))
    return out


def uniforms(seed, index, instance, stream, n_values):
    """[len(index), n_values]: value i of block i // 2 - words 0, 1 for an even i, words 2, 3 for an odd one."""
    index = np.atleast_1d(index)
    out = np.empty((index.size, n_values))
    for d in range((n_values + 1) // 2):
        r = pfr.words(seed, 0, index, instance, stream, d)
        out[:, 2 * d] = pfr.uniform(r[0], r[1])
        if 2 * d + 1 < n_values:
            out[:, 2 * d + 1] = pfr.uniform(r[2], r[3])
    return out


def normals(seed, index, instance, stream, n_values):
    """[len(index), n_values] standard normals by Box-Muller on the same blocks (pf_device_reference.normals with the index in the
    counter's second word)."""
    index = np.atleast_1d(index)
    z = np.empty((index.size, (n_values + 1) // 2 * 2))
    for d in range((n_values + 1) // 2):
        r = pfr.words(seed, 0, index, instance, stream, d)
        rad, ang = np.sqrt(-2. * np.log(pfr.uniform(r[0], r[1]))), 6.283185307179586 * pfr.uniform(r[2], r[3])
        z[:, 2 * d], z[:, 2 * d + 1] = rad * np.cos(ang), rad * np.sin(ang)
    return z[:, :n_values]


def staircase(kind, seed, n_samples, steps, a, b, B, instance_offset=0):
    """U [n_samples * steps, B, n_u]: `random_uniform` (a, b = lower, upper bound) or `random_normal` (a, b = mean, variance) -
    np.repeat(samples, steps, axis=0) of data.py:827 / 852."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    n_u = a.size
    s = np.arange(n_samples)
    out = np.empty((n_samples, B, n_u))
    for i in range(B):
        if kind == 'random_uniform':
            out[:, i] = fma(b - a, uniforms(seed, s, i + instance_offset, STREAM_INPUT_UNIFORM, n_u), a)
        else:
            out[:, i] = np.sqrt(b) * normals(seed, s, i + instance_offset, STREAM_INPUT_NORMAL, n_u) + a
    return np.repeat(out, steps, axis=0)


# ---- data.py:687-755, as written -----------------------------------------------------------------------------------------------------
def _linear_chirp(t, chirp_rate, initial_phase=None, initial_frequency=None):
    if initial_phase is None:
        initial_phase = np.pi / 2.
    if initial_frequency is None:
        initial_frequency = .0001
    return np.sin(initial_phase + 2. * np.pi * (chirp_rate / 2. * t + initial_frequency) * t)


def _exponential_chirp(t, chirp_rate, initial_phase=None, initial_frequency=None):
    if initial_phase is None:
        initial_phase = np.pi / 2.
    if initial_frequency is None:
        initial_frequency = .0001
    return np.sin(initial_phase + 2. * np.pi * initial_frequency * (chirp_rate ** t - 1) / np.log(chirp_rate))


def _hyperbolic_chirp(t, dt, initial_frequency_ratio, initial_phase=None, initial_frequency=None):
    if initial_phase is None:
        initial_phase = np.pi / 2.
    if initial_frequency is None:
        initial_frequency = .0001
    fraction = 1. - 1. / initial_frequency_ratio
    return np.sin(initial_phase - 2. * np.pi * dt * initial_frequency / fraction * np.log(1. - fraction / dt * t))


def chirp(dt, segments):
    """One input's signal (data.py:966-988): segments = [dict(type, amplitude, length, mean, chirp_rate, initial_phase,
    initial_frequency, initial_frequency_ratio)], the last three optional."""
    ui = []
    for s in segments:
        t = np.arange(0., s['length'], dt)
        kw = dict(initial_phase=s.get('initial_phase'), initial_frequency=s.get('initial_frequency'))
        if s['type'] == 'linear':
            c = _linear_chirp(t, s['chirp_rate'], **kw)
        elif s['type'] == 'exponential':
            c = _exponential_chirp(t, s['chirp_rate'], **kw)
        else:
            c = _hyperbolic_chirp(t, dt, s['initial_frequency_ratio'], **kw)
        ui.append(s['mean'] + s['amplitude'] * c)
    return np.concatenate(ui)


def noise(specs, T, B, n_x, default_seed, instance_offset=0):
    """n [T + 1, B, n_x]: specs {state index: dict(distribution=, seed=, lb=, ub= / std=)}; a state without an entry gets zeros."""
    n = np.zeros((T + 1, B, n_x))
    j = np.arange(T + 1)
    for k, s in specs.items():
        seed = s.get('seed', default_seed)
        for i in range(B):
            if s['distribution'] == 'random_uniform':
                n[:, i, k] = fma(s['ub'] - s['lb'], uniforms(seed, j, i + instance_offset, STREAM_NOISE_UNIFORM, k + 1)[:, k], s['lb'])
            else:
                n[:, i, k] = s['std'] * normals(seed, j, i + instance_offset, STREAM_NOISE_NORMAL, k + 1)[:, k]
    return n


def assemble(x, u, n, keep, shift, output):
    """data.py:1048-1141 per instance.  x [T + 1, B, n_x], u [T, B, n_u], n like x or None -> F [N, B, n_f], L [N, B, n_l]: the
    reference's `inputs + input_noise` and `outputs + output_noise`, transposed to the kernel's [row, instance, column]."""
    T, B = u.shape[0], u.shape[1]
    F, L = [], []
    for b in range(B):
        xs, us = x[:, b].T, u[:, b].T                              # the reference's [quantity, time]
        if output == 'difference':
            outputs = np.diff(xs, axis=1)[keep, shift:]
        else:
            outputs = xs[keep, shift + 1:]
        inputs = np.concatenate([xs[keep, k:-(shift + 1 - k)] for k in range(shift + 1)] + [us[:, shift:]], axis=0)
        if n is not None:
            nz = n[:, b].T[keep, :]
            if output == 'difference':
                output_noise = np.diff(nz, axis=1)[:, shift:]
            else:
                output_noise = nz[:, shift + 1:]
            input_noise = np.concatenate([nz[:, k:-(shift + 1 - k)] for k in range(shift + 1)] + [np.zeros((us.shape[0], T - shift))],
                                         axis=0)
            # the kernel adds noise only where a state has some, so -0.0 + 0.0 never replaces a clean entry; values are equal
            inputs, outputs = inputs + input_noise, outputs + output_noise
        F.append(inputs.T)
        L.append(outputs.T)
    return np.stack(F, axis=1), np.stack(L, axis=1)


def names(state_names, input_names, keep, output, shift):
    """data.py:1060-1131."""
    if output == 'difference':
        features = [name for index, name in enumerate(state_names) if index in keep] + input_names
        labels = ['delta_' + name for index, name in enumerate(state_names) if index in keep]
    else:
        features = [name + '_k' for index, name in enumerate(state_names) if index in keep] + input_names
        labels = [name + '_k+1' for index, name in enumerate(state_names) if index in keep]
    if shift > 0:
        if output == 'difference':
            features = [name + '_k' if name in state_names else name for name in features]
        for k in range(shift):
            features = [name + f'_k-{k + 1}' for index, name in enumerate(state_names) if index in keep] + features
    return features, labels


# ---- the cases and the comparisons that the host build and the device share -----------------------------------------------------------
SEED = 0x9E3779B97F4A7C15          # both halves of the key in use
T, HOLD = 6, 2                     # 3 samples x 2 steps
KINDS = {'random_uniform': 0, 'random_normal': 1, 'chirp': 2}
CHIRP_TYPES = {'linear': 0, 'exponential': 1, 'hyperbolic': 2}
NOISES = {
    'none': {},
    'uniform': {'all': dict(distribution='random_uniform', lb=-.01, ub=.03)},
    'normal': {'all': dict(distribution='random_normal', std=.02, seed=77)},
    'per_state': {'last': dict(distribution='random_uniform', lb=0., ub=.05, seed=(1 << 40) + 3)},   # the last state alone, its own key
}


def case(model, B):
    """dt, x0 [B, nx], p [B, np], (a, b) of the two staircases, the chirp segments per input, the states that are skipped.  Instance
    b's initial state and parameters are spread by factors 1 + .1 w_b, w_b in [-1, 1]."""
    w = (1. + .1 * np.cos(1.7 * np.arange(B)))[:, None]
    if model == 'lti211':       # x+ = A x + B u, y = C x: p = [A, B, C] row by row
        return dict(dt=.5, continuous=0, nx=2, nu=1, x0=np.array([[1., -.5]]) * w,
                    p=np.concatenate([[.9, .45, 0., .8], [.125, .5], [1., 0.]])[None, :] * w[::-1],
                    uniform=([-1.], [2.]), normal=([.5], [.04]), skip=[0],
                    chirps=[[dict(type='linear', amplitude=2., length=2., mean=.5, chirp_rate=.3),
                             dict(type='exponential', amplitude=.5, length=1., mean=0., chirp_rate=1.5, initial_phase=.2,
                                  initial_frequency=.1)]])
    if model == 'linear2':
        return dict(dt=.25, continuous=1, nx=2, nu=1, x0=np.array([[.4, .7]]) * w, p=np.array([[1.2, .8]]) * w[::-1],
                    uniform=([-1.], [2.]), normal=([.5], [.04]), skip=[0],
                    chirps=[[dict(type='linear', amplitude=2., length=1., mean=.5, chirp_rate=.3),
                             dict(type='exponential', amplitude=.5, length=.5, mean=0., chirp_rate=1.5, initial_phase=.2,
                                  initial_frequency=.1)]])
    assert model == 'chemostat4'
    return dict(dt=1., continuous=1, nx=4, nu=2, x0=np.array([[2., 30., 1., .3]]) * w, p=np.array([[100., 4., 1., 0.]]) * w[::-1],
                uniform=([0., .05], [.3, .2]), normal=([.15, .1], [.0004, .0001]), skip=[0, 2],
                chirps=[[dict(type='linear', amplitude=.1, length=4., mean=.15, chirp_rate=.05),
                         dict(type='exponential', amplitude=.05, length=2., mean=.1, chirp_rate=1.5)],
                        [dict(type='hyperbolic', amplitude=.05, length=6., mean=.1, chirp_rate=0., initial_frequency=.05,
                              initial_frequency_ratio=1.1)]])


def noise_specs(noise_name, keep, nx):
    specs = {}
    for which, s in NOISES[noise_name].items():
        for k in (keep if which == 'all' else [nx - 1]):
            specs[k] = s
    return specs


def chirp_table(c):
    t = np.zeros((c['nu'], 8, 8))
    for i, segs in enumerate(c['chirps']):
        for j, s in enumerate(segs):
            t[i, j] = [CHIRP_TYPES[s['type']], len(np.arange(0., s['length'], c['dt'])), s['amplitude'], s['mean'], s['chirp_rate'],
                       s.get('initial_phase', np.pi / 2.), s.get('initial_frequency', 1e-4), s.get('initial_frequency_ratio', 0.)]
    return t


def check(tag, c, signal, noise_name, shift, output, keep, got, X_ref, offset, seed=SEED):
    """got: F [N, B, n_f], L [N, B, n_l], X [T + 1, B, nx], U [T, B, nu] of a run of case c.  Uniform inputs, uniform noise, the scatter
    (every feature entry that is a copy) and the difference labels given the same states: bit for bit.  Normals: rtol 1e-11 / atol
    1e-13 (tests/test_pf_device_gpu.py); chirps: 1e-10 x amplitude (phase arguments far below 1e4); plant states against X_ref (None:
    not compared here): the tolerance of tests/test_pid_host.py."""
    nx, nu = c['nx'], c['nu']
    B = got['U'].shape[1]
    # ---- the signal
    if signal == 'chirp':
        for i, segs in enumerate(c['chirps']):
            ref = chirp(c['dt'], segs)
            amp = max(s['amplitude'] for s in segs)
            assert ref.shape == (T,), tag
            for b in range(B):
                np.testing.assert_allclose(got['U'][:, b, i], ref, rtol=0., atol=1e-10 * amp, err_msg=tag)
    else:
        a, b_ = c[signal.split('_')[-1]]
        ref = staircase(signal, seed, T // HOLD, HOLD, a, b_, B, offset)
        if signal == 'random_uniform':
            np.testing.assert_array_equal(got['U'], ref, err_msg=tag)                      # bit for bit
            assert np.all(got['U'] >= np.asarray(a)) and np.all(got['U'] <= np.asarray(b_))
        else:
            np.testing.assert_allclose(got['U'], ref, rtol=1e-11, atol=1e-13, err_msg=tag)
        np.testing.assert_array_equal(got['U'][0::2], got['U'][1::2])                       # held for two intervals
    # ---- the plant, driven by the inputs it was given
    if X_ref is not None:
        np.testing.assert_allclose(got['X'], X_ref, rtol=1e-11, atol=1e-13, err_msg=tag)
    # ---- noise and assembly, given these states and inputs
    specs = noise_specs(noise_name, keep, nx)
    n = noise(specs, T, B, nx, seed, offset) if specs else None
    F, L = assemble(got['X'], got['U'], n, keep, shift, output)
    assert got['F'].shape == F.shape and got['L'].shape == L.shape, tag
    nk = len(keep)
    if noise_name == 'normal':
        np.testing.assert_allclose(got['F'], F, rtol=1e-11, atol=1e-13, err_msg=tag)
        np.testing.assert_allclose(got['L'], L, rtol=1e-11, atol=1e-13, err_msg=tag)
        assert np.max(np.abs(got['F'][:, :, :nk] - got['X'][:T - shift][:, :, keep])) > 1e-3       # the noise is there
    else:
        np.testing.assert_array_equal(got['F'], F, err_msg=tag)                             # bit for bit
        np.testing.assert_array_equal(got['L'], L, err_msg=tag)
    # every feature entry that is a copy is one: the input block, and the state blocks of one row against the next block's earlier row
    np.testing.assert_array_equal(got['F'][:, :, (shift + 1) * nk:], got['U'][shift:], err_msg=tag)
    for s in range(shift):
        np.testing.assert_array_equal(got['F'][1:, :, s * nk:(s + 1) * nk], got['F'][:-1, :, (s + 1) * nk:(s + 2) * nk], err_msg=tag)
    if output == 'absolute' and T - shift > 1:
        np.testing.assert_array_equal(got['L'][:-1], got['F'][1:, :, shift * nk:(shift + 1) * nk], err_msg=tag)   # one n_j in both


def plant_reference(model, c, U):
    """X [T + 1, B, nx] of case c under the inputs U with the fixed-step map."""
    if c['continuous']:
        from tests import sim_reference as sr
        return rollout_rk4(sr.oracle_model(model), c['x0'], U, c['p'], c['dt'])
    X = [rollout_lti(c['p'][b, :4].reshape(2, 2), c['p'][b, 4:6].reshape(2, 1), c['x0'][b:b + 1], U[:, b:b + 1])
         for b in range(U.shape[1])]
    return np.concatenate(X, axis=1)


# ---- plants --------------------------------------------------------------------------------------------------------------------------
def rollout_rk4(om, x0, U, P, dt, n_sub=8):
    """X [T + 1, B, n_x]: the fixed-step map of a continuous zoo model (n_sub classic Runge-Kutta steps per interval, inputs held)."""
    f = lambda x, u: om.f(x, u, P, 1.)
    x = np.array(x0, dtype=float)
    X = [x.copy()]
    hs = dt / n_sub
    for k in range(U.shape[0]):
        for _ in range(n_sub):
            k1 = f(x, U[k])
            k2 = f(x + .5 * hs * k1, U[k])
            k3 = f(x + .5 * hs * k2, U[k])
            k4 = f(x + hs * k3, U[k])
            x = x + hs / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
        X.append(x.copy())
    return np.array(X)


def rollout_lti(A, Bm, x0, U):
    """X [T + 1, B, n_x] of x+ = A x + B u."""
    x = np.array(x0, dtype=float)
    X = [x.copy()]
    for k in range(U.shape[0]):
        x = x @ np.asarray(A).T + U[k] @ np.asarray(Bm).T
        X.append(x.copy())
    return np.array(X)
