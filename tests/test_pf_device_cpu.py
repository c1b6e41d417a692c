"""The particle filter's device mode without a device: the generator's known answers, the maps to uniforms and normals, the share of
frail resampling draws, the restatement (tests/pf_device_reference.py) against the Kalman filter on a linear-Gaussian model, and the
refusals of `ParticleFilter(generator='device')`, which are raised before any device call."""
import numpy as np
import pytest

from tests import pf_device_reference as ref


def test_philox_known_answers():
    """Philox4x32-10: the zero and all-ones vectors of Random123's known-answer file and the digits-of-pi one."""
    for counter, key, want in (((0, 0, 0, 0), (0, 0), '6627e8d5 e169c58d bc57ac4c 9b00dbd8'),
                               ((0xffffffff,) * 4, (0xffffffff,) * 2, '408f276d 41c83b0e a20bc7c6 6d5451fd'),
                               ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
                                'd16cfe09 94fdcceb 5001e420 24126ea1')):
        assert ' '.join('%08x' % int(v[0]) for v in ref.philox4x32_10(counter, key)) == want
    # vectorised over the counter like one word at a time
    r = ref.philox4x32_10((np.array([0, 0x243f6a88]), np.array([0, 0x85a308d3]), np.array([0, 0x13198a2e]), np.array([0, 0x03707344])), (0, 0))
    assert '%08x' % int(r[0][0]) == '6627e8d5'


def test_uniform_map_end_points():
    """All-zero words give 2^-54 (never 0: the logarithm is safe).  All-one words give the top cell's centre 1 - 2^-54, which a double
    cannot hold: it rounds to 1, where the logarithm is 0 and the resampling search ends at the last particle."""
    lo, hi = float(ref.uniform(0, 0)), float(ref.uniform(0xffffffff, 0xffffffff))
    assert lo == 2. ** -54 and hi == 1.
    # (from 2^52 cells on the half is below a double's spacing and the centre rounds to the cell's even edge) the next cell down
    assert float(ref.uniform(0xffffffff, 0xffffffff - 64)) == 1. - 2. ** -52
    assert float(ref.uniform(1 << 5, 0)) == (2. ** 26 + .5) * 2. ** -53 and float(ref.uniform(0, 1 << 6)) == 1.5 * 2. ** -53


def test_normal_map_moments():
    n = 100000
    z = ref.normals(7, np.arange(n // 2), 3, 11, ref.STREAM_PROCESS, 2).ravel()
    assert z.size == n and abs(z.mean()) < 4 / np.sqrt(n) and abs(z.var() - 1) < 4 * np.sqrt(2 / n)
    # the streams, steps and filters are separate draws
    a = ref.normals(7, np.arange(8), 3, 11, ref.STREAM_PROCESS, 3)
    for other in (ref.normals(7, np.arange(8), 3, 11, ref.STREAM_MEASUREMENT, 3), ref.normals(7, np.arange(8), 4, 11, ref.STREAM_PROCESS, 3),
                  ref.normals(7, np.arange(8), 3, 12, ref.STREAM_PROCESS, 3), ref.normals(8, np.arange(8), 3, 11, ref.STREAM_PROCESS, 3)):
        assert not np.any(a == other)
    np.testing.assert_array_equal(a[:, :2], ref.normals(7, np.arange(8), 3, 11, ref.STREAM_PROCESS, 2))      # block 0 is block 0


def test_tolerant_cholesky():
    A = np.array([[4., 2., 0.], [2., 5., 0.], [0., 0., 0.]])                       # the third state is not excited
    L = ref.cholesky_tolerant(A)
    np.testing.assert_allclose(L @ L.T, A, atol=1e-15)
    assert np.all(L[:, 2] == 0) and np.all(np.triu(L, 1) == 0)
    rng = np.random.default_rng(0)
    S = rng.standard_normal((5, 5))
    S = S @ S.T + np.eye(5)
    np.testing.assert_allclose(ref.cholesky_tolerant(S), np.linalg.cholesky(S), rtol=1e-13, atol=1e-15)


@pytest.mark.parametrize('N', [2, 32, 63, 64, 65, 255, 257, 300, 500, 512, 8192])
def test_frail_draws_stay_under_the_cap(N):
    """Sizes and seeds of tests/test_pf_device_gpu.py: the restatement alone stays under the cap of 0.5 % exempt draws a step (the
    expected share is 2e-9 N)."""
    from oracle import models as omodels
    f = ref.Filter(omodels.get('toy1d'), 1., N, seed=5, number=0)
    f.set_initial_guess([1.5], [[.01]])
    for k in range(2):
        out = f.step([7.6], [], [], [[.01]], [[.1]])
        assert out['frail'].mean() <= ref.FRAIL_CAP and np.all(np.isfinite(out['q']))
        assert abs(out['q'].sum() - 1) < 1e-12 and 1. <= out['ess'] <= N * (1 + 1e-12)


def test_restatement_meets_the_kalman_filter():
    """`Lti<2, 1, 1>`, linear-Gaussian, 10 steps, N = 4096: the particle mean stays within 6 sqrt(diag(P_kf) (1/N + 1/ess)) of the
    Kalman filter's estimate (oracle/kf.py) at every step.  The Kalman filter runs with the measurement covariance 2 R: the flow
    (pf.py:131-166) adds a draw v ~ N(0, R) to every particle's predicted measurement BEFORE it weighs the particle with
    normpdf(y; h(x) + v, sqrt(R)), so a particle's expected weight is normpdf(y; h(x), sqrt(2 R)) - the posterior the particles
    converge to is the one of a measurement with covariance 2 R.  (With R itself the velocity estimate is 10 of these sigmas away at
    step 1 and up to 13 later: measured, not a rounding matter.)"""
    from oracle import kf as okf
    dt, N, steps = .5, 4096, 10
    om = ref.double_integrator()
    rng = np.random.default_rng(4)
    Q, R, P0 = .05 * np.eye(2), np.array([[.1]]), np.eye(2)
    x0 = np.array([1., -.5])
    xt = x0 + rng.standard_normal(2)
    f = ref.Filter(om, dt, N, seed=2024)
    f.set_initial_guess(x0, P0)
    tile = okf.pack(x0[None], P0[None])
    for k in range(steps):
        u = np.array([.3 * np.sin(.7 * k)])
        xt = om.f(xt[None], u[None], np.zeros((1, 0)), dt)[0] + np.sqrt(.05) * rng.standard_normal(2)
        y = om.h(xt[None], u[None], np.zeros((1, 0)), dt)[0] + np.sqrt(.1) * rng.standard_normal(1)
        out = f.step(y, u, [], Q, R)
        tile, _ = okf.kf_step(om, tile, y[None], u[None], np.zeros((1, 0)), Q, 2 * R, dt)
        x_kf, P_kf = tile[0, :, 0], tile[0, :, 1:]
        bound = 6 * np.sqrt(np.diag(P_kf) * (1 / N + 1 / out['ess']))
        assert np.all(np.abs(out['x'] - x_kf) <= bound), (k, out['x'] - x_kf, bound)
    assert f.status == (0, 0)


def test_not_finite_weights_are_recorded_and_skipped():
    from oracle import models as omodels
    f = ref.Filter(omodels.get('toy1d'), 1., 16, seed=1)
    f.set_initial_guess([1.5], [[.01]])
    f.step([7.6], [], [], [[.01]], [[.1]])
    out = f.step([np.nan], [], [], [[.01]], [[.1]])
    assert f.status == (1, 1) and np.array_equal(out['index'], np.arange(16)) and np.array_equal(out['X'], out['X_prop'])
    assert np.all(np.isfinite(f.step([7.6], [], [], [[.01]], [[.1]])['x'])) and f.status == (1, 1)


# ---- the host side of ParticleFilter(generator='device') -------------------------------------------------------------------------
def _toy():
    from hilo_mpc_amd import Model
    return Model('toy1d').setup(dt=1.)


def test_device_mode_is_opt_in_and_its_options_belong_to_it():
    from hilo_mpc_amd import PF
    pf = PF(_toy())
    assert pf._generator == 'numpy'
    for kw in (dict(seed=3), dict(resampling='systematic'), dict(filter_offset=2)):
        with pytest.raises(ValueError, match="belong to generator='device'"):
            PF(_toy(), **kw)
    with pytest.raises(ValueError, match="Use 'numpy'"):
        PF(_toy(), generator='cuda')
    with pytest.raises(ValueError, match="'multinomial' or 'systematic'"):
        PF(_toy(), generator='device', resampling='stratified')
    pf = PF(_toy(), generator='device', seed=2 ** 40 + 5, resampling='systematic', filter_offset=7, roughening=True, K=.3)
    assert (pf._seed, pf._resampling, pf._filter_offset, pf._roughening_tuning_param) == (2 ** 40 + 5, 'systematic', 7, .3)


def test_device_mode_refusals_come_before_any_device_call(monkeypatch):
    """prior editing, a sampler of the user's, a time-variant model, a particle count outside 2..8192 and more than 16 states: each
    refusal says what to use instead, and none of them reaches the library."""
    from hilo_mpc_amd import Model, PF, _lib

    def no_library():
        raise AssertionError("a refusal must not reach the library")
    monkeypatch.setattr(_lib, 'lib', no_library)
    with pytest.raises(NotImplementedError, match="Use generator='numpy' for prior editing"):
        PF(_toy(), generator='device', prior_editing=True)
    pf = PF(_toy(), generator='device')
    with pytest.raises(NotImplementedError, match="Use generator='numpy' with a probability_density_function"):
        pf.probability_density_function = lambda mu, s, n: np.random.multivariate_normal(mu, s, size=n)
    from tests.test_timevar_gpu import FORCED2_TEXT
    m = Model(name='forced2')
    m.set_parameters(['k', 'c', 'w'])
    m.set_equations(FORCED2_TEXT)
    md = m.discretize('rk4')
    md.setup(dt=.5)
    with pytest.raises(NotImplementedError, match="depends on time explicitly.*write the time dependence as an input"):
        PF(md, generator='device')
    for n in (1, 8193):
        with pytest.raises(ValueError, match="2 to 8192 particles"):
            PF(_toy(), generator='device').setup(n_samples=n)
    wide = Model(discrete=True)
    x = wide.set_dynamical_states([f'x_{i}' for i in range(17)])
    wide.set_dynamical_equations([.5 * x[i] for i in range(17)])
    wide.set_measurement_equations([x[0]])
    wide.setup(dt=1.)
    with pytest.warns(UserWarning):
        pfw = PF(wide, generator='device')
    with pytest.raises(NotImplementedError, match="up to 16 states, the model has 17. Use generator='numpy'"):
        pfw.setup(n_samples=10)


def test_options_struct_matches_the_header(tmp_path):
    """`hilo_pf_opts` of include/hilo_hip.h compiled by gcc against its ctypes mirror: names, order, offsets, size (the way
    tests/test_abi.py::test_descriptor_layouts_match_the_header checks the descriptors)."""
    import ctypes as C
    import os
    import re
    import shutil
    import subprocess
    from hilo_mpc_amd import _lib
    if shutil.which('gcc') is None:
        pytest.skip('gcc not available')
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'hilo_hip.h')).read()
    body = re.search(r'typedef struct hilo_pf_opts \{(.*?)\} hilo_pf_opts;', header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = [part.replace('*', ' ').split()[-1] for decl in body.split(';') if decl.strip() for part in decl.split(',')]
    assert fields == [f[0] for f in _lib.PfOpts._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hilo_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(hilo_pf_opts));']
    lines += [f'  printf("{f} %zu\\n", offsetof(hilo_pf_opts, {f}));' for f in fields] + ['  return 0;', '}']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    subprocess.check_call(['gcc', '-I', os.path.join(root, 'include'), str(src), '-o', str(tmp_path / 'layout')])
    got = dict(l.split() for l in subprocess.check_output([str(tmp_path / 'layout')], text=True).strip().split('\n'))
    assert int(got['size']) == C.sizeof(_lib.PfOpts)
    for f, _ in _lib.PfOpts._fields_:
        assert int(got[f]) == getattr(_lib.PfOpts, f).offset, f
    assert hasattr(_lib.lib(), 'hilo_pf_run')
