"""DataGenerator without a device wherever that is possible: the surface (names, messages, defaults), the body of
csrc/hilo_datagen.h compiled for the HOST (into tmp_path with `hipcc -x hip --cuda-host-only`, like tests/test_pid_host.py) against
the numpy restatement of tests/datagen_reference.py, and the statistics of the draws on that restatement (the device equals it bit
for bit, tests/test_datagen_gpu.py)."""
import os
import shutil
import subprocess
import warnings

import numpy as np
import pytest

from hilo_mpc_amd import DataGenerator, DataSet, Model
from hilo_mpc_amd import data as hd
from tests import datagen_reference as dr
from tests import pf_device_reference as pfr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'hilo_mpc_amd', 'csrc')
SEED = dr.SEED


# ---- the surface ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('shift', [0, 1, 2])
@pytest.mark.parametrize('output', ['absolute', 'difference'])
def test_feature_and_label_names(shift, output):
    xs, us = ['X', 'S', 'P', 'I'], ['DS', 'DI']
    for keep in ([0, 1, 2, 3], [0, 2, 3]):
        assert hd.feature_label_names(xs, us, keep, output, shift) == dr.names(xs, us, keep, output, shift)
    f, l = hd.feature_label_names(xs, us, [0, 2, 3], output, shift)
    past = [n + f'_k-{k}' for k in range(shift, 0, -1) for n in ('X', 'P', 'I')]
    if output == 'absolute':
        assert f == past + ['X_k', 'P_k', 'I_k', 'DS', 'DI'] and l == ['X_k+1', 'P_k+1', 'I_k+1']
    else:
        now = ['X_k', 'P_k', 'I_k'] if shift else ['X', 'P', 'I']
        assert f == past + now + ['DS', 'DI'] and l == ['delta_X', 'delta_P', 'delta_I']


def _linear2():
    return Model('linear2').setup(dt=.25)


def test_constructor_messages():
    m = _linear2()
    with pytest.raises(RuntimeError) as e:
        DataGenerator(m)
    assert str(e.value) == ("No initial dynamical states found. Please supply initial dynamical states or set "
                            "initial conditions of the model before generating data!")
    with pytest.raises(RuntimeError) as e:
        DataGenerator(m, x0=[0., 0.])
    assert str(e.value) == ("No parameter values found. Please supply parameter values or set values for the "
                            "parameters of the model before generating data!")
    dae = _linear2()
    dae.n_z = 1
    with pytest.raises(RuntimeError) as e:
        DataGenerator(dae, x0=[0., 0.], p0=[1., 1.])
    assert str(e.value) == ("No initial algebraic states found. Please supply initial algebraic states or set "
                            "initial conditions of the model before generating data!")
    with pytest.raises(NotImplementedError, match='algebraic states'):
        DataGenerator(dae, x0=[0., 0.], p0=[1., 1.], z0=[0.])
    with pytest.raises(NotImplementedError, match='use_input_as_label'):
        DataGenerator(m, x0=[0., 0.], p0=[1., 1.], use_input_as_label=True)
    with pytest.raises(RuntimeError, match=r"Model is not set up. Run Model.setup\(\)"):
        DataGenerator(Model('linear2'), x0=[0., 0.], p0=[1., 1.])
    stiff = _linear2()
    stiff._solver = 'bdf'
    with pytest.raises(NotImplementedError, match=r"Model.setup\(solver='dopri5'\)"):
        DataGenerator(stiff, x0=[0., 0.], p0=[1., 1.])
    # the model's own initial conditions and parameter values serve
    m.set_initial_conditions([.1, .2])
    m.set_initial_parameter_values([1., 2.])
    g = DataGenerator(m)
    assert np.asarray(g._x0).ravel().tolist() == [.1, .2] and np.asarray(g._p0).tolist() == [1., 2.]
    with pytest.raises(RuntimeError, match='No excitation signal set'):
        g.run('absolute')
    with pytest.raises(NotImplementedError, match='closed_loop'):
        g.closed_loop(None, 3)


def test_signal_messages():
    g = DataGenerator(_linear2(), x0=[0., 0.], p0=[1., 1.])
    with pytest.raises(ValueError) as e:
        g.chirp([['linear', 'linear']], [[1., 2., 3.]], 1., 0., 1.)
    assert str(e.value) == "Dimension mismatch between types (2) and amplitudes (3)"
    with pytest.raises(ValueError) as e:
        g.chirp('cubic', 1., 1., 0., 1.)
    assert str(e.value) == "Type 'cubic' not recognized for chirp signal"
    with pytest.raises(ValueError) as e:
        g.chirp('hyperbolic', 1., 1., 0., 1.)
    assert str(e.value) == "Initial frequency ratio for hyperbolic chirp signal was not supplied"
    with pytest.raises(ValueError, match='not positive on the whole segment'):
        g.chirp('hyperbolic', 1., 2., 0., 1., initial_frequency_ratio=5.)        # 1 - .8 t / dt < 0 from t = .5 on
    g.chirp('hyperbolic', 1., 2., 0., 1., initial_frequency_ratio=1.1)
    assert g._signal['T'] == 8 and g._signal['table'][0, 0].tolist() == [2., 8., 1., 0., 1., np.pi / 2., 1e-4, 1.1]
    with pytest.raises(ValueError, match='must not be negative'):
        g.random_normal(3, 2, 0., -1.)
    with pytest.raises(ValueError, match='Dimension mismatch'):
        g.random_uniform(3, 2, [0., 0.], 1.)
    g.random_uniform(3, 2, 0., 1.)
    assert isinstance(g.seed, int) and 0 <= g.seed < 2 ** 64          # a fresh seed is drawn and recorded
    g.random_uniform(3, 2, 0., 1., seed=7)
    assert g.seed == 7
    with pytest.raises(ValueError, match="Output 'relative' not recognized"):
        g.run('relative')
    with pytest.raises(ValueError, match='leaves no row'):
        g.run('absolute', shift=6)
    with pytest.raises(ValueError, match="no dynamical state 'z'"):
        g.run('absolute', skip=['z'])
    two = DataGenerator(Model('chemostat4').setup(dt=1.), x0=4 * [1.], p0=4 * [1.])
    with pytest.raises(ValueError, match=r"different lengths: \[4, 6\] points"):
        two.chirp('linear', 1., [[4.], [6.]], 0., 1.)


def test_noise_specifications():
    g = DataGenerator(Model('chemostat4').setup(dt=1.), x0=4 * [1.], p0=4 * [1.])
    g.random_uniform(3, 2, 0., 1., seed=11)
    with pytest.warns(UserWarning, match='Assuming a standard deviation of 1.'):
        n = g._noise({}, [0, 2, 3])
    assert n == {k: (hd.NOISE_NORMAL, 11, 1., 0.) for k in (0, 2, 3)}
    with pytest.warns(UserWarning) as w:
        n = g._noise({'distribution': 'random_uniform', 'seed': 5}, [1])
    assert n == {1: (hd.NOISE_UNIFORM, 5, 0., 1.)}
    assert sorted(str(v.message) for v in w) == [
        "No lower bound was supplied for random uniform distribution. Assuming lower bound of 0.",
        "No upper bound was supplied for random uniform distribution. Assuming upper bound of 1."]
    with warnings.catch_warnings():
        warnings.simplefilter('error')
        # one dict per state name; with a skipped state in front the entry of P still acts on P (state 2)
        n = g._noise({'P': {'distribution': 'random_uniform', 'lower_bound': -1., 'upper_bound': 2.}, 'I': {'var': 4., 'seed': 3}},
                     [0, 2, 3])
    assert n == {2: (hd.NOISE_UNIFORM, 11, -1., 2.), 3: (hd.NOISE_NORMAL, 3, 2., 0.)}
    with pytest.raises(ValueError) as e:
        g._noise({'distribution': 'cauchy'}, [0])
    assert str(e.value) == "Distribution 'cauchy' not available/recognized for adding noise to generated data"


def test_generate_data_defaults_and_messages(monkeypatch):
    seen = {}

    def run(self, output, skip=None, shift=0, add_noise=None):
        seen.update(signal=self._signal, output=output, skip=skip, shift=shift, add_noise=add_noise, seed=self.seed)
    monkeypatch.setattr(DataGenerator, 'run', run)
    m = Model('chemostat4').setup(dt=1.)
    kw = dict(x0=4 * [1.], p0=4 * [1.])
    for sig in ('random uniform', 'random_normal'):
        with pytest.raises(ValueError) as e:
            m.generate_data(sig, steps=2, **kw)
        assert str(e.value) == (f"Generating data using the {sig.replace('_', ' ')} signal requires information about the number of "
                                f"samples by supplying the keyword 'n_samples'")
        with pytest.raises(ValueError) as e:
            m.generate_data(sig, n_samples=2, **kw)
        assert str(e.value) == (f"Generating data using the {sig.replace('_', ' ')} signal requires information about the number of "
                                f"steps by supplying the keyword 'steps'")
    m.generate_data('Random Normal', n_samples=3, steps=2, bounds={'DS': {'lb': .1, 'upper_bound': .5}}, variance={'DI': .25},
                    seed=9, add_noise={'std': .1}, skip=['S'], shift=1, output='difference', **kw)
    s = seen['signal']
    assert s['kind'] == hd.NORMAL and s['hold'] == 2 and s['T'] == 6
    np.testing.assert_array_equal(s['a'], [.1 + (.5 - .1) / 2, .5])                       # the middle of the bounds (default 0, 1)
    np.testing.assert_array_equal(s['b'], [(1. / 3. * (.5 - .1) / 2) ** 2, .25])
    assert seen['skip'] == [1] and seen['shift'] == 1 and seen['output'] == 'difference' and seen['seed'] == 9
    assert seen['add_noise'] == {'std': .1, 'seed': 9}                                    # the signal's seed serves the noise
    m.generate_data('random_uniform', n_samples=3, steps=2, **kw)
    np.testing.assert_array_equal(seen['signal']['a'], [0., 0.])
    np.testing.assert_array_equal(seen['signal']['b'], [1., 1.])
    with pytest.raises(ValueError) as e:
        m.generate_data('chirp', chirps={'DS': {'length': 3., 'chirp_rate': 1.}}, **kw)
    assert str(e.value) == "No chirp signals supplied for input'DI'"
    with pytest.raises(ValueError) as e:
        m.generate_data('chirp', chirps={'DS': {'chirp_rate': 1.}, 'DI': {}}, **kw)
    assert str(e.value) == "No length(s) supplied for input 'DS'"
    with pytest.raises(ValueError) as e:
        m.generate_data('chirp', chirps={'DS': {'length': 3.}, 'DI': {}}, **kw)
    assert str(e.value) == "No chirp rate(s) supplied for input 'DS'"
    m.generate_data('chirp', chirps={'DS': {'length': 3., 'chirp_rate': 1.}, 'DI': {'length': [1., 2.], 'chirp_rate': .5, 'mean': 2.}}, **kw)
    t = seen['signal']['table']
    assert seen['signal']['T'] == 3 and t[0, 0].tolist() == [0., 3., 1., 0., 1., np.pi / 2., 1e-4, 0.]
    assert t[1, 0].tolist() == [0., 1., 1., 2., .5, np.pi / 2., 1e-4, 0.] and t[1, 1, 1] == 2.
    with pytest.raises(ValueError) as e:
        m.generate_data('random_uniform', n_samples=3, steps=2, skip=['S', 2], **kw)
    assert str(e.value) == ("Mixed iterables for the keyword argument 'skip' are not allowed. Either use only "
                            "strings or only indices (integers) in your iterable.")
    with pytest.raises(ValueError, match='No controller supplied for closed loop setup'):
        m.generate_data('closed_loop', **kw)
    with pytest.raises(ValueError, match="Signal type 'prbs' not recognized"):
        m.generate_data('prbs', **kw)


def test_data_set_holder():
    N, B = 4, 3
    F = np.arange(N * B * 3, dtype=float).reshape(N, B, 3)
    L = -np.arange(N * B * 2, dtype=float).reshape(N, B, 2)
    F[2, 1, 0] = np.nan
    L[3, 2, 1] = np.nan
    ds = DataSet(['a_k', 'b_k', 'u'], ['a_k+1', 'b_k+1'], F, L, np.arange(N) * .5, np.zeros(B, dtype=int), None, None, .5)
    f, l = ds.raw_data
    assert len(ds) == 12 and f.shape == (3, 12) and l.shape == (2, 12) and ds.sampling_time == .5 and ds.dt == .5
    assert np.shares_memory(f, F) and np.shares_memory(l, L)                      # views
    np.testing.assert_array_equal(f[:, 2 * B + 1], F[2, 1])
    assert ds.finite_rows().tolist() == [c for c in range(12) if c not in (2 * B + 1, 3 * B + 2)]
    assert ds.train_data[0].shape == (3, 0)
    ds.select_train_data('downsample', downsample_factor=5)
    ds.select_test_data('downsample', downsample_factor=4)
    np.testing.assert_array_equal(ds.train_data[1], l[:, [0, 5, 10]])
    np.testing.assert_array_equal(ds.test_data[0], f[:, [0, 4, 8]])
    with pytest.raises(NotImplementedError, match='sequential host work'):
        ds.select_train_data('euclidean_distance', distance_threshold=.1)
    with pytest.raises(NotImplementedError) as e:
        ds.select_test_data('kmeans')
    assert str(e.value) == "Data selection method 'kmeans' not implemented or recognized"
    assert ds.features == ['a_k', 'b_k', 'u'] and ds.labels == ['a_k+1', 'b_k+1']


# ---- the draws, on the restatement ---------------------------------------------------------------------------------------------------
def test_draw_statistics():
    """16384 input uniforms (B = 4096 instances, 4 samples): the mean within 5 sigma / sqrt(n) of the midpoint (sigma^2 = 1 / 12), no
    two neighbours equal across instances or across samples, every value inside (0, 1)."""
    s, b = np.arange(4)[:, None], np.arange(4096)[None, :]
    r = pfr.words(SEED, 0, s, b, dr.STREAM_INPUT_UNIFORM, 0)
    U = pfr.uniform(r[0], r[1]).reshape(4, 4096)
    np.testing.assert_array_equal(U[:, 17], dr.uniforms(SEED, np.arange(4), 17, dr.STREAM_INPUT_UNIFORM, 1)[:, 0])
    n = U.size
    print(f"mean - .5 = {U.mean() - .5:.3e}, bound {5 / np.sqrt(12 * n):.3e}")
    assert abs(U.mean() - .5) <= 5. / np.sqrt(12. * n)
    assert U.min() > 0. and U.max() < 1.
    assert not np.any(U[:, 1:] == U[:, :-1]) and not np.any(U[1:] == U[:-1])
    # the second value of a block, another stream and another seed are other numbers
    V = pfr.uniform(r[2], r[3]).reshape(4, 4096)
    r2 = pfr.words(SEED, 0, s, b, dr.STREAM_NOISE_UNIFORM, 0)
    r3 = pfr.words(SEED + 1, 0, s, b, dr.STREAM_INPUT_UNIFORM, 0)
    for W in (V, pfr.uniform(r2[0], r2[1]).reshape(4, 4096), pfr.uniform(r3[0], r3[1]).reshape(4, 4096)):
        assert not np.any(W == U)


# ---- csrc/hilo_datagen.h compiled for the host -----------------------------------------------------------------------------------------
DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "hilo_datagen.h"
#include "hilo_kf_params.h"
using namespace hilo;

static double next(FILE* f) {
  double v;
  if (fscanf(f, "%lf", &v) != 1) { fprintf(stderr, "short input\n"); exit(2); }
  return v;
}
static unsigned long long next_seed(FILE* f) {   // two 32-bit halves, low first (a double holds neither a 64-bit seed)
  const unsigned long long lo = (unsigned long long)next(f), hi = (unsigned long long)next(f);
  return lo | hi << 32;
}
static void dump(const char* tag, const std::vector<double>& v) {
  printf("%s", tag);
  for (double q : v) printf(" %.17g", q);
  printf("\n");
}

// input: continuous B T dt kind hold shift difference skip_mask instance_offset seed(lo hi), a [4], b [4], per state of 12: noise_kind
// seed(lo hi) na nb, the chirp table [NU][8][8], then per instance x0 and [u; p]
template <class M>
int run(FILE* f) {
  constexpr int NX = M::NX, NU = M::NU, NUP = M::NU + M::NP;
  KfParams kp;
  kp.kind = 0; kp.erk_order = 0; kp.n_sub = 8;
  kp.continuous = (int)next(f);
  const int B = (int)next(f), T = (int)next(f);
  kp.dt = next(f);
  DatagenParams dg;
  memset(&dg, 0, sizeof(dg));
  dg.kind = (int)next(f); dg.hold = (int)next(f); dg.shift = (int)next(f); dg.difference = (int)next(f);
  dg.skip_mask = (int)next(f); dg.instance_offset = (long long)next(f);
  dg.seed = next_seed(f);
  for (int i = 0; i < DG_MAX_NU; ++i) dg.a[i] = next(f);
  for (int i = 0; i < DG_MAX_NU; ++i) dg.b[i] = next(f);
  for (int i = 0; i < DG_MAX_NX; ++i) {
    dg.noise_kind[i] = (int)next(f);
    dg.noise_seed[i] = next_seed(f);
    dg.na[i] = next(f); dg.nb[i] = next(f);
  }
  std::vector<double> table(NU * DG_MAX_SEG * DG_SEG_FIELDS), x0(B * NX), up(B * NUP);
  for (auto& v : table) v = next(f);
  for (int b = 0; b < B; ++b) {
    for (int i = 0; i < NX; ++i) x0[b * NX + i] = next(f);
    for (int i = 0; i < NUP; ++i) up[b * NUP + i] = next(f);
  }
  int nk = 0;
  for (int i = 0; i < NX; ++i) nk += (dg.skip_mask >> i & 1) ? 0 : 1;
  const int N = T - dg.shift, nf = (dg.shift + 1) * nk + NU;
  std::vector<double> F(N * B * nf, -7.0), L(N * B * nk, -7.0), X((T + 1) * B * NX, -7.0), U(T * B * NU, -7.0);
  std::vector<int> stats(B * 4);
  SimParams sim = {SIM_MAP, 10000, 1e-6, 1e-8, 0.0};
  for (int b = 0; b < B; ++b)
    datagen_instance<M, SIM_MAP>(kp, sim, dg, table.data(), b, B, T, x0.data(), up.data(), NUP, F.data(), L.data(), X.data(), U.data(),
                                 stats.data(), 0.0);
  dump("F", F); dump("L", L); dump("X", X); dump("U", U);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[2], "r");
  if (!f) return 2;
  if (!strcmp(argv[1], "lti211")) return run<Lti<2, 1, 1>>(f);
  if (!strcmp(argv[1], "chemostat4")) return run<Chemostat4>(f);
  return 2;
}
"""


def _hipcc():
    for c in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', shutil.which('hipcc')):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip('hipcc not available')
    d = tmp_path_factory.mktemp('datagen_host')
    src = d / 'driver.hip'
    src.write_text(DRIVER)
    exe = d / 'driver'
    subprocess.check_call([hipcc, '-x', 'hip', '--cuda-host-only', '-std=c++17', '-O2', '-I', CSRC, str(src), '-o', str(exe)])
    count = [0]

    def run(what, numbers):
        count[0] += 1
        fin = d / f'in{count[0]}.txt'
        fin.write_text(' '.join(repr(float(v)) for v in numbers))
        out = subprocess.check_output([str(exe), what, str(fin)], text=True).strip().split('\n')
        return {ln.split()[0]: np.array([float(v) for v in ln.split()[1:]]) for ln in out}
    return run




B_, OFFSET = 3, 5
T_ = dr.T


def _halves(seed):
    return [seed & 0xFFFFFFFF, seed >> 32]


def _host_run(driver, model, signal, noise, shift, output, skip):
    case = dr.case(model, B_)
    nx, nu = case['nx'], case['nu']
    keep = [k for k in range(nx) if k not in skip]
    specs = dr.noise_specs(noise, keep, nx)
    a, b = case.get(signal.split('_')[-1], ([0.] * nu, [0.] * nu))
    nums = [case['continuous'], B_, T_, case['dt'], dr.KINDS[signal], dr.HOLD if signal != 'chirp' else 0, shift,
            int(output == 'difference'), sum(1 << k for k in skip), OFFSET] + _halves(SEED)
    nums += list(a) + (4 - nu) * [0.] + list(b) + (4 - nu) * [0.]
    for k in range(12):
        s = specs.get(k)
        if s is None:
            nums += [0, 0, 0, 0., 0.]
        elif s['distribution'] == 'random_uniform':
            nums += [1] + _halves(s.get('seed', SEED)) + [s['lb'], s['ub']]
        else:
            nums += [2] + _halves(s.get('seed', SEED)) + [s['std'], 0.]
    nums += list(dr.chirp_table(case).ravel())
    for i in range(B_):
        nums += list(case['x0'][i]) + nu * [123.] + list(case['p'][i])          # the inputs of `up` are never read
    out = driver(model, nums)
    N, nk = T_ - shift, len(keep)
    got = dict(F=out['F'].reshape(N, B_, (shift + 1) * nk + nu), L=out['L'].reshape(N, B_, nk), X=out['X'].reshape(T_ + 1, B_, nx),
               U=out['U'].reshape(T_, B_, nu))
    return case, keep, got


@pytest.mark.parametrize('model', ['lti211', 'chemostat4'])
@pytest.mark.parametrize('signal', ['random_uniform', 'random_normal', 'chirp'])
def test_host_compiled_body_against_the_restatement(driver, model, signal):
    """T = 6 (3 samples x 2), B = 3 with instance_offset 5: shift 0, 1, 2 x both outputs x each noise kind, states skipped in every
    other run.  The comparisons and their tolerances: tests/datagen_reference.py::check."""
    runs = 0
    for shift in (0, 1, 2):
        for output in ('absolute', 'difference'):
            for noise in dr.NOISES:
                skip = dr.case(model, B_)['skip'] if (shift + runs + runs // 4) % 2 else []
                runs += 1
                case, keep, got = _host_run(driver, model, signal, noise, shift, output, skip)
                tag = f"{model} {signal} noise={noise} shift={shift} {output} skip={skip}"
                dr.check(tag, case, signal, noise, shift, output, keep, got, dr.plant_reference(model, case, got['U']), OFFSET)
    assert runs == 24


def test_host_single_row_and_instance_numbers(driver):
    """shift = T - 1 leaves ONE row that holds every state; the same instance number gives the same draws whatever its place."""
    case, keep, got = _host_run(driver, 'lti211', 'random_uniform', 'uniform', T_ - 1, 'difference', [])
    assert got['F'].shape == (1, B_, T_ * 2 + 1) and got['L'].shape == (1, B_, 2)
    dr.check('single row', case, 'random_uniform', 'uniform', T_ - 1, 'difference', keep, got,
             dr.plant_reference('lti211', case, got['U']), OFFSET)
    a, b = case['uniform']
    np.testing.assert_array_equal(got['U'][:, 1], dr.staircase('random_uniform', SEED, 3, 2, a, b, 1, OFFSET + 1)[:, 0])


def test_opts_layout_matches_the_header(tmp_path):
    """`hilo_datagen_opts` of include/hilo_hip.h compiled by gcc against its ctypes mirror: names, order, offsets, size."""
    import ctypes as C
    import re
    from hilo_mpc_amd import _lib
    if shutil.which('gcc') is None:
        pytest.skip('gcc not available')
    header = open(os.path.join(ROOT, 'include', 'hilo_hip.h')).read()
    body = re.search(r'typedef struct hilo_datagen_opts \{(.*?)\} hilo_datagen_opts;', header, re.S).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    fields = [re.sub(r'\[.*\]', '', part.split()[-1]) for decl in body.split(';') if decl.strip() for part in decl.split(',')]
    assert fields == [f[0] for f in _lib.DatagenOpts._fields_]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "hilo_hip.h"', 'int main(void) {',
             '  printf("size %zu\\n", sizeof(hilo_datagen_opts));']
    lines += [f'  printf("{f} %zu\\n", offsetof(hilo_datagen_opts, {f}));' for f in fields] + ['  return 0;', '}']
    src = tmp_path / 'layout.c'
    src.write_text('\n'.join(lines))
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    got = dict(ln.split() for ln in subprocess.check_output([str(exe)], text=True).strip().split('\n'))
    assert int(got['size']) == C.sizeof(_lib.DatagenOpts)
    for f, _ in _lib.DatagenOpts._fields_:
        assert int(got[f]) == getattr(_lib.DatagenOpts, f).offset, f
