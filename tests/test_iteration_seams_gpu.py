"""GPU: the seams of the interior-point iteration that are wave-wide reductions and wave-uniform decisions (csrc/hilo_ocp.h: the
transposing WaveReduceN of kkt_pass, the step lengths and eval_values_call; the filter acceptance by one ballot in the line search,
the second-order correction and the restoration; the scaling tail of kkt_pass) - C2's problem at B = 8 against the oracle's dense
interior-point solver, with the tolerances of tests/test_nmpc_gpu.py:

* N = 1, 2, 3 (test_minimal_horizons_vs_oracle): status and iteration counts exact, u_0 rtol 1e-9 / atol 1e-12;
* N = 20 and NCAP + 1, the run-time LDS layout (test_c2_cold_and_warm_vs_oracle): status exact, KKT error <= 1e-8, v within 1e-6 of
  max(1, |v|), u_0 rtol 1e-6 / atol 1e-7, f rtol 1e-8.

Three instances take the rare branches.  Which starts do is decided with the ORACLE ALONE (a line trace of DenseIpm.solve_data reads
the size of the instance's filter whenever a trial point is rejected, and its result counts the second-order corrections); the
product must then walk the same path: same status, same iteration count.

* FAR (filter): substrate far above the feed's, product and inhibitor present - the oracle rejects four trial points while the filter
  holds all 16 entries.
* SOC: the oracle accepts two second-order corrections.
* a NaN parameter: status -1, and the other instances of the batch bit for bit what they are without it.
"""
import ctypes as C
import inspect
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle.nmpc import DenseIpm                                      # noqa: E402
from tests.problems import C2, c2_x0, oracle_problem, product_nmpc    # noqa: E402

B = 8
FAR, SOC = 5, 6                                   # rows of the batch
X_FAR = [.2239, 228.3435, 1.7885, .1145]
X_SOC = [.484, 194.2899, 2.9657, 1.3488]


def _batch():
    x0 = c2_x0(B)
    x0[FAR] = X_FAR
    x0[SOC] = X_SOC
    return x0


def _solve_traced(ipm, x0, p):
    """ipm.solve and [(instance, filter size)] at every rejected trial point (the line that shortens the step)."""
    src, first = inspect.getsourcelines(DenseIpm.solve_data)
    rej = [first + i for i, ln in enumerate(src) if 'alpha[b] *= o.alpha_red' in ln]
    assert len(rej) == 1
    code, seen = DenseIpm.solve_data.__code__, []

    def local(frame, event, arg):
        if event == 'line' and frame.f_lineno == rej[0]:
            gb = int(frame.f_locals['gb'])
            seen.append((gb, len(frame.f_locals['filt'][gb])))
        return local

    old = sys.gettrace()
    sys.settrace(lambda frame, event, arg: local if frame.f_code is code else None)
    try:
        ref = ipm.solve(x0, p)
    finally:
        sys.settrace(old)
    return ref, seen


@pytest.fixture(scope='module')
def oracle20():
    ipm = DenseIpm(oracle_problem(C2))
    ref, seen = _solve_traced(ipm, _batch(), C2['p'])
    return ipm, ref, seen


@pytest.fixture(scope='module')
def product20():
    nmpc = product_nmpc(C2)
    u = nmpc.optimize(_batch(), cp=C2['p'])
    st = nmpc.stats()
    sol = {k: nmpc._nlp_solution[k].cpu().numpy().copy() for k in ('x', 'f', 'lam_g', 'status', 'iter_count', 'kkt_error')}
    return dict(u=np.asarray(u).copy(), status=nmpc.solver_status_code.copy(), iters=np.asarray(st['iter_count']).copy(),
                kkt=np.asarray(st['kkt_error']).copy(), sol=sol)


def _ncap():
    from hilo_mpc_amd import _lib
    n, a, b = C.c_int(), C.c_longlong(), C.c_longlong()
    _lib.check(_lib.lib().hilo_nmpc_layout_capacity(3, 0, C.byref(n), C.byref(a), C.byref(b)))
    return n.value


def _assert_like_test_nmpc_gpu(got, ipm, ref, rows):
    assert np.array_equal(got['status'][rows], ref['status'][rows])
    assert np.all(got['kkt'][rows] <= 1e-8)
    v, vr = got['sol']['x'][rows], ipm.to_v(ref)[rows]
    err = np.max(np.abs(v - vr) / np.maximum(1., np.abs(vr)))
    print('v', err, 'u0', np.max(np.abs(got['u'][rows] - ref['u0'][rows])), 'f', np.max(np.abs(got['sol']['f'][rows] / ref['f'][rows] - 1)))
    assert err < 1e-6
    np.testing.assert_allclose(got['u'][rows], ref['u0'][rows], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(got['sol']['f'][rows], ref['f'][rows], rtol=1e-8)


@pytest.mark.parametrize('N', [1, 2, 3])
def test_minimal_horizons(N):
    spec = dict(C2, N=N)
    x0 = c2_x0(B)
    ref = DenseIpm(oracle_problem(spec)).solve(x0, spec['p'])
    nmpc = product_nmpc(spec)
    u = nmpc.optimize(x0, cp=spec['p'])
    print('status', nmpc.solver_status_code.tolist(), ref['status'].tolist(), 'iterations', nmpc.stats()['iter_count'].tolist(), ref['iters'].tolist())
    assert np.array_equal(nmpc.solver_status_code, ref['status'])
    assert np.array_equal(nmpc.stats()['iter_count'], ref['iters'])
    np.testing.assert_allclose(u, ref['u0'], rtol=1e-9, atol=1e-12)


def test_benchmark_horizon(oracle20, product20):
    ipm, ref, _ = oracle20
    rows = [r for r in range(B) if r not in (FAR, SOC)]
    assert np.all(ref['status'] == 1)
    _assert_like_test_nmpc_gpu(product20, ipm, ref, rows)


def test_horizon_beyond_the_capacity_layout():
    N = _ncap() + 1
    spec = dict(C2, N=N)
    x0 = c2_x0(B)
    ipm = DenseIpm(oracle_problem(spec))
    ref = ipm.solve(x0, spec['p'])
    nmpc = product_nmpc(spec)
    u = nmpc.optimize(x0, cp=spec['p'])
    st = nmpc.stats()
    got = dict(u=np.asarray(u), status=nmpc.solver_status_code, kkt=np.asarray(st['kkt_error']),
               sol={k: nmpc._nlp_solution[k].cpu().numpy() for k in ('x', 'f')})
    assert np.all(ref['status'] == 1)
    _assert_like_test_nmpc_gpu(got, ipm, ref, list(range(B)))


def test_rejected_trial_points_with_a_full_filter(oracle20, product20):
    _, ref, seen = oracle20
    sizes = [n for b, n in seen if b == FAR]
    print('oracle: filter sizes at the rejected trial points of the far start', sizes, 'iterations', int(ref['iters'][FAR]),
          'product iterations', int(product20['iters'][FAR]), 'status', int(product20['status'][FAR]), int(ref['status'][FAR]))
    assert sizes and max(sizes) >= 3                 # the premise, from the oracle alone
    assert ref['n_resto'][FAR] == 0
    assert product20['status'][FAR] == ref['status'][FAR]
    assert product20['iters'][FAR] == ref['iters'][FAR]


def test_second_order_correction(oracle20, product20):
    _, ref, _ = oracle20
    print('oracle: corrections', int(ref['n_soc'][SOC]), 'iterations', int(ref['iters'][SOC]), 'product iterations', int(product20['iters'][SOC]),
          'status', int(product20['status'][SOC]), int(ref['status'][SOC]))
    assert ref['n_soc'][SOC] >= 1                    # the premise, from the oracle alone
    assert product20['status'][SOC] == ref['status'][SOC]
    assert product20['iters'][SOC] == ref['iters'][SOC]


def test_nan_parameter_is_status_minus_one_and_leaves_its_neighbours_alone(product20):
    p = np.tile(C2['p'], (B, 1))
    p[2, 0] = np.nan
    nmpc = product_nmpc(C2)
    nmpc.optimize(_batch(), cp=p)
    st = nmpc.solver_status_code
    assert st[2] == -1
    others = [r for r in range(B) if r != 2]
    for k, want in product20['sol'].items():
        got = nmpc._nlp_solution[k].cpu().numpy()
        assert np.ascontiguousarray(got[others]).tobytes() == np.ascontiguousarray(want[others]).tobytes(), k
