"""GPU tests of the solve kernel's load section (problem constants, parameter row and warm start into LDS), of the values it forms
once per solve for one instance, and of the NaN handling of its wave reductions.

Tolerances are those of tests/test_nmpc_gpu.py for the same quantities: both solvers stop at a scaled KKT
error of 1e-8, so primal solutions agree to 1e-6 relative (5e-5 where x_0 is free: tests/test_gen_gpu.py), inputs to
rtol 1e-6 / atol 1e-7, the objective to 1e-8, multipliers to rtol 1e-5 / atol 1e-6 (rtol 2e-4 / atol 1e-5 against the general
oracle of the free-x_0 case, as in tests/test_gen_gpu.py); status codes are compared exactly, iteration
counts exactly at N = 1 (identical iterate paths on short horizons) and within 10 in the mean otherwise.  Batch composition,
order and the phase profile must not change a single bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle.nmpc import DenseIpm                                                       # noqa: E402
from tests.problems import C2, c2_x0, oracle_gen, oracle_problem, product_nmpc          # noqa: E402

import functools                                                                       # noqa: E402

B3 = 3
U_UB = np.array([.3, .6, .3])                # per-instance input limits of the per-call bounds case
# N: slots SL = (N + 1) * 6 a wave of 64 lanes loads in trips of 64 -> 12 (one partial trip, odd horizon), 72 (second trip partial),
# 126 (the benchmark's shape), 138 (a third trip)
HORIZONS = [1, 11, 20, 22]


def _scaled_err(v, vr):
    return np.max(np.abs(v - vr) / np.maximum(1., np.abs(vr)))


@functools.lru_cache(maxsize=None)
def _cold(N):
    """The oracle's cold solve of horizon N, computed once for the tests that need it (never modified)."""
    spec = dict(C2, N=N)
    pb = oracle_problem(spec)
    ipm = DenseIpm(pb)
    ref = ipm.solve(c2_x0(B3), spec['p'])
    assert np.all(ref['status'] == 1)
    return spec, pb, ipm, ref


def _lam_ref(pb, ref):
    """The oracle's multipliers of the shooting constraints in the product's convention: L = f + lam^T g, terminal term on
    Phi_{N-1} (tests/test_nmpc_gpu.py)."""
    lam = ref['lam'].copy()
    lam[:, -pb.nx:] += 2 * (ref['X'][:, -1] - pb.xrefN) @ pb.WN
    return lam


def _same_iterations(N, got, want):
    if N == 1:
        assert np.array_equal(got, want)          # short horizons: identical iterate paths (tests/test_nmpc_gpu.py)
    assert abs(int(got.mean()) - int(want.mean())) <= 10


@pytest.mark.parametrize('N', HORIZONS)
def test_loader_cold_start_pinned_x0_vs_oracle(N):
    spec, pb, ipm, ref = _cold(N)
    x0 = c2_x0(B3)
    nmpc = product_nmpc(spec)
    u = nmpc.optimize(x0, cp=spec['p'])
    st = nmpc.stats()
    assert np.array_equal(nmpc.solver_status_code, ref['status'])
    assert np.all(st['kkt_error'] <= 1e-8)
    _same_iterations(N, st['iter_count'], ref['iters'])
    assert _scaled_err(nmpc._nlp_solution['x'].cpu().numpy(), ipm.to_v(ref)) < 1e-6
    np.testing.assert_allclose(u, ref['u0'], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(nmpc._nlp_solution['f'].cpu().numpy(), ref['f'], rtol=1e-8)
    np.testing.assert_allclose(nmpc._nlp_solution['lam_g'].cpu().numpy(), _lam_ref(pb, ref), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize('N', HORIZONS)
def test_loader_warm_start_vs_oracle(N):
    """Closed-loop step 2: the start vector is the previous solution (mpc.py:725-726), x_0 follows the new measurement."""
    spec, pb, ipm, ref = _cold(N)
    x0 = c2_x0(B3)
    x1 = pb.phi(x0 / pb.sx, ref['U'][:, 0], spec['p']) * pb.sx
    ref2 = ipm.solve(x1, spec['p'], w0=ref['w'])
    nmpc = product_nmpc(spec)
    nmpc.optimize(x0, cp=spec['p'])
    cold_iters = nmpc.stats()['iter_count']
    u2 = nmpc.optimize(x1, cp=spec['p'])
    assert np.array_equal(nmpc.solver_status_code, ref2['status']) and np.all(ref2['status'] == 1)
    np.testing.assert_allclose(u2, ref2['u0'], rtol=1e-6, atol=1e-7)
    assert _scaled_err(nmpc._nlp_solution['x'].cpu().numpy(), ipm.to_v(ref2)) < 1e-6
    np.testing.assert_allclose(nmpc._nlp_solution['f'].cpu().numpy(), ref2['f'], rtol=1e-8)
    np.testing.assert_allclose(nmpc._nlp_solution['lam_g'].cpu().numpy(), _lam_ref(pb, ref2), rtol=1e-5, atol=1e-6)
    assert abs(int(nmpc.stats()['iter_count'].mean()) - int(ref2['iters'].mean())) <= 10
    if N > 1:
        assert nmpc.stats()['iter_count'].mean() < cold_iters.mean()         # the start vector was really read


@pytest.mark.parametrize('N', HORIZONS)
def test_loader_bounds_of_the_call_vs_oracle(N):
    """`optimize(v_lb=, v_ub=)`: one input limit per instance, against the oracle set up with that limit."""
    spec = dict(C2, N=N)
    x0 = c2_x0(B3)
    nmpc = product_nmpc(spec)
    lb, ub = (a.cpu().numpy() for a in nmpc._v_bounds())
    LB, UB = np.tile(lb, (B3, 1)), np.tile(ub, (B3, 1))
    for b in range(B3):
        for k in range(N):
            UB[b, nmpc._u_ind[k]] = U_UB[b]
    u = nmpc.optimize(x0, cp=spec['p'], v_lb=LB, v_ub=UB)
    v, lam = nmpc._nlp_solution['x'].cpu().numpy(), nmpc._nlp_solution['lam_g'].cpu().numpy()
    for lim in np.unique(U_UB):
        rows = np.flatnonzero(U_UB == lim)
        pb = oracle_problem(dict(spec, u_ub=[lim, lim]))
        ipm = DenseIpm(pb)
        ref = ipm.solve(x0[rows], spec['p'])
        np.testing.assert_allclose(lam[rows], _lam_ref(pb, ref), rtol=1e-5, atol=1e-6)
        assert np.all(ref['status'] == 1) and np.array_equal(nmpc.solver_status_code[rows], ref['status'])
        np.testing.assert_allclose(u[rows], ref['u0'], rtol=1e-6, atol=1e-7)
        assert _scaled_err(v[rows], ipm.to_v(ref)) < 1e-6
        assert abs(int(nmpc.stats()['iter_count'][rows].mean()) - int(ref['iters'].mean())) <= 10
    assert np.all(u <= U_UB[:, None] * (1 + 1e-7))


@pytest.mark.parametrize('N', HORIZONS)
def test_loader_free_initial_state_with_its_own_box_vs_oracle(N):
    from oracle.nmpc_gen import GenIpm
    spec = dict(C2, N=N, x_lb=[1., 10., 0., 0.], x_ub=[8., 60., 5., 20.], x_guess=[4., 30., 1., 5.])
    box = ([2., 20., 0., 1.], [3., 35., 2., 8.])
    x0 = c2_x0(B3)
    pb = oracle_gen(spec)
    ipm = GenIpm(pb, free_x0=True, x0_box=box)
    ref = ipm.solve(x0, spec['p'])
    assert np.all(ref['status'] == 1)
    nmpc = product_nmpc(spec)
    u = nmpc.optimize(x0, cp=spec['p'], fix_x0=False, x0_lb=box[0], x0_ub=box[1])
    v, vr = nmpc._nlp_solution['x'].cpu().numpy(), ipm.to_v(ref)
    assert np.array_equal(nmpc.solver_status_code, ref['status'])
    assert _scaled_err(v, vr) < 5e-5
    np.testing.assert_allclose(nmpc._nlp_solution['f'].cpu().numpy(), ref['f'], rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(u, ref['u0'], rtol=5e-5, atol=5e-5)
    # multipliers: the tolerance tests/test_gen_gpu.py states for this oracle (its primal tolerance is 5e-5, the multipliers of two
    # solves that far apart cannot be asked to agree to 1e-5)
    lam = ipm.lam_g(ref).reshape(B3, pb.N, -1)
    lam[:, -1, :pb.nxa] += 2 * (ref['X'][:, -1] - pb.xrefNa) @ pb.WNa          # terminal cost on Phi_{N-1} (mpc.py:1682)
    np.testing.assert_allclose(nmpc._nlp_solution['lam_g'].cpu().numpy(), lam.reshape(B3, -1), rtol=2e-4, atol=1e-5)
    assert np.all(v[:, :4] >= np.array(box[0]) - 1e-6) and np.all(v[:, :4] <= np.array(box[1]) + 1e-6)
    assert abs(int(nmpc.stats()['iter_count'].mean()) - int(ref['iters'].mean())) <= 10


# ---- values formed once per solve belong to ONE instance ------------------------------------------------------------------------
SCALED = dict(C2, x_scaling=[.1, 40., 2., 1.], u_scaling=[2., 2.])
P4 = np.array([[100., 4., 1., 0.], [90., 5., 1.1, .1], [110., 3., .9, .2], [95., 4.5, 1.05, .05]])
KEYS = ('x', 'f', 'lam_g')


def _solve(x0, p, profile=False):
    nmpc = product_nmpc(SCALED)
    if profile:
        nmpc.phase_profile(True)
    u = nmpc.optimize(x0, cp=p)
    out = {k: nmpc._nlp_solution[k].cpu().numpy().copy() for k in KEYS}
    out.update(u=np.array(u), status=np.array(nmpc.solver_status_code), iters=np.array(nmpc.stats()['iter_count']))
    if profile:
        pr = nmpc.phase_profile(False)
        ends = nmpc.phase_profile_ends()
        assert pr['derivatives'] > 0 and ends['setup'] > 0 and ends['finish'] > 0
    return out


def _assert_same_bits(a, b, rows=slice(None), rows_b=slice(None)):
    for k in a:
        np.testing.assert_array_equal(a[k][rows], b[k][rows_b], err_msg=k)


def test_per_instance_values_are_per_instance():
    x0 = c2_x0(4)
    batch = _solve(x0, P4)
    assert np.all(batch['status'] == 1)
    assert len({batch['u'][b].tobytes() for b in range(4)}) == 4             # four different problems
    for b in range(4):
        _assert_same_bits(_solve(x0[b:b + 1], P4[b:b + 1]), batch, rows_b=slice(b, b + 1))
    rev = _solve(x0[::-1].copy(), P4[::-1].copy())
    _assert_same_bits({k: a[::-1] for k, a in rev.items()}, batch)
    _assert_same_bits(_solve(x0, P4, profile=True), batch)


# ---- a NaN anywhere in the iterate ends in status -1, and only in that instance ----------------------------------------------------
def test_nan_ends_in_status_minus_one_and_only_there():
    # the state P without a lower bound: the start's push into the interior (fmax / fmin) drops a NaN in a bounded slot
    spec = dict(C2, x_lb=[0., 0., -np.inf, 0.])
    N = spec['N']
    x0 = c2_x0(B3)
    nm = product_nmpc(spec)
    v0 = nm._guess_vector(B3).cpu().numpy().copy()

    def run(x, v):
        n = product_nmpc(spec)
        n.optimize(x, cp=spec['p'], v0=v)
        out = {k: n._nlp_solution[k].cpu().numpy().copy() for k in KEYS}
        out.update(status=np.array(n.solver_status_code), iters=np.array(n.stats()['iter_count']))
        return out

    clean = run(x0, v0)
    assert np.all(clean['status'] == 1)
    # one late slot of the start vector, stage N: slot N * 6 + 2 = 122 of the kernel's layout, a single lane's partial in the
    # first reduction
    vn = v0.copy()
    vn[1, nm._x_ind[N][2]] = np.nan
    got = run(x0, vn)
    assert got['status'][1] == -1
    _assert_same_bits({k: np.delete(a, 1, axis=0) for k, a in got.items()}, {k: np.delete(a, 1, axis=0) for k, a in clean.items()})
    # the measurement
    xn = x0.copy()
    xn[2, 1] = np.nan
    got = run(xn, v0)
    assert got['status'][2] == -1
    _assert_same_bits({k: np.delete(a, 2, axis=0) for k, a in got.items()}, {k: np.delete(a, 2, axis=0) for k, a in clean.items()})
