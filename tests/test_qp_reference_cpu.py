"""The inputs of tests/test_qp_gpu.py, pinned without a GPU: the oracle (oracle.lmpc.solve_qp, tol = reg = 1e-12) alone solves
EVERY instance of every case - status 1, the KKT conditions within the limits the device results are held to
(tests/qp_reference.py), at most 40 iterations - so no GPU case has a reason to leave an instance out.  Plus the self-tests of
the generators and of the KKT report."""
import numpy as np
import pytest

from tests import qp_reference as qr


def _check_oracle(qps, refs, label, compared=True):
    margins = []
    for i, (qp, ref) in enumerate(zip(qps, refs)):
        assert ref['status'] == 1, f"{label}: instance {i} has status {ref['status']}"
        assert ref['iters'] <= 40, f"{label}: instance {i} took {ref['iters']} iterations"
        margins.append(qr.kkt_margins(qp, ref['x'], ref['lam_a'], ref['lam_x'], polished=True))
    gap = min(qr.complementarity_margin(qp, ref) for qp, ref in zip(qps, refs))
    print(f"{label}: iterations <= {max(r['iters'] for r in refs)}; {qr.fmt(qr.worst(margins))}; "
          f"complementarity margin {gap:.2e} (at least {qr.MARGIN:.0e})")
    assert gap >= qr.MARGIN or not compared        # (only where the GPU tests compare x and lam_a with the oracle)
    for i, mg in enumerate(margins):
        assert qr.kkt_ok(mg), f"{label}: instance {i}: {qr.fmt(mg)}"


@pytest.mark.parametrize('n,m,kind,bounds', qr.DENSE_CASES)
def test_oracle_solves_every_general_qp(n, m, kind, bounds):
    qps, refs = qr.dense_batch(n, m, kind, bounds)
    assert len(qps) == qr.DENSE_BATCH
    _check_oracle(qps, refs, f"({n},{m}) {kind} {bounds}")
    active = sum(qr.active_bounds(qp, ref['x']) for qp, ref in zip(qps, refs))
    for qp in qps:
        fixed = qp['lb'] == qp['ub']
        assert np.all(qp['lb'][~fixed] < qp['x_f'][~fixed]) and np.all(qp['x_f'][~fixed] < qp['ub'][~fixed])
        assert (bounds == 'fixed') == bool(fixed.any()) and n - fixed.sum() > m - (n == m)
        if kind == 'diag':
            assert np.count_nonzero(qp['H'] - np.diag(np.diag(qp['H']))) == 0
    if bounds == 'none':
        assert all(not np.isfinite(qp['lb']).any() and not np.isfinite(qp['ub']).any() for qp in qps)
    elif m == n:
        # (1, 1): the row alone determines x = x_f, strictly inside every bound - no bound can be active here
        assert active == 0 and all(abs(ref['x'][0] - qp['x_f'][0]) < 1e-9 for qp, ref in zip(qps, refs))
    else:
        assert active >= 1
    if bounds != 'none' and n >= 7:
        kinds ={(bool(np.isfinite(l)), bool(np.isfinite(u))) for qp in qps for l, u in zip(qp['lb'], qp['ub']) if l != u}
        assert kinds == {(True, True), (True, False), (False, True), (False, False)}      # all four branches of the bound handling


@pytest.mark.parametrize('nx,nu,N', qr.STAGE_CASES)
def test_oracle_solves_every_stage_qp(nx, nu, N):
    qps, refs = qr.stage_batch(nx, nu, N)
    _check_oracle(qps, refs, f"nx={nx} nu={nu} N={N}")
    n = (N + 1) * nx + N * nu
    uo = (N + 1) * nx
    assert sum(int((np.abs(np.abs(ref['x'][uo:]) - 1.0) <= 1e-9).sum()) for ref in refs) >= 1     # an input bound is active
    for qp in qps:
        assert qp['H'].shape == (n, n) and qp['A'].shape == (N * nx, n) and np.any(qp['b'] != 0)
        assert np.array_equal(qp['lb'][:nx], qp['ub'][:nx]) and np.all(qp['lb'][nx:] < qp['ub'][nx:])
        for k in range(N):
            assert np.abs(np.linalg.eigvals(qp['Ak'][k])).max() <= 1.05 + 1e-12
            r = slice(k * nx, (k + 1) * nx)
            np.testing.assert_array_equal(qp['A'][r, k * nx:(k + 1) * nx], qp['Ak'][k])
            np.testing.assert_array_equal(qp['A'][r, uo + k * nu:uo + (k + 1) * nu], qp['Bk'][k])
            np.testing.assert_array_equal(qp['A'][r, (k + 1) * nx:(k + 2) * nx], -np.eye(nx))
        # nothing outside the stage blocks
        mask = np.zeros((n, n), dtype=bool)
        for k in range(N + 1):
            mask[k * nx:(k + 1) * nx, k * nx:(k + 1) * nx] = True
        for k in range(N):
            mask[uo + k * nu:uo + (k + 1) * nu, uo + k * nu:uo + (k + 1) * nu] = True
        assert np.count_nonzero(qp['H'][~mask]) == 0 and np.all(np.linalg.eigvalsh(qp['H']) >= 0.5 - 1e-12)


def test_oracle_solves_the_refused_horizon():
    qps, refs = qr.stage_batch(1, 1, 64, 2)
    _check_oracle(qps, refs, "nx=1 nu=1 N=64")
    assert qps[0]['H'].shape == (129, 129) and qps[0]['A'].shape == (64, 129)
    assert qr.dense_working_set_bytes(129, 64) > 160 * 1024


def test_oracle_solves_the_fixed_input_batch():
    """The batch of test_stage_kernel_refuses_a_fixed_input_for_that_instance_only: a fixed input leaves the QP solvable."""
    qps = qr.stage_problems(2, 1, 15, 8)
    j = 16 * 2 + 3
    lb, ub = qps[5]['lb'].copy(), qps[5]['ub'].copy()
    lb[j] = ub[j] = qps[5]['x_f'][j]
    mixed = list(qps)
    mixed[5] = dict(qps[5], lb=lb, ub=ub)
    assert -1 < lb[j] < 1
    _check_oracle(mixed, [qr.oracle_solve(q) for q in mixed], "nx=2 nu=1 N=15, one input fixed", compared=False)


@pytest.mark.parametrize('case', qr.CONTAINMENT_DENSE + qr.CONTAINMENT_STAGE)
def test_containment_batches(case):
    """The clean batch is solved by the oracle like every other input; of the four edited instances the oracle can judge the
    infeasible one (status 3 by OOQP's rule within 15 iterations); the others differ from their clean twins as described."""
    dense = len(case) == 3 and isinstance(case[2], str)
    clean, bad, idx = qr.containment_dense(*case) if dense else qr.containment_stage(*case)
    assert len(clean) == len(bad) == 9 and idx == ((2, 4, 6, 7) if dense else (2, 4, 6))
    _check_oracle(clean, [qr.oracle_solve(q) for q in clean], f"containment {case}", compared=False)
    for i in range(9):
        assert (bad[i] is clean[i]) == (i not in idx)
    q = bad[qr.BAD_INFEASIBLE]
    ref = qr.oracle_solve(q)
    print(f"containment {case}: infeasible instance: oracle status {ref['status']} after {ref['iters']} iterations")
    assert ref['status'] == 3 and ref['iters'] <= 15
    q, c = bad[qr.BAD_NAN_G], clean[qr.BAD_NAN_G]
    k = np.nonzero(np.isnan(q['g']))[0]
    assert k.size == 1 and c['lb'][k[0]] != c['ub'][k[0]] and (dense or k[0] >= (case[2] + 1) * case[0])
    q, c = bad[qr.BAD_ROW], clean[qr.BAD_ROW]
    assert (q['b_hi'] != q['b']).sum() == 1 and np.array_equal(q['b'], c['b'])
    if dense:
        q = bad[qr.BAD_INDEFINITE]
        j = np.nonzero(np.diag(q['H']) < 0)[0]
        assert j.size == 1 and q['lb'][j[0]] == -np.inf and q['ub'][j[0]] == np.inf


def test_batches_are_deterministic_and_read_only():
    a, _ = qr.dense_batch(7, 3, 'dense', 'fixed')
    rng = np.random.default_rng(qr.case_seed(7, 3, 'dense', 'fixed'))
    again = qr.random_qp(7, 3, rng, kind='dense', bounds='fixed')
    for key in again:
        np.testing.assert_array_equal(a[0][key], again[key])
    with pytest.raises(ValueError):
        a[0]['H'][0, 0] = 1.0
    assert qr.dense_batch(7, 3, 'dense', 'fixed')[0] is a


def test_kernel_selection_of_the_cases():
    """The helper's picture of hilo_qp_create: every register-kernel instantiation, the LDS-column kernel and the workspace are
    among the general cases; both stage variants and a workspace twin among the stage cases."""
    sel = {qr.register_kernel(n, m) for (n, m) in qr.DENSE_SIZES}
    assert sel == {(32, 24), (32, 32), (64, 48), None}
    big = [(n, m) for (n, m) in qr.DENSE_SIZES if qr.dense_working_set_bytes(n, m) > 160 * 1024]
    assert big == [(96, 8)]
    assert qr.register_kernel(64, 48) == (64, 48) and qr.register_kernel(64, 49) is None and qr.register_kernel(50, 49) is None
    assert qr.register_kernel(32, 24) == (32, 24) and qr.register_kernel(32, 25) == (32, 32) and qr.register_kernel(33, 24) == (64, 48)
    assert qr.stage_batch_size(1, 1, 15) == 8 and qr.stage_batch_size(4, 2, 15) == 4 and qr.stage_batch_size(1, 1, 63) == 4


def test_kkt_report_rejects_perturbed_solutions():
    qps, refs = qr.dense_batch(32, 28, 'dense', 'fixed')
    rejected_sign = 0
    for qp, ref in zip(qps, refs):
        assert qr.kkt_ok(qr.kkt_margins(qp, ref['x'], ref['lam_a'], ref['lam_x'], polished=True))
        free = np.nonzero(qp['lb'] != qp['ub'])[0]
        for i in (free[0], free[-1]):
            x = ref['x'].copy()
            x[i] += 1e-9
            mg = qr.kkt_margins(qp, x, ref['lam_a'], ref['lam_x'])
            assert not qr.kkt_ok(mg) and mg['stat'][0] > mg['stat'][1]
        # one multiplier of an active bound with its sign flipped: stationarity, and sign or complementarity
        act = [i for i in free if abs(ref['lam_x'][i]) > 1e-3]
        if act:
            lam_x = ref['lam_x'].copy()
            lam_x[act[0]] = -lam_x[act[0]]
            mg = qr.kkt_margins(qp, ref['x'], ref['lam_a'], lam_x)
            assert not qr.kkt_ok(mg)
            assert mg['sign'][0] > 0 or mg['comp'][0] > mg['comp'][1]
            rejected_sign += 1
        y = ref['lam_a'].copy()
        y[0] += 1e-9
        assert not qr.kkt_ok(qr.kkt_margins(qp, ref['x'], y, ref['lam_x']))
    assert rejected_sign >= 1


def test_kkt_report_of_a_hand_made_problem():
    """min 1/2 x^2 - 2 x, x <= 1: x = 1 with lam_x = 1; x slightly outside, or lam_x at a lower bound that is not there, fail."""
    qp = dict(H=np.array([[1.0]]), g=np.array([-2.0]), A=np.zeros((0, 1)), b=np.zeros(0), lb=np.array([-np.inf]), ub=np.array([1.0]))
    e = np.zeros(0)
    assert qr.kkt_ok(qr.kkt_margins(qp, np.array([1.0]), e, np.array([1.0])))
    assert qr.kkt_margins(qp, np.array([1.0 + 1e-12]), e, np.array([1.0]))['bound'][0] > 0
    assert qr.kkt_margins(qp, np.array([0.5]), e, np.array([1.5]))['comp'][0] == pytest.approx(0.75)
    qp2 = dict(qp, g=np.array([2.0]))                                        # minimum at -2, no bound there
    assert qr.kkt_ok(qr.kkt_margins(qp2, np.array([-2.0]), e, np.array([0.0])))
    assert qr.kkt_margins(qp2, np.array([-1.0]), e, np.array([-1.0]))['sign'][0] == pytest.approx(1.0)
