"""GPU: the seams of the tracking solve's iteration (csrc/hilo_ocp.h) -
* the cost section of eval_derivs_sym: free-slot test from scalar registers, the terminal gradient formed by every lane next to the
  reads of cost_cols (csrc/hilo_nmpc_track.h::term_cols), only the gradient stores under a condition;
* the right-hand side grad - mu q behind the barrier update (finish_rhs), with one and with two trips of its slot loop;
* the accepted trial point's defects copied by the update phase instead of a pass in front of the derivative phase.

Terminal-cost cases: symbolic path against the Taylor path of the SAME build, with the mechanism and the measure of
tests/test_sym_phase_gpu.py (cold and warm solve, equal `status` and `iter_count`, scaled difference d of `x`, `f`, `lam_g`).  The
terminal cost has a different weight and reference on every state, so that a swapped row or column of its gradient shows.  The
tolerance is measured, not chosen: the largest d over the cases of TERM_CASES, both steps and the three arrays is 7.106e-15 on the
parent commit cfe2cb6 ("Cut the per-launch and per-phase fixed costs of the tracking NMPC solve"), run with this very file:
chemostat4, N = 1, warm step, `lam_g`; every case has equal `status` and `iter_count` there.  TOL is ten times that figure.  The
per-case figures of the parent and of this code are in profiles/seams_sym_vs_taylor.txt.

Right-hand-side cases: against the oracle's dense interior-point solver with the tolerances of DESIGN 6 at the default `tol`
(status codes exact, objective 1e-8 relative, primal solution 5e-5 scaled, multipliers of the defects rtol 1e-5 / atol 1e-6 as in
tests/test_nmpc_gpu.py::test_c2_cold_and_warm_vs_oracle) and equal iteration counts.
"""
import numpy as np
import pytest

import tests.test_sym_phase_gpu as sp
from tests.problems import C2, c2_x0, oracle_problem, product_nmpc

pytestmark = pytest.mark.gpu

PARENT_MAX = 7.106e-15
TOL = 10 * PARENT_MAX

TERM = [([0, 1, 2, 3], [.3, .001, 10., .2], [.1, 40., 2., 0.])]
TERM_CASES = {
    # N = 1: pin and terminal store on the same lanes; 2: the two apart; 21: one full pass of the wave; 22: the last interval alone
    'chemostat4-N1': dict(C2, N=1, terminal_states=TERM), 'chemostat4-N2': dict(C2, N=2, terminal_states=TERM),
    'chemostat4-N21': dict(C2, N=21, terminal_states=TERM), 'chemostat4-N22': dict(C2, N=22, terminal_states=TERM),
    # NZ = 5: the third lane of an interval owns one real column and one beyond NZ
    'pendulum4': dict(sp.PENDULUM, terminal_states=[([0, 1, 2, 3], [10., .5, 5., .2], [.1, 0., .05, 0.])]),
    # NZ = 4, scaled variables
    'cstr3': dict(sp.CSTR3, terminal_states=[([0, 1, 2], [1., .5, 1e-4], [.45, .55, 440.])]),
    # interval-0 branch of the cost columns, pin and terminal store in the same lanes
    'chemostat4-N1-du': dict(C2, N=1, terminal_states=TERM, input_change=([0, 1], [.5, .5])),
}


def _sym_vs_taylor(spec, x0, rows=None):
    sym, x1 = sp._two_steps(spec, x0, taylor=False)
    tay, _ = sp._two_steps(spec, x0, taylor=True, x1=x1)
    worst = 0.
    for step, (a, b) in enumerate(zip(sym, tay)):
        d = {k: sp._scaled_diff(a[k], b[k], rows) for k in sp.KEYS}
        print(f"step {step}: status {a['status'].tolist()} / {b['status'].tolist()}  iter_count {a['iter_count'].tolist()} / "
              f"{b['iter_count'].tolist()}  scaled differences {d}")
        worst = max(worst, max(d.values()))
    return sym, tay, worst


@pytest.mark.parametrize('case', list(TERM_CASES))
def test_terminal_gradient_symbolic_path_equals_taylor_path(case):
    spec = TERM_CASES[case]
    sym, tay, worst = _sym_vs_taylor(spec, sp._x0(spec['model'])[:5])
    print(f"{case}: largest scaled difference {worst:.3e} (TOL {TOL:.3e})")
    for step, (a, b) in enumerate(zip(sym, tay)):
        assert np.all(a['status'] == 1), (case, step)
        assert np.array_equal(a['status'], b['status']), (case, step)
        assert np.array_equal(a['iter_count'], b['iter_count']), (case, step)
    assert worst <= TOL, (case, worst)


def test_nan_state_reaches_the_error_measure_through_the_predicated_stores():
    """A NaN in x0 of one instance ends in status -1 for that instance on both paths; the others are not touched."""
    x0 = c2_x0(5)
    x0[3, 1] = np.nan
    ok = np.array([0, 1, 2, 4])
    sym, tay, worst = _sym_vs_taylor(dict(C2, terminal_states=TERM), x0, ok)
    for a, b in zip(sym, tay):
        assert a['status'][3] == -1 and b['status'][3] == -1
        assert np.all(a['status'][ok] == 1) and np.array_equal(a['status'], b['status'])
        assert np.array_equal(a['iter_count'][ok], b['iter_count'][ok])
    assert worst <= TOL, worst


RHS_CASES = {
    'N20': (dict(C2), slice(0, 3)),              # (N + 1) NZ = 126: one trip of the slot loops (two slots per lane)
    'N21': (dict(C2, N=21), slice(0, 3)),        # 132: two trips
    # input limit of tests/test_nmpc_gpu.py::test_bounds_of_the_solver_call_per_instance_and_per_call on its instance: the cold
    # solve lowers the barrier parameter several times and accepts a second-order correction (one factorisation more than iterations)
    'N20-u_ub.3': (dict(C2, u_ub=[.3, .3]), slice(2, 5)),
}


@pytest.mark.parametrize('case', list(RHS_CASES))
def test_right_hand_side_paths_vs_oracle(case):
    from oracle.nmpc import DenseIpm
    spec, rows = RHS_CASES[case]
    x0 = c2_x0(5)[rows]
    pb = oracle_problem(spec)
    ipm = DenseIpm(pb)
    ref = ipm.solve(x0, spec['p'])
    nmpc = product_nmpc(spec)
    nmpc.phase_profile(True)
    nmpc.optimize(x0, cp=spec['p'])
    prof = nmpc.phase_profile(True)
    sol = {k: nmpc._nlp_solution[k].cpu().numpy() for k in sp.KEYS + ('status', 'iter_count')}
    vr = ipm.to_v(ref)
    lam_ref = ref['lam'].copy()
    lam_ref[:, -pb.nx:] += 2 * (ref['X'][:, -1] - pb.xrefN) @ pb.WN     # terminal term on Phi_{N-1} in the reference's g
    dx = float(np.max(np.abs(sol['x'] - vr) / np.maximum(1., np.abs(vr))))
    df = float(np.max(np.abs(sol['f'] - ref['f']) / np.abs(ref['f'])))
    dl = float(np.max(np.abs(sol['lam_g'] - lam_ref) / (1e-6 + 1e-5 * np.abs(lam_ref))))
    print(f"{case}: status {sol['status'].tolist()} / {ref['status'].tolist()}  iter_count {sol['iter_count'].tolist()} / "
          f"{ref['iters'].tolist()}  n_soc (oracle) {ref['n_soc'].tolist()}  factorisations of instance 0 {prof['n_factorizations']}  "
          f"x {dx:.3e} (5e-5)  f {df:.3e} (1e-8)  lam_g in units of its tolerance {dl:.3e}")
    assert np.all(ref['status'] == 1) and np.array_equal(sol['status'], ref['status'])
    assert np.array_equal(sol['iter_count'], ref['iters'])
    if case == 'N20-u_ub.3':
        assert ref['n_soc'][0] > 0 and prof['n_factorizations'] > sol['iter_count'][0]
    assert dx <= 5e-5
    np.testing.assert_allclose(sol['f'], ref['f'], rtol=1e-8)
    np.testing.assert_allclose(sol['lam_g'], lam_ref, rtol=1e-5, atol=1e-6)
