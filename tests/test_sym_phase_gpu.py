"""GPU: the symbolic-derivative path of the tracking solve (csrc/hilo_ocp.h::eval_derivs_sym and the SYM branch of eval_values_call)
against the Taylor path of the SAME build, on the smallest shapes where the symbolic path's lane map, its stage-0 shortcut (unit
seeds: no exchange of the tangent block) and its reads-first values pass can go wrong.

The two paths compute the same derivatives with different roundings, so `status` and `iter_count` must be equal and `x`, `f`,
`lam_g` agree to a tolerance.  The tolerance is measured, not chosen: the largest scaled difference
    d = max |a - b| / max(1, max |b|)
over all cases below, both steps and the three arrays is 1.079e-15 on the parent commit ba3d993 ("Add ANN: chained f64-MFMA batched
predict, neural terms in models", the last one before the stage-0 shortcut), run with this very file: chemostat4, N = 22, cold
step, `x`; every case has equal `status` and `iter_count` there.  The two paths take the same iterations from the same start, so
their results differ by roundings only.  TOL is ten times that figure.  The per-case figures of the parent and of this code are in
profiles/symtrim_sym_vs_taylor.txt.

`HILO_NMPC_TAYLOR` is read at every launch of a zoo model (csrc/hilo_nmpc.hip::nmpc_launch): it is set around the second solve only.
"""
import os

import numpy as np
import pytest

from tests.problems import C2, c2_x0, product_nmpc

pytestmark = pytest.mark.gpu

PARENT_MAX = 1.079e-15
TOL = 10 * PARENT_MAX

PENDULUM = dict(model='pendulum4', dt=.1, N=15, order=4, stage_states=[([0, 2], [10., 5.], [0., 0.])],
                stage_inputs=[([0], [.1], None)], terminal_states=[([0, 2], [10., 5.], [0., 0.])],
                u_lb=[-20.], u_ub=[20.], x_guess=[0., 0., 0., 0.], u_guess=[0.], p=[])
CSTR3 = dict(model='cstr3', dt=1., N=10, order=4, stage_states=[([0], [1.], [.45])], stage_inputs=[([0], [1e-12], None)],
             terminal_states=[([0], [1.], [.45])], x_lb=[0., 0., 400.], x_ub=[1., 1., 500.], u_lb=[0.], u_ub=[1e5],
             x_scaling=[1., 1., 1e2], u_scaling=[1e5], x_guess=[.4912, .5088, 438.47], u_guess=[59881.84], p=[])


def _x0(name):
    if name == 'pendulum4':
        return np.array([.5, 0., .3, 0.]) * (1 + .2 * np.random.default_rng(1).uniform(-1, 1, (16, 4)))
    if name == 'cstr3':
        return np.array([.6, .4, 430.]) * (1 + .02 * np.random.default_rng(2).uniform(-1, 1, (16, 3)))
    return c2_x0(5)


CASES = {
    # chemostat4: NZ = 6, three full lanes per interval, 21 intervals per pass of the wave
    'chemostat4-N1': dict(C2, N=1), 'chemostat4-N2': dict(C2, N=2), 'chemostat4-N20': dict(C2),
    'chemostat4-N21': dict(C2, N=21), 'chemostat4-N22': dict(C2, N=22),
    # stage 0 is the only stage, or feeds a10 / a20 / a21
    'chemostat4-order1': dict(C2, N=3, order=1), 'chemostat4-order2': dict(C2, N=3, order=2),
    'chemostat4-order3': dict(C2, N=3, order=3),
    'pendulum4': PENDULUM,          # NZ = 5: the third lane of an interval owns one real column
    'cstr3': CSTR3,                 # NZ = 4: two lanes per interval, scaled variables
    'chemostat4-du': dict(C2, input_change=([0, 1], [.5, .5])),   # interval-0 branch of the cost columns
}
KEYS = ('x', 'f', 'lam_g')


def _two_steps(spec, x0, taylor, x1=None):
    """Cold solve from x0, then one warm-started solve from x1 (default: the plant's answer to the first input)."""
    nmpc = product_nmpc(spec)
    p = spec['p'] or None
    out = []
    if taylor:
        os.environ['HILO_NMPC_TAYLOR'] = '1'
    try:
        u = nmpc.optimize(x0, cp=p)
        out.append({k: nmpc._nlp_solution[k].cpu().numpy().copy() for k in KEYS + ('status', 'iter_count')})
        if x1 is None:
            x1 = nmpc.plant_step(x0, u, cp=p).cpu().numpy()
        nmpc.optimize(x1, cp=p)
        out.append({k: nmpc._nlp_solution[k].cpu().numpy().copy() for k in KEYS + ('status', 'iter_count')})
    finally:
        os.environ.pop('HILO_NMPC_TAYLOR', None)
    return out, x1


def _scaled_diff(a, b, rows=None):
    if rows is not None:
        a, b = a[rows], b[rows]
    return float(np.max(np.abs(a - b)) / max(1., float(np.max(np.abs(b)))))


@pytest.mark.parametrize('case', list(CASES))
def test_symbolic_path_equals_taylor_path(case):
    spec = CASES[case]
    x0 = _x0(spec['model'])
    sym, x1 = _two_steps(spec, x0, taylor=False)
    tay, _ = _two_steps(spec, x0, taylor=True, x1=x1)
    worst = 0.
    for step, (a, b) in enumerate(zip(sym, tay)):
        d = {k: _scaled_diff(a[k], b[k]) for k in KEYS}
        print(f"{case} step {step}: status {a['status'].tolist()} / {b['status'].tolist()}  iter_count "
              f"{a['iter_count'].tolist()} / {b['iter_count'].tolist()}  scaled differences {d}")
        worst = max(worst, max(d.values()))
    print(f"{case}: largest scaled difference {worst:.3e} (TOL {TOL:.3e})")
    for step, (a, b) in enumerate(zip(sym, tay)):
        assert np.array_equal(a['status'], b['status']), (case, step)
        assert np.array_equal(a['iter_count'], b['iter_count']), (case, step)
    assert worst <= TOL, (case, worst)


def test_nan_state_ends_in_status_minus_one_on_both_paths():
    """A NaN in x0 reaches J_0 / H_0 of every interval's first stage through the stage points: the stage-0 shortcut must hand it on
    like the products did (status -1, IPOPT's Invalid_Number_Detected); the other instances of the batch are not touched."""
    x0 = _x0('chemostat4')
    x0[3, 1] = np.nan
    ok = np.array([0, 1, 2, 4])
    sym, x1 = _two_steps(dict(C2), x0, taylor=False)
    tay, _ = _two_steps(dict(C2), x0, taylor=True, x1=x1)
    worst = 0.
    for step, (a, b) in enumerate(zip(sym, tay)):
        d = {k: _scaled_diff(a[k], b[k], ok) for k in KEYS}
        print(f"nan step {step}: status {a['status'].tolist()} / {b['status'].tolist()}  iter_count {a['iter_count'].tolist()} / "
              f"{b['iter_count'].tolist()}  scaled differences {d}")
        worst = max(worst, max(d.values()))
    for a, b in zip(sym, tay):
        assert a['status'][3] == -1 and b['status'][3] == -1
        assert np.all(a['status'][ok] == 1) and np.array_equal(a['status'], b['status'])
        assert np.array_equal(a['iter_count'][ok], b['iter_count'][ok])
    assert worst <= TOL, worst
