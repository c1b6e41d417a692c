"""The Kalman filter kernels of csrc/hilo_kf_kernel.h at every state / measurement size that takes a path of its own, against a
50-digit truth (tests/kf_reference.py) and, instance by instance, against oracle/kf.py.

Shapes (tests/kf_shape_cases.py): expression models (run-time compiled) (1,1) [EKF team of 1 lane; UKF 3 points on 4 lanes],
(1,2) [n_y > team: the serial y_pred tail], (3,3) discrete [team_ekf_step's branch for n_x that do not divide the team, n_y = n_x],
(5,3) [25 entries on 8 lanes, every P- | Pxy | Pyy boundary inside a pass], (6,2) [13 points], (7,4) [15 points on 16 lanes],
(8,3) [the dividing branch with 8 passes; UKF on 32 lanes]; the zoo functors toy1d, linear2, bioreactor3, pendulum4 (n_y = n_x) and
Lti<2,1,2>, Lti<4,2,2>; (5,3) under ERK orders 1-3 with two sub-steps; the continuous-time EKF (augmented system) of bioreactor3, (5,3).

Rule of every assertion (kf_reference.bound): the kernels' norm-wise relative error against the truth is at most MARGIN = 16 times
the error of oracle/kf.py against the truth ON THE SAME INPUTS (the kernels divide through 2-ulp reciprocals and the compiler may
contract multiply-adds where the oracle is IEEE: a small constant times a rounding-limited error), with a floor of 4 ulp of the
largest entry; every instance of a batch is within twice that bound of oracle/kf.py (triangle inequality, the truth instances'
oracle error standing in for the batch).  The bound is never formed from a kernel's output.  Oracle errors: ~3e-16 (EKF, UKF
alpha = 1), ~2e-10 (UKF alpha = 1e-3: the weights 1 / (n + lambda) are rounded from a six-digit cancellation, in the kernels' host
code, the oracle and not in the truth).  The measured ratios are printed by every test (`pytest -s`); also in DESIGN.md 5.2.

Measured on the MI355X: (kernel error against the truth) / (oracle error against the truth), worst quantity and run of each case
('ekf' is the Kalman filter for the linear models; ukf1 / ukf1e-3: alpha = 1 / 1e-3).  The largest, 14.7 (toy1d EKF, P after three
chained steps of a map with |F| = 2.5: 2e-13 against the oracle's 6e-14), is inside the margin, so the margin stays at 16.

    case              filter    team  predict/update  one-lane fused/multi  large
    f11               ekf       2.4   2.6             2.4                     -
    f11               ukf1      3.9   1.1             3.9                     -
    f11               ukf1e-3   3.4   1.0             3.4                     -
    f12               ekf       2.6   2.6             2.6                     -
    f12               ukf1      2.0   1.6             2.0                     -
    f12               ukf1e-3   1.8   1.1             1.8                     -
    f33d              ekf       3.1   1.6             3.1                   1.5
    f33d              ukf1      1.9   1.3             1.8                     -
    f33d              ukf1e-3   1.6   1.3             2.9                     -
    f53               ekf       2.2   1.4             2.2                     -
    f53               ukf1      2.0   1.6             2.0                     -
    f53               ukf1e-3   1.9   1.0             1.9                     -
    f62               ekf       1.5   2.0             1.5                     -
    f62               ukf1      1.3   2.1             1.5                     -
    f62               ukf1e-3   1.3   1.0             2.4                     -
    f74               ekf       2.0   1.0             2.0                     -
    f74               ukf1      1.7   1.1             1.7                     -
    f74               ukf1e-3   1.2   1.1             1.3                     -
    f83               ekf       2.0   2.3             2.0                     -
    f83               ukf1      1.4   1.4             2.2                     -
    f83               ukf1e-3   2.1   1.0             3.6                     -
    toy1d             ekf      14.7   2.6            14.7                     -
    toy1d             ukf1      2.3   2.8             2.3                     -
    toy1d             ukf1e-3   2.8   1.6             2.8                     -
    linear2           ekf       3.6   1.4             3.6                     -
    linear2           ukf1      2.0   1.7             2.1                     -
    linear2           ukf1e-3   3.0   1.0             1.8                     -
    bioreactor3       ekf       2.6   1.0             2.6                     -
    bioreactor3       ukf1      1.0   1.4             1.0                   1.0
    bioreactor3       ukf1e-3   1.0   1.0             1.0                     -
    pendulum4         ekf       2.0   1.3             1.7                     -
    pendulum4         ukf1      1.2   1.2             1.2                     -
    pendulum4         ukf1e-3   1.0   1.0             1.0                     -
    lti212            ekf       1.9   1.9             1.9                     -
    lti212            ukf1      3.4   1.6             3.4                     -
    lti212            ukf1e-3   1.4   1.1             1.4                     -
    lti422            ekf       2.2   1.8             2.2                     -
    lti422            ukf1      2.7   1.7             2.7                     -
    lti422            ukf1e-3   1.5   1.0             1.5                     -
    f53_erk1          ekf       1.6   1.4             1.6                     -
    f53_erk1          ukf1      1.8   2.5             1.8                     -
    f53_erk2          ekf       1.8   1.8             1.8                     -
    f53_erk2          ukf1      2.4   2.3             2.4                     -
    f53_erk3          ekf       2.5   1.3             2.5                     -
    f53_erk3          ukf1      2.4   1.7             2.4                     -
    bioreactor3_cont  ekf       1.7     -             1.7                     -
    f53_cont          ekf       1.9     -             1.9                     -
"""
import json
import os
import pickle
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import kf as okf                                    # noqa: E402
from tests import kf_reference as ref, kf_shape_cases as S      # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = S.all_cases()
IDS = [f'{c}-{k}' for c, k in ALL]


def _assert(res, label):
    bad = S.failures(res, label=label)
    assert not bad, f'{label}: outside the bound (run, quantity, kernel vs truth, oracle vs truth, kernel vs oracle): {bad}'


# ---- estimate(): the team kernels (a continuous-time EKF always runs one instance per lane) -----------------------------------------
@pytest.mark.parametrize('cid,kind', ALL, ids=IDS)
def test_estimate_small_batch(cid, kind):
    """B = 129 and B = 1; one fused step and three steps in one launch with per-step inputs, every step asserted; Q, R per instance
    and shared; one input row shared by the batch."""
    _assert(S.estimate_runs(cid, kind), f'{cid}/{kind} team')


# ---- predict() / update(): kf_kernel modes 0 and 1, one instance per lane at every batch --------------------------------------------
@pytest.mark.parametrize('cid,kind', [a for a in ALL if a[0] not in S.CONT], ids=[i for i, a in zip(IDS, ALL) if a[0] not in S.CONT])
def test_predict_and_update_tiles(cid, kind):
    """B = 129: nine workgroups of 16 instances, the last with one.  The UKF's prediction tile is [x | P | X]."""
    c = S.case(cid)
    d = c.data()
    x, P, Q, R, p, y = d['x'], d['P'], d['Q'], d['R'], d['p'], d['ys'][0]
    u = d['us'][0]
    flt = c.filter(kind)
    lti_p = np.tile(c.product().lti_parameters(), (S.B, 1)) if c.lti is not None else None
    up = np.concatenate([u, lti_p if lti_p is not None else p], axis=1)
    a = S.KINDS[kind]
    n = c.nx
    # predict
    if kind == 'ekf':
        po = okf.kf_predict(c.omap, okf.pack(x, P), u, p, Q, c.dt)
        pt = [ref.ekf_predict(c.tm, x[b], P[b], u[b], p[b], Q[b], c.dt) for b in S.TI]
    else:
        po = okf.ukf_predict(c.omap, okf.pack(x, P), u, p, Q, c.dt, alpha=a)
        pt = [ref.ukf_predict(c.tm, x[b], P[b], u[b], p[b], Q[b], c.dt, alpha=a) for b in S.TI]
    pg = np.asarray(flt.predict(okf.pack(x, P), up if up.shape[1] else None, Q))
    assert pg.shape == po.shape == (S.B, n, (2 + 3 * n) if kind != 'ekf' else n + 1)
    split = lambda t: (t[None, :, :, 0], t[None, :, :, 1:1 + n], t[None, :, :, 1 + n:])          # noqa: E731
    tru = tuple(np.stack([t[q] for t in pt])[None] for q in range(len(pt[0])))
    names = 'xPX' if kind != 'ekf' else 'xP'
    res = {'predict': {q: v for q, v in zip(names, S.errors(split(pg)[:len(names)], split(po)[:len(names)], tru, S.TI).values())}}
    # update, from the oracle's prediction tile
    if kind == 'ekf':
        uo, yo = okf.kf_update(c.omap, po, y, u, p, R, c.dt)
        ut = [ref.ekf_update(c.tm, po[b, :, 0], po[b, :, 1:], y[b], u[b], p[b], R[b], c.dt) for b in S.TI]
    else:
        uo, yo = okf.ukf_update(c.omap, po, y, u, p, R, c.dt, alpha=a)
        ut = [ref.ukf_update(c.tm, po[b, :, 0], po[b, :, 1:1 + n], po[b, :, 1 + n:], y[b], u[b], p[b], R[b], c.dt, alpha=a) for b in S.TI]
    ug, yg = flt.update(po, y, up if up.shape[1] else None, R)
    ug, yg = np.asarray(ug), np.asarray(yg)
    tru = tuple(np.stack([t[q] for t in ut])[None] for q in range(3))
    res['update'] = S.errors((ug[None, :, :, 0], ug[None, :, :, 1:], yg[None]), (uo[None, :, :, 0], uo[None, :, :, 1:], yo[None]), tru, S.TI)
    _assert(res, f'{cid}/{kind} one-lane')


# ---- two large batches ------------------------------------------------------------------------------------------------------------
def _large(cid, kind, n, steps, shared):
    """All instances against oracle/kf.py, the first and the last workgroup (64 instances per workgroup) against the truth."""
    c = S.case(cid)
    d = c.data(n=n, seed=1)
    Q, R = (d['Q'][0], d['R'][0]) if shared else (d['Q'], d['R'])
    args = (d['x'], d['P'], d['ys'], d['us'], d['p'], Q, R)
    idx = list(range(64)) + list(range(n - n % 64, n))
    got = S.product_steps(c, kind, *args, steps)
    orc = S.oracle_steps(c, kind, *args, steps)
    tru = S.truth_steps(c, kind, *args, steps, idx)
    _assert({f'B{n}': S.errors(got, orc, tru, idx)}, f'{cid}/{kind} large')


def test_lean2_ukf_of_a_three_state_model_at_a_large_batch():
    """bioreactor3, UKF, B = 131073 (2 x 1024 x 64 + 1), two steps, Q and R shared: `kf_multi_kernel<.., true, 2>` (one sigma point at a
    time), which only chemostat4 reached."""
    _large('bioreactor3', 'ukf1', 131073, 2, True)


def test_full_wave_tiles_of_a_three_state_model_at_a_large_batch():
    """(3,3) EKF at B = 65539: 64 instances per workgroup, tile staging with rows of 12 doubles on every lane, three instances in the last."""
    _large('f33d', 'ekf', 65539, 1, False)
    _large('f33d', 'ekf', 65539, 2, False)


# ---- the same estimate() runs on the one-lane fused / multi-step kernels: a child process with HILO_KF_TEAM=0 ---------------------------
@pytest.fixture(scope='module')
def one_lane_report(tmp_path_factory):
    for cid, kind in ALL:                                # (the truth sets of the runs above, computed where a test was deselected)
        for variant in ('per', 'shared'):
            S.truth(cid, kind, variant)
    path = tmp_path_factory.mktemp('kf_shapes') / 'truth.pkl'
    with open(path, 'wb') as fh:
        pickle.dump(S._TRUTH, fh)
    env = dict(os.environ, HILO_KF_TEAM='0')
    run = subprocess.run([sys.executable, '-m', 'tests.kf_shape_cases', str(path)], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=900)
    assert run.returncode == 0, f'child process ended with {run.returncode}:\n{run.stdout[-2000:]}\n{run.stderr[-4000:]}'
    line = [ln for ln in run.stdout.splitlines() if ln.startswith('KF_SHAPES_JSON ')]
    assert len(line) == 1, run.stdout[-2000:]
    return json.loads(line[0][len('KF_SHAPES_JSON '):])


@pytest.mark.parametrize('cid,kind', ALL, ids=IDS)
def test_estimate_small_batch_on_the_one_lane_kernels(one_lane_report, cid, kind):
    """`kf_kernel<.., 2>`, `kf_multi_kernel` and, for continuous models under `discretize('rk4')` with shared Q and R,
    `ekf_multi_lean_kernel` / `kf_multi_kernel<.., true, 1>` at B = 129 and B = 1."""
    _assert(one_lane_report[f'{cid}/{kind}'], f'{cid}/{kind} one-lane')
