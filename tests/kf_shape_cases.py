"""The cases of tests/test_kf_shapes_gpu.py: models, inputs, the three computations of a case (product kernels, oracle/kf.py,
50-digit truth) and the errors between them.  TEST INFRASTRUCTURE ONLY.

Run as a program (`python -m tests.kf_shape_cases TRUTH.pkl`, with HILO_KF_TEAM=0 in the environment) it is the child process of
that test module: csrc/hilo_kf.hip reads the knob once per process, so the one-lane fused / multi-step kernels at a small batch
need a process of their own.  It runs `estimate_runs` of every case and prints the errors as one JSON line.
"""
import functools
import json
import pickle
import sys

import numpy as np

from oracle import kf as okf, models as omodels
from tests import kf_reference as ref
from tests.util import spd_batch

B, K = 129, 3                       # 129 = 2 TEAMS k + 1 for every team count 1 .. 64; ipw = 16 gives nine workgroups, the last with one
TI = list(range(8)) + list(range(B - 8, B))          # instances compared with the truth: first and last eight
TI_SHARED = [0, 1, B - 2, B - 1]
KINDS = {'ekf': None, 'ukf1': 1., 'ukf1e-3': 1e-3}    # UKF alpha; 'ekf' is the Kalman filter for a linear model
P_BIO = [.15, 303.15, .13, .00025, 15., .14]

_LTI = {
    'lti212': (np.array([[.9, .2], [-.15, .8]]), np.array([[.1], [.3]]), np.array([[1., .5], [-.3, .7]])),
    'lti422': (np.array([[.9, .1, -.05, .02], [.04, .85, .12, -.07], [-.03, .06, .8, .11], [.08, -.02, .05, .75]]),
               np.array([[.1, -.2], [.3, .05], [-.15, .25], [.07, .12]]), np.array([[1., .5, -.2, .1], [-.3, .7, .4, .6]])),
}
# id: (n_x, n_y, discrete) of the family, or a zoo name; then what differs from the defaults
FAMILY = {'f11': (1, 1, False), 'f12': (1, 2, False), 'f33d': (3, 3, True), 'f53': (5, 3, False), 'f62': (6, 2, False),
          'f74': (7, 4, False), 'f83': (8, 3, False)}
ZOO = {'toy1d': dict(x0=[1.5], u0=[], p0=[], dt=1.), 'linear2': dict(x0=[.8, .3], u0=[.8], p0=[.5, .4], dt=1., linear=True),
       'bioreactor3': dict(x0=[299.9, .217, 20.], u0=[.01], p0=P_BIO, dt=.1),
       'pendulum4': dict(x0=[.5, .1, .3, -.2], u0=[.2], p0=[], dt=.05)}
MATRIX = list(FAMILY) + list(ZOO) + list(_LTI)
ERK = {f'f53_erk{o}': o for o in (1, 2, 3)}          # (5,3) under discretize('erk', order, n_sub=2)
CONT = ['bioreactor3_cont', 'f53_cont']               # continuous=True: the EKF integrates the augmented system, n_sub = 2


class Case:
    def __init__(self, cid):
        self.id, self.order, self.n_sub, self.continuous, self.linear, self.lti = cid, 4, 1, False, False, None
        base = cid.split('_')[0]
        if cid in ERK:
            self.order, self.n_sub = ERK[cid], 2
        if cid in CONT:
            self.continuous, self.n_sub = True, 2
        if base in FAMILY:
            self.shape = FAMILY[base]
            self.om = ref.family_oracle(*self.shape)
            self.x0, self.u0, self.p0 = ref.family_point(self.shape[0])
            self.dt = .1
        elif base in ZOO:
            z = ZOO[base]
            self.om = omodels.get(base)
            self.x0, self.u0, self.p0, self.dt = np.array(z['x0']), np.array(z['u0']), np.array(z['p0']), z['dt']
            self.linear = z.get('linear', False)
        else:
            self.lti = _LTI[base]
            self.om = ref.lti_oracle(*self.lti)
            n, m = self.lti[1].shape
            self.x0, self.u0, self.p0, self.dt, self.linear = np.linspace(.5, 1.1, n), np.linspace(.4, .7, m), np.array([]), .5, True
        self.base = base
        self.nx, self.ny, self.nu, self.np = self.om.nx, self.om.ny, self.om.nu, self.om.np_
        self.omap = ref.oracle_map(self.om, self.order, self.n_sub)
        self.tm = ref.TruthModel(self.om, self.order, self.n_sub)
        self.kinds = ['ekf'] if self.continuous else (['ekf', 'ukf1'] if cid in ERK else list(KINDS))

    @functools.lru_cache(maxsize=None)
    def product(self):
        """The product model, set up once per process (a model written as expressions is compiled once per source: JIT disk cache)."""
        from hilo_mpc_amd import Model
        if self.base in FAMILY:
            m = ref.family_product(*self.shape)
        elif self.lti is not None:
            m = Model('lti', A=self.lti[0], B=self.lti[1], C=self.lti[2])
        else:
            m = Model(self.base)
        if not self.om.discrete and not self.continuous:
            m = m.discretize('erk', order=self.order, n_sub=self.n_sub) if self.order != 4 or self.n_sub != 1 else m.discretize('rk4')
        return m.setup(dt=self.dt)

    def filter(self, kind):
        import hilo_mpc_amd as H
        kw = dict(n_sub=self.n_sub) if self.continuous else {}
        if kind == 'ekf':
            f = (H.KF if self.linear else H.EKF)(self.product(), **kw)
        else:
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')              # (a UKF on a linear model: the reference's efficiency hint)
                f = H.UKF(self.product(), alpha=KINDS[kind], **kw)
        f.setup()
        return f

    @functools.lru_cache(maxsize=None)
    def data(self, n=B, seed=0):
        """States near the operating point, random SPD P, full SPD Q and R (distinct per instance, distinct off-diagonals), inputs
        per step, measurements = the propagated nominal output + noise."""
        rng = np.random.default_rng(seed + sum(map(ord, self.id)))
        x = self.x0 * (1 + .05 * rng.uniform(-1, 1, (n, self.nx)))
        P = spd_batch(rng, n, self.nx)
        Q = spd_batch(rng, n, self.nx, scale=.03, diag=1e-3)
        R = spd_batch(rng, n, self.ny, scale=.05, diag=1e-2)
        us = self.u0 * (1 + .1 * rng.uniform(-1, 1, (K, n, self.nu)))
        p = self.p0 * (1 + .02 * rng.uniform(-1, 1, (n, self.np)))
        ys, xn = [], x
        for k in range(K):
            xn = self.omap.f(xn, us[k], p, self.dt)
            ys.append(self.omap.h(xn, us[k], p, self.dt) + .02 * rng.normal(size=(n, self.ny)))
        return dict(x=x, P=P, Q=Q, R=R, us=us, p=p, ys=np.stack(ys))


@functools.lru_cache(maxsize=None)
def case(cid):
    return Case(cid)


# ---- the three computations ---------------------------------------------------------------------------------------------------
def product_steps(c, kind, x, P, ys, us, p, Q, R, steps):
    """`estimate()` (steps = 1) or `estimate(steps=K)`; us [K, n, nu] per step or [1, nu] held and shared.  -> x, P, y with a
    leading step axis."""
    f = c.filter(kind)
    f.Q, f.R = Q, R
    f.set_initial_guess(x, P0=P)
    pa = p if c.np and c.lti is None else None
    if steps == 1:
        u0 = (us[0] if us.ndim == 3 else us) if c.nu else None
        sol = f.estimate(y=ys[0], u=u0, p=pa)
        return f.x.cpu().numpy()[None], f.P.cpu().numpy()[None], np.asarray(sol['y']).reshape(1, x.shape[0], c.ny)
    sol = f.estimate(y=ys[:steps], u=(us[:steps] if us.ndim == 3 else us) if c.nu else None, p=pa, steps=steps)
    return np.asarray(sol['x']), np.asarray(sol['P']), np.asarray(sol['y'])


def oracle_predict_continuous(c, x, P, u, p, Q):
    """fp64 twin of `kf_reference.ekf_predict(continuous=True)`: classic RK4 with n_sub steps on [x; vec P] (batched)."""
    h = c.dt / c.n_sub
    Q = np.broadcast_to(Q, P.shape)

    def d(xs, Ps):
        F = c.om.fx(xs, u, p, c.dt)
        return c.om.f(xs, u, p, c.dt), F @ Ps + Ps @ np.swapaxes(F, 1, 2) + Q
    for _ in range(c.n_sub):
        k1, K1 = d(x, P)
        k2, K2 = d(x + .5 * h * k1, P + .5 * h * K1)
        k3, K3 = d(x + .5 * h * k2, P + .5 * h * K2)
        k4, K4 = d(x + h * k3, P + h * K3)
        x = x + h / 6. * (k1 + 2. * k2 + 2. * k3 + k4)
        P = P + h / 6. * (K1 + 2. * K2 + 2. * K3 + K4)
    return okf.pack(x, P)


def oracle_steps(c, kind, x, P, ys, us, p, Q, R, steps):
    tile, out = okf.pack(x, P), []
    n = x.shape[0]
    p = p if c.np else np.zeros((n, 0))
    for k in range(steps):
        u = (us[k] if us.ndim == 3 else us) if c.nu else np.zeros((n, 0))
        if c.continuous:
            tile, yp = okf.kf_update(c.om, oracle_predict_continuous(c, tile[:, :, 0], tile[:, :, 1:], u, p, Q), ys[k], u, p, R, c.dt)
        elif kind == 'ekf':
            tile, yp = okf.kf_step(c.omap, tile, ys[k], u, p, Q, R, c.dt)
        else:
            tile, yp = okf.ukf_step(c.omap, tile, ys[k], u, p, Q, R, c.dt, alpha=KINDS[kind])
        out.append((tile[:, :, 0], tile[:, :, 1:], yp))
    return tuple(np.stack(v) for v in zip(*out))


def truth_steps(c, kind, x, P, ys, us, p, Q, R, steps, idx):
    """The instances `idx`, `steps` steps chained in 50 digits.  -> x, P, y as object arrays [steps, len(idx), ...]."""
    out = []
    for b in idx:
        xb, Pb, row = x[b], P[b], []
        Qb, Rb = (Q[b] if Q.ndim == 3 else Q), (R[b] if R.ndim == 3 else R)
        pb = p[b] if c.np else []
        for k in range(steps):
            u = ((us[k, b] if us.ndim == 3 else us[0]) if c.nu else [])
            if c.lti is not None and kind == 'ekf':
                xb, Pb, yp = ref.lti_step(*c.lti, xb, Pb, ys[k, b], u, Qb, Rb)
            elif kind == 'ekf':
                xb, Pb, yp = ref.ekf_step(c.tm, xb, Pb, ys[k, b], u, pb, Qb, Rb, c.dt, c.continuous, c.n_sub)
            else:
                xb, Pb, yp = ref.ukf_step(c.tm, xb, Pb, ys[k, b], u, pb, Qb, Rb, c.dt, alpha=KINDS[kind])
            row.append((xb, Pb, yp))
        out.append(row)
    return tuple(np.stack([np.stack([out[i][k][q] for i in range(len(idx))]) for k in range(steps)]) for q in range(3))


# ---- truth sets: computed once per process, handed to the child process in a file ---------------------------------------------------
_TRUTH = {}


def _variant(c, variant):
    d = c.data()
    if variant == 'per':
        return dict(d, idx=TI)
    return dict(d, Q=d['Q'][0], R=d['R'][0], us=d['us'][0, :1], idx=TI_SHARED)       # Q, R and ONE input row shared by the batch


def truth(cid, kind, variant):
    key = (cid, kind, variant)
    if key not in _TRUTH:
        c = case(cid)
        v = _variant(c, variant)
        _TRUTH[key] = truth_steps(c, kind, v['x'], v['P'], v['ys'], v['us'], v['p'], v['Q'], v['R'], K, v['idx'])
    return _TRUTH[key]


def all_cases():
    return [(cid, kind) for cid in MATRIX + list(ERK) + CONT for kind in case(cid).kinds]


# ---- errors -----------------------------------------------------------------------------------------------------------------
def errors(got, orc, tru, idx):
    """{quantity: (kernel vs truth, oracle vs truth, kernel vs oracle over ALL instances)}: norm-wise relative, worst instance and step."""
    out = {}
    for name, g, o, t in zip('xPy', got, orc, tru):
        steps = g.shape[0]
        flat = lambda a: a.reshape((-1,) + a.shape[2:])                    # noqa: E731
        gi, oi = flat(g[:, idx]), flat(o[:steps][:, idx])
        out[name] = (ref.rel_err(gi, flat(t[:steps])), ref.rel_err(oi, flat(t[:steps])), ref.rel_err(flat(g), flat(o[:steps])))
    return out


def estimate_runs(cid, kind):
    """The `estimate()` runs of one case: {run: errors}.  Team kernels by default, the one-lane kernels under HILO_KF_TEAM=0."""
    c = case(cid)
    res = {}
    for variant in ('per', 'shared'):
        v = _variant(c, variant)
        args = (v['x'], v['P'], v['ys'], v['us'], v['p'], v['Q'], v['R'])
        orc = oracle_steps(c, kind, *args, K)
        tru = truth(cid, kind, variant)
        res[f'{variant}{K}'] = errors(product_steps(c, kind, *args, K), orc, tru, v['idx'])        # K steps in one launch, every step
        if variant == 'per':
            res['per1'] = errors(product_steps(c, kind, *args, 1), orc, tru, v['idx'])            # one fused step
            one = tuple(a[:1] if a.ndim and a.shape[0] == B else a[:, :1] for a in args)             # B = 1: instance 0
            for steps in (1, K):
                res[f'one{steps}'] = errors(product_steps(c, kind, *one, steps), tuple(o[:, :1] for o in orc),
                                            tuple(t[:, :1] for t in tru), [0])
    return res


def failures(res, margin=ref.MARGIN, label=''):
    """The runs / quantities outside the bound, and one line per entry with the measured ratio (printed by the tests)."""
    bad = []
    for run, qs in res.items():
        for q, (ek, eo, ea) in qs.items():
            bk = ref.bound(eo, margin)
            print(f'{label} {run:8s} {q}: kernel {ek:.2e} oracle {eo:.2e} ratio {ek / max(eo, 1e-300):6.2f} bound {bk:.2e} | all instances vs oracle {ea:.2e}')
            if not ek <= bk or not ea <= 2 * bk:
                bad.append((run, q, ek, eo, ea))
    return bad


if __name__ == '__main__':
    with open(sys.argv[1], 'rb') as fh:
        _TRUTH.update(pickle.load(fh))
    report = {f'{cid}/{kind}': estimate_runs(cid, kind) for cid, kind in all_cases()}
    print('KF_SHAPES_JSON ' + json.dumps(report))
