"""A numpy restatement of the PID law and of the closed loop around a plant (not a test module), and the case tables of the PID
tests.

The law is written from the reference's equations (hilo_mpc/modules/controller/pid.py:244-293), one instance at a time with plain
numpy arithmetic - no fused multiply-adds, so it agrees with csrc/hilo_pid.h to rounding, not to the bit.  The plant is advanced per
sampling interval with the inputs held: by `n_sub` classic Runge-Kutta steps (the map of a continuous model that was not
discretised, like tests/sim_reference.py::rk4_substeps) or by scipy's `solve_ivp` started afresh at every sampling instant."""
import numpy as np
from scipy.integrate import solve_ivp

from tests import sim_reference as sr

FACTOR = sr.FACTOR
MEM = 5   # pv[-2], pv[-1], sp[-2], sp[-1], u_prev


def law(mem, pv, sp, k_p, t_i, t_d, dt, p_on_pv=False, d_on_pv=False, limits=None):
    """One call for [..., nsp] loops: mem [..., nsp, 5] is updated in place; returns (u, e), each [..., nsp]."""
    pv, sp = np.asarray(pv, dtype=float), np.asarray(sp, dtype=float)
    pv3, pv2, sp3, sp2, u_prev = (mem[..., i].copy() for i in range(MEM))
    e1, e2, e3 = sp - pv, sp2 - pv2, sp3 - pv3
    with np.errstate(invalid='ignore', over='ignore'):
        delta = -(pv - pv2) if p_on_pv else e1 - e2
        delta = delta + dt / t_i * e1
        delta = delta + (-(t_d / dt) * (pv - 2. * pv2 + pv3) if d_on_pv else (t_d / dt) * (e1 - 2. * e2 + e3))
        u = u_prev + k_p * delta
        if limits is not None:
            u = np.where(u < limits[0], limits[0], u)
            u = np.where(u > limits[1], limits[1], u)
    mem[..., 0], mem[..., 1], mem[..., 2], mem[..., 3], mem[..., 4] = pv2, pv, sp2, sp + 0. * pv, u
    return u, e1


def oracle_plant(om):
    """(f(t, x, u, p), h(t, x, u, p)), each for rows of instances, of a model of oracle/models.py."""
    return (lambda t, x, u, p: om.f(x, u, p, 1.)), (lambda t, x, u, p: om.h(x, u, p, 1.))


def batch(plant, X0, U_held, P, K_p, T_i, T_d, set_point, steps, dt, pv_sel, out_idx, p_on_pv=False, d_on_pv=False, limits=None,
          advance=('map', 8), mem=None, t0=0.):
    """The closed loop of B instances.  plant = (f, h) on rows of instances; X0 [B, nx], U_held [B, nu] (the inputs no loop drives
    keep it), P [B, np], the gains [B, nsp]; set_point [nsp], [B, nsp] or [steps, B, nsp]; pv_sel: per loop ('y', i) or ('x', i);
    out_idx: per loop the driven input; advance ('map', n_sub) or (scipy method, rtol, atol); mem [B, nsp, 5] or None (zeros).
    Returns a dict like `PID.closed_loop`: x [steps + 1, B, nx], u [steps, B, nsp], y [steps, B, ny], e [steps, B, nsp] (the errors the
    law saw), indices {ise, iae, itae, tvu} [B, nsp], mem [B, nsp, 5]."""
    f, h = plant
    K_p, T_i, T_d = (np.asarray(v, dtype=float) for v in (K_p, T_i, T_d))
    B, nsp = K_p.shape
    mem = np.zeros((B, nsp, MEM)) if mem is None else np.array(mem, dtype=float)
    sp = np.asarray(set_point, dtype=float)
    x, p = np.array(X0, dtype=float), np.asarray(P, dtype=float)
    u = np.array(U_held, dtype=float)
    out_idx = list(out_idx)
    u[:, out_idx] = mem[:, :, 4]
    X, U, Y, E = [x.copy()], [], [], []
    J = np.zeros((B, nsp, 4))
    for k in range(steps):
        tk = t0 + k * dt
        y = h(tk, x, u, p) if any(kind == 'y' for kind, _ in pv_sel) else None
        pv = np.stack([y[:, i] if kind == 'y' else x[:, i] for kind, i in pv_sel], axis=1)
        u_before = mem[:, :, 4].copy()
        uo, e = law(mem, pv, sp[k] if sp.ndim == 3 else sp, K_p, T_i, T_d, dt, p_on_pv, d_on_pv, limits)
        u[:, out_idx] = uo
        J[:, :, 0] += e * e * dt
        J[:, :, 1] += np.abs(e) * dt
        J[:, :, 2] += (k * dt) * np.abs(e) * dt
        J[:, :, 3] += np.abs(uo - u_before)
        uk = u.copy()
        if advance[0] == 'map':
            n_sub = advance[1]
            hs = dt / n_sub
            for i in range(n_sub):
                ts = tk + i * hs
                k1 = f(ts, x, uk, p)
                k2 = f(ts + .5 * hs, x + .5 * hs * k1, uk, p)
                k3 = f(ts + .5 * hs, x + .5 * hs * k2, uk, p)
                k4 = f(ts + hs, x + hs * k3, uk, p)
                x = x + hs / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
        else:
            xn = np.empty_like(x)
            for b in range(B):
                s = solve_ivp(lambda t, z: f(t, z[None], uk[b:b + 1], p[b:b + 1])[0], (tk, tk + dt), x[b], method=advance[0],
                              rtol=advance[1], atol=advance[2])
                assert s.success, s.message
                xn[b] = s.y[:, -1]
            x = xn
        X.append(x.copy())
        U.append(uo.copy())
        E.append(e.copy())
        Y.append(h(tk + dt, x, uk, p))
    return {'x': np.array(X), 'u': np.array(U), 'y': np.array(Y), 'e': np.array(E), 'mem': mem,
            'indices': {'ise': J[:, :, 0], 'iae': J[:, :, 1], 'itae': J[:, :, 2], 'tvu': J[:, :, 3]}}


# ---- the cases ---------------------------------------------------------------------------------------------------------------
def linear2_case(B=130, seed=0):
    """linear2 (y = x_2 driven by u), dt .25, 40 intervals, set point 1, per-instance gains and rate constants."""
    rng = np.random.default_rng(seed)
    return dict(k_p=rng.uniform(.5, 3., (B, 1)), t_i=rng.uniform(1., 5., (B, 1)), t_d=rng.uniform(0., .3, (B, 1)),
                p=rng.uniform(.5, 2., (B, 2)), x0=rng.uniform(0., 1., (B, 2)), set_point=np.array([1.]), dt=.25, steps=40,
                pv_sel=[('y', 0)], out_idx=[0])


def chemostat4_case(B=130, seed=1):
    """chemostat4, dt 1, p = [100, 4, 1, 0]: X by DS with k_p < 0 and P by DI, t_i 20, limits (0, .5), set points (5, 1).  The
    biomass starts between .1 and 12.1 - below and above its set point, so that DS is driven into either limit - and the product
    between .2 and 2.2."""
    rng = np.random.default_rng(seed)
    k_p = rng.uniform(.02, .1, (B, 2)) * np.array([-1., 1.])
    return dict(k_p=k_p, t_i=np.full((B, 2), 20.), t_d=np.zeros((B, 2)), p=np.tile([100., 4., 1., 0.], (B, 1)),
                x0=np.array([.1, 40., .2, .2]) + rng.uniform(0., 1., (B, 4)) * np.array([12., 0., 2., 0.]), set_point=np.array([5., 1.]), dt=1., steps=40, limits=(0., .5),
                pv_sel=[('x', 0), ('x', 2)], out_idx=[0, 1], process_values=['X', 'P'], outputs=['DS', 'DI'])


def dopri5_bound(plant, case, rows, steps, rtol, atol, **kw):
    """The bound of tests/sim_reference.py for the closed loop of instances `rows` of a case: (tight solution x [steps + 1, n, nx],
    admissible error [n], RK45's error [n], DOP853 vs Radau [n]) - every solver in the same loop, started afresh at each sampling
    instant, the law in numpy; errors relative to |x| + abstol / reltol."""
    nu = len(case['out_idx']) if 'outputs' in case else 1
    args = (case['x0'][rows], np.zeros((len(rows), nu)), case['p'][rows], case['k_p'][rows], case['t_i'][rows], case['t_d'][rows],
            case['set_point'], steps, case['dt'], case['pv_sel'], case['out_idx'])
    kw = dict(kw, limits=case.get('limits'))
    ref = batch(plant, *args, advance=('DOP853', 1e-13, 1e-15), **kw)['x']
    radau = batch(plant, *args, advance=('Radau', 1e-12, 1e-15), **kw)['x']
    rk45 = batch(plant, *args, advance=('RK45', rtol, atol), **kw)['x']
    n = len(rows)
    e45 = np.array([sr.rel_err(rk45[:, i], ref[:, i], rtol, atol) for i in range(n)])
    e_tight = np.array([sr.rel_err(radau[:, i], ref[:, i], rtol, atol) for i in range(n)])
    return ref, FACTOR * np.maximum(e45, e_tight), e45, e_tight


CASES = {'linear2': linear2_case, 'chemostat4': chemostat4_case}


def _one(job):
    name, row, steps, rtol, atol = job
    from oracle import models as omodels
    return dopri5_bound(oracle_plant(omodels.get(name)), CASES[name](), [row], steps, rtol, atol)


def dopri5_bounds_batch(name, rows, steps, rtol, atol):
    """`dopri5_bound` for the rows of CASES[name]().  The instances are independent and Radau at 1e-12 takes a second each, so they
    are spread over worker processes - of a fresh interpreter that never opens the GPU, not forks of the test process."""
    import os
    import subprocess
    import sys
    import tempfile
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with tempfile.TemporaryDirectory() as d:
        fin, fout = os.path.join(d, 'in.npz'), os.path.join(d, 'out.npz')
        np.savez(fin, name=name, rows=np.asarray(rows), steps=steps, rtol=rtol, atol=atol)
        subprocess.check_call([sys.executable, '-m', 'tests.pid_reference', fin, fout], cwd=root)
        with np.load(fout) as z:
            return z['ref'], z['admissible'], z['e45'], z['e_tight']


def _main(fin, fout):
    import multiprocessing
    import os
    with np.load(fin) as z:
        name, rows, steps, rtol, atol = str(z['name']), z['rows'], int(z['steps']), float(z['rtol']), float(z['atol'])
    jobs = [(name, int(r), steps, rtol, atol) for r in rows]
    with multiprocessing.Pool(min(16, os.cpu_count() or 1, len(jobs))) as pool:
        res = pool.map(_one, jobs)
    np.savez(fout, ref=np.concatenate([r[0] for r in res], axis=1), admissible=np.concatenate([r[1] for r in res]),
             e45=np.concatenate([r[2] for r in res]), e_tight=np.concatenate([r[3] for r in res]))


if __name__ == '__main__':
    import sys
    _main(sys.argv[1], sys.argv[2])
