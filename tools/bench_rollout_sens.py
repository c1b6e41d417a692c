"""Forward sensitivities of a roll-out on the GPU: the one launch of `Model.rollout(..., sensitivities=True)` against what a user
could do before it existed - central differences through 21 plain `'dopri5'` roll-outs (the nominal one and two per column), code
this feature does not touch.  Writes profiles/rollout_sens.json (bench.py measures the flagship NMPC workload and is not touched).

    python tools/bench_rollout_sens.py [--batch 8192] [--steps 10] [--reps 7] [--inner 20] [--out profiles/rollout_sens.json]

chemostat4 at dt = 4, all 10 columns (x0, u, p), reltol 1e-8 / abstol 1e-10 (the tolerances of the accuracy tests).  Shape of a
measurement, as in tools/bench_rollout.py: device events around synchronised work, after a warm-up of every shape that is timed,
the two variants alternated within the process, `inner` calls per timed window; the median over `reps` windows is reported per call
together with the smallest and largest.  Device tensors in and out.  Both results are also compared with the tight solution of the
augmented system (tests/sens_reference.py: scipy DOP853 at 1e-13) on 8 instances: the error relative to |.| + abstol / reltol.
Central differences perturb entry j of [x0; u; p] by delta_j = 1e-4 max(|theta_j|, 1e-2) per instance.  No ratio is promised: the
file records what was measured."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RTOL, ATOL = 1e-8, 1e-10
FD_REL, FD_FLOOR = 1e-4, 1e-2


def _windows(fn, reps, inner):
    import torch
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e-3 / inner)
    return out


def _summary(ts):
    return {'median_s': float(np.median(ts)), 'min_s': float(min(ts)), 'max_s': float(max(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8192)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rollout_sens.json'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_rollout_sens.py needs the GPU: a CPU run says nothing about these times")
    from hilo_mpc_amd import Model
    from tests import sens_reference as sn
    from tests import sim_reference as sr
    dev = torch.device('cuda')
    B, steps, dt = args.batch, args.steps, 4.
    x0, u, p, _, _ = sr.CASES['chemostat4']
    rng = np.random.default_rng(11)
    X0 = np.asarray(x0) * (1 + .1 * rng.uniform(-1, 1, (B, 4)))
    U = np.asarray(u) * (1 + .1 * rng.uniform(-1, 1, (B, 2)))
    P = np.tile(np.asarray(p, dtype=float), (B, 1))
    theta = torch.as_tensor(np.hstack([X0, U, P]), dtype=torch.float64, device=dev)          # [B, 10]: the columns' own order
    delta = FD_REL * torch.clamp(theta.abs(), min=FD_FLOOR)
    m = Model('chemostat4').setup(dt=dt, solver='dopri5', solver_options={'reltol': RTOL, 'abstol': ATOL})

    def sens_launch():
        return m.rollout(theta[:, :4], theta[:, 4:6], theta[:, 6:], steps=steps, sensitivities=True)

    def central_differences():
        """x [steps + 1, B, 4] and S [steps + 1, B, 10, 4] from 21 plain roll-outs"""
        x, _ = m.rollout(theta[:, :4], theta[:, 4:6], theta[:, 6:], steps=steps)
        cols = []
        for j in range(10):
            xs = []
            for sgn in (1., -1.):
                th = theta.clone()
                th[:, j] += sgn * delta[:, j]
                xs.append(m.rollout(th[:, :4].contiguous(), th[:, 4:6].contiguous(), th[:, 6:].contiguous(), steps=steps)[0])
            cols.append((xs[0] - xs[1]) / (2. * delta[:, j])[None, :, None])
        return x, torch.stack(cols, dim=2)

    xa, _, sens = sens_launch()                                                        # warm-up of both variants
    xb, Sb = central_differences()
    groups = ('x0', 'u', 'p')
    Sa = torch.cat([sens['x'][g].permute(0, 1, 3, 2) for g in groups], dim=2)          # [steps + 1, B, 10, 4]
    t_sens, t_fd = [], []
    for _ in range(args.reps):                                                         # alternated, one window each
        t_sens += _windows(sens_launch, 1, args.inner)
        t_fd += _windows(central_differences, 1, args.inner)
    sub = np.linspace(0, B - 1, 8).astype(int)
    ref = np.stack([sn.tight('chemostat4', groups, X0[i], U[i], P[i], dt, steps) for i in sub], axis=1)
    wa = sn.join(xa[:, sub].cpu().numpy(), Sa[:, sub].cpu().numpy())
    wb = sn.join(xb[:, sub].cpu().numpy(), Sb[:, sub].cpu().numpy())
    res = {'device': torch.cuda.get_device_name(0), 'model': 'chemostat4', 'dt': dt, 'batch': B, 'steps': steps, 'columns': 10,
           'reltol': RTOL, 'abstol': ATOL, 'reps': args.reps, 'calls_per_window': args.inner,
           'sensitivity_rollout_one_launch': _summary(t_sens),
           'central_differences_21_rollouts': _summary(t_fd),
           'ratio_of_medians_fd_over_sens': float(np.median(t_fd) / np.median(t_sens)),
           'fd_step': f'{FD_REL:g} * max(|theta_j|, {FD_FLOOR:g})',
           'error_vs_tight_solution_8_instances': {
               'measure': 'max |w - ref| / (|ref| + abstol / reltol) over the augmented trajectory [x; vec S]',
               'sensitivity_rollout': float(max(sr.rel_err(wa[:, i], ref[:, i], RTOL, ATOL) for i in range(len(sub)))),
               'central_differences': float(max(sr.rel_err(wb[:, i], ref[:, i], RTOL, ATOL) for i in range(len(sub))))}}
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
