"""Roll-outs of models with algebraic states on the GPU: `solver='idas'` against the fixed-step map.  Writes
profiles/rollout_dae.json (bench.py measures the flagship NMPC workload and is not touched by this).

    python tools/bench_rollout_dae.py [--batch 8192] [--steps 10] [--reps 5] [--out profiles/rollout_dae.json]

Shape of a measurement as in tools/bench_rollout.py: device events around synchronised work, after a warm-up of every shape that
is timed; the median over `reps` with the smallest and largest time.

  robertson_dae   Robertson's kinetics with the conservation law as algebraic equation, dt = 4, k1 perturbed by +-10 %
  alg_u           two coupled algebraic states, dt = .5, initial states perturbed by +-10 %
both of tests/dae_reference.py, written as expressions, at the default tolerances (reltol 1e-6, abstol 1e-8).  For 'idas': the time
of a roll-out, the accepted steps and the right-hand-side evaluations.  The fixed-step map - classic Runge-Kutta steps with a nested
Newton iteration on the algebraic equations per evaluation - is run with n_sub = 8, 16, ... sub-steps per interval until the
largest error of `--check` instances against the tight solution of the reduced equation is no larger than that of 'idas', or
`--max-sub` is passed: the first n_sub that gets there with its time, or the fact that none does.  scipy's BDF on the reduced
equation at the same tolerances gives the step counts next to it."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_rollout import _summary, _time     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8192)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--check', type=int, default=4)
    ap.add_argument('--max-sub', type=int, default=4096)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rollout_dae.json'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_rollout_dae.py needs the GPU: a CPU run says nothing about these times")
    from tests import dae_reference as dr
    from tests import sim_reference as sr
    dev = torch.device('cuda')
    rng = np.random.default_rng(0)
    rtol, atol = 1e-6, 1e-8
    B, steps, nc = args.batch, args.steps, args.check
    res = {'device': torch.cuda.get_device_name(0), 'batch': B, 'steps': steps, 'reps': args.reps, 'reltol': rtol, 'abstol': atol,
           'checked_instances': nc, 'rows': []}
    dev_t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    for case in ('robertson_dae', 'alg_u'):
        x0, u, p, dt, _ = dr.CASES[case]
        X0 = np.tile(np.asarray(x0, dtype=float), (B, 1))
        P = np.tile(np.asarray(p, dtype=float), (B, 1))
        U = np.tile(np.asarray(u, dtype=float), (B, 1))
        if case == 'robertson_dae':
            P[:, 0] *= 1 + .1 * rng.uniform(-1, 1, B)
        else:
            X0 *= 1 + .1 * rng.uniform(-1, 1, X0.shape)
        ref = dr.run_jobs([(case, X0[i], U[i], P[i], dt, steps, [(rtol, atol)]) for i in range(nc)])
        xt, ut, pt = dev_t(X0), dev_t(U if U.shape[1] else None), dev_t(P if P.shape[1] else None)

        def error(x):
            x = x[:, :nc].cpu().numpy()
            return max(sr.rel_err(x[:, i], ref[i][0]['x'], rtol, atol) if np.isfinite(x[:, i]).all() else np.inf for i in range(nc))

        m = dr.symbolic_model(case).setup(dt=dt, solver='idas')
        run = lambda: m.rollout(xt, ut, pt, steps=steps, return_z=True, return_stats=True)
        x, _, _, st = run()                                                   # warm-up
        ts = _time(run, args.reps)
        acc, rej, rhs = (st[k].cpu().numpy().astype(np.int64) for k in ('n_accepted', 'n_rejected', 'n_rhs'))
        e_idas = error(x)
        row = {'model': f'{case} dt={dt:g}', 'solver': 'idas', 'time': _summary(ts), 'all_ok': bool((st['status'] == 0).all().item()),
               'error': e_idas, 'accepted_min': int(acc.min()), 'accepted_median': float(np.median(acc)), 'accepted_max': int(acc.max()),
               'rejected_share': float(rej.sum() / max(1, acc.sum() + rej.sum())), 'n_rhs_min': int(rhs.min()),
               'n_rhs_median': float(np.median(rhs)), 'n_rhs_max': int(rhs.max()),
               'scipy_bdf_steps': [int(r[0]['counts'][0]) for r in ref], 'scipy_bdf_nfev': [int(r[0]['counts'][1]) for r in ref],
               'scipy_bdf_error': max(float(r[0]['e_bdf_x']) for r in ref)}
        res['rows'].append(row)
        print(json.dumps(row), flush=True)
        n_sub, tried = 8, []
        while n_sub <= args.max_sub:
            f = dr.symbolic_model(case).discretize('rk4', n_sub=n_sub).setup(dt=dt)
            runf = lambda: f.rollout(xt, ut, pt, steps=steps)
            e = error(runf()[0])
            tried.append({'n_sub': n_sub, 'error': e if np.isfinite(e) else None})      # (None: a non-finite trajectory)
            if e <= e_idas:
                break
            n_sub *= 2
        met = e <= e_idas
        row = {'model': f'{case} dt={dt:g}', 'solver': 'fixed-step map', 'meets_the_error_of_idas': bool(met), 'tried': tried}
        if met:
            row.update(n_sub=tried[-1]['n_sub'], time=_summary(_time(runf, args.reps)))
        res['rows'].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fo:
        json.dump(res, fo, indent=1)
    print("wrote", args.out)


if __name__ == '__main__':
    main()
