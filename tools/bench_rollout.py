"""Roll-outs on the GPU: one launch (`Model.rollout`) against the loop of `Model.step`, and the error-controlled integrator's
rates.  Writes profiles/rollout.json (bench.py measures the flagship NMPC workload and is not touched by this).

    python tools/bench_rollout.py [--sizes 4096 65536] [--steps 100] [--reps 5] [--out profiles/rollout.json]

Shape of a measurement: device events around synchronised work, after a warm-up of every shape that is timed, the variants of one
size alternated within the process; the median over `reps` is reported together with the smallest and largest time.  Device
tensors in and out (no host copies inside the timed window).

  fixed map   chemostat4 discretised with the classic Runge-Kutta step, dt = .1: `rollout` over `steps` intervals in one launch
              against `steps` calls of `step` (the code path that existed before `rollout`, untouched), states per second, and
              the largest relative difference of the two final states.  (dt = .1, not 1: with held inputs and no controller the
              biomass grows until the classic step at dt = 1 is unstable for one instance in twenty, and a difference of one unit
              in the last place then grows to O(100) within 100 steps - in the CPU oracle's map just as well.  At dt = .1 the
              same perturbation stays at 3e-15.  The time per interval does not depend on dt.)
  dopri5      chemostat4 at dt = 4 and pendulum4 at dt = .5, reltol 1e-8 / abstol 1e-10: right-hand-side evaluations per second,
              the spread of accepted steps across the batch and the rejected share.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _time(fn, reps):
    import torch
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) * 1e-3)
    return out


def _summary(ts):
    return {'median_s': float(np.median(ts)), 'min_s': float(min(ts)), 'max_s': float(max(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[4096, 65536])
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rollout.json'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_rollout.py needs the GPU: a CPU run says nothing about these times")
    from hilo_mpc_amd import Model
    dev = torch.device('cuda')
    rng = np.random.default_rng(0)
    res = {'device': torch.cuda.get_device_name(0), 'steps': args.steps, 'reps': args.reps, 'fixed_map': [], 'dopri5': []}
    dev_t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    for B in args.sizes:
        # ---- the fixed map: one launch against the loop of Model.step ------------------------------------------------------
        m = Model('chemostat4').discretize('rk4').setup(dt=.1)
        X0 = dev_t(np.array([.1, 40., .5, .2]) * (1 + .1 * rng.uniform(-1, 1, (B, 4))))
        U = dev_t(rng.uniform(0, .3, (B, 2)))
        P = dev_t([100., 4., 1., 0.])

        def one_launch():
            return m.rollout(X0, U, P, steps=args.steps)

        def loop():
            x = X0
            for _ in range(args.steps):
                x, _ = m.step(x, U, P)
            return x
        xa, xb = one_launch()[0][-1], loop()                      # warm-up of both, and the same result
        # (one map compiled into two kernels: the two differ by rounding, carried through `steps` intervals)
        diff = float(((xa - xb).abs() / (xb.abs() + 1e-300)).max().item())
        ta, tb = [], []
        for _ in range(args.reps):                                 # alternated
            ta += _time(one_launch, 1)
            tb += _time(loop, 1)
        row = {'batch': B, 'model': 'chemostat4 rk4 dt=0.1', 'max_rel_diff_of_final_states': diff, 'one_launch': _summary(ta), 'step_loop': _summary(tb),
               'speedup_median': float(np.median(tb) / np.median(ta)),
               'states_per_s_one_launch': B * args.steps / float(np.median(ta)),
               'states_per_s_step_loop': B * args.steps / float(np.median(tb))}
        res['fixed_map'].append(row)
        print(json.dumps(row), flush=True)
        # ---- the error-controlled integrator ----------------------------------------------------------------------------------
        for name, dt, x0, u, p in (('chemostat4', 4., [.1, 40., .5, .2], [.1, .2], [100., 4., 1., 0.]),
                                   ('pendulum4', .5, [0., 0., .3, 0.], [.5], None)):
            c = Model(name).setup(dt=dt, solver='dopri5', solver_options={'reltol': 1e-8, 'abstol': 1e-10})
            X0 = dev_t(np.asarray(x0) * (1 + .1 * rng.uniform(-1, 1, (B, 4))) + .03 * rng.uniform(-1, 1, (B, 4)) * (np.asarray(x0) == 0.))
            U = dev_t(np.asarray(u) * (1 + .1 * rng.uniform(-1, 1, (B, len(u)))))
            Pt = None if p is None else dev_t(p)
            run = lambda: c.rollout(X0, U, Pt, steps=args.steps, return_stats=True)
            st = run()[2]
            ts = []
            for _ in range(args.reps):
                ts += _time(run, 1)
            acc, rej, rhs = (st[k].cpu().numpy().astype(np.int64) for k in ('n_accepted', 'n_rejected', 'n_rhs'))
            row = {'batch': B, 'model': f'{name} dt={dt:g}', 'reltol': 1e-8, 'abstol': 1e-10, 'time': _summary(ts),
                   'all_ok': bool((st['status'] == 0).all().item()), 'rhs_evaluations': int(rhs.sum()),
                   'rhs_per_s': float(rhs.sum() / np.median(ts)), 'states_per_s': B * args.steps / float(np.median(ts)),
                   'accepted_min': int(acc.min()), 'accepted_median': float(np.median(acc)), 'accepted_max': int(acc.max()),
                   'rejected_share': float(rej.sum() / (acc.sum() + rej.sum()))}
            res['dopri5'].append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == '__main__':
    main()
