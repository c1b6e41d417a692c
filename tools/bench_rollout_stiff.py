"""Roll-outs of stiff models on the GPU: `solver='bdf'` against `solver='dopri5'`.  Writes profiles/rollout_stiff.json (bench.py
measures the flagship NMPC workload and is not touched by this).

    python tools/bench_rollout_stiff.py [--sizes 4096 65536] [--steps 10] [--reps 5] [--out profiles/rollout_stiff.json]

Shape of a measurement as in tools/bench_rollout.py: device events around synchronised work, after a warm-up of every shape that
is timed, the two solvers of one case alternated within the process; the median over `reps` with the smallest and largest time.

  robertson3   Robertson's kinetics, k = (0.04, 3e7, 1e4) as parameters, from (1, 0, 0), dt = 4
  vdp2         van der Pol's oscillator, mu = 100 as parameter, from (2, 0), dt = 20
both written as expressions (the run-time compiled kernels), initial states perturbed by +-10 %, the default tolerances (reltol
1e-6, abstol 1e-8): time, right-hand-side evaluations per second and the spread of accepted steps across the batch."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.bench_rollout import _summary, _time     # noqa: E402


def robertson():
    from hilo_mpc_amd import Model
    m = Model(name='robertson3')
    x = m.set_dynamical_states(['a', 'b', 'c'])
    k = m.set_parameters(['k1', 'k2', 'k3'])
    m.set_dynamical_equations([-k[0] * x[0] + k[2] * x[1] * x[2], k[0] * x[0] - k[2] * x[1] * x[2] - k[1] * x[1] * x[1],
                               k[1] * x[1] * x[1]])
    m.set_measurement_equations([x[0]])
    return m


def vdp():
    from hilo_mpc_amd import Model
    m = Model(name='vdp2')
    x = m.set_dynamical_states(['x', 'v'])
    mu = m.set_parameters(['mu'])
    m.set_dynamical_equations([x[1], mu[0] * ((1. - x[0] * x[0]) * x[1]) - x[0]])
    m.set_measurement_equations([x[0]])
    return m


CASES = (('robertson3', robertson, 4., [1., 0., 0.], [.04, 3e7, 1e4]), ('vdp2', vdp, 20., [2., 0.], [100.]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[4096, 65536])
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rollout_stiff.json'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_rollout_stiff.py needs the GPU: a CPU run says nothing about these times")
    dev = torch.device('cuda')
    rng = np.random.default_rng(0)
    res = {'device': torch.cuda.get_device_name(0), 'steps': args.steps, 'reps': args.reps, 'reltol': 1e-6, 'abstol': 1e-8, 'rows': []}
    dev_t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    for B in args.sizes:
        for name, build, dt, x0, p in CASES:
            X0 = dev_t(np.asarray(x0) * (1 + .1 * rng.uniform(-1, 1, (B, len(x0)))))
            P = dev_t(p)
            models = {s: build().setup(dt=dt, solver=s) for s in ('bdf', 'dopri5')}
            runs = {s: (lambda m=m: m.rollout(X0, None, P, steps=args.steps, return_stats=True)) for s, m in models.items()}
            stats = {s: run()[2] for s, run in runs.items()}                  # warm-up of both
            ts = {s: [] for s in runs}
            for _ in range(args.reps):                                        # alternated
                for s, run in runs.items():
                    ts[s] += _time(run, 1)
            for s in runs:
                st = stats[s]
                acc, rej, rhs = (st[k].cpu().numpy().astype(np.int64) for k in ('n_accepted', 'n_rejected', 'n_rhs'))
                row = {'batch': B, 'model': f'{name} dt={dt:g}', 'solver': s, 'time': _summary(ts[s]),
                       'all_ok': bool((st['status'] == 0).all().item()), 'rhs_evaluations': int(rhs.sum()),
                       'rhs_per_s': float(rhs.sum() / np.median(ts[s])), 'states_per_s': B * args.steps / float(np.median(ts[s])),
                       'accepted_min': int(acc.min()), 'accepted_median': float(np.median(acc)), 'accepted_max': int(acc.max()),
                       'rejected_share': float(rej.sum() / max(1, acc.sum() + rej.sum()))}
                res['rows'].append(row)
                print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == '__main__':
    main()
