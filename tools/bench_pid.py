"""A PID gain study on the GPU: the one launch of `PID.closed_loop` - with the trajectories stored and in the sweep mode that keeps
only the indices - against what a user could do before it existed: the law in torch element-wise operations plus
`Model.rollout(steps=1)` per sampling interval, code this feature does not touch.  Writes profiles/pid.json (bench.py measures the
flagship NMPC workload and is not touched).

    python tools/bench_pid.py [--batches 8192 65536] [--steps 100] [--reps 7] [--inner 5] [--out profiles/pid.json]

chemostat4 at dt = 1 with its fixed-step map, two loops - X by DS (k_p < 0) and P by DI - with output limits (0, .5), set points
(5, 1), one gain set per instance, 100 sampling intervals.  Shape of a measurement, as in tools/bench_rollout_sens.py: device events
around synchronised work, after a warm-up of every shape that is timed, the variants alternated within the process in an order that rotates from round to round, `inner` calls per
timed window; the median over `reps` windows is reported per call together with the smallest and largest.  Device tensors in and out.
The three variants are also compared with each other (relative differences of the final states and of ISE: median, 99th
percentile, largest; the two fused variants agree bit for bit, the torch law rounds differently and the loops that chatter between
the limits amplify that).  No ratio is promised: the file records what was measured."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LO, HI = 0., .5


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


def _one_batch(B, steps, reps, inner):
    import torch
    from hilo_mpc_amd import PID, Model
    dev = torch.device('cuda')
    rng = np.random.default_rng(3)
    t = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev)
    k_p = t(rng.uniform(.02, .1, (B, 2)) * np.array([-1., 1.]))
    t_i, t_d = t(np.full((B, 2), 20.)), t(np.zeros((B, 2)))
    x0 = t(np.array([.1, 40., .2, .2]) + rng.uniform(0., 1., (B, 4)) * np.array([12., 0., 2., 0.]))
    p = t(np.tile([100., 4., 1., 0.], (B, 1)))
    sp = t([5., 1.])
    dt = 1.
    m = Model('chemostat4').setup(dt=dt)
    pid = PID(n_set_points=2, k_p=k_p, t_i=t_i, t_d=t_d, output_limits=(LO, HI)).setup(dt=dt)
    pid.set_point = [5., 1.]

    def fused(store):
        pid.reset()
        return pid.closed_loop(m, x0, p=p, steps=steps, process_values=['X', 'P'], outputs=['DS', 'DI'], store=store)

    def before():
        """the velocity-form law in torch element-wise operations, the plant by one-interval roll-outs"""
        x = x0
        pv2 = pv1 = sp2 = sp1 = u = torch.zeros(B, 2, dtype=torch.float64, device=dev)
        ise = torch.zeros(B, 2, dtype=torch.float64, device=dev)
        for _ in range(steps):
            pv = x[:, [0, 2]]
            e1, e2 = sp - pv, sp1 - pv1
            u = torch.clamp(u + k_p * ((e1 - e2) + dt / t_i * e1 + t_d / dt * (e1 - 2. * e2 + (sp2 - pv2))), LO, HI)
            pv2, pv1, sp2, sp1 = pv1, pv, sp1, sp.expand(B, 2)
            ise = ise + e1 * e1 * dt
            x = m.rollout(x, u, p, steps=1)[0][1]
        return x, ise

    ra, rb, (xc, isec) = fused(False), fused(True), before()            # warm-up of every variant
    times = {'closed_loop_store_false': [], 'closed_loop_store_true': [], 'torch_law_plus_rollout_per_interval': []}
    variants = [('closed_loop_store_false', lambda: fused(False), inner), ('closed_loop_store_true', lambda: fused(True), inner),
                ('torch_law_plus_rollout_per_interval', before, max(1, inner // 5))]
    for r in range(reps):                                               # alternated, one window each; the order rotates
        for name, fn, n in variants[r % 3:] + variants[:r % 3]:
            times[name] += _windows(fn, 1, n)

    def rel(a, b):
        d = ((a - b).abs() / b.abs().clamp(min=1e-300)).flatten()
        return {'median': float(d.median()), 'quantile_99': float(torch.quantile(d, .99)), 'max': float(d.max())}
    res = {'batch': B, **{k: _summary(v) for k, v in times.items()},
           'calls_per_window': {'closed_loop': inner, 'torch_law_plus_rollout_per_interval': max(1, inner // 5)},
           'relative_difference': {'x_final_store_false_vs_true': rel(ra['x_final'], rb['x_final']),
                                   'x_final_torch_vs_closed_loop': rel(xc, rb['x_final']),
                                   'ise_torch_vs_closed_loop': rel(isec, rb['indices']['ise'])},
           'note_on_differences': 'the torch law rounds differently (no fused multiply-adds); loops that chatter between the limits '
                                  'amplify that - the numpy restatement moves as far under a 1e-15 perturbation of x0',
           'share_of_outputs_at_a_limit': float(((rb['u'] == LO) | (rb['u'] == HI)).double().mean())}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[8192, 65536])
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--inner', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pid.json'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_pid.py needs the GPU: a CPU run says nothing about these times")
    res = {'device': torch.cuda.get_device_name(0), 'model': 'chemostat4', 'dt': 1., 'steps': args.steps, 'loops': 'X by DS, P by DI',
           'output_limits': [LO, HI], 'reps': args.reps, 'runs': [_one_batch(B, args.steps, args.reps, args.inner) for B in args.batches]}
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
