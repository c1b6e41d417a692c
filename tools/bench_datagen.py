"""Data generation on the GPU: the one launch of `DataGenerator.run` against the route a user had before it existed - the input
sequence drawn with `torch.rand` and repeated with `repeat_interleave`, `Model.rollout`, the noise drawn with `torch.randn`, and the
features and labels put together by slicing, differencing and `torch.cat` - code this feature does not touch.  Writes
profiles/datagen.json (bench.py measures the flagship NMPC workload and is not touched).

    python tools/bench_datagen.py [--batches 8192] [--samples 10] [--steps 10] [--reps 7] [--inner 20] [--out profiles/datagen.json]

chemostat4 at dt = .1 with its fixed-step map (over 100 intervals of dt = 1 the unregulated plant leaves every bound), B = 8192
experiments of 10 samples x 10 steps, shift = 1, labels as differences, normal measurement noise on every state.  Shape of a
measurement, as in tools/bench_pid.py: device events around synchronised work, after a warm-up of every shape that is timed, the two variants alternated within the process in an order that rotates from round to round,
`inner` calls per timed window; the median over `reps` windows is reported per call together with the smallest and largest.  Device
tensors in and out.  The two routes draw different random numbers, so their data sets are compared in distribution only (mean and
standard deviation of inputs and labels); what the fused launch computes is checked bit by bit in tests/test_datagen_gpu.py.  The
bytes each route has to move are counted from the shapes and recorded next to the times.  No ratio is promised: the file records
what was measured."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LB, UB = [0., .05], [.3, .2]
STD = .01
SHIFT = 1
DT = .1


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


def _one_batch(B, n_samples, steps, reps, inner):
    import torch
    from hilo_mpc_amd import DataGenerator, Model
    dev = torch.device('cuda')
    rng = np.random.default_rng(5)
    t = lambda a: torch.as_tensor(a, dtype=torch.float64, device=dev)
    x0 = t(np.array([.1, 40., .2, .2]) + rng.uniform(0., 1., (B, 4)) * np.array([12., 0., 2., 0.]))
    p = t(np.tile([100., 4., 1., 0.], (B, 1)))
    lb, ub = t(LB), t(UB)
    m = Model('chemostat4').setup(dt=DT)
    T = n_samples * steps
    gen = DataGenerator(m, x0=x0, p0=p)
    seed = [0]

    def fused():
        seed[0] += 1
        gen.random_uniform(n_samples, steps, LB, UB, seed=seed[0])
        return gen.run('difference', shift=SHIFT, add_noise={'distribution': 'random_normal', 'std': STD})

    def before():
        """draw, repeat, roll out, draw the noise, slice / diff / cat"""
        u = (lb + (ub - lb) * torch.rand(n_samples, B, 2, dtype=torch.float64, device=dev)).repeat_interleave(steps, dim=0)
        x = m.rollout(x0, u, p, steps=T)[0]
        n = STD * torch.randn(T + 1, B, 4, dtype=torch.float64, device=dev)
        xt = x + n
        F = torch.cat([xt[k:T - SHIFT + k] for k in range(SHIFT + 1)] + [u[SHIFT:]], dim=2)
        L = torch.diff(xt, dim=0)[SHIFT:]
        return F, L, u

    ds, (F, L, u) = fused(), before()                                     # warm-up of both variants
    assert tuple(ds._F.shape) == tuple(F.shape) and tuple(ds._L.shape) == tuple(L.shape)
    times = {'datagen_one_launch': [], 'torch_draw_rollout_slice': []}
    variants = [('datagen_one_launch', fused), ('torch_draw_rollout_slice', before)]
    for r in range(reps):                                                 # alternated, one window each; the order rotates
        for name, fn in variants[r % 2:] + variants[:r % 2]:
            times[name] += _windows(fn, 1, inner)
    N, nf, nl = T - SHIFT, F.shape[2], L.shape[2]
    d = 8
    # written once by either route: F, L; the fused launch also writes X and U once.  The route before writes u (rand), u again
    # (repeat), X (rollout), Y (rollout), n (randn), xt, the slices through cat, the difference - and reads what it wrote
    out_bytes = (N * B * (nf + nl)) * d
    traffic = {'datagen_one_launch_written': out_bytes + ((T + 1) * B * 4 + T * B * 2) * d,
               'torch_route_written': out_bytes + (n_samples * B * 2 + T * B * 2 + (T + 1) * B * 4 + T * B * 2 + 2 * (T + 1) * B * 4 +
                                                   T * B * 4) * d}

    def moments(a):
        return {'mean': [float(v) for v in a.reshape(-1, a.shape[-1]).mean(dim=0)],
                'std': [float(v) for v in a.reshape(-1, a.shape[-1]).std(dim=0)]}
    return {'batch': B, 'rows': N * B, 'features': nf, 'labels': nl, **{k: _summary(v) for k, v in times.items()},
            'calls_per_window': inner, 'bytes': traffic,
            'distribution': {'u_datagen': moments(ds.u), 'u_torch': moments(u), 'labels_datagen': moments(ds._L), 'labels_torch': moments(L)},
            'failed_instances': int((ds.status != 0).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[8192])
    ap.add_argument('--samples', type=int, default=10)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--inner', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'datagen.json'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_datagen.py needs the GPU: a CPU run says nothing about these times")
    res = {'device': torch.cuda.get_device_name(0), 'model': 'chemostat4', 'dt': DT, 'n_samples': args.samples, 'steps': args.steps,
           'shift': SHIFT, 'output': 'difference', 'noise': f'normal, std {STD}', 'reps': args.reps,
           'runs': [_one_batch(B, args.samples, args.steps, args.reps, args.inner) for B in args.batches]}
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
