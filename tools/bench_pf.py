"""A batch of particle filters on the GPU: `ParticleFilter(generator='device')` - a run of `steps` steps as ONE launch, every random
number drawn on the device - against the host mode, a loop of `estimate()` whose draws come from numpy filter after filter, with
`probability_density_function = multivariate_normal` (its fastest sampler; the default `lhsnorm` adds a sort and an inverse normal
cdf per draw).  Writes profiles/pf.json (bench.py measures the flagship NMPC workload and is not touched).

    python tools/bench_pf.py [--batches 256 4096] [--particles 64 1024] [--steps 50] [--reps 7] [--host-reps 3] [--out profiles/pf.json]

chemostat4 under `rk4` at dt = 0.5, measurements of a simulated plant, per-filter initial guesses.  Shape of a measurement, as in
tools/bench_pid.py: device events around synchronised work after a warm-up of every shape that is timed; the device mode is one
call per window (`set_initial_guess` + `estimate(steps=)`: the initial sample is part of the run), the host mode one run of `steps`
calls per window, timed with the wall clock - it is host-bound, which is the point.  The median over the windows is reported with
the smallest and largest.  Device tensors in and out for the device mode.  The two modes draw different random numbers (and the
host mode another sampler), so they are compared by what a filter is for: the median error of the final estimate against the
simulated plant.  No ratio is promised: the file records what was measured."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

X0 = np.array([.1, 40., .5, .2])
U, P = [.1, .2], [100., 4., 1., 0.]
DT = .5


def _summary(ts):
    return {'median_s': float(np.median(ts)), 'min_s': float(min(ts)), 'max_s': float(max(ts)), 'windows': len(ts)}


def _one_shape(B, N, steps, reps, host_reps):
    import torch
    from hilo_mpc_amd import PF, Model
    dev = torch.device('cuda')
    rng = np.random.default_rng(B + N)
    m = Model('chemostat4').discretize('rk4').setup(dt=DT)
    Q, R, P0 = np.diag((.01 * X0) ** 2), np.diag([1e-4, 1e-3]), np.diag((.05 * X0) ** 2)
    xt = X0[None, :] * (1 + .05 * rng.standard_normal((B, 4)))
    guess = xt * (1 + .05 * rng.standard_normal((B, 4)))
    ys = []
    for _ in range(steps):                                               # the plant: the model's own map with process noise
        xt = m.step(xt, U, P)[0] + rng.standard_normal((B, 4)) * np.sqrt(np.diag(Q))
        ys.append(xt[:, [0, 2]] + rng.standard_normal((B, 2)) * np.sqrt(np.diag(R)))
    ys = np.stack(ys)
    y_dev, guess_dev = torch.as_tensor(ys, device=dev), torch.as_tensor(guess, device=dev)

    def make(**kw):
        pf = PF(m, **kw)
        pf.setup(n_samples=N)
        pf.Q, pf.R = Q, R
        return pf
    dpf, hpf = make(generator='device', seed=1), make()
    hpf.probability_density_function = lambda mu, s, n: np.random.multivariate_normal(mu, s, size=n)

    def device_run():
        dpf.set_initial_guess(guess_dev, P0=P0)
        return dpf.estimate(y=y_dev, u=U, p=P, steps=steps)['x'][-1]

    def host_run():
        hpf._X = None
        hpf.set_initial_guess(guess_dev, P0=P0)
        for k in range(steps):
            s = hpf.estimate(y=y_dev[k], u=U, p=P)
        return s['x']
    xd = device_run()                                                    # warm-up of both
    np.random.seed(0)
    xh = host_run()
    torch.cuda.synchronize()
    td, th = [], []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        device_run()
        b.record()
        torch.cuda.synchronize()
        td.append(a.elapsed_time(b) * 1e-3)
    for _ in range(host_reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host_run()
        torch.cuda.synchronize()
        th.append(time.perf_counter() - t0)
    err = lambda x: float(np.median(np.abs(x.cpu().numpy() - xt) / np.abs(xt)))
    d, h = _summary(td), _summary(th)
    return {'batch': B, 'particles': N, 'device_one_launch': d, 'host_loop_of_estimate': h, 'host_over_device': h['median_s'] / d['median_s'],
            'median_relative_error_of_final_estimate': {'device': err(xd), 'host': err(xh)}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', type=int, nargs='+', default=[256, 4096])
    ap.add_argument('--particles', type=int, nargs='+', default=[64, 1024])
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--host-reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pf.json'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_pf.py needs the GPU: a CPU run says nothing about these times")
    res = {'device': torch.cuda.get_device_name(0), 'model': 'chemostat4', 'discretisation': 'rk4', 'dt': DT, 'steps': args.steps,
           'host_sampler': 'numpy.random.multivariate_normal', 'reps': args.reps, 'host_reps': args.host_reps,
           'runs': [_one_shape(B, N, args.steps, args.reps, args.host_reps) for B in args.batches for N in args.particles]}
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
