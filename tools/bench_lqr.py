"""Regulator gains on the GPU: batched linearisation + Riccati + feedback (`LQR.call`, csrc/hilo_lqr.h) and, for scale, the path that
existed before it - `system_matrices` per instance plus scipy.linalg.solve_discrete_are on the CPU.  Writes profiles/lqr.json
(bench.py measures the flagship NMPC workload and is not touched by this).

    python tools/bench_lqr.py [--sizes 4096 65536] [--reps 5] [--cpu-batch 256] [--out profiles/lqr.json]

Shape of a measurement: device events around synchronised work, after a warm-up of every shape that is timed; the median over `reps`
is reported together with the smallest and largest time.  Device tensors in and out (no host copies inside the timed window).

Model: pendulum4 as hilo_mpc_amd/zoo_expr.py writes it, classic Runge-Kutta step, dt = .1, Q = I, R = .1; the operating points are
the upright position with a per-instance cart position and a small angle (the gains differ from lane to lane).
  fused_horizon20   one `hilo_lqr_call` per batch: Jacobians at per-instance operating points, 20 backward Riccati steps, feedback
  fused_stationary  the same with the stationary gain (structure-preserving doubling)
  cached            a second `call` with the same operating data: `hilo_lqr_apply` alone
  linearize         `Model.linearization` alone (the Jacobians of the batch)
  cpu               at `--cpu-batch` instances: `set_equilibrium_point` + `system_matrices` + `solve_discrete_are` per instance
No speed-up is asserted anywhere: the file records what the run shows.
"""
import argparse
import json
import os
import sys
import time

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


def _pendulum():
    from hilo_mpc_amd import Model, zoo_expr
    m = zoo_expr.define(Model(), 'pendulum4')
    m.discretize('rk4', inplace=True)
    return m.setup(dt=.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[4096, 65536])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--cpu-batch', type=int, default=256)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lqr.json'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_lqr.py needs the GPU: a CPU run says nothing about these times")
    from hilo_mpc_amd import LQR
    dev = torch.device('cuda')
    rng = np.random.default_rng(0)
    res = {'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'model': 'pendulum4 rk4 dt=0.1, Q = I, R = 0.1', 'gpu': [], 'cpu': None}
    dev_t = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
    plant = _pendulum()

    def operating_points(B):
        xe = np.zeros((B, 4))
        xe[:, 0], xe[:, 2] = rng.uniform(-1, 1, B), rng.uniform(-.2, .2, B)
        return xe, np.zeros((B, 1))
    for B in args.sizes:
        xe, ue = operating_points(B)
        Xe, Ue = dev_t(xe), dev_t(ue)
        X = dev_t(xe + .01 * rng.standard_normal((B, 4)))
        row = {'batch': B}
        for name, horizon in (('fused_horizon20', 20), ('fused_stationary', None)):
            c = LQR(plant.linearize())
            c.horizon = horizon
            c.setup()
            c.Q, c.R = np.ones(4), [.1]

            def fused():
                c._keys = None                                     # forget the gain: every call solves
                return c.call(x=X, x_eq=Xe, u_eq=Ue)
            fused()                                                # warm-up
            st = c.status.cpu().numpy()
            it = c.iterations.cpu().numpy()
            ts = _time(fused, args.reps)
            row[name] = dict(_summary(ts), gains_per_s=B / float(np.median(ts)), all_ok=bool(np.all(st == 0)),
                             iterations_min=int(it.min()), iterations_max=int(it.max()))
            if horizon is None:
                c.call(x=X, x_eq=Xe, u_eq=Ue)                      # the gain is kept from here on
                ts = _time(lambda: c.call(x=X, x_eq=Xe, u_eq=Ue), args.reps)
                row['cached'] = dict(_summary(ts), controls_per_s=B / float(np.median(ts)))
        plant.linearization(x=Xe, u=Ue)
        ts = _time(lambda: plant.linearization(x=Xe, u=Ue), args.reps)
        row['linearize'] = dict(_summary(ts), jacobians_per_s=B / float(np.median(ts)))
        res['gpu'].append(row)
        print(json.dumps(row), flush=True)
    # ---- the path that existed before: one instance at a time on the host -------------------------------------------------------
    from scipy.linalg import solve_discrete_are
    Bc = args.cpu_batch
    xe, ue = operating_points(Bc)
    ml = plant.linearize()
    Q, R = np.eye(4), np.array([[.1]])

    def cpu():
        for b in range(Bc):
            ml.set_equilibrium_point(x_eq=xe[b], u_eq=ue[b])
            A, Bm, _ = ml.system_matrices()
            P = solve_discrete_are(A, Bm, Q, R)
            np.linalg.solve(R + Bm.T @ P @ Bm, Bm.T @ P @ A)
    cpu()
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        cpu()
        ts.append(time.perf_counter() - t0)
    res['cpu'] = dict(_summary(ts), batch=Bc, gains_per_s=Bc / float(np.median(ts)),
                      path='set_equilibrium_point + system_matrices + scipy.linalg.solve_discrete_are per instance')
    print(json.dumps(res['cpu']), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == '__main__':
    main()
