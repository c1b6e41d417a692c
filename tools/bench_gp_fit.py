"""Hyper-parameter fits of many GPs: the one launch of `GPArray.fit_model` against the same fits as a loop of
`GaussianProcess.fit_model` (host BFGS on the device objective, code this feature does not touch).  Writes profiles/gp_fit.json
(bench.py measures the flagship NMPC workload and is not touched).

    python tools/bench_gp_fit.py [--gps 12] [--n 200] [--restarts 1 8 21] [--gtols 1e-6 1e-5] [--reps 5] [--out profiles/gp_fit.json]

G = 12 squared-exponential ARD GPs over nf = 3 features, n = 200 training points each, one label each (twelve different smooth
functions of the same inputs plus noise), all from noise variance 0.1 and unit kernel hyper-parameters.  Every call that is timed
is synchronous (host arrays in and out), so a host clock around it measures finished work; every variant runs once untimed first,
the variants are alternated within a repetition in an order that rotates, and the median over `reps` repetitions is reported
with the smallest and largest.  Before every timed call the members are put back to the start (untimed).  Reported per variant:
the whole `fit_model` call (pack, launch, read back, set-up of the fitted members), the launch alone (`hilo_gp_fit_batch`: pack,
upload, kernel, read back), iterations and objective evaluations per problem, and the launch time over the largest evaluation
count of a problem - the problems run side by side, so that is the time of one objective value inside the kernel with its share
of the gradients.  Measured at the default `gtol = 1e-6` and at `1e-5`: with 200 points the central-difference gradient's noise
floor lies near 1e-6, and a problem that cannot get below it spends its line searches on halvings until `maxiter`.  No ratio is
promised: the file records what was measured."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NF = 3
START = dict(noise=.1, length_scales=[1.] * NF, signal_variance=1.)


def _data(G, n):
    rng = np.random.default_rng(12)
    X = rng.uniform(-2., 2., (NF, n))
    w = rng.normal(size=(G, NF))
    ph = rng.uniform(0., np.pi, (G, NF))
    Y = np.stack([np.sum(np.sin(w[g][:, None] * X + ph[g][:, None]), axis=0) for g in range(G)]) + .1 * rng.normal(size=(G, n))
    return X, Y


def _reset(members):
    for m in members:
        m._set_hyperparameters([START['noise']] + START['length_scales'] + [START['signal_variance']])
        m.setup()


def _timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def _summary(ts):
    return {'median_s': float(np.median(ts)), 'min_s': float(min(ts)), 'max_s': float(max(ts))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gps', type=int, default=12)
    ap.add_argument('--n', type=int, default=200)
    ap.add_argument('--restarts', type=int, nargs='+', default=[1, 8, 21])
    ap.add_argument('--gtols', type=float, nargs='+', default=[1e-6, 1e-5])
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gp_fit.json'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_gp_fit.py needs the GPU: a CPU run says nothing about these times")
    from hilo_mpc_amd import GPArray, Kernel
    G, n = args.gps, args.n
    X, Y = _data(G, n)
    arr = GPArray.from_labels([f'x{i}' for i in range(NF)], [f'y{g}' for g in range(G)],
                              kernel=Kernel.squared_exponential(active_dims=list(range(NF)), ard=True, length_scales=START['length_scales']),
                              noise_variance=START['noise'])
    arr.set_training_data(X, Y)
    arr.setup()
    members = list(arr)
    warnings.simplefilter('ignore')

    def host_loop():
        for m in members:
            m.fit_model()
        return [list(m.hyperparameter_values) for m in members]

    def batched(R, gtol):
        def run():
            arr.fit_model(n_restarts=R, seed=0, gtol=gtol)
            return [list(m.hyperparameter_values) for m in members]
        return run

    def launch(R, gtol):
        def run():
            problems = [arr._fit_problem(g, m) for g, m in enumerate(members)]
            return arr._launch(problems, arr._start_points(problems, R, None, 0, 1.), gtol, 200)
        return run
    cases = [(R, gtol) for gtol in args.gtols for R in args.restarts]
    variants = [('host_loop', host_loop)] + [(f'fit_model_R{R}_{gtol:g}', batched(R, gtol)) for R, gtol in cases] + \
               [(f'launch_R{R}_{gtol:g}', launch(R, gtol)) for R, gtol in cases]
    results, times = {}, {name: [] for name, _ in variants}
    for name, fn in variants:                                             # warm-up of every variant
        _reset(members)
        results[name] = fn()
    for r in range(args.reps):
        k = r % len(variants)
        for name, fn in variants[k:] + variants[:k]:
            _reset(members)
            times[name].append(_timed(fn)[0])
    res = {'device': torch.cuda.get_device_name(0), 'gps': G, 'n': n, 'nf': NF, 'kernel': 'squared exponential, ARD', 'reps': args.reps,
           'maxiter': 200, 'host_loop': dict(_summary(times['host_loop']), what='loop of GaussianProcess.fit_model (gtol 1e-8)'),
           'runs': []}
    base = np.array(results['host_loop'])
    for R, gtol in cases:
        rows = results[f'launch_R{R}_{gtol:g}']
        ev = np.array([r['evaluations'] for r in rows])
        it = np.array([r['iterations'] for r in rows])
        st = np.array([r['status'] for r in rows])
        lt = _summary(times[f'launch_R{R}_{gtol:g}'])
        fitted = np.array(results[f'fit_model_R{R}_{gtol:g}'])
        gmax = np.array([np.max(np.abs(r['grad']), axis=1) for r in rows])
        res['runs'].append({
            'gtol': gtol, 'n_restarts': R, 'problems': int(G * R), 'fit_model': _summary(times[f'fit_model_R{R}_{gtol:g}']), 'launch': lt,
            'host_loop_over_fit_model': float(np.median(times['host_loop']) / np.median(times[f'fit_model_R{R}_{gtol:g}'])),
            'largest_final_max_gradient': float(np.nanmax(gmax)),
            'iterations': {'min': int(it.min()), 'median': float(np.median(it)), 'max': int(it.max())},
            'evaluations': {'min': int(ev.min()), 'median': float(np.median(ev)), 'max': int(ev.max())},
            'status_counts': {str(s): int((st == s).sum()) for s in np.unique(st)},
            'launch_s_per_evaluation_of_the_longest_problem': float(lt['median_s'] / max(int(ev.max()), 1)),
            'max_rel_difference_to_host_loop': float(np.max(np.abs(fitted - base) / np.abs(base))) if R == 1 else None})
    print(json.dumps(res, indent=1))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    main()
