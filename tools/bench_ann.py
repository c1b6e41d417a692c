"""Throughput of `ANN.predict` (csrc/hilo_ann.hip: the layers chained in registers on the f64 matrix cores) against the forward pass
of a torch fp64 `nn.Sequential` with the same weights on the same GPU.  Writes profiles/ann.json (bench.py measures the flagship NMPC
workload and is not touched by this).

    python tools/bench_ann.py [--m 1048576] [--reps 20] [--out profiles/ann.json]

Shape of a measurement: device-resident inputs and outputs (torch sees the queries as rows, [m, nf]; the product as columns,
[nf, m] - each side its native layout, no transposes inside the timed window), a warm-up of every shape that is timed, device events
around synchronised work, results checked against the numpy oracle before anything is timed, the median over `reps` together with the smallest and largest time.  The roof of the product's kernel is
the traffic of X and Y (8 (nf + nl) bytes per query) against the issue rate of the matrix-core products (16 queries x 16 neurons x 4
inputs per instruction) and of the exponentials; both are reported per network.  No speed-up is asserted anywhere: the file records
what the run shows.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NETS = [('2-10-3 sigmoid', 2, [10], ['sigmoid'], 3), ('8-32-32-4 tanh', 8, [32, 32], ['tanh', 'tanh'], 4),
        ('8-64-64-64-4 softplus', 8, [64, 64, 64], ['softplus'] * 3, 4)]


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
    ap.add_argument('--m', type=int, default=1 << 20)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ann.json'))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_ann.py needs the GPU: a CPU run says nothing about these times")
    from tests import ann_reference as ar
    dev = torch.device('cuda')
    m = args.m
    res = {'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'm': m, 'networks': []}
    for name, nf, widths, acts, nl in NETS:
        W, b = ar.random_net(nf, widths, nl, seed=1)
        ann = ar.make_ann([f'f{i}' for i in range(nf)], [f'l{i}' for i in range(nl)], widths, acts, W, b).setup()
        seq = ar.torch_sequential(W, b, acts).to(dev)
        X = torch.randn(nf, m, dtype=torch.float64, device=dev)
        Xt = X.t().contiguous()
        Y = torch.empty(nl, m, dtype=torch.float64, device=dev)
        with torch.no_grad():
            for _ in range(3):                                      # warm-up of both sides
                ann.predict(X, out=Y)
                yt = seq(Xt)
            err = float((Y.t() - yt).abs().max())
            # results before times: a slice of the queries against the numpy oracle within the bound of tests/test_ann_gpu.py,
            # and the two sides against each other within twice that bound
            nchk = min(m, 4096)
            ref, atol = ar.tolerance(X[:, :nchk].cpu().numpy(), W, b, acts)
            err_oracle = float(np.max(np.abs(Y[:, :nchk].cpu().numpy() - ref)))
            err_torch = float(np.max(np.abs(yt[:nchk].t().cpu().numpy() - ref)))
            assert err_oracle <= atol, f"{name}: ANN.predict differs from the oracle by {err_oracle:.3e} (bound {atol:.3e})"
            assert err_torch <= atol, f"{name}: torch differs from the oracle by {err_torch:.3e} (bound {atol:.3e})"
            t_hip = _time(lambda: ann.predict(X, out=Y), args.reps)
            t_torch = _time(lambda: seq(Xt), args.reps)
        dims = [nf] + widths + [nl]
        pad16 = lambda n: -(-n // 16) * 16
        mfma = sum((pad16(dims[k + 1]) // 16) * (pad16(dims[k]) // 4) for k in range(len(dims) - 1))    # per tile of 16 queries
        row = {'network': name, 'hip': dict(_summary(t_hip), queries_per_s=m / float(np.median(t_hip))),
               'torch_fp64': dict(_summary(t_torch), queries_per_s=m / float(np.median(t_torch))),
               'torch_over_hip': float(np.median(t_torch) / np.median(t_hip)), 'max_abs_difference': err,
               'checked_queries': nchk, 'hip_error_against_oracle': err_oracle, 'torch_error_against_oracle': err_torch,
               'oracle_bound': atol,
               'bytes_per_query': 8 * (nf + nl), 'hip_GBps_of_X_and_Y': 8 * (nf + nl) * m / float(np.median(t_hip)) * 1e-9,
               'mfma_per_16_queries': mfma, 'hip_mfma_per_s': mfma * (m / 16) / float(np.median(t_hip)),
               'exp_per_query': sum(w for w, a in zip(widths, acts) if a in ('sigmoid', 'tanh', 'softplus'))}
        res['networks'].append(row)
        print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == '__main__':
    main()
