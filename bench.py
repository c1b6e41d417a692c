#!/usr/bin/env python3
"""Benchmark of the hot path named by BASELINE.json: batched MPC / MHE / Kalman / GP steps per second.

    python bench.py --gpus N --steps K --warmup W [--config C2] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

`python bench.py --gpus N` with N > 1 and no WORLD_SIZE in the environment re-executes itself under
`torch.distributed.run` with one process per GPU (RCCL over xGMI for the one collective of a step).

Default workload = BASELINE.json configs[1] (SURVEY.md 8d "C2"): tracking NMPC on the CSTR-sized chemostat (nx=4, nu=2,
N=20), B=1024 instances PER GPU (weak scaling), closed loop, warm-started (mpc.py:725-726).  `--config` selects the other
configurations of SURVEY 8d, each printing its own JSON line:

  C1          LMPC double integrator (nx=2, nu=1, N=10), batch of 1024 QPs (+ single-instance latency in `config`)
  C2          tracking NMPC chemostat4, B = 1024 per GPU (weak)
  C3-mhe      MHE chemostat4 N=30, B = 4096 per GPU (weak): one add_measurements + estimate per step
  C3-ekf      EKF step chemostat4, B = 4096 per GPU (weak)      } HBM-bound: 8 (2 nx (nx+1) + 2 ny + nu + np) bytes per step
  C3-ukf      UKF step chemostat4, B = 4096 per GPU (weak)      }
  C4          GP-hybrid NMPC (GP with 200 training points inside the model), B = 2048 in total (strong sharding)
  C5          path-following NMPC robot6 N=50 with a soft constraint, B = 8192 in total (strong sharding): the ODE, pre-discretised
  C5-dae      BASELINE configuration 5 as it is written: the robot as a DAE (squared speed as algebraic state), the soft limit on the
              algebraic state, the reference's default transcription (collocation Radau 3, continuous objective), B = 8192 in total
  gp-predict  GaussianProcess.predict with variance, n = 200 training points, 2^18 query columns per GPU and step

A "step" of the harness is one pass of the configuration's hot call over the whole (sharded) batch + (closed loops) the plant
step + the per-step gather of (u0, status, iters); `value` = instances (or query columns) processed per second over the whole
job, inputs resident in HBM.

Every line carries
  roofline      the dominant kernel against the roof that bounds it: algorithmic flops (solves, GP) or
                algorithmic bytes (filters) per launch / the HIP-event time of that launch on the stream it runs on

A plain run sets up, warms up, times the K steps and prints the line.  `--full` adds what takes runs of its own:
  cpu_baseline  (N = 1 only, unless --no-cpu-baseline) the oracle's CPU restatement of the same computation on a bounded sample
                of the same workload
  settled_loop  (C2) the same closed loop continued for 50 more steps after the timed region
  single_instance_latency_us  (C1, in `config`) one QP solved alone, 20 timed calls

`--dump-outputs DIR` writes what the timed path computed in its last timed step - the arrays its caller receives - as
DIR/<name>.npy (float64; integer results converted).  The inputs are seeded, so two builds run with the same arguments can be
compared output for output.  Above 64 MB in all, every array keeps the same fixed, seeded sample of instances.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FP64_PEAK_TFLOPS = 78.6     # MI355X fp64 vector = fp64 matrix (MFMA) peak, dense
HBM_PEAK_GBS = 8000.0       # MI355X_MICROARCH.md
CONFIGS = ('C1', 'C2', 'C3-mhe', 'C3-ekf', 'C3-ukf', 'C4', 'C5', 'C5-dae', 'gp-predict')

# algorithmic flop model: per interior-point iteration and shooting interval
#   F_ric = 7/3 nx^3 + 4 nx^2 nu + 2 nx nu^2 + nu^3/3 + 8 nx^2 + 8 nx nu + 2 nu^2          
#   F_dyn = s (C_f + C_J + C_H) + s 2 nx^2 nz + s 4 nz^3        (RHS + Jacobian + contracted Hessian, chain rules)
# op counts of the right-hand sides (sympy CSE): chemostat4 C_f = 33, C_J = 60, C_H = 121; robot6 6 / 8 / 8;
# a GP term of n training points over two features adds n * 22 per stage point (kernel value, gradient, Hessian)
C_F, C_J, C_H = 33, 60, 121
MODEL_OPS = {'chemostat4': (33, 60, 121), 'robot6': (6, 8, 8), 'chemostat4_gp': (33 + 200 * 22, 60, 121)}


def f_ric(nx, nu):
    return 7 / 3 * nx ** 3 + 4 * nx ** 2 * nu + 2 * nx * nu ** 2 + nu ** 3 / 3 + 8 * nx ** 2 + 8 * nx * nu + 2 * nu ** 2


def flops_per_iteration(nx, nu, N, s=4, ops=(C_F, C_J, C_H)):
    """DESIGN model: includes the lambda-contracted Hessian of the shooting map (the exact-Hessian interior point needs it)."""
    nz = nx + nu
    f_dyn = s * sum(ops) + s * 2 * nx ** 2 * nz + s * 4 * nz ** 3
    return N * (f_ric(nx, nu) + f_dyn)


def flops_per_iteration_survey(nx, nu, N, s=4, ops=(C_F, C_J, C_H)):
    """SURVEY 8d formula as written: F_dyn = s (C_f + C_J + 2 nx^2 (nx + nu))."""
    return N * (f_ric(nx, nu) + s * (ops[0] + ops[1] + 2 * nx ** 2 * (nx + nu)))


STALE_BAND = (0.75, 1.33)    # a committed profile whose kernel ran this much faster / slower than this run's is not this kernel's


def _stale(profile_ns, kernel_ms):
    """The counters on the line come from COMMITTED rocprofv3 passes, not from this run (a counter pass cannot share a process with the
    timed region).  They belong to the kernel that was profiled: when this run's HIP-event time of the dominant kernel differs from the
    profile's by more than STALE_BAND (a changed kernel, another batch size), the counters are withheld and the line says why."""
    if profile_ns is None or kernel_ms is None or not profile_ns > 0:
        return None
    r = (kernel_ms * 1e6) / profile_ns
    if r < STALE_BAND[0] or r > STALE_BAND[1]:
        return f"withheld: the committed profile's kernel ran {profile_ns * 1e-6:.4g} ms, this run's {kernel_ms:.4g} ms - re-profile (profiles/run_round.sh)"
    return None


def pmc_traffic_bytes(tag_key, with_source=False, kernel_ms=None):
    """HBM bytes per launch of the dominant kernel from the COMMITTED rocprofv3 PMC passes (profiles/rNN_<config>_summary.json:
    FETCH_SIZE and WRITE_SIZE collected in separate --pmc runs of this same command), newest round first; None if this
    configuration has no committed PMC pass - or if that pass profiled a kernel of another duration than this run's (`_stale`).
    Not measured in this run: `traffic_source` of the line names the file.  Calibration: see DESIGN.md 5 (8-byte lanes: no 2x
    correction)."""
    import glob
    import re
    best, src = None, None
    files = [f for f in glob.glob(os.path.join(ROOT, 'profiles', f'r*_{tag_key}_summary.json'))
             if re.fullmatch(rf'r\d\d_{re.escape(tag_key)}_summary\.json', os.path.basename(f))]     # round tags only (r02, not r02a)
    if tag_key == 'C2':
        files += [f for f in glob.glob(os.path.join(ROOT, 'profiles', 'r*_summary.json'))
                  if re.fullmatch(r'r\d\d_summary\.json', os.path.basename(f))]                      # round 1's single summary
    for f in sorted(files, key=lambda q: os.path.basename(q)[:3]):
        try:
            d = json.load(open(f))
            best = (d['FETCH_SIZE_KB_per_launch']['warm_launches_mean'] + d['WRITE_SIZE_KB_per_launch']['warm_launches_mean']) * 1024
            src = f"committed profile profiles/{os.path.basename(f)} (separate --pmc passes of this command; not measured in this run)"
            why = _stale((d.get('timed_region') or {}).get('avg_ns'), kernel_ms)
            if why:
                best, src = None, f"profiles/{os.path.basename(f)} {why}"
        except Exception:
            pass
    return (best, src) if with_source else best


def pmc_issue(tag_key, kernel_key=None, kernel_ms=None):
    """Issue / matrix-core counters of the dominant kernel from the COMMITTED passes of profiles/run_pmc_valu.sh (newest round first):
    (dict of derived fractions, source) or (None, None).  Files: profiles/rNN_pmc_issue_<config>.json, and for C2 / gp-predict the
    older profiles/rNN_pmc_issue.json.  `mfma_busy_frac` = SQ_VALU_MFMA_BUSY_CYCLES / (1024 SIMDs x kernel duration in shader
    clocks) when the summary holds it (round 5 on), else None."""
    import glob
    import re
    cands = [f for f in glob.glob(os.path.join(ROOT, 'profiles', f'r*_pmc_issue_{tag_key}.json'))]
    if tag_key in ('C2', 'gp-predict'):
        cands += [f for f in glob.glob(os.path.join(ROOT, 'profiles', 'r*_pmc_issue.json'))]
    for f in sorted(cands, key=lambda q: os.path.basename(q)[:3], reverse=True):
        try:
            d = json.load(open(f))
            if kernel_key and kernel_key in d and isinstance(d[kernel_key], dict):
                d = d[kernel_key]
            out = {k: d[k] for k in ('mfma_busy_frac', 'valu_busy_frac', 'valu_insts_per_wave', 'lds_wait_frac', 'valu_issue_floor_frac') if k in d}
            if 'mfma_busy_frac' not in out and 'SQ_VALU_MFMA_BUSY_CYCLES' in d and 'kernel_cycles' in d:
                out['mfma_busy_frac'] = d['SQ_VALU_MFMA_BUSY_CYCLES']['steady_mean'] / (1024.0 * d['kernel_cycles'])
            if 'valu_busy_frac' not in out and 'SQ_ACTIVE_INST_VALU' in d and 'SQ_WAVE_CYCLES' in d:
                out['valu_busy_frac'] = d['SQ_ACTIVE_INST_VALU']['steady_mean'] / d['SQ_WAVE_CYCLES']['steady_mean']
            if out:
                why = _stale(d.get('kernel_ns_under_pmc'), kernel_ms)
                if why:
                    return None, f"profiles/{os.path.basename(f)} {why}"
                return out, (f"committed profile profiles/{os.path.basename(f)} (separate --pmc passes of "
                             f"`bench.py --config {tag_key}`; not measured in this run)")
        except Exception:
            pass
    return None, None


# ---------------------------------------------------------------------------------------------------------------------
# workloads: each returns dict(step=callable, events=list filled by step, finish=callable -> (extra config, roofline dict),
#                              units=instances per step on this rank, cpu=callable -> cpu_baseline dict,
#                              outputs=callable -> {name: (tensor, instance axis)} of the last step, for --dump-outputs)
# ---------------------------------------------------------------------------------------------------------------------
def _events(torch, n):
    return [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]


def _ipm_stats(torch, log):
    iters = torch.stack([i for i, _, _ in log]).to(torch.float64)
    status = torch.stack([s for _, s, _ in log])
    kkt = torch.stack([k for _, _, k in log])
    ok = ((status == 1) | (status == 2))
    return float(iters.mean().item()), float(ok.to(torch.float64).mean().item()), float(kkt[ok].max().item()) if bool(ok.any()) else float('nan')


def _solve_roofline(kernel, B, mean_iters, nx, nu, N, ops, kern_ms, tag, n_v, n_g, n_p, s=4):
    """Primary figures follow SURVEY 8d as written: flops = K N [F_ric + F_dyn], F_dyn = s (C_f + C_J + 2 nx^2 (nx + nu)); the count
    that also prices the lambda-contracted Hessian of the shooting map (what an exact-Hessian interior point evaluates, DESIGN.md
    5.1) is the secondary `frac_with_hessian`."""
    fl = B * mean_iters * flops_per_iteration(nx, nu, N, s=s, ops=ops)
    fl_s = B * mean_iters * flops_per_iteration_survey(nx, nu, N, s=s, ops=ops)
    tf = fl_s / (kern_ms * 1e-3) / 1e12
    bytes_launch = B * 8 * (2 * n_v + 2 * n_g + nx + n_p + nu)      # SURVEY 8d bytes_nmpc (compulsory)
    gbs = bytes_launch / (kern_ms * 1e-3) / 1e9
    traffic, src = pmc_traffic_bytes(tag, with_source=True, kernel_ms=kern_ms)
    issue, isrc = pmc_issue(tag, kernel_ms=kern_ms)
    return {"bound": "mfma", "achieved": tf, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": tf / FP64_PEAK_TFLOPS,
            "traffic": traffic, "traffic_source": src, "kernel": kernel, "kernel_ms": kern_ms,
            "mfma_busy_frac": (issue or {}).get('mfma_busy_frac'), "valu_busy_frac": (issue or {}).get('valu_busy_frac'),
            "mfma_busy_frac_source": isrc,
            "frac_with_hessian": fl / (kern_ms * 1e-3) / 1e12 / FP64_PEAK_TFLOPS,
            "algorithmic_flops_per_launch": fl_s,
            "note": "fp64 roof: MI355X fp64 vector peak == fp64 MFMA peak = 78.6 TFLOP/s; the solve is fp64 VALU/latency bound "
                    "(f64 MFMA for the Riccati stage products); algorithmic flops = B * mean_iters * N * (F_ric + F_dyn) with SURVEY "
                    "8d's F_dyn = s (C_f + C_J + 2 nx^2 (nx + nu)) in the reference's dimensions; `frac_with_hessian` adds the "
                    "contracted Hessian (s C_H + s 4 nz^3, DESIGN.md 5.1)",
            "hbm": {"achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
                    "algorithmic_bytes_per_launch": bytes_launch, "note": "compulsory bytes only; not the binding roof"}}


def host_cores():
    """The cores this process can actually use: the OpenMP runtime's count, the scheduler affinity AND the container's CPU quota
    (cgroup) bound it, whatever os.cpu_count() reports.  Returns (cores, quota)."""
    # threads pinned to cores (set before the OpenMP runtime of the baseline library starts)
    os.environ.setdefault('OMP_PROC_BIND', 'close')
    os.environ.setdefault('OMP_PLACES', 'cores')
    from oracle.cpu import max_threads
    quota = None
    try:
        q, per = open('/sys/fs/cgroup/cpu.max').read().split()
        quota = None if q == 'max' else float(q) / float(per)
    except Exception:
        pass
    C = min(max_threads(), len(os.sched_getaffinity(0)))
    if quota is not None:
        C = max(1, min(C, int(quota + 1e-9)))
    return C, quota


def cpu_model_name():
    try:
        return [ln.split(':', 1)[1].strip() for ln in open('/proc/cpuinfo') if ln.startswith('model name')][0]
    except Exception:
        return ''


def cpu_baseline_c2(spec, nst=50, slsqp=True, pb=None, label='C2', per_thread=64):
    """the C++17 / OpenMP Riccati interior point of oracle/cpu (validated against the numpy oracle in
    tests/test_cpu_baseline.py: same statuses, iteration counts and solutions) on the SAME closed-loop workload - 5 warm-up
    + `nst` timed warm-started steps - with all host cores and with one; plus scipy SLSQP on the identical transcribed NLP.
    `pb`: another tracking problem of the same shape (C4: the chemostat with the learned growth rate, oracle.cpu.set_gp first)."""
    C, quota = host_cores()
    from oracle.cpu import CpuNmpc
    from tests import problems as P
    pb = P.oracle_problem(spec) if pb is None else pb
    cpu = CpuNmpc(pb)

    def loop(nb, nt, nst=nst, nwarm=5):
        xs, v, t0, its = P.c2_x0(nb), None, 0.0, []
        for k in range(nwarm + nst):
            if k == nwarm:
                t0 = time.perf_counter()
            r = cpu.solve(xs, spec['p'], v0=v, n_threads=nt)
            xs, v = cpu.plant_step(xs, r['u0'], spec['p'], n_threads=nt), r['v']
            if k >= nwarm:
                its.append(r['iters'].mean())
        secs = time.perf_counter() - t0
        return nb * nst / secs, secs, float(np.mean(its)), float(np.mean((r['status'] == 1) | (r['status'] == 2)))
    nb_all = max(16 * per_thread, per_thread * C)       # at least `per_thread` instances per thread and call
    v_all, s_all, it_all, ok_all = loop(nb_all, C)
    n_one = min(nst, 20)
    v_one, s_one, _, _ = loop(2 * per_thread, 1, nst=n_one)
    slsqp_ms, sol = None, None
    if slsqp:
        # secondary reference point: an off-the-shelf dense NLP solver (scipy SLSQP) cold on one instance of the same NLP, with the
        # oracle's exact gradient and constraint Jacobian (x_0 substituted: the free variables of the oracle are v without x_0)
        from oracle.nmpc import DenseIpm
        from scipy.optimize import minimize
        ipm = DenseIpm(pb)
        data = {'x0': P.c2_x0(1) / pb.sx, 'p': np.atleast_2d(np.asarray(spec['p'], dtype=float))}
        lam0, cache = np.zeros((1, ipm.m)), {}

        def ev(w):
            k = w.tobytes()
            if k not in cache:
                cache.clear()
                f, g, c, J, _ = ipm.eval_all(w[None], lam0, data)
                cache[k] = (f[0], g[0], c[0], J[0])
            return cache[k]
        nx = pb.nx
        t0 = time.perf_counter()
        sol = minimize(lambda w: ev(w)[0], np.concatenate([np.tile(pb.x_guess, pb.N), np.tile(pb.u_guess, pb.N)]),
                       jac=lambda w: ev(w)[1], method='SLSQP', bounds=list(zip(pb.v_lb[nx:], pb.v_ub[nx:])),
                       constraints=[{'type': 'eq', 'fun': lambda w: ev(w)[2], 'jac': lambda w: ev(w)[3]}],
                       options={'ftol': 1e-12, 'maxiter': 500})
        slsqp_ms = (time.perf_counter() - t0) * 1e3
    return {"value": v_all, "unit": "steps/s", "cores": C, "kind": "port", "one_core_value": v_one,
            "cpu_model": cpu_model_name(), "cgroup_cpu_quota": quota, "sched_affinity_cpus": len(os.sched_getaffinity(0)),
            "mean_ipm_iters": it_all, "frac_status_1_or_2": ok_all,
            "slsqp_ms_per_solve": slsqp_ms, "slsqp_iterations": int(sol.nit) if sol is not None else None,
            "sample": f"oracle/cpu C++17/OpenMP Riccati interior point (same algorithm and constants as the numpy oracle, validated "
                      f"against it): {label} closed loop, {nb_all} instances x {nst} warm-started steps on {C} pinned threads = min(OpenMP, affinity, cgroup quota) ({s_all:.1f} s); "
                      f"one_core_value: {2 * per_thread} instances x {n_one} steps on 1 thread ({s_one:.1f} s)"
                      + (f"; slsqp: scipy SLSQP with the oracle's exact derivatives, cold, one instance of the same NLP (converged: "
                         f"{bool(sol.success)})" if sol is not None else "") + "; the reference's CasADi/IPOPT is not installable",
            "host_cpus": os.cpu_count()}


def cpu_leg_c5(spec, nst=20, per_thread=32, dae=False):
    """oracle/cpu/pf_cpu.cpp (C++17 / OpenMP: C5's transcription - path variable, soft speed limit - on the Riccati interior point of
    the other legs in the form the device engine uses, validated against oracle/nmpc_gen.py::GenIpm in tests/test_cpu_baseline.py)
    on the benchmark's own closed loop: warm-started from the previous solution, state advanced by the plant.
    dae=True: oracle/cpu/pfdae_cpu.cpp - configuration 5 as BASELINE writes it (the DAE under collocation with the soft limit on the
    algebraic state at the collocation points and the node; validated against oracle/nmpc_coll_gen.py)."""
    C, quota = host_cores()
    from oracle.cpu import CpuPathDaeNmpc, CpuPathNmpc
    from tests import problems as P
    if dae:
        cpu = CpuPathDaeNmpc(spec, P.oracle_coll_gen(spec))
        nst, per_thread = 8, 2           # a solve costs ~100 x the ODE leg's (21 x 21 collocation systems in second-order forward mode)
    else:
        cpu = CpuPathNmpc(spec, P.oracle_gen(spec))

    def loop(nb, nt, nst=nst, nwarm=3):
        xs, w, t0, its = P.c5_x0(nb), None, 0.0, []
        for k in range(nwarm + nst):
            if k == nwarm:
                t0 = time.perf_counter()
            r = cpu.solve(xs, w0=w, n_threads=nt)
            xs, w = cpu.plant_step(xs, r['u0'], n_threads=nt), r['w']
            if k >= nwarm:
                its.append(r['iters'].mean())
        secs = time.perf_counter() - t0
        return nb * nst / secs, secs, float(np.mean(its)), float(np.mean((r['status'] == 1) | (r['status'] == 2)))
    nb_all = max(4, 2 * C) if dae else max(min(64, 16 * per_thread), per_thread * C)
    v_all, s_all, it_all, ok_all = loop(nb_all, C)
    n_one, n_inst_one = (3, 2) if dae else (min(nst, 5), max(1, min(2 * per_thread, 16)))
    v_one, s_one, _, _ = loop(n_inst_one, 1, nst=n_one)
    return {"value": v_all, "unit": "steps/s", "cores": C, "kind": "port", "one_core_value": v_one,
            "cpu_model": cpu_model_name(), "cgroup_cpu_quota": quota, "sched_affinity_cpus": len(os.sched_getaffinity(0)),
            "mean_ipm_iters": it_all, "frac_status_1_or_2": ok_all,
            "sample": f"oracle/cpu C++17/OpenMP Riccati interior point on C5's transcription{' AS BASELINE WRITES IT (DAE, collocation Radau 3, rows at the collocation points)' if dae else ''} (path variable and slack as engine states, "
                      f"inequality rows with IPOPT's slacks; validated against the dense numpy oracle): closed loop, {nb_all} instances "
                      f"x {nst} warm-started steps on {C} pinned threads = min(OpenMP, affinity, cgroup quota) ({s_all:.1f} s); "
                      f"one_core_value: {n_inst_one} instances x {n_one} steps on 1 thread ({s_one:.1f} s); the reference's "
                      f"CasADi/IPOPT is not installable", "host_cpus": os.cpu_count()}


def cpu_leg_mhe(spec, nst=40, per_thread=128):
    """oracle/cpu/mhe_cpu.cpp (C++17 / OpenMP: the estimator's transcription on the Riccati interior point of the NMPC leg, validated
    against oracle/mhe.py in tests/test_cpu_baseline.py) on the benchmark's own loop: window filled, one cold estimate, then per step
    one new sample shifts the window, arrival guess = x_2 of the previous solution, warm start = the previous solution."""
    C, quota = host_cores()
    from oracle.cpu import CpuMhe
    from tests import problems as P
    pb = P.oracle_mhe(spec)
    cpu = CpuMhe(pb)
    npar, nx = pb.np_, pb.nx

    def loop(nb, nt, nst=nst, nwarm=3):
        xa, u, y, _ = P.c3_data(nb, seed=11)
        noise = .01 * np.random.default_rng(5).normal(size=(64, nb, 2))
        r = cpu.solve(xa, spec['p'], u, y, n_threads=nt)
        t0, its = 0.0, []
        for k in range(nwarm + nst):
            if k == nwarm:
                t0 = time.perf_counter()
            y = np.concatenate([y[:, 1:], (y[:, -1] + noise[k % 64])[:, None]], axis=1)
            u = np.concatenate([u[:, 1:], u[:, -1:]], axis=1)
            r = cpu.solve(r['v'][:, npar + 2 * nx:npar + 3 * nx], spec['p'], u, y, v0=r['v'], n_threads=nt)
            if k >= nwarm:
                its.append(r['iters'].mean())
        secs = time.perf_counter() - t0
        return nb * nst / secs, secs, float(np.mean(its)), float(np.mean((r['status'] == 1) | (r['status'] == 2)))
    nb_all = max(min(256, 16 * per_thread), per_thread * C)
    v_all, s_all, it_all, ok_all = loop(nb_all, C)
    n_one = min(nst, 10)
    n_inst_one = max(1, min(2 * per_thread, 128))
    v_one, s_one, _, _ = loop(n_inst_one, 1, nst=n_one)
    return {"value": v_all, "unit": "steps/s", "cores": C, "kind": "port", "one_core_value": v_one,
            "cpu_model": cpu_model_name(), "cgroup_cpu_quota": quota, "sched_affinity_cpus": len(os.sched_getaffinity(0)),
            "mean_ipm_iters": it_all, "frac_status_1_or_2": ok_all,
            "sample": f"oracle/cpu C++17/OpenMP Riccati interior point on the estimator's transcription (same algorithm and constants as "
                      f"the numpy oracle, validated against it): C3 window loop, {nb_all} instances x {nst} warm-started estimates on "
                      f"{C} pinned threads = min(OpenMP, affinity, cgroup quota) ({s_all:.1f} s); one_core_value: {n_inst_one} "
                      f"instances x {n_one} estimates on 1 thread ({s_one:.1f} s); the reference's CasADi/IPOPT is not installable",
            "host_cpus": os.cpu_count()}


def cpu_leg_kf(kind, K, budget=6., min_batch=4096):
    # oracle/cpu/kf_cpu.cpp (C++17 / OpenMP, validated against oracle/kf.py in tests/test_cpu_baseline.py): the same K sampling
    # instants per call for a larger batch, all host cores and one
    from oracle.cpu import kf_steps
    from oracle import kf as okf
    C, quota = host_cores()
    nb = max(min_batch, (min_batch // 2) * C)
    rs = np.random.default_rng(5)
    xs = np.array([.1, 40., .5, .2]) * (1 + .1 * rs.uniform(-1, 1, (nb, 4)))
    xP = okf.pack(xs, np.tile(np.eye(4), (nb, 1, 1)))
    yy = xs[None, :, [0, 2]] * (1 + .02 * rs.normal(size=(K, nb, 2)))
    uu, pp = rs.uniform(0, .3, (nb, 2)), np.tile([100., 4., 1., 0.], (nb, 1))

    def run(nt, budget):
        kf_steps(kind, xP, yy, uu, pp, 1e-4, 1e-2, dt=1., n_threads=nt)
        t0, n = time.perf_counter(), 0
        while time.perf_counter() - t0 < budget:
            kf_steps(kind, xP, yy, uu, pp, 1e-4, 1e-2, dt=1., n_threads=nt)
            n += 1
        secs = time.perf_counter() - t0
        return n * nb * K / secs, secs, n
    v_all, s_all, n_all = run(C, budget)
    v_one, s_one, n_one = run(1, budget * 2 / 3)
    return {"value": v_all, "unit": "steps/s", "cores": C, "kind": "port", "one_core_value": v_one,
            "cpu_model": cpu_model_name(), "cgroup_cpu_quota": quota,
            "sample": f"oracle/cpu C++17/OpenMP {kind.upper()} (validated against the numpy oracle): {n_all} calls x {nb} instances x "
                      f"{K} filter steps on {C} pinned threads ({s_all:.1f} s); one_core_value: {n_one} calls on 1 thread ({s_one:.1f} s)",
            "host_cpus": os.cpu_count()}


def cpu_leg_gp(Xq, budget=6.):
    # oracle/cpu/gp_cpu.cpp (C++17 / OpenMP over blocks of query columns; validated against oracle/gp.py::Posterior.predict in
    # tests/test_cpu_baseline.py) on query columns of the benchmark's own draw, all host cores and one
    from oracle.cpu import gp_predict
    from tests import problems as P
    C, quota = host_cores()
    post = P.oracle_c4()[1]
    mq = Xq.shape[1]

    def run(nt, budget):
        gp_predict(post, Xq, n_threads=nt)
        t0, n = time.perf_counter(), 0
        while time.perf_counter() - t0 < budget:
            gp_predict(post, Xq, n_threads=nt)
            n += 1
        secs = time.perf_counter() - t0
        return n * mq / secs, secs, n
    v_all, s_all, n_all = run(C, budget)
    v_one, s_one, n_one = run(1, budget * 2 / 3)
    return {"value": v_all, "unit": "predictions/s", "cores": C, "kind": "port", "one_core_value": v_one,
            "cpu_model": cpu_model_name(), "cgroup_cpu_quota": quota,
            "sample": f"oracle/cpu C++17/OpenMP prediction (mean + variance; validated against the numpy oracle): {n_all} calls x {mq} query "
                      f"columns on {C} pinned threads ({s_all:.1f} s); one_core_value: {n_one} calls on 1 thread ({s_one:.1f} s)",
            "host_cpus": os.cpu_count()}


def cpu_leg_qp(budget=6., min_batch=4096, warmup=5, steps=50):
    # oracle/cpu/qp_cpu.cpp (C++17 / OpenMP; the kernels' predictor-corrector iteration, validated against oracle/lmpc.py in
    # tests/test_cpu_baseline.py) on THE SAME closed loop as the GPU line: measured states drawn uniformly in [-4, 4]^2 with the
    # benchmark's seed, then warm-up + timed steps x+ = A x + B u_0 of the command - status fractions and iteration counts are
    # those of the loop's TIMED steps, like the GPU line's; all host cores and one
    from oracle.cpu import qp_solve
    from oracle.lmpc import LmpcProblem
    from tests.problems import C1, LMPC_A, LMPC_B
    C, quota = host_cores()
    pb = LmpcProblem(**C1, kron_bug=False)
    nb = max(min_batch, (min_batch // 4) * C)
    x_start = np.random.default_rng(20260926).uniform(-4, 4, (nb, 2))
    iu = pb.u_ind[0]
    loop_steps = warmup + steps

    def loop(nt):
        """one closed loop of `loop_steps` steps over the batch; returns (iterations, status) of all its solves"""
        x, its, sts = x_start, [], []
        for _ in range(loop_steps):
            lb = np.tile(pb.v_lb, (nb, 1))
            ub = np.tile(pb.v_ub, (nb, 1))
            lb[:, pb.x_ind[0]] = ub[:, pb.x_ind[0]] = x / pb.sx                       # mpc.py:2361-2362
            r = qp_solve(pb.H, pb.g, pb.Aeq, pb.beq, lb, ub, tol=1e-12, reg=1e-12, n_threads=nt)
            its.append(r['iters'])
            sts.append(r['status'])
            x = x @ LMPC_A.T + (r['x'][:, iu] * pb.su) @ LMPC_B.T
        return np.concatenate(its[warmup:]), np.concatenate(sts[warmup:])

    def run(nt, budget):
        loop(nt)
        t0, n = time.perf_counter(), 0
        while time.perf_counter() - t0 < budget:
            its, sts = loop(nt)
            n += 1
        secs = time.perf_counter() - t0
        return n * loop_steps * nb / secs, secs, n, its, sts
    v_all, s_all, n_all, its, sts = run(C, budget)
    v_one, s_one, n_one, _, _ = run(1, budget * 2 / 3)
    return {"value": v_all, "unit": "steps/s", "cores": C, "kind": "port", "one_core_value": v_one,
            "cpu_model": cpu_model_name(), "cgroup_cpu_quota": quota, "mean_qp_iters": float(its.mean()),
            "frac_status_1": float((sts == 1).mean()),
            "sample": f"oracle/cpu C++17/OpenMP dense predictor-corrector QP (the kernels' iteration and tolerances) on the benchmark's own "
                      f"closed loop (same draw of measured states, {loop_steps} steps): {n_all} loops x {loop_steps} steps x {nb} QPs on {C} "
                      f"pinned threads ({s_all:.1f} s, host-side assembly of the bound rows included); one_core_value: {n_one} loops on 1 "
                      f"thread ({s_one:.1f} s); the reference's CasADi/qpOASES is not installable", "host_cpus": os.cpu_count()}


def wl_nmpc(cfg, args, torch, dev, rank, world):
    from hilo_mpc_amd.dist import ClosedLoop, shard_range
    from tests import problems as P
    if cfg == 'C2':
        spec, B, gB = P.C2, args.batch or 1024, (args.batch or 1024) * world
        nmpc = P.product_nmpc(spec)
        x0 = P.c2_x0(B, seed=P.SEED + rank)
        kernel, model, ex, eu = "ocp_solve_kernel<NmpcTrack<Chemostat4>, 64>", 'chemostat4', 4, 2
        workload = "C2 tracking NMPC chemostat4 nx=4 nu=2 N=20 rk4+discrete, closed loop warm-started"
    elif cfg == 'C4':
        spec, gB = P.C4, args.batch or 2048
        lo, hi = shard_range(gB, rank, world)
        B = hi - lo
        nmpc = P.product_nmpc(spec)
        x0 = P.c2_x0(gB)[lo:hi]
        kernel, model, ex, eu = "ocp_solve_kernel<NmpcTrack<Chemostat4Gp>, 64>", 'chemostat4_gp', 4, 2
        workload = "C4 GP-hybrid NMPC chemostat4 + GP(200 points, SE-ARD) nx=4 nu=2 N=20, closed loop warm-started"
    elif cfg == 'C5-dae':
        spec, gB = P.C5D, args.batch or 8192
        lo, hi = shard_range(gB, rank, world)
        B = hi - lo
        nmpc = P.product_gen(spec)
        x0 = P.c5_x0(gB)[lo:hi]
        kernel, model, ex, eu = ("hilo_user_solve (general policy NmpcUser<robot6 DAE, path variable, soft constraint on the algebraic "
                                 "state, collocation Radau 3>, compiled at run time)"), 'robot6', 7, 3
        workload = ("C5 as BASELINE writes it: path-following NMPC on the robot's DAE (algebraic state z = vx^2 + vy^2, soft limit z <= 4 at "
                    "the 3 collocation points and the node of every interval), collocation Radau 3 with the continuous objective, N=50; "
                    "collocation and algebraic states eliminated inside the shooting map, iterate in a global-memory workspace, closed "
                    "loop warm-started")
    else:
        spec, gB = P.C5, args.batch or 8192
        lo, hi = shard_range(gB, rank, world)
        B = hi - lo
        nmpc = P.product_gen(spec)
        x0 = P.c5_x0(gB)[lo:hi]
        # flops with the REFERENCE's dimensions: nx = 6 + theta = 7, nu = 2 + u_theta = 3 (the slack is one variable of v there, not a state)
        kernel, model, ex, eu = "hilo_user_solve (general policy NmpcUser<Robot6, path variable, soft constraint>, compiled at run time)", 'robot6', 7, 3
        workload = ("C5 path-following NMPC robot6 (ODE; engine nx=6+theta+slack, nu=2+u_theta) N=50 soft constraint, Riccati "
                    "interior point with the iterate in a global-memory workspace, closed loop warm-started")
    N = nmpc.horizon
    x = torch.as_tensor(x0, device=dev)
    p = torch.as_tensor(np.asarray(spec['p'], dtype=np.float64), device=dev) if len(spec['p']) else None
    # the closed loop of a shard (hilo_mpc_amd/dist.py::ClosedLoop; the same object tests/test_dist_cpu.py drives with a stub
    # controller over gloo): one hilo_nmpc_solve launch for the whole shard, the one collective of the step (RCCL all-gather;
    # plain tracking problems: the solve writes the gather rows itself), the plant step
    loop = ClosedLoop(nmpc, gB if cfg != 'C2' else B * world, nmpc._n_u, rank, world, dev, x, p)
    ev, log = [], []

    def step(timed):
        e = _events(torch, 1)[0]        # warm-up steps run the identical path (event creation included)
        loop.step(before=e[0].record, after=e[1].record)
        if timed:
            ev.append(e)
            sol = nmpc._nlp_solution
            log.append((sol['iter_count'], sol['status'], sol['kkt_error']))

    def finish():
        kern_ms = float(np.mean([a.elapsed_time(b) for a, b in ev]))
        mean_iters, ok_frac, kkt_max = _ipm_stats(torch, log)
        roof = _solve_roofline(kernel, B, mean_iters, ex, eu, N, MODEL_OPS[model], kern_ms, cfg, nmpc._n_v, nmpc._n_g, len(spec['p']),
                               s=3 if cfg == 'C5-dae' else 4)
        extra = {"workload": workload, "batch_per_gpu": B, "global_batch": gB if cfg != 'C2' else B * world,
                 "parallelism": f"instances sharded x{world}", "mean_ipm_iters": mean_iters, "frac_status_1_or_2": ok_frac,
                 "max_kkt_error": kkt_max}
        return extra, roof, ("weak" if cfg == 'C2' else "strong")

    def cpu():
        if cfg == 'C2':
            return cpu_baseline_c2(spec)
        if cfg == 'C5':
            return cpu_leg_c5(spec)
        if cfg == 'C5-dae':
            return cpu_leg_c5(spec, dae=True)
        else:
            # the C++ baseline with the learned growth rate (oracle/cpu/models_cpu.h::Chemostat4Gp, validated against the numpy oracle)
            from oracle.cpu import set_gp
            pb, post = P.oracle_c4()
            Xtr, _ = P.c4_training_data()
            set_gp(Xtr, post.alpha, P.C4_GP['length_scales'], P.C4_GP['signal_variance'])
            return cpu_baseline_c2(spec, nst=10, slsqp=False, pb=pb, label='C4 (200 kernel terms per right-hand side)', per_thread=8)

    def outputs():
        # what the closed loop hands its caller (the gathered rows of all shards), the shard's advanced plant states and the solution
        g, sol = loop.last, nmpc._nlp_solution
        out = {'u0': (g.u0, 0), 'status': (g.status, 0), 'iters': (g.iters, 0), 'x_next': (loop.x, 0)}
        out.update({'nlp_' + k: (sol[k], 0) for k in ('x', 'f', 'lam_g', 'kkt_error') if sol.get(k) is not None})
        return out
    return dict(step=step, finish=finish, units=B, cpu=cpu, outputs=outputs, unit="steps/s",
                metric="MPC steps/sec (batched instances, whole node) at fixed (nx,nu,N)")


def wl_mhe(args, torch, dev, rank, world):
    from tests import problems as P
    from tests.problems import product_mhe
    spec, B = P.C3B, args.batch or 4096
    xa, u, y, xt = P.c3_data(B, seed=11 + rank)
    mhe = product_mhe(spec)
    N = spec['N']
    yd, ud = torch.as_tensor(y, device=dev), torch.as_tensor(u, device=dev)
    for k in range(N):
        mhe.add_measurements(yd[:, k], ud[:, k])
    mhe.estimate(x_arrival=torch.as_tensor(xa, device=dev))
    rng = np.random.default_rng(5 + rank)
    noise = torch.as_tensor(.01 * rng.normal(size=(64, B, 2)), device=dev)
    ev, log, cnt, last = [], [], [0], [None]

    def step(timed):
        k = cnt[0] % 64
        cnt[0] += 1
        mhe.add_measurements(yd[:, -1] + noise[k], ud[:, -1])      # window shifts by one sample (device ring buffer)
        e = _events(torch, 1)[0]        # warm-up steps run the identical path (event creation included)
        e[0].record()
        last[0] = mhe.estimate()
        e[1].record()
        if timed:
            ev.append(e)
            s = mhe._nlp_solution
            log.append((s['iter_count'], s['status'], s['kkt_error']))

    def finish():
        kern_ms = float(np.mean([a.elapsed_time(b) for a, b in ev]))
        mean_iters, ok_frac, kkt_max = _ipm_stats(torch, log)
        roof = _solve_roofline("ocp_solve_kernel<MheNoise<Chemostat4>, 64>", B, mean_iters, 4, 4, N, MODEL_OPS['chemostat4'], kern_ms,
                               'C3-mhe', mhe._n_v, mhe._n_g, 4 + 4 * N)
        extra = {"workload": "C3 MHE chemostat4 nx=4 ny=2 N=30 with state noise (boxed), one new sample per step, warm-started",
                 "batch_per_gpu": B, "global_batch": B * world, "parallelism": f"instances sharded x{world}",
                 "mean_ipm_iters": mean_iters, "frac_status_1_or_2": ok_frac, "max_kkt_error": kkt_max}
        return extra, roof, "weak"

    def cpu():
        return cpu_leg_mhe(spec)

    def outputs():
        (x_est, p_est), sol = last[0], mhe._nlp_solution
        out = {'x_est': (x_est, 0), 'p_est': (p_est, 0)}
        out.update({'nlp_' + k: (sol[k], 0) for k in ('x', 'f', 'lam_g', 'status', 'iter_count', 'kkt_error') if sol.get(k) is not None})
        return out
    return dict(step=step, finish=finish, units=B, cpu=cpu, outputs=outputs, unit="steps/s",
                metric="MHE estimates/sec (batched instances, whole node) at fixed (nx,ny,N)")


def wl_kf(kind, args, torch, dev, rank, world):
    from hilo_mpc_amd import EKF, UKF, Model
    B = args.batch or 4096
    rng = np.random.default_rng(20260926 + rank)
    x = np.array([.1, 40., .5, .2]) * (1 + .1 * rng.uniform(-1, 1, (B, 4)))
    Pm = np.tile(np.eye(4), (B, 1, 1))
    f = (EKF if kind == 'ekf' else UKF)(Model('chemostat4').discretize('rk4').setup(dt=1.))
    f.setup()
    f.Q, f.R = 1e-4, 1e-2
    f.set_initial_guess(torch.as_tensor(x, device=dev), P0=torch.as_tensor(Pm, device=dev))
    u = torch.as_tensor(rng.uniform(0, .3, (B, 2)), device=dev)
    p = torch.as_tensor(np.tile([100., 4., 1., 0.], (B, 1)), device=dev)
    # K filter steps per launch: the reference's `mapaccum(steps)` (kf.py:296-306), hilo_kf_steps - measurements of K sampling
    # instants handed over at once (a filter step at this batch is launch-latency bound)
    K = max(1, int(getattr(args, 'kf_steps', 16) or 16))
    ybase = torch.as_tensor(x[:, [0, 2]], device=dev)
    ynoise = torch.as_tensor(.02 * rng.normal(size=(4, K, B, 2)), device=dev)
    ys = [ybase[None] * (1 + ynoise[q]) for q in range(4)]
    # A launch here lasts tens of microseconds and creating + recording a pair of HIP events costs the host about as much: one
    # event pair brackets G consecutive launches (G divides the number of timed steps), the launch duration is elapsed / G -
    # inter-launch gaps included, so it can only be longer than the kernel's own time (the rocprofv3 summary holds that)
    G = max(g for g in (1, 2, 3, 4, 5) if args.steps % g == 0)
    ev, cnt, nt, cur = [], [0], [0], [None]

    def step(timed):
        y = ys[cnt[0] % 4]
        cnt[0] += 1
        first = last = True
        if timed:
            first, last = nt[0] % G == 0, nt[0] % G == G - 1
            nt[0] += 1
        if first:
            cur[0] = _events(torch, 1)[0]
            cur[0][0].record()
        if K > 1:
            f.estimate(y=y, u=u, p=p, steps=K)
        else:
            f.estimate(y=y[0], u=u, p=p)
        if last:
            cur[0][1].record()
            if timed:
                ev.append(cur[0])

    def finish():
        kern_ms = float(np.sum([a.elapsed_time(b) for a, b in ev])) / (len(ev) * G)
        nx, ny, nu, npar = 4, 2, 2, 4
        bytes_step = 8 * (2 * nx * (nx + 1) + 2 * ny + nu + npar)          # SURVEY 8d bytes_kf
        gbs_eq = B * K * bytes_step / (kern_ms * 1e-3) / 1e9
        comp = B * 8 * ((nx * (nx + 1) + 2 * ny) * K + nx * (nx + 1) + nu + npar + nx * nx + ny * ny)
        gbs = comp / (kern_ms * 1e-3) / 1e9
        # primary figure: the bytes ONE launch must move (compulsory) against the HBM peak; the per-step formula of SURVEY 8d times K
        # is an equivalent bandwidth (what K separate steps would move) and is carried as the secondary figure
        roof = {"bound": "hbm", "achieved": gbs, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": gbs / HBM_PEAK_GBS,
                "equivalent_achieved": gbs_eq, "equivalent_frac": gbs_eq / HBM_PEAK_GBS,
                "traffic": pmc_traffic_bytes('C3-' + kind, kernel_ms=kern_ms), "traffic_source": pmc_traffic_bytes('C3-' + kind, with_source=True, kernel_ms=kern_ms)[1],
                # csrc/hilo_kf.hip::use_team: a team of lanes per instance (4 for the EKF's Jacobian columns, 16 for the UKF's 9
                # sigma points) up to two waves per SIMD of teams, one instance per lane beyond
                "kernel": (f"kf_team_kernel<Chemostat4, {'true' if kind == 'ukf' else 'false'}>"
                           if B * (16 if kind == 'ukf' else 4) <= 2 * 1024 * 64 else
                           # `discretize('rk4')` with shared Q, R: the multi-step kernels' LEAN variants (csrc/hilo_kf.hip::launch_multi)
                           (("kf_multi_kernel<Chemostat4, true, 2>" if B >= 2 * 1024 * 64 else "kf_multi_kernel<Chemostat4, true, 1>") if kind == 'ukf' else "ekf_multi_lean_kernel<Chemostat4>") if K > 1 else
                           f"kf_kernel<Chemostat4, {'true' if kind == 'ukf' else 'false'}, 2>"),
                "kernel_ms": kern_ms, "launches_per_event_pair": G, "algorithmic_bytes_per_launch": B * K * bytes_step,
                "filter_steps_per_launch": K,
                # one instance per lane (B >= 2^20): what binds is the fp64 issue rate, not HBM - `valu_issue_floor_frac` = 4 clocks x
                # VALU instructions / (1024 SIMDs x kernel clocks) from the committed counter passes of the same command
                **({"issue_counters": pmc_issue(f'C3-{kind}_B1M', kernel_ms=kern_ms)[0],
                    "issue_counters_source": pmc_issue(f'C3-{kind}_B1M', kernel_ms=kern_ms)[1]} if B >= (1 << 20) and K > 1 else {}),
                "compulsory_bytes_per_launch": comp,
                "note": "`achieved` / `frac`: the bytes one launch must move (tile in once, y in and tile + y_pred out per step, "
                        "[u; p], Q, R = `compulsory_bytes_per_launch`) per launch time against the HBM peak.  bytes_kf = 8 (2 nx "
                        "(nx+1) + 2 ny + nu + np) per filter step (SURVEY 8d) times K steps is what K separate steps would move: "
                        "`equivalent_achieved` / `equivalent_frac` (the tile stays on chip between the K steps of a launch); at the configuration's B = 4096 a launch is "
                        "bound by the latency of one instance's dependent chain (DESIGN 5.2); `--batch 1048576` measures the "
                        "bandwidth-bound regime"}
        extra = {"workload": f"C3 {kind.upper()} step chemostat4 nx=4 ny=2 (predict + update fused, {K} sampling instants per "
                             f"launch like the reference's mapaccum(steps)), Q = 1e-4 I, R = 1e-2 I",
                 "batch_per_gpu": B, "global_batch": B * world, "parallelism": f"instances sharded x{world}"}
        return extra, roof, "weak"

    def cpu():
        return cpu_leg_kf(kind, K)

    def outputs():
        # the call's solution: the sequences over its K sampling instants (K > 1: [K, B, ...]) or the one step's ([B, ...])
        ax = 1 if K > 1 else 0
        return {'x': (f.solution['x'], ax), 'P': (f.solution['P'], ax), 'y_pred': (f.solution['y'], ax)}
    return dict(step=step, finish=finish, units=B * K, cpu=cpu, outputs=outputs, unit="steps/s",
                metric="Kalman filter steps/sec (batched instances, whole node)")


def wl_gp(args, torch, dev, rank, world):
    from tests import problems as P
    gp = P.product_gp()
    m = args.batch or (1 << 18)
    rng = np.random.default_rng(3 + rank)
    Xq = torch.as_tensor(np.stack([rng.uniform(0, 40, m), rng.uniform(0, 4, m)]), device=dev)
    n, nf = 200, 2
    ev, last = [], [None]

    def step(timed):
        e = _events(torch, 1)[0]        # warm-up steps run the identical path (event creation included)
        e[0].record()
        last[0] = gp.predict(Xq)
        e[1].record()
        if timed:
            ev.append(e)

    def finish():
        kern_ms = float(np.mean([a.elapsed_time(b) for a, b in ev]))
        fl_q = n * (3 * nf + 20) + 2 * n + n * n                        # mean + triangular product per query
        tf = m * fl_q / (kern_ms * 1e-3) / 1e12
        by = m * 8 * (nf + 2)
        roof = {"bound": "mfma", "achieved": tf, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": tf / FP64_PEAK_TFLOPS,
                "traffic": pmc_traffic_bytes('gp-predict', kernel_ms=kern_ms), "traffic_source": pmc_traffic_bytes('gp-predict', with_source=True, kernel_ms=kern_ms)[1], "kernel": "gp_predict_kernel", "kernel_ms": kern_ms,
                "mfma_busy_frac": (pmc_issue('gp-predict', 'gp_predict_reg_kernel', kernel_ms=kern_ms)[0] or {}).get('mfma_busy_frac'),
                "mfma_busy_frac_source": pmc_issue('gp-predict', 'gp_predict_reg_kernel', kernel_ms=kern_ms)[1],
                "note": "fp64 compute roof: flops per query = n (3 nf + 20) + 2 n (mean) + n^2 (|L^-1 k*|^2), n = 200; "
                        "compulsory HBM traffic is 8 (nf + 2) bytes per query (arithmetic intensity ~1400 flop/B)",
                "hbm": {"achieved": by / (kern_ms * 1e-3) / 1e9, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": by / (kern_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, "algorithmic_bytes_per_launch": by}}
        extra = {"workload": "GaussianProcess.predict (mean + variance), SE-ARD kernel, n = 200 training points, nf = 2",
                 "queries_per_gpu": m, "global_queries": m * world, "parallelism": f"query columns sharded x{world}"}
        return extra, roof, "weak"

    def cpu():
        return cpu_leg_gp(Xq[:, :1 << 16].cpu().numpy())

    def outputs():
        mean, var = last[0]
        return {'mean': (mean, 1), 'var': (var, 1)}
    return dict(step=step, finish=finish, units=m, cpu=cpu, outputs=outputs, unit="predictions/s",
                metric="GP predictions/sec (query columns with variance, whole node)")


def wl_lmpc(args, torch, dev, rank, world):
    from tests.problems import product_lmpc
    B = args.batch or 1024
    mpc = product_lmpc('corrected')
    rng = np.random.default_rng(20260926 + rank)
    x = torch.as_tensor(rng.uniform(-4, 4, (B, 2)), device=dev)
    AdT = torch.as_tensor(np.array([[1., .5], [0., 1.]]).T.copy(), device=dev)       # the plant x+ = A x + B u, row vectors
    BdT = torch.as_tensor(np.array([[.125], [.5]]).T.copy(), device=dev)
    ev, log, solved, last = [], [], [], [None]

    def step(timed):
        nonlocal x
        e = _events(torch, 1)[0]        # warm-up steps run the identical path (event creation included)
        e[0].record()
        u = last[0] = mpc.optimize(x)
        e[1].record()
        if timed:
            ev.append(e)
            log.append(mpc._nlp_solution['iter_count'])
            solved.append(mpc._nlp_solution['status'])          # (device tensors: looked at after the timed region)
        x = torch.addmm(torch.mm(u, BdT), x, AdT)        # (two launches; the step is bound by the host's time)

    def finish():
        kern_ms = float(np.mean([a.elapsed_time(b) for a, b in ev]))
        iters = float(torch.stack(log).double().mean().item())
        # flops = K N F_ric(nx, nu), no model evaluation in a linear MPC; the kernel takes its Newton steps by that
        # recursion (csrc/hilo_qp_ocp.h) when the QP has the stage shape, else (HILO_QP_DENSE=1) the dense count applies
        nx_, nu_, N_ = 2, 1, 10
        staged = bool(getattr(mpc, '_qp_stages', False))
        n, mq = 32, 20
        fl_it = (N_ * (7 / 3 * nx_ ** 3 + 4 * nx_ * nx_ * nu_ + 2 * nx_ * nu_ * nu_ + nu_ ** 3 / 3 + 8 * nx_ * nx_ + 8 * nx_ * nu_ + 2 * nu_ * nu_)
                 if staged else 2 * mq * mq * n + mq ** 3 / 3 + 4 * mq * mq + 6 * n * mq)
        tf = B * iters * fl_it / (kern_ms * 1e-3) / 1e12
        latency = {}
        if args.full:           # one QP alone: a run of its own
            one = product_lmpc('corrected')
            x1 = torch.as_tensor(np.array([[1., 1.]]), device=dev)
            for _ in range(3):
                one.optimize(x1)
            torch.cuda.synchronize(dev)
            e1 = _events(torch, 20)
            for a, b in e1:
                a.record()
                one.optimize(x1)
                b.record()
            torch.cuda.synchronize(dev)
            latency["single_instance_latency_us"] = float(np.mean([a.elapsed_time(b) for a, b in e1])) * 1e3
        roof = {"bound": "mfma", "achieved": tf, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": tf / FP64_PEAK_TFLOPS,
                "traffic": pmc_traffic_bytes('C1', kernel_ms=kern_ms), "traffic_source": pmc_traffic_bytes('C1', with_source=True, kernel_ms=kern_ms)[1],
                "kernel": "qp_ocp_kernel<2, 1, 16>" if staged else "qp_solve_reg_kernel<32, 24>", "kernel_ms": kern_ms,
                "flops_per_iteration": fl_it,
                "note": ("Mehrotra predictor-corrector with the Newton step by a Riccati recursion over the 10 stages (a stage per "
                         "lane, 4 QPs per wave): flops per iteration = N F_ric(nx, nu) of SURVEY 8(d) = 890 - a chain of 10 "
                         "dependent 2x2 steps is latency bound, the figure of merit is `single_instance_latency_us`") if staged else
                        ("dense Mehrotra predictor-corrector, 32 variables / 20 equalities: flops per iteration = 2 m^2 n + m^3/3 "
                         "+ 4 m^2 + 6 n m; a 32-variable QP per workgroup is latency bound")}
        extra = {"workload": "C1 LMPC discrete double integrator nx=2 nu=1 N=10 (corrected input block), closed loop from x0 drawn "
                             "uniformly in [-4, 4]^2: about 5 % of these measured states cannot keep the box (infeasible QPs, reported "
                             "as status 3 after a few iterations - `frac_status_1` is the rest)",
                 "batch_per_gpu": B, "global_batch": B * world, "mean_qp_iters": iters, "frac_status_1": float((torch.stack(solved) == 1).double().mean().item()),
                 **latency}
        return extra, roof, "weak"

    def cpu():
        return cpu_leg_qp(warmup=args.warmup, steps=args.steps)

    def outputs():
        sol = mpc._nlp_solution
        out = {'u0': (last[0], 0), 'x_next': (x, 0)}
        out.update({'nlp_' + k: (sol[k], 0) for k in ('x', 'f', 'status', 'iter_count') if sol.get(k) is not None})
        return out
    return dict(step=step, finish=finish, units=B, cpu=cpu, outputs=outputs, unit="steps/s",
                metric="LMPC steps/sec (batched QPs, whole node)")


def build_workload(cfg, args, torch, dev, rank, world):
    if cfg in ('C2', 'C4', 'C5', 'C5-dae'):
        return wl_nmpc(cfg, args, torch, dev, rank, world)
    if cfg == 'C3-mhe':
        return wl_mhe(args, torch, dev, rank, world)
    if cfg in ('C3-ekf', 'C3-ukf'):
        return wl_kf(cfg[3:], args, torch, dev, rank, world)
    if cfg == 'gp-predict':
        return wl_gp(args, torch, dev, rank, world)
    return wl_lmpc(args, torch, dev, rank, world)


def timed_region(wl, warmup, steps, world, dev):
    """The driver's contract: W untimed warm-up steps, then EXACTLY K steps bracketed by a barrier + device synchronisation on both
    sides; the time is the MAX over the ranks, the units the SUM of what the ranks processed per step.  Returns (elapsed seconds,
    units per step of the whole job).  (Its own function so that the world-2 gloo test of tests/test_dist_cpu.py drives THIS loop -
    with a stub controller on CPU tensors - and not a copy of it.)"""
    import torch
    import torch.distributed as dist

    def sync():
        if world > 1:
            dist.barrier()
        if dev.type == 'cuda':
            torch.cuda.synchronize(dev)

    for _ in range(warmup):
        wl['step'](False)
    sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        wl['step'](True)
    sync()
    elapsed = time.perf_counter() - t0
    units = float(wl['units'])
    if world > 1:
        tmax = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
        elapsed = float(tmax.item())
        tot = torch.tensor([units], dtype=torch.float64, device=dev)
        dist.all_reduce(tot, op=dist.ReduceOp.SUM)
        units = float(tot.item())
    return elapsed, units


DUMP_BYTES = 64 * 10 ** 6       # --dump-outputs: at most this much in all (float64)


def dump_outputs(outputs, out_dir, rank=0, world=1, budget=DUMP_BYTES):
    """Write `outputs` ({name: (tensor, instance axis)}, None entries skipped) as <out_dir>/<name>.npy in float64, one file set
    per rank (`<name>_rank<r>.npy` when world > 1).  Above `budget` bytes in all (shared by the ranks), every array keeps the same
    fraction of its instances: a fixed, seeded sample along its instance axis, the same rows for arrays of the same length."""
    import torch
    os.makedirs(out_dir, exist_ok=True)
    arrs = {k: v for k, v in outputs.items() if v[0] is not None}
    total = sum(8 * t.numel() for t, _ in arrs.values())
    frac = min(1.0, budget / world / max(total, 1))
    paths = []
    for name, (t, ax) in arrs.items():
        t = torch.as_tensor(t)
        if frac < 1.0:
            n = t.shape[ax]
            rows = np.sort(np.random.default_rng(0).choice(n, max(1, int(n * frac)), replace=False))
            t = t.index_select(ax, torch.as_tensor(rows, device=t.device))
        path = os.path.join(out_dir, f"{name}{f'_rank{rank}' if world > 1 else ''}.npy")
        np.save(path, np.ascontiguousarray(t.detach().to(torch.float64).cpu().numpy()))
        paths.append(path)
    return paths


def respawn(args):
    """`python bench.py --gpus N` without a torchrun environment: one process per GPU under torch.distributed.run."""
    import socket
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={args.gpus}',
           '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    return subprocess.call(cmd, env=env)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--config', choices=CONFIGS, default='C2')
    ap.add_argument('--batch', type=int, default=0, help='instances per GPU (weak configs) / in total (C4, C5); 0 = the config default')
    ap.add_argument('--no-cpu-baseline', action='store_true', help='with --full: leave the CPU baseline out')
    ap.add_argument('--kf-steps', type=int, default=16, help='C3-ekf / C3-ukf: filter steps per launch (1 = one launch per step)')
    ap.add_argument('--full', action='store_true',
                    help='also measure what takes runs of its own: CPU baseline, C2 settled loop, C1 single-instance latency')
    ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                    help="write the last timed step's results as DIR/<name>.npy (float64, at most 64 MB in all)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error('--steps must be at least 1 and --warmup at least 0')

    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        sys.exit(respawn(args))

    import torch
    import torch.distributed as dist
    from hilo_mpc_amd.dist import init_from_env

    rank, world, local = init_from_env()
    if world != args.gpus:
        if rank == 0:
            print(f"error: WORLD_SIZE={world} but --gpus {args.gpus}", file=sys.stderr)
        sys.exit(2)
    torch.cuda.set_device(local if world > 1 else 0)
    dev = torch.device('cuda', torch.cuda.current_device())

    wl = build_workload(args.config, args, torch, dev, rank, world)

    def sync():
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize(dev)

    elapsed, units = timed_region(wl, args.warmup, args.steps, world, dev)
    if args.dump_outputs:
        dump_outputs(wl['outputs'](), args.dump_outputs, rank, world)
    extra, roof, scaling = wl['finish']()
    # the headline configuration's value moves with how far the closed loop has settled (fewer interior-point iterations per step
    # later on): the SAME loop continued for 50 more steps, timed the same way, is reported next to the driver's command
    settled = None
    if args.full and args.config == 'C2':
        sync()
        t1 = time.perf_counter()
        for _ in range(50):
            wl['step'](False)
        sync()
        e2 = time.perf_counter() - t1
        if world > 1:
            t2 = torch.tensor([e2], dtype=torch.float64, device=dev)
            dist.all_reduce(t2, op=dist.ReduceOp.MAX)
            e2 = float(t2.item())
        settled = {"value": units * 50 / e2, "ms_per_step": e2 / 50 * 1e3,
                   "steps": f"{args.warmup + args.steps + 1}..{args.warmup + args.steps + 50} of the same closed loop (after the timed region)"}

    if rank == 0:
        out = {"metric": wl['metric'], "value": units * args.steps / elapsed, "unit": wl['unit'], "n_gpus": world,
               "steps": args.steps, "warmup": args.warmup, "ms_per_step": elapsed / args.steps * 1e3, "higher_is_better": True,
               "scaling": scaling, "vs_baseline": None, "dtype": "f64", "data": "synthetic",
               "config": dict(extra, name=args.config, rccl_world_size=world), "roofline": roof}
        if settled is not None:
            out["settled_loop"] = settled
        if 'hbm' in roof:
            out["roofline_hbm"] = dict(roof.pop('hbm'), bound="hbm", traffic=roof['traffic'])
        if args.full and not args.no_cpu_baseline and world == 1:      # the CPU leg is timed at N = 1 only
            out["cpu_baseline"] = wl['cpu']()
        print(json.dumps(out))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
