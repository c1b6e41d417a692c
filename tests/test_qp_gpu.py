"""GPU: the batched QP solver on general QPs through its C ABI (`hilo_qp_create / set_stages / solve / solve_pinned`,
csrc/hilo_qp.hip, csrc/hilo_qp_ocp.h) - per-instance H, g, A, b and bounds with their real strides, one-sided / missing / fixed
bounds, m = 0, every kernel instantiation and the edges of the dispatch between them.  References: the oracle's QP solver
(oracle/lmpc.py, which tests/test_qp_reference_cpu.py shows to solve every instance used here) and the KKT conditions in
extended precision with limits derived from the termination rule (tests/qp_reference.py).  Every other limit is the one of the
test of tests/test_lmpc_gpu.py named next to it, or an exact comparison.

Which case runs which kernel
    qp_solve_reg_kernel<32, 24>   (1,0) (1,1) (2,1) (7,0) (7,3) (31,24) (32,24)         test_general_qp_*, test_both_dense_kernels_*
    qp_solve_reg_kernel<32, 32>   (32,25) (32,28) (32,31)                               the same, test_containment_dense[32-28-*]
    qp_solve_reg_kernel<64, 48>   (33,24) (63,48) (64,48)                               the same, test_containment_dense[63-48-dense]
    qp_solve_kernel, LDS          (64,49) (50,49) (65,30); every register case again under HILO_QP_LDS_COLUMNS
    qp_solve_kernel, workspace    (96,8), the dense twins of the long stage cases, test_workspace_follows_the_batch
    qp_ocp_kernel<NX, NU, 16>     all seven sizes at N = 1, 2, 15                       test_stage_kernel_*
    qp_ocp_kernel<NX, NU, 64>     all seven sizes at N = 16, 63
"""
import contextlib
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import qp_reference as qr          # noqa: E402

OUT = ('x', 'f', 'lam_a', 'lam_x', 'status', 'iter_count')
SENTINEL = -777.0


def _api():
    from hilo_mpc_amd import _lib
    return _lib


@contextlib.contextmanager
def qp_handle(n, m):
    import torch
    _lib = _api()
    h = C.c_void_p()
    _lib.check(_lib.lib().hilo_qp_create(n, m, 0, C.byref(h)))
    try:
        yield h
    finally:
        torch.cuda.synchronize()
        _lib.lib().hilo_qp_destroy(h)


def set_stages(h, nx, nu, N):
    _lib = _api()
    used = C.c_int(-1)
    _lib.check(_lib.lib().hilo_qp_set_stages(h, nx, nu, N, C.byref(used)))
    return used.value


def solve(h, qps, *, shared=False, pin=0):
    """One call of hilo_qp_solve on the stacked problems with their real strides (hs = n n, gs = n, as = m n, bs = n, bas = m).
    shared: the problems are copies of one - H, g, A, b are passed once with stride 0 (the bounds stay per instance: the entry
    point takes shared bound rows only with pinned values).  pin > 0: hilo_qp_solve_pinned with the first `pin` variables given
    per instance and ONE pair of bound rows (bs = 0).  Returns the six result tensors (pre-filled with a sentinel)."""
    import torch
    from hilo_mpc_amd._device import ptr, stream_ptr
    _lib = _api()
    dev = torch.device('cuda', 0)
    B, n, m = len(qps), qps[0]['H'].shape[0], qps[0]['A'].shape[0]
    src = qps[:1] if shared else qps

    def stack(key, items=src):
        return torch.as_tensor(np.ascontiguousarray(np.stack([np.asarray(q[key], dtype=np.float64) for q in items])), device=dev)
    H, g, A, lba = stack('H'), stack('g'), stack('A'), stack('b')
    uba = torch.as_tensor(np.stack([q.get('b_hi', q['b']) for q in src]), device=dev)
    if shared:
        assert all(np.array_equal(q[k], qps[0][k]) for q in qps for k in ('H', 'g', 'A', 'b'))
    hs, gs, as_, bas = (0, 0, 0, 0) if shared else (n * n, n, m * n, m)
    lb, ub = stack('lb', qps[:1] if pin else qps), stack('ub', qps[:1] if pin else qps)
    out = dict(x=torch.full((B, n), SENTINEL, dtype=torch.float64, device=dev), f=torch.full((B,), SENTINEL, dtype=torch.float64, device=dev),
               lam_a=torch.full((B, m), SENTINEL, dtype=torch.float64, device=dev),
               lam_x=torch.full((B, n), SENTINEL, dtype=torch.float64, device=dev),
               status=torch.full((B,), -777, dtype=torch.int32, device=dev), iter_count=torch.full((B,), -777, dtype=torch.int32, device=dev))
    res = [ptr(out[k]) for k in OUT]
    if pin:
        xpin = torch.as_tensor(np.stack([q['lb'][:pin] for q in qps]), device=dev).contiguous()
        assert all(np.array_equal(q['lb'][pin:], qps[0]['lb'][pin:]) and np.array_equal(q['ub'][pin:], qps[0]['ub'][pin:]) for q in qps)
        _lib.check(_lib.lib().hilo_qp_solve_pinned(h, B, ptr(H), hs, ptr(g), gs, ptr(A), as_, ptr(lb), ptr(ub), 0, ptr(xpin), pin, pin,
                                                   ptr(lba), ptr(uba), bas, *res, stream_ptr(dev)))
    else:
        _lib.check(_lib.lib().hilo_qp_solve(h, B, ptr(H), hs, ptr(g), gs, ptr(A), as_, ptr(lb), ptr(ub), n, ptr(lba), ptr(uba), bas,
                                            *res, stream_ptr(dev)))
    torch.cuda.synchronize()
    return out


def identical(a, b, ia=None, ib=None):
    """Keys whose tensors (rows ia of a, ib of b) differ in any bit."""
    import torch
    sel = (lambda t, i: t if i is None else t[i])
    return [k for k in OUT if not torch.equal(sel(a[k], ia), sel(b[k], ib))]


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def check_against_oracle_and_kkt(qps, refs, out, label):
    """Status 1 everywhere; KKT within the derived limits; x, f, lam_a against the oracle at the tolerances of
    test_lmpc_gpu.py::test_c1_vs_oracle; f against 1/2 x^T H x + g^T x of the returned x, 1e-13 relative to the size of the
    terms 1/2 |x|^T |H| |x| + |g|^T |x| (the round-off of a sum is relative to its terms: where they cancel - f = 1.2e-3 from terms
    of order 1 in one instance of nx = 3, nu = 2, N = 1 - an error of 4e-16 is 3.5e-13 of f itself)."""
    o = host(out)
    assert np.all(o['status'] == 1), f"{label}: statuses {o['status'].tolist()}"
    margins, ferr, dx, df, dla = [], 0.0, 0.0, 0.0, 0.0
    for i, (qp, ref) in enumerate(zip(qps, refs)):
        assert ref['status'] == 1
        margins.append(qr.kkt_margins(qp, o['x'][i], o['lam_a'][i], o['lam_x'][i]))
        xl, Hl, gl = o['x'][i].astype(np.longdouble), qp['H'].astype(np.longdouble), qp['g'].astype(np.longdouble)
        fl = 0.5 * xl @ (Hl @ xl) + gl @ xl
        scale = 0.5 * np.abs(xl) @ (np.abs(Hl) @ np.abs(xl)) + np.abs(gl) @ np.abs(xl)     # the size of the terms, not of their sum
        ferr = max(ferr, float(abs(o['f'][i] - fl) / scale))
        dx = max(dx, float(np.abs(o['x'][i] - ref['x']).max()))
        df = max(df, float(abs(o['f'][i] - ref['f'])))
        dla = max(dla, float(np.abs(o['lam_a'][i] - ref['lam_a']).max(initial=0)))
    print(f"{label}: iterations <= {o['iter_count'].max()}; {qr.fmt(qr.worst(margins))}; f vs x: {ferr:.2e} (limit 1e-13); "
          f"vs oracle: x {dx:.2e} (1e-7 + 1e-7 |x|), f {df:.2e} (1e-10 + 1e-8 |f|), lam_a {dla:.2e} (1e-6 + 1e-5 |lam_a|)")
    for i, mg in enumerate(margins):
        assert qr.kkt_ok(mg), f"{label}: instance {i}: {qr.fmt(mg)}"
    assert ferr <= 1e-13
    np.testing.assert_allclose(o['x'], np.stack([r['x'] for r in refs]), rtol=1e-7, atol=1e-7)
    np.testing.assert_allclose(o['f'], np.array([r['f'] for r in refs]), rtol=1e-8, atol=1e-10)
    np.testing.assert_allclose(o['lam_a'], np.stack([r['lam_a'] for r in refs]), rtol=1e-5, atol=1e-6)


# ---- (a) general QPs against the oracle and KKT ----
@pytest.mark.parametrize('n,m,kind,bounds', qr.DENSE_CASES)
def test_general_qp_against_oracle_and_kkt(n, m, kind, bounds):
    qps, refs = qr.dense_batch(n, m, kind, bounds)
    with qp_handle(n, m) as h:
        out = solve(h, qps)
    check_against_oracle_and_kkt(qps, refs, out, f"({n},{m}) {kind} {bounds}")


# ---- (b) the same problems on both dense kernels ----
@pytest.mark.parametrize('n,m,kind,bounds', [c for c in qr.DENSE_CASES if qr.register_kernel(c[0], c[1])])
def test_both_dense_kernels_solve_the_same_iteration(n, m, kind, bounds, monkeypatch):
    """Register-resident kernel against the LDS-column kernel (HILO_QP_LDS_COLUMNS, read in hilo_qp_create): limits of
    test_lmpc_gpu.py::test_register_resident_kernel_equals_the_lds_column_kernel."""
    qps, _ = qr.dense_batch(n, m, kind, bounds)
    with qp_handle(n, m) as h:
        fast = host(solve(h, qps))
    monkeypatch.setenv('HILO_QP_LDS_COLUMNS', '1')
    with qp_handle(n, m) as h:
        slow = host(solve(h, qps))
    dit = np.abs(fast['iter_count'] - slow['iter_count']).max()
    d = {k: float(np.abs(fast[k] - slow[k]).max(initial=0)) for k in ('x', 'lam_a', 'lam_x')}
    print(f"({n},{m}) {kind} {bounds}: iterations differ by {dit} (limit 1); x {d['x']:.2e} (1e-8 + 1e-7 |x|), "
          f"lam_a {d['lam_a']:.2e}, lam_x {d['lam_x']:.2e} (1e-7 + 1e-6 |lam|)")
    assert np.array_equal(fast['status'], slow['status']) and np.all(fast['status'] == 1)
    assert dit <= 1
    np.testing.assert_allclose(fast['x'], slow['x'], atol=1e-8)
    np.testing.assert_allclose(fast['lam_a'], slow['lam_a'], rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(fast['lam_x'], slow['lam_x'], rtol=1e-6, atol=1e-7)


# ---- (c) shared against per-instance data; order of the instances ----
FAMILIES = [(7, 3, 'dense'), (32, 28, 'dense'), (32, 28, 'diag'), (63, 48, 'dense'), (64, 49, 'dense'), (65, 30, 'diag'), (96, 8, 'dense')]


@pytest.mark.parametrize('n,m,kind', FAMILIES)
def test_strides_and_instance_order_dense(n, m, kind):
    qps, _ = qr.dense_batch(n, m, kind, 'fixed' if (n, m) in qr.EXTRA_BOUNDS_SIZES else 'mixed')
    B = 7
    with qp_handle(n, m) as h:
        one = [qps[3]] * B
        a, b = solve(h, one, shared=True), solve(h, one)
        assert identical(a, b) == [] and int(a['status'][0]) == 1
        assert all(identical(a, a, 0, i) == [] for i in range(B))
        first = solve(h, qps[:B])
        perm = np.random.default_rng(1).permutation(B)
        second = solve(h, [qps[i] for i in perm])
    assert (perm != np.arange(B)).sum() >= 4
    for i in range(B):
        assert identical(second, first, i, int(perm[i])) == [], (i, int(perm[i]))
    assert identical(first, a, 3, 0) == []                      # the replicated problem at its own place in the mixed batch


@pytest.mark.parametrize('nx,nu,N,B', [(2, 1, 15, 1), (2, 1, 15, 3), (2, 1, 15, 5), (2, 1, 15, 8), (4, 2, 2, 5), (2, 2, 16, 5)])
def test_strides_and_instance_order_stages(nx, nu, N, B):
    """The 16-lane variant packs four instances into a wave and lets idle groups repeat instance `batch - 1`: B = 1, 3, 5, 8 leave
    3, 1, 3, 0 groups idle.  A result may depend neither on the wave-mates nor on the position in the batch."""
    qps = qr.stage_problems(nx, nu, N, 8)
    n, m = qps[0]['H'].shape[0], qps[0]['A'].shape[0]
    with qp_handle(n, m) as h:
        assert set_stages(h, nx, nu, N) == 1
        full = solve(h, qps)
        assert np.all(host(full)['status'] == 1)
        one = [qps[2]] * B
        a, b = solve(h, one, shared=True), solve(h, one)
        assert identical(a, b) == []
        first = solve(h, qps[:B])
        perm = np.random.default_rng(2).permutation(B)
        second = solve(h, [qps[i] for i in perm])
        alone = [solve(h, [qps[i]]) for i in range(B)]
    for i in range(B):
        assert identical(a, full, i, 2) == []
        assert identical(first, full, i, i) == [], i
        assert identical(second, full, i, int(perm[i])) == [], i
        assert identical(alone[i], full, 0, i) == [], i


# ---- (d) the stage kernel against the dense kernels and the oracle ----
@pytest.mark.parametrize('nx,nu,N', qr.STAGE_CASES)
def test_stage_kernel_against_dense_kernels_and_oracle(nx, nu, N):
    """Per-instance, per-stage random blocks.  x_0 through per-instance rows lbx == ubx and through hilo_qp_solve_pinned with one
    shared pair of rows: the same bytes.  Against the dense kernels on the same handle: limits of
    test_lmpc_gpu.py::test_stage_kernel_equals_the_dense_kernels."""
    qps, refs = qr.stage_batch(nx, nu, N)
    n, m = qps[0]['H'].shape[0], qps[0]['A'].shape[0]
    label = f"nx={nx} nu={nu} N={N} (G = {16 if N + 1 <= 16 else 64}, B = {len(qps)})"
    with qp_handle(n, m) as h:
        assert set_stages(h, nx, nu, N) == 1
        st = solve(h, qps)
        pinned = solve(h, qps, pin=nx)
        assert set_stages(h, nx, nu, 0) == 0
        de = solve(h, qps)
    assert identical(st, pinned) == []
    check_against_oracle_and_kkt(qps, refs, st, label)
    a, b = host(st), host(de)
    dit = np.abs(a['iter_count'] - b['iter_count']).max()
    lim = dict(x=1e-8, f=1e-9, lam_a=1e-7, lam_x=1e-7)
    d = {k: float(np.abs(a[k] - b[k]).max()) for k in lim}
    print(f"{label} stages vs dense: iterations differ by {dit} (limit 1); " + ', '.join(f"{k} {d[k]:.2e} (limit {lim[k]:.0e} (1 + |.|))" for k in lim))
    assert np.array_equal(a['status'], b['status'])
    assert dit <= 1
    for k, tol in lim.items():
        np.testing.assert_allclose(a[k], b[k], rtol=tol, atol=tol, err_msg=k)


def test_horizon_64_stays_on_the_dense_kernels():
    """N + 1 = 65 stages do not fit a wave: the declaration is accepted, `used` is 0 and the dense path solves the QP."""
    qps, refs = qr.stage_batch(1, 1, 64, 2)
    with qp_handle(129, 64) as h:
        assert set_stages(h, 1, 1, 64) == 0
        out = solve(h, qps)
    check_against_oracle_and_kkt(qps, refs, out, "nx=1 nu=1 N=64 (dense)")
    with qp_handle(127, 63) as h:
        assert set_stages(h, 1, 1, 63) == 1
        assert set_stages(h, 1, 1, 0) == 0


def test_stage_kernel_refuses_a_fixed_input_for_that_instance_only():
    """The stage kernel is built for `x_0 pinned, nothing else`: an instance with a fixed input gets status -1, its wave-mates
    (16 lanes each, four to a wave) the bytes of the clean call; the dense kernels solve the whole batch."""
    nx, nu, N, bad = 2, 1, 15, 5
    qps = list(qr.stage_problems(nx, nu, N, 8))
    n, m = qps[0]['H'].shape[0], qps[0]['A'].shape[0]
    j = (N + 1) * nx + 3 * nu
    lb, ub = qps[bad]['lb'].copy(), qps[bad]['ub'].copy()
    lb[j] = ub[j] = qps[bad]['x_f'][j]
    mixed = list(qps)
    mixed[bad] = dict(qps[bad], lb=lb, ub=ub)
    with qp_handle(n, m) as h:
        assert set_stages(h, nx, nu, N) == 1
        clean, out = solve(h, qps), solve(h, mixed)
        assert set_stages(h, nx, nu, 0) == 0
        dense = solve(h, mixed)
    assert host(out)['status'].tolist() == [1] * bad + [-1] + [1] * (8 - bad - 1)
    for i in range(8):
        if i != bad:
            assert identical(out, clean, i, i) == [], i
    d = host(dense)
    assert np.all(d['status'] == 1) and d['x'][bad][j] == lb[j]
    mg = [qr.kkt_margins(mixed[i], d['x'][i], d['lam_a'][i], d['lam_x'][i]) for i in range(8)]
    print("fixed input, dense kernels: " + qr.fmt(qr.worst(mg)))
    assert all(qr.kkt_ok(x) for x in mg)


# ---- (e) containment and statuses ----
def _check_containment(clean_qps, bad_qps, bad_idx, clean, out, expected, label):
    o = host(out)
    print(f"{label}: statuses {o['status'].tolist()}, iterations {o['iter_count'].tolist()}")
    assert np.all(host(clean)['status'] == 1)
    for i, st in expected.items():
        assert o['status'][i] == st, (i, o['status'][i], st)
    assert o['iter_count'][qr.BAD_INFEASIBLE] <= 15       # OOQP's rule (test_lmpc_gpu.py::test_infeasible_states_are_reported_early)
    for i in range(len(clean_qps)):
        if i not in bad_idx:
            assert o['status'][i] == 1 and identical(out, clean, i, i) == [], i


@pytest.mark.parametrize('n,m,kind', qr.CONTAINMENT_DENSE)
def test_containment_dense(n, m, kind, monkeypatch):
    """A NaN, an infeasible box, an inequality row and an indefinite H in four instances of nine: their documented statuses, and
    every other instance bit-identical to the call without them."""
    clean_qps, bad_qps, bad_idx = qr.containment_dense(n, m, kind)
    with qp_handle(n, m) as h:
        clean, out = solve(h, clean_qps), solve(h, bad_qps)
    expected = {qr.BAD_NAN_G: 3, qr.BAD_INFEASIBLE: 3, qr.BAD_ROW: -1, qr.BAD_INDEFINITE: -1}
    _check_containment(clean_qps, bad_qps, bad_idx, clean, out, expected, f"({n},{m}) {kind}")
    if qr.register_kernel(n, m):                           # the same on the LDS-column kernel
        monkeypatch.setenv('HILO_QP_LDS_COLUMNS', '1')
        with qp_handle(n, m) as h:
            clean, out = solve(h, clean_qps), solve(h, bad_qps)
        _check_containment(clean_qps, bad_qps, bad_idx, clean, out, expected, f"({n},{m}) {kind} LDS columns")


@pytest.mark.parametrize('nx,nu,N', qr.CONTAINMENT_STAGE)
def test_containment_stages(nx, nu, N):
    clean_qps, bad_qps, bad_idx = qr.containment_stage(nx, nu, N)
    n, m = clean_qps[0]['H'].shape[0], clean_qps[0]['A'].shape[0]
    with qp_handle(n, m) as h:
        assert set_stages(h, nx, nu, N) == 1
        clean, out = solve(h, clean_qps), solve(h, bad_qps)
    _check_containment(clean_qps, bad_qps, bad_idx, clean, out, {qr.BAD_NAN_G: 3, qr.BAD_INFEASIBLE: 3, qr.BAD_ROW: -1},
                       f"nx={nx} nu={nu} N={N}")


# ---- (f) the workspace follows the batch ----
def test_workspace_follows_the_batch():
    qps, _ = qr.dense_batch(96, 8, 'dense', 'mixed')
    assert qr.dense_working_set_bytes(96, 8) > 160 * 1024
    with qp_handle(96, 8) as h:
        first, small, third = solve(h, qps[:8]), solve(h, qps[8:11]), solve(h, qps[:8])
    with qp_handle(96, 8) as h:
        fresh = solve(h, qps[8:11])
    assert np.all(host(first)['status'] == 1) and np.all(host(small)['status'] == 1)
    assert identical(first, third) == [] and identical(small, fresh) == []
    with qp_handle(96, 8) as h:
        both = solve(h, qps[:11])
    assert identical(both, first, slice(0, 8), slice(0, 8)) == [] and identical(both, small, slice(8, 11), slice(0, 3)) == []


# ---- (g) argument checks ----
def test_argument_checks():
    import torch
    from hilo_mpc_amd._device import ptr, stream_ptr
    _lib = _api()
    dev = torch.device('cuda', 0)
    n, m, B = 7, 3, 4
    qps, _ = qr.dense_batch(n, m, 'dense', 'mixed')
    t = {k: torch.as_tensor(np.stack([q[k] for q in qps[:B]]), device=dev) for k in ('H', 'g', 'A', 'b', 'lb', 'ub')}
    out = dict(x=torch.full((B, n), SENTINEL, dtype=torch.float64, device=dev), f=torch.full((B,), SENTINEL, dtype=torch.float64, device=dev),
               lam_a=torch.full((B, m), SENTINEL, dtype=torch.float64, device=dev),
               lam_x=torch.full((B, n), SENTINEL, dtype=torch.float64, device=dev),
               status=torch.full((B,), -777, dtype=torch.int32, device=dev), iter_count=torch.full((B,), -777, dtype=torch.int32, device=dev))
    res = [ptr(out[k]) for k in OUT]

    def call(h, batch, A):
        return _lib.lib().hilo_qp_solve(h, batch, ptr(t['H']), n * n, ptr(t['g']), n, A, m * n, ptr(t['lb']), ptr(t['ub']), n,
                                        ptr(t['b']), ptr(t['b']), m, *res, stream_ptr(dev))
    with qp_handle(n, m) as h:
        _lib.check(call(h, 0, ptr(t['A'])))                       # an empty batch: nothing is launched, nothing is written
        torch.cuda.synchronize()
        assert all(bool((out[k] == (SENTINEL if out[k].dtype == torch.float64 else -777)).all()) for k in OUT)
        with pytest.raises(Exception, match='3 rows but A / lba / uba is NULL'):
            _lib.check(call(h, B, None))
        with pytest.raises(Exception, match='negative batch'):
            _lib.check(call(h, -1, ptr(t['A'])))
        torch.cuda.synchronize()
        assert all(bool((out[k] == (SENTINEL if out[k].dtype == torch.float64 else -777)).all()) for k in OUT)
        with pytest.raises(Exception, match=r'n = 7, m = 3 do not match \(N\+1\) nx \+ N nu = 8, N nx = 4'):
            set_stages(h, 2, 1, 2)
        with pytest.raises(Exception, match='need nx, nu, N >= 1'):
            set_stages(h, 0, 1, 2)
        _lib.check(call(h, B, ptr(t['A'])))                       # the handle is still good
        torch.cuda.synchronize()
        assert out['status'].tolist() == [1] * B
    hh = C.c_void_p()
    with pytest.raises(Exception, match=r'need n >= 1, m >= 0 \(got 0, 0\)'):
        _lib.check(_lib.lib().hilo_qp_create(0, 0, 0, C.byref(hh)))
    assert not hh.value
    with pytest.raises(Exception, match=r'need n >= 1, m >= 0 \(got 3, -1\)'):
        _lib.check(_lib.lib().hilo_qp_create(3, -1, 0, C.byref(hh)))
    with qp_handle(64, 49) as h:                                  # no register kernel beyond MP = 48 and no stage shape: still accepted
        assert set_stages(h, 1, 1, 0) == 0
