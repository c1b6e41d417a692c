"""GPU: the derivative arithmetic of csrc/hilo_ad.h and the postfix interpreter of csrc/hilo_expr.h on the device, on their own,
against a 60-digit reference (tests/ad_reference.py: points, closed forms, bounds).

hilo_ad_selftest: one launch evaluates every operation at its points in double, FastD, Dual<1>, Dual<12> and Jet2.  Asserted per
operation: the value components of all types are bit-identical to the plain double overload; the plain double value is within twice
the measured device figure of the exact one (tests/ad_reference_ulp.py, floor 1 ulp); Dual's and Jet2's derivative components are
within the reference's own bound; at a = +-0 the derivative components of fabs and sign are exactly 0; on the named edges the
derivative components are non-finite and the plain value is what IEEE gives; the composed sinh and cosh (hilo_mpc_amd/expr.py) are
finite and within their mixed bound up to |a| = 709.78; rcp_fast meets the contract stated at its definition.

hilo_expr_selftest: programs built by hilo_mpc_amd.expr's program(), back to back in one block, selected by index - every opcode,
X_POWI for every n in -16..16 (base 0 with n < 0 included), an expression of depth exactly 8."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ad_reference as ar
from tests.ad_reference_ulp import VALUE_ULPS

pytestmark = pytest.mark.gpu

INF, NAN = float('inf'), float('nan')
# rcp_fast at the edges of its domain, as measured on the device (csrc/hilo_ad.h states the same): argument -> result
RCP_EDGES = [(0.0, NAN), (-0.0, NAN), (INF, NAN), (-INF, NAN), (NAN, NAN)]
# arguments whose result is only pinned to be non-finite or within 1 ulp (of the denormal spacing where the reciprocal is denormal)
RCP_RANGE_EDGES = [5e-324, -5e-324, 2. ** -1060, 2. ** -1025, 2. ** -1024, 1.5 * 2. ** -1024, 2. ** -1023, -2. ** -1023, 1.75 * 2. ** -1023,
                   2. ** 1022, 1.5 * 2. ** 1022, 2. ** 1023, -2. ** 1023, 1.9999 * 2. ** 1023, 1.7976931348623157e308]


@pytest.fixture(scope='module')
def dev_out():
    """{op: out[n][20]}: one launch over the points of every operation, then the rcp_fast edge arguments."""
    from hilo_mpc_amd import _lib
    edges = np.zeros((len(RCP_EDGES) + len(RCP_RANGE_EDGES), 7))
    edges[:, 0] = ar.CODE['rcp']
    edges[:, 1] = [a for a, _ in RCP_EDGES] + RCP_RANGE_EDGES
    P = np.concatenate([ar.points(op)[0] for op in ar.OPS] + [edges])
    dev = torch.as_tensor(np.ascontiguousarray(P), device='cuda')
    out = torch.full((len(P), ar.OUT), -7.0, dtype=torch.float64, device='cuda')
    _lib.check(_lib.lib().hilo_ad_selftest(len(P), dev.data_ptr(), out.data_ptr(), None))
    out = out.cpu().numpy()
    res, q = {}, 0
    for op in ar.OPS:
        n = len(ar.points(op)[0])
        res[op] = out[q:q + n]
        q += n
    res['rcp_edges'] = out[q:, 0]
    return res


@pytest.mark.parametrize('op', [o for o in ar.OPS if o not in ('rcp', 'valof')])
def test_device_operation_against_the_reference(dev_out, op):
    info = ar.check(op, dev_out[op], VALUE_ULPS.get(op.split('_')[0] if op.startswith('atan2') else op, 0.5), 'device')
    print('MEASURED', op, info)


def test_device_valof(dev_out):
    P, _ = ar.points('valof')
    for c in (0, 1, 2, 3, 4, 5, 17, 18, 19):
        assert ar.same_bits(dev_out['valof'][:, c], P[:, 1]).all(), c


def test_rcp_fast_meets_its_contract(dev_out):
    """csrc/hilo_ad.h: on normal arguments whose reciprocal is normal rcp_fast(x) is within 1 ulp of 1 / x (and a * rcp_fast(b) within
    2 ulp of a / b: the 'div' cases of the parametrised test, a third of them over the whole exponent range); at the edges it returns
    what the header pins."""
    R = ar.reference('rcp')
    got = dev_out['rcp'][:, 0]
    err = np.abs((got - R['v_hi']) - R['v_lo']) / R['v_ulp']
    print('MEASURED rcp_fast max ulp', err.max(), 'at', R['in'][np.argmax(err), 1])
    e = dev_out['rcp_edges']
    for (a, _), r in zip(RCP_EDGES, e):
        print('MEASURED rcp_fast(%r) = %r' % (a, r))
    for a, r in zip(RCP_RANGE_EDGES, e[len(RCP_EDGES):]):
        print('MEASURED rcp_fast(%r) = %r, 1/x = %r' % (a, r, 1. / a))
    assert err.max() <= 1.0
    for (a, want), r in zip(RCP_EDGES, e):
        assert (np.isnan(r) and np.isnan(want)) or r == want, f"rcp_fast({a}) = {r}, pinned {want}"
    for a, r in zip(RCP_RANGE_EDGES, e[len(RCP_EDGES):]):
        # never a finite wrong number: non-finite, or within 1 ulp of the exact reciprocal (ulp: the spacing of the doubles there)
        exact = 1 / ar.mpf(a)
        assert not np.isfinite(r) or abs(ar.mpf(float(r)) - exact) <= ar.ulp(exact), f"rcp_fast({a}) = {r}, exact {float(exact)}"


# ---- the interpreter -----------------------------------------------------------------------------------------------------------
NX, NU, NP = 4, 2, 3


def _programs():
    from hilo_mpc_amd import expr as ex
    x, u, p = ex.SymVector('x', ['x0', 'x1', 'x2', 'x3']), ex.SymVector('u', ['u0', 'u1']), ex.SymVector('p', ['p0', 'p1', 'p2'])
    every = (ex.sin(x[0]) * ex.cos(x[1]) + ex.exp(-u[0]) / ex.sqrt(x[2] ** 2 + p[0]) - ex.log(x[3] * x[3] + 1.5)
             + (x[1] - p[1]) ** 3 + 0.25 * u[1])
    deep = x[0] + (x[1] * (x[2] - (x[3] / (u[0] + (u[1] * (p[0] - p[1]))))))
    assert deep.depth() == ex.STACK == 8
    progs = [('every opcode', every)]
    progs += [(f'x1^{n}', ex.Expr('powi', (x[1],), value=n)) for n in range(-16, 17)]
    progs += [('depth 8', deep), ('last', ex.sqrt(x[0] * x[0] + u[0] * u[0]) / (2.0 + p[2]))]
    ops = set()
    for _, e in progs:
        ops |= set(e.program()[1::2])
    assert ops == {0., 1., 2., 3.} | {float(c) for c in range(10, 22)}, ops            # every opcode of hilo_expr.h
    return progs


def _expr_points():
    rng = np.random.default_rng(77)
    n = 64
    Q = np.zeros((n, 18))
    Q[:, :4] = rng.uniform(.3, 2., (n, 4)) * rng.choice([-1., 1.], (n, 4))
    Q[:, 12:14] = rng.uniform(.3, 2., (n, 2))
    Q[:, 4:12] = rng.normal(size=(n, 8))
    Q[:, 14:18] = rng.normal(size=(n, 4))
    Q[:4, 1] = [0.0, -0.0, 0.0, 0.0]                      # base 0 of the integer powers
    Q[2, 5], Q[2, 9] = 1.0, 0.0
    Q[3, 5], Q[3, 9] = 0.0, 0.0
    return Q, np.array([1.7, -0.6, 0.9])


def _expr_reference(e, Q, p):
    """exact (v, a, b) per point, the bound per component, and the points where the expression is undefined."""
    nops = len(e.program()) // 2
    n = len(Q)
    ref, allow, undefined = np.zeros((n, 3)), np.zeros((n, 3)), np.zeros(n, dtype=bool)
    cols = []                                                # the inputs the expression depends on
    for leaf in e.nodes().values():
        if leaf.op == 'x':
            cols += [int(leaf.value), 4 + int(leaf.value), 8 + int(leaf.value)]
        elif leaf.op == 'u':
            cols += [12 + int(leaf.value), 14 + int(leaf.value), 16 + int(leaf.value)]

    def at(q):
        x = [(q[c], q[4 + c], q[8 + c]) for c in range(4)]
        u = [(q[12 + c], q[14 + c], q[16 + c]) for c in range(2)]
        return ar.jet_eval(e, x, u, [ar.mpf(float(v)) for v in p])
    for i in range(n):
        q0 = [ar.mpf(float(v)) for v in Q[i]]
        try:
            r = at(q0)
        except ZeroDivisionError:
            undefined[i] = True
            continue
        sens = [ar.mpf(0)] * 3
        for c in cols:
            if not (c < 4 or 12 <= c < 14) and q0[c] == 0:
                continue                                     # a zero tangent stays zero
            best = [ar.mpf(0)] * 3
            for s in (-1, 1):
                q = list(q0)
                q[c] = q0[c] + s * ar.ulp(q0[c])
                try:
                    r2 = at(q)
                except ZeroDivisionError:
                    continue
                best = [max(b, abs(t - w)) for b, t, w in zip(best, r2, r)]
            sens = [s_ + b for s_, b in zip(sens, best)]
        ref[i] = [float(t) for t in r]
        allow[i] = [float(2 * nops * (s_ + ar.ulp(t))) for s_, t in zip(sens, r)]
    return ref, allow, undefined


def test_interpreter_programs_back_to_back():
    """Every program of the block is selected by its index (first, middle, last and all between) and evaluated at 64 points in
    double and in Jet2; Jet2's value is bit-identical to the double evaluation in programs without a division.

    Bound per component: 2 n (S + 1 ulp of the exact value), n = the number of operations of the program, S = the change of the exact
    component when each input the program reads moves by one ulp either way, summed.  Reasoning: every operation is within a few ulp
    (tests above), which equals moving its operands by a few ulp; the programs here have no cancellation between their constants, so
    each operation's share of the result's sensitivity is bounded by the sensitivity to the inputs.  A wrong opcode, operand order,
    stack slot, power count or program offset is an error of order one.  An integer power n < 0 of the base 0 is 1 / 0: the double
    result is +-inf, Jet2's components are non-finite (rcp_fast(0) is NaN)."""
    from hilo_mpc_amd import _lib
    progs = _programs()
    block = []
    for _, e in progs:
        block += e.program()
    Q, p = _expr_points()
    count = len(progs)
    assert count >= 3
    blk = (C.c_double * len(block))(*block)
    dQ = torch.as_tensor(Q, device='cuda')
    dp = torch.as_tensor(p, device='cuda')

    def divides(e):                                          # Jet2 divides through rcp_fast, the double through the IEEE quotient
        return any(n.op == 'div' or (n.op == 'powi' and n.value < 0) for n in e.nodes().values())
    for which, (name, e) in enumerate(progs):
        out = torch.full((len(Q), 4), -7.0, dtype=torch.float64, device='cuda')
        _lib.check(_lib.lib().hilo_expr_selftest(blk, len(block), count, which, len(Q), dQ.data_ptr(), dp.data_ptr(), out.data_ptr(), None))
        out = out.cpu().numpy()
        ref, allow, undefined = _expr_reference(e, Q, p)
        ok = ~undefined
        if name.startswith('x1^-'):
            assert undefined.sum() == 4 and np.all(np.isinf(out[undefined, 0])) and not np.isfinite(out[undefined, 1:]).any(), name
        else:
            assert not undefined.any(), name
        if not divides(e):
            assert ar.same_bits(out[ok, 0], out[ok, 1]).all(), f"{name}: Jet2's value differs from the double evaluation"
        err = np.abs(out[ok][:, [0, 1, 2, 3]] - ref[ok][:, [0, 0, 1, 2]])
        ratio = err / allow[ok][:, [0, 0, 1, 2]]
        print('MEASURED interpreter', name, 'max error / bound', ratio.max(axis=0))
        assert np.all(ratio <= 1.0), f"{name}: {out[ok][np.argmax(ratio.max(axis=1))]} vs {ref[ok][np.argmax(ratio.max(axis=1))]}"
    assert any(divides(e) for _, e in progs) and not all(divides(e) for _, e in progs)


def test_interpreter_rejects_bad_programs():
    """expr_check runs in front of the launch: a stack of 9, an unknown opcode and a power of 17 are refused with HILO_EINVAL."""
    from hilo_mpc_amd import _lib
    from hilo_mpc_amd import expr as ex
    Q, p = _expr_points()
    dQ, dp = torch.as_tensor(Q, device='cuda'), torch.as_tensor(p, device='cuda')
    out = torch.zeros((len(Q), 4), dtype=torch.float64, device='cuda')
    nine = [float(2 * 9 + 2 * 8)] + [ex.X_CONST, 1.0] * 9 + [ex.X_ADD, 0.0] * 8
    for bad in (nine, [2.0, 99.0, 0.0], [4.0, ex.X_VARX, 0.0, ex.X_POWI, 17.0], [2.0, ex.X_VARX, 4.0]):
        blk = (C.c_double * len(bad))(*bad)
        with pytest.raises(ValueError):
            _lib.check(_lib.lib().hilo_expr_selftest(blk, len(bad), 1, 0, len(Q), dQ.data_ptr(), dp.data_ptr(), out.data_ptr(), None))
