"""Points, 50-digit reference and error bounds for the derivative arithmetic of csrc/hilo_ad.h, shared by the host driver test
(tests/test_ad_ops_host.py) and the device self-test (tests/test_ad_ops_gpu.py).

One point = (op, a, b, da, db, dda, ddb), csrc/hilo_ad_selftest.h; every operation gets its own points.  The reference (mpmath, 60
digits) evaluates the closed forms at the same double arguments:

    value        g(a [, b])
    Dual d       sum of `d terms`                    g' da                    |  da b + a db  | ...
    Jet2 a       the same with Jet2's tangents
    Jet2 b       sum of `b terms`                    g'' da^2 + g' dda        |  dda b + 2 da db + a ddb  | ...

The bound of a derivative component comes from the reference alone:

    allowed = sum over the value operands v in (a, b) of max |component(v +- 1 ulp) - component(v)|  +  8 ulp(sum |terms|)

For unit tangents (da = 1, dda = 0 or da = 0, dda = 1: a third of the points each) the component is g' or g'' itself and the sum
has one term: the change of the exact derivative when v moves by one ulp either way plus 8 ulp of the exact value.  With general
tangents the terms can cancel, and the roundings of each term (at most six operations per formula) stay relative to that term -
hence 8 ulp of the sum of their magnitudes.  sech2's second derivative 2 s (3 t^2 - 1) is such a difference in the closed form
itself (terms 6 s t^2 and -2 s).

fabs and sign are piecewise linear / constant: their one-ulp neighbourhood does not reach across the kink, and at a = +-0 every
derivative component is asserted to be exactly 0 (sign(0) = 0, CasADi's convention).

sinh and cosh are not functions of the header but compositions (hilo_mpc_amd/expr.py: 0.5 e -+ 0.5 / e, e = exp(a)), run as
operations of their own.  Their terms are the e / 2 part and the 1 / (2 e) part of each component, also for the VALUE: 8 ulp of
their magnitudes is relative far out and absolute next to 0, where sinh cancels.  Where e or 1 / e is denormal (|a| > 708.4) the
ulp of the part computed from it is the coarser relative spacing of the doubles there (`coarse`).

Named edge sets (EDGES below) hold the points where the exact value or a derivative is infinite or undefined; there the tests
assert a non-finite result.  `reference(op)` raises if mpmath fails or returns a non-finite number at any other point.
"""
import functools
import math

import mpmath
import numpy as np

M = mpmath.mp.clone()
M.dps = 60
mpf = M.mpf

OPS = ['neg', 'sq', 'sin', 'cos', 'exp', 'log', 'sqrt', 'log10', 'fabs', 'sign', 'asin', 'acos', 'atan', 'asinh', 'acosh', 'atanh',
       'tanh', 'sech2', 'add', 'sub', 'mul', 'div', 'atan2', 'add_tc', 'sub_tc', 'mul_tc', 'div_tc', 'atan2_tc', 'add_ct', 'sub_ct',
       'mul_ct', 'div_ct', 'atan2_ct', 'rcp', 'valof', 'sinh', 'cosh']
CODE = {n: i for i, n in enumerate(OPS)}                    # AD_* of csrc/hilo_ad_selftest.h
COMPOSED = ('sinh', 'cosh')                                 # e = exp(a), 0.5 * e -+ 0.5 / e: hilo_mpc_amd/expr.py
UNARY = OPS[:18] + list(COMPOSED)
KINKED = ('fabs', 'sign')                                   # piecewise linear / constant: the convention decides at 0, not a limit
FUNCTIONS = ['sin', 'cos', 'exp', 'log', 'sqrt', 'log10', 'asin', 'acos', 'atan', 'asinh', 'acosh', 'atanh', 'tanh', 'sech2', 'atan2']
SEED = np.array([1.0, -1.0, 2.0, 0.0, 0.5, -4.0, 16.0, -0.25, 0.125, 0.0, -8.0, 32.0])      # ad_seed of the header
N_FUN, N_ARITH = 2000, 1000
OUT = 20
INF = float('inf')

# where the exact value or derivative is infinite or undefined: (a, b) -> what is
EDGES = {
    'log': [((0.0, 1.0), 'log(0) = -inf, 1/0')], 'log10': [((0.0, 1.0), 'log10(0) = -inf, 1/0')],
    'sqrt': [((0.0, 1.0), "sqrt'(0) = 1/0")],
    'asin': [((1.0, 1.0), "asin'(1) = 1/0"), ((-1.0, 1.0), "asin'(-1) = 1/0")],
    'acos': [((1.0, 1.0), "acos'(1) = -1/0"), ((-1.0, 1.0), "acos'(-1) = -1/0")],
    'acosh': [((1.0, 1.0), "acosh'(1) = 1/0")],
    'atanh': [((1.0, 1.0), 'atanh(1) = inf'), ((-1.0, 1.0), 'atanh(-1) = -inf')],
    'div': [((1.5, 0.0), 'x / 0'), ((-2.0, -0.0), 'x / -0'), ((0.0, 0.0), '0 / 0')],
    'div_ct': [((1.5, 0.0), 'c / 0'), ((0.0, -0.0), '0 / -0')],
    'atan2': [((0.0, 0.0), "atan2'(0, 0) = 0/0"), ((-0.0, 0.0), "atan2'(-0, 0)"), ((0.0, -0.0), "atan2'(0, -0)"),
              ((-0.0, -0.0), "atan2'(-0, -0)")],
    'atan2_tc': [((0.0, 0.0), "atan2'(0, 0)"), ((-0.0, -0.0), "atan2'(-0, -0)")],
    'atan2_ct': [((0.0, 0.0), "atan2'(0, 0)"), ((-0.0, -0.0), "atan2'(-0, -0)")],
}
# sinh / cosh are composed (expr.py); tanh is native.  |a| at which the tanh tests go: up to 1e4 (ISSUE: tanh(k a), k a = +-1000)
# sinh / cosh: finite and within bound wherever the exact value is (|a| < ln(2^1024) = 709.7827); exp(a) or 1 / exp(a) is denormal
# beyond |a| = 708.396, and rcp_fast leaves its normal range there (e >= 2^1022, e < 2^-1022).  Beyond FAR the tangents are unit ones
SINH_FAR = 690.0
SINH_SPECIAL = [0.0, -0.0, 1e-8, -1e-8, 1e-3, 354.9, -354.9, 690.0, -690.0, 700.0, -700.0, 708.3, -708.3, 708.4, -708.4, 709.0, -709.0,
                709.5, -709.5, 709.78, -709.78]
TANH_SPECIAL = [0.0, -0.0, 354.0, 354.9, 355.0, 400.0, 709.0, 710.0, 745.2, 1000.0, 1e4, -354.9, -400.0, -1000.0, -1e4]


def ulp(x):
    """Spacing of the doubles at |x| (x a number or an mpf); 2^-1074 below the normal range."""
    x = abs(mpf(x))
    if x == 0:
        return mpf(2) ** -1074
    e = M.frexp(x)[1] - 1
    return mpf(2) ** (max(e, -1022) - 52)


def ulp_f(x):
    x = abs(np.asarray(x, dtype=float))
    with np.errstate(over='ignore', invalid='ignore'):
        return np.where(np.isfinite(x), np.spacing(np.minimum(x, 1.7e308)), np.nan)


def _signed_decades(rng, n, lo, hi):
    return rng.choice([-1., 1.], n) * 10. ** rng.uniform(lo, hi, n)


def _operand_a(op, rng, n):
    """n arguments in the domain of the unary function `op`: random over several decades, then the edges from inside."""
    k = np.arange(1, 53)
    if op in ('asin', 'acos', 'atanh'):
        edge = np.concatenate([1 - 2. ** -k, -(1 - 2. ** -k)])
        v = np.minimum(np.abs(_signed_decades(rng, n, -8, 0)), 1 - 2. ** -53) * rng.choice([-1., 1.], n)
    elif op == 'acosh':
        edge = 1 + 2. ** -k
        v = 1 + 10. ** rng.uniform(-8, 8, n)
    elif op in ('log', 'log10', 'sqrt'):
        edge = np.array([1e-100, 1e100, 1 - 2. ** -53, 1 + 2. ** -52])
        v = 10. ** rng.uniform(-8, 8, n)
    elif op == 'exp':
        edge = np.array([0.0, -0.0, 690., -690., 1e-300])
        v = _signed_decades(rng, n, -8, np.log10(690.))
    elif op in ('tanh', 'sech2'):
        edge = np.array(TANH_SPECIAL)
        v = _signed_decades(rng, n, -8, 4)
    elif op in COMPOSED:
        edge = np.array(SINH_SPECIAL)
        v = _signed_decades(rng, n, -8, np.log10(709.78))
    elif op in KINKED:
        # +-0 with each class of tangents (points(): index % 3 = 0: da = 1, dda = 0; 1: da = 0, dda = 1; 2: random ones)
        edge = np.array([0.0, -0.0, 0.0, -0.0, 0.0, -0.0, 5e-324, -5e-324, 5e-324, -5e-324, 5e-324, -5e-324])
        v = _signed_decades(rng, n, -8, 8)
    else:
        edge = np.array([0.0, -0.0]) if op in ('neg', 'sq', 'sin', 'cos', 'atan', 'asinh') else np.array([])
        v = _signed_decades(rng, n, -8, 8)
    v[:len(edge)] = edge
    return v


def points(op):
    """[n][7] = code, a, b, da, db, dda, ddb; and the edge flags [n] (index into EDGES[op] + 1, 0 = none)."""
    rng = np.random.default_rng(1000 + CODE[op])
    n = N_FUN if (op in FUNCTIONS or op in COMPOSED or op in ('atan2_tc', 'atan2_ct', 'fabs', 'sign', 'rcp')) else N_ARITH
    P = np.zeros((n, 7))
    P[:, 0] = CODE[op]
    P[:, 3:] = _signed_decades(rng, 4 * n, -2, 2).reshape(n, 4)
    cls = np.arange(n) % 3
    P[cls == 0, 3:] = [1., 0., 0., 0.]                       # d = g' (or dg/da), Jet2.b = g''
    P[cls == 1, 3:] = [0., 1., 1., 0.]                       # d = dg/db, Jet2.b = g'
    if op in UNARY:
        P[:, 1] = _operand_a(op, rng, n)
        P[:, 2] = _signed_decades(rng, n, -2, 2)            # not used by the operation
        if op in COMPOSED:
            # next to the overflow of the exact value: unit tangents alone (index % 2), so that no product with a tangent leaves
            # the range or falls among the denormals, which would measure the number format and not the formulas
            far = np.flatnonzero(np.abs(P[:, 1]) > SINH_FAR)
            P[far, 3:] = np.where((far % 2 == 0)[:, None], [1., 0., 0., 0.], [0., 1., 1., 0.])
    elif op == 'rcp':
        P[:, 1] = rng.choice([-1., 1.], n) * np.ldexp(rng.uniform(1., 2., n), rng.integers(-1022, 1022, n))   # 1/x normal too
        P[:32, 1] = np.ldexp(1., np.arange(-16, 16))
    elif op == 'valof':
        P[:, 1] = _signed_decades(rng, n, -300, 300)
        P[:4, 1] = [0.0, -0.0, INF, -INF]
    else:
        a, b = _signed_decades(rng, n, -6, 6), _signed_decades(rng, n, -6, 6)
        if op.startswith('div'):
            # a third of the divisors over the whole exponent range with a quotient of moderate size (a * rcp_fast(b) <= 2 ulp
            # of the exact quotient is claimed for every normal b); tangents 0 there: the derivatives would leave the range
            w = np.arange(n) % 3 == 2
            b[w] = rng.choice([-1., 1.], w.sum()) * np.ldexp(rng.uniform(1., 2., w.sum()), rng.integers(-1000, 1000, w.sum()))
            a[w] = b[w] * _signed_decades(rng, w.sum(), -3, 3)
            a[w & ~np.isfinite(a) | (np.abs(a) < 1e-300)] = 1.0
            P[w, 3:] = 0.
        if op.startswith('atan2'):
            # both axes, y = +-0 with x < 0, and all four quadrants from the signs above
            ax = [(0.0, 2.0), (-0.0, 2.0), (0.0, -2.0), (-0.0, -2.0), (3.0, 0.0), (3.0, -0.0), (-3.0, 0.0), (-3.0, -0.0),
                  (1e-300, -1.0), (-1e-300, -1.0), (1.0, 1e-300), (1e70, 1e70), (1e-70, -1e-70)]
            for i, (y, x) in enumerate(ax):
                a[i], b[i] = y, x
        P[:, 1], P[:, 2] = a, b
    edge = np.zeros(n, dtype=int)
    for j, ((ea, eb), _) in enumerate(EDGES.get(op, [])):
        P[n - 1 - j, 1:3] = [ea, eb]
        edge[n - 1 - j] = j + 1
    return P, edge


# ---- closed forms ---------------------------------------------------------------------------------------------------
def _unary(op, v):
    """(g, g', [terms of g''])"""
    one = mpf(1)
    if op == 'neg':
        return -v, -one, [mpf(0)]
    if op == 'sq':
        return v * v, 2 * v, [mpf(2)]
    if op == 'sin':
        return M.sin(v), M.cos(v), [-M.sin(v)]
    if op == 'cos':
        return M.cos(v), -M.sin(v), [-M.cos(v)]
    if op == 'exp':
        e = M.exp(v)
        return e, e, [e]
    if op == 'log':
        return M.log(v), 1 / v, [-1 / (v * v)]
    if op == 'sqrt':
        s = M.sqrt(v)
        return s, 1 / (2 * s), [-1 / (4 * s * v)]
    if op == 'log10':
        c = 1 / M.log(10)
        return M.log10(v), c / v, [-c / (v * v)]
    if op == 'fabs':
        return abs(v), mpf(M.sign(v)), [mpf(0)]             # CasADi: d|a| = sign(a) da, sign(0) = 0
    if op == 'sign':
        return mpf(M.sign(v)), mpf(0), [mpf(0)]
    if op in ('asin', 'acos'):
        r = 1 / M.sqrt(1 - v * v)
        s = 1 if op == 'asin' else -1
        return (M.asin(v) if op == 'asin' else M.acos(v)), s * r, [s * v * r ** 3]
    if op == 'atan':
        r = 1 / (1 + v * v)
        return M.atan(v), r, [-2 * v * r * r]
    if op == 'asinh':
        r = 1 / M.sqrt(v * v + 1)
        return M.asinh(v), r, [-v * r ** 3]
    if op == 'acosh':
        r = 1 / M.sqrt(v * v - 1)
        return M.acosh(v), r, [-v * r ** 3]
    if op == 'atanh':
        r = 1 / (1 - v * v)
        return M.atanh(v), r, [2 * v * r * r]
    t, s = M.tanh(v), 1 / M.cosh(v) ** 2
    if op == 'tanh':
        return t, s, [-2 * t * s]
    if op == 'sech2':
        return s, -2 * t * s, [6 * s * t * t, -2 * s]
    raise KeyError(op)


def composed_parts(op, v):
    """sinh / cosh and their derivatives as the two terms of the composition, p = e / 2 and q = 1 / (2 e): (g, g', g'') each a
    pair of signed (p part, q part)."""
    e = M.exp(v)
    p, q = e / 2, 1 / (2 * e)
    odd, even = (p, -q), (p, q)
    return (odd, even, odd) if op == 'sinh' else (even, odd, even)


def coarse(op, v):
    """(cp, cq) >= 1: how much coarser than 2^-52 relative the doubles are at e = exp(v) (the p part is computed from e) and at e and
    1 / e (the q part is computed from both): 1 while they are normal, up to 4 at |v| = 709.78."""
    e = M.exp(v)
    ce, ci = ulp(e) / e * mpf(2) ** 52, ulp(1 / e) * e * mpf(2) ** 52
    return max(1, ce), max(1, ce, ci)


def exact(op, a, b, da, db, dda, ddb):
    """(value, d terms, b terms): mpf; d terms with the tangents (da, db) - Jet2's .a has the same formula."""
    base = op.split('_')[0]
    if op in COMPOSED:                                      # terms in the order p part, q part, p part, q part
        g, g1, g2 = composed_parts(op, a)
        return g[0] + g[1], [g1[0] * da, g1[1] * da], [g2[0] * da * da, g2[1] * da * da, g1[0] * dda, g1[1] * dda]
    if op.endswith('_tc'):
        db = ddb = mpf(0)
    if op.endswith('_ct'):
        da = dda = mpf(0)
    if op in UNARY:
        g, g1, g2 = _unary(op, a)
        return g, [g1 * da], [t * da * da for t in g2] + [g1 * dda]
    if base in ('add', 'sub'):
        s = 1 if base == 'add' else -1
        return a + s * b, [da, s * db], [dda, s * ddb]
    if base == 'mul':
        return a * b, [da * b, a * db], [dda * b, 2 * da * db, a * ddb]
    if base == 'div':
        v = a / b
        d = (da - v * db) / b
        return v, [da / b, -v * db / b], [dda / b, -2 * d * db / b, -v * ddb / b]
    if base == 'atan2':                                     # f(y = a, x = b)
        r = a * a + b * b
        n = [b * da, -a * db]
        r1 = [2 * b * db, 2 * a * da]
        return M.atan2(a, b), [t / r for t in n], [b * dda / r, -a * ddb / r] + [-p * q / (r * r) for p in n for q in r1]
    raise KeyError(op)


def _operands(op):
    if op in UNARY:
        return (0,)
    return (0, 1)


@functools.lru_cache(maxsize=None)
def reference(op):
    """dict of float arrays for the points of `op`: in, edge; v_hi + v_lo the exact value in two doubles, v_ulp; for c in d, ja, jb:
    c_hi, c_lo, c_allow.  Raises where mpmath is not finite outside the named edge set."""
    P, edge = points(op)
    n = len(P)
    R = {'in': P, 'edge': edge}
    for k in ('v', 'd', 'ja', 'jb'):
        R[k + '_hi'], R[k + '_lo'] = np.full(n, np.nan), np.zeros(n)
    R['v_ulp'] = np.full(n, np.nan)
    for k in ('v', 'd', 'ja', 'jb'):
        R[k + '_allow'] = np.full(n, np.nan)

    def put(k, i, x):
        hi = float(x)
        R[k + '_hi'][i], R[k + '_lo'][i] = hi, float(x - mpf(hi))

    for i in range(n):
        if edge[i]:
            continue
        arg = [mpf(float(x)) for x in P[i, 1:]]
        if op == 'rcp':
            put('v', i, 1 / arg[0])
            R['v_ulp'][i] = float(ulp(1 / arg[0]))
            continue
        if op == 'valof':
            put('v', i, arg[0]) if np.isfinite(P[i, 1]) else None
            continue

        def comps(args):
            return exact(op, *args)
        try:
            v, dt, bt = comps(arg)
            d, jb = M.fsum(dt), M.fsum(bt)
            pert_d = pert_b = mpf(0)
            for o in _operands(op):
                u = ulp(arg[o])
                cd = cb = mpf(0)
                for s in (-1, 1):
                    q = list(arg)
                    q[o] = arg[o] + s * u
                    if op in KINKED and (q[o] == 0 or arg[o] == 0 or (q[o] > 0) != (arg[o] > 0)):
                        continue                             # not across the kink: each side is linear, at 0 the convention holds
                    try:
                        _, dt2, bt2 = comps(q)
                    except (ValueError, ZeroDivisionError):
                        continue                             # the neighbour lies outside the domain: the inner side alone
                    d2, b2 = M.fsum(dt2), M.fsum(bt2)
                    if M.isfinite(d2) and M.isfinite(b2) and M.im(d2) == 0 and M.im(b2) == 0:
                        cd, cb = max(cd, abs(d2 - d)), max(cb, abs(b2 - jb))
                pert_d, pert_b = pert_d + cd, pert_b + cb
        except (ValueError, ZeroDivisionError) as e:
            raise AssertionError(f"{op}: the reference is undefined at point {i} {P[i, 1:3]} outside the named edges: {e}")
        for x in (v, d, jb):
            if not M.isfinite(x) or M.im(x) != 0:
                raise AssertionError(f"{op}: the reference is not finite and real at point {i} {P[i, 1:3]} outside the named edges")
        put('v', i, v)
        R['v_ulp'][i] = float(ulp(v))
        put('d', i, d)
        put('ja', i, d)
        put('jb', i, jb)
        if op in COMPOSED:
            # 8 ulp of the p terms and of the q terms, each in the spacing the doubles have where its factors lie; the value likewise
            # (its argument is exact: no perturbation part) - relative far out, absolute (8 ulp of cosh a = 1) next to 0
            cp, cq = coarse(op, arg[0])
            def a8(terms):
                return 8 * (cp * ulp(M.fsum(abs(t) for t in terms[0::2])) + cq * ulp(M.fsum(abs(t) for t in terms[1::2])))
            g = composed_parts(op, arg[0])[0]
            R['v_allow'][i] = float(a8([g[0], g[1]]))
            R['d_allow'][i] = R['ja_allow'][i] = float(pert_d + a8(dt))
            R['jb_allow'][i] = float(pert_b + a8(bt))
            continue
        R['d_allow'][i] = R['ja_allow'][i] = float(pert_d + 8 * ulp(M.fsum(abs(t) for t in dt)))
        R['jb_allow'][i] = float(pert_b + 8 * ulp(M.fsum(abs(t) for t in bt)))
    return R


# ---- checks on an output array [n][20] of the driver ----------------------------------------------------------------------------
def same_bits(x, y):
    x, y = np.ascontiguousarray(x, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    return (x.view(np.uint64) == y.view(np.uint64)) | (np.isnan(x) & np.isnan(y))


def edge_value(op, a, b):
    """The plain double value at a point of the named edge sets: the derivative is infinite or undefined there, the value is what
    IEEE 754 / C Annex F give - log(0) = -inf, x / +-0 = +-inf, 0 / 0 = NaN, atanh(+-1) = +-inf, atan2(+-0, +0) = +-0, atan2(+-0, -0)
    = +-pi, and the finite values of sqrt, asin, acos, acosh at the end of their domains."""
    base = op.split('_')[0]
    if base in ('log', 'log10'):
        return -INF
    if base == 'div':
        return math.nan if a == 0 else math.copysign(INF, a) * math.copysign(1., b)
    if base == 'atanh':
        return math.copysign(INF, a)
    if base == 'atan2':
        return math.atan2(a, b)
    return {'sqrt': math.sqrt, 'asin': math.asin, 'acos': math.acos, 'acosh': math.acosh}[base](a)


def value_ulp_error(op, out):
    """max |plain double value - exact| in ulp of the exact value over the points outside the edge set."""
    R = reference(op)
    ok = R['edge'] == 0
    if op.startswith('atan2'):
        ok &= R['in'][:, 1] != 0                              # y = +-0: the sign of the zero decides (checked on its own)
    err = np.abs((out[ok, 0] - R['v_hi'][ok]) - R['v_lo'][ok]) / R['v_ulp'][ok]
    return float(np.max(err))


def check(op, out, value_ulps, where):
    """All assertions on one operation's output: bit-identical value components, the plain double value within `value_ulps` of the
    exact one, derivative components within the reference's bound, non-finite results on the named edges.  Returns the measured
    figures."""
    R = reference(op)
    P, edge = R['in'], R['edge']
    n = len(P)
    base = op.split('_')[0]
    plain, fast, d1v, d1, d12v, d12, jv, ja, jb = (out[:, 0], out[:, 1], out[:, 2], out[:, 3], out[:, 4], out[:, 5:17], out[:, 17],
                                                    out[:, 18], out[:, 19])
    reg = edge == 0
    info = {}
    if op in COMPOSED:
        # the plain double divides by IEEE, FastD, Dual and Jet2 through rcp_fast: identical among themselves, and both within the
        # mixed bound (8 ulp of cosh a: relative far out, absolute next to 0), finite at every point
        for name, v in (('Dual<1>', d1v), ('Dual<12>', d12v), ('Jet2', jv)):
            bad = ~same_bits(fast, v)
            assert not bad.any(), f"{where} {op}: {name}'s value differs from FastD's at {P[bad][:3, 1]}"
        fin = np.isfinite(out)
        fin[np.ix_(np.abs(P[:, 1]) > SINH_FAR, 5 + np.flatnonzero(np.abs(SEED) != 1.))] = True     # 32 g' may leave the range there
        assert reg.all() and fin.all(), f"{where} {op}: not finite at {P[~fin.all(axis=1)][:5, 1]}"
        for name, v in (('double', plain), ('FastD', fast)):
            r = np.abs((v - R['v_hi']) - R['v_lo']) / R['v_allow']
            info['value_' + name] = float(r.max())
            print(f"MEASURED {where} {op} {name} value error / bound {r.max():.4f} at {P[np.argmax(r), 1]!r}")
            assert r.max() <= 1.0, f"{where} {op}: {name} value {v[np.argmax(r)]!r} at {P[np.argmax(r), 1]!r}, {r.max():.2f} of the bound"
    elif base == 'div':
        # FastD, Dual and Jet2 divide through the same a * rcp_fast(b) (T / c: a * (1 / c)): identical among themselves, within 2
        # ulp of the exact quotient; the plain double is the IEEE quotient
        for name, v in (('Dual<1>', d1v), ('Dual<12>', d12v), ('Jet2', jv)):
            bad = reg & ~same_bits(fast, v)
            assert not bad.any(), f"{where} {op}: {name}'s quotient differs from FastD's at {P[bad][:3, 1:3]}"
        e = np.abs((fast[reg] - R['v_hi'][reg]) - R['v_lo'][reg]) / R['v_ulp'][reg]
        info['quotient_ulp'] = float(e.max())
        assert e.max() <= 2.0, f"{where} {op}: a * rcp_fast(b) is {e.max():.2f} ulp from the exact quotient at {P[reg][np.argmax(e), 1:3]}"
    else:
        for name, v in (('FastD', fast), ('Dual<1>', d1v), ('Dual<12>', d12v), ('Jet2', jv)):
            bad = ~same_bits(plain, v)
            assert not bad.any(), f"{where} {op}: the value of {name} differs from the plain double overload at {P[bad][:3, 1:3]}"
    e = value_ulp_error(op, out)
    info['value_ulp'] = e
    print(f"MEASURED {where} {op} value_ulp {e:.4f}")
    if op not in COMPOSED:                                    # theirs is the mixed bound above: next to 0 the error is absolute
        assert e <= value_ulps, f"{where} {op}: plain double value {e:.3f} ulp from the exact one (allowed {value_ulps})"
    if op.startswith('atan2'):
        z = reg & (P[:, 1] == 0)                              # C Annex F: atan2(+-0, x > 0) = +-0, atan2(+-0, x < 0) = +-pi
        want = np.array([math.atan2(y, x) for y, x in P[z, 1:3]])
        assert np.all(np.abs(plain[z] - want) <= ulp_f(want)) and np.all(np.signbit(plain[z]) == np.signbit(want)), f"{where} {op}: +-0"
    # derivative components
    for name, got, key in (('Dual<1>.d', d1, 'd'), ('Jet2.a', ja, 'ja'), ('Jet2.b', jb, 'jb')):
        err = np.abs((got[reg] - R[key + '_hi'][reg]) - R[key + '_lo'][reg])
        ratio = err / R[key + '_allow'][reg]
        bad = ~(ratio <= 1.0)
        info[key] = float(np.nanmax(ratio)) if not np.isnan(ratio).all() else float('nan')
        if bad.any():
            i = np.flatnonzero(reg)[np.argmax(np.where(np.isnan(ratio), np.inf, ratio))]
            raise AssertionError(f"{where} {op}: {name} = {got[i]!r} at {P[i, 1:].tolist()}, exact {R[key + '_hi'][i]!r}, error "
                                 f"{abs(got[i] - R[key + '_hi'][i]):.3e} > allowed {R[key + '_allow'][i]:.3e} ({bad.sum()} of {reg.sum()} points)")
    if op in KINKED:
        # d|a| = sign(a) da with sign(0) = 0, d sign = 0 (CasADi's convention, csrc/hilo_ad.h): at a = +-0 every derivative component
        # is exactly 0 - Dual's d and Jet2's a with da = 1 (g' = 0), Jet2's b with da = 1 (g'' = 0) and with dda = 1 (g' again)
        z = P[:, 1] == 0
        for sel, what in ((z & (P[:, 3] == 1.), 'da = 1'), (z & (P[:, 5] == 1.), 'dda = 1'), (z, 'any tangents')):
            assert {(float(s_), bool(n_)) for s_, n_ in zip(np.sign(P[sel, 1]), np.signbit(P[sel, 1]))} == {(0., False), (0., True)}, what
            comp = np.concatenate([d1[sel, None], d12[sel], ja[sel, None], jb[sel, None]], axis=1)
            assert np.all(comp == 0.), f"{where} {op} at +-0 with {what}: derivative components {comp[np.any(comp != 0., axis=1)][:2]}, exactly 0 wanted"
    # Dual<12>: the tangents of component k are ad_seed(k) (a power of two, or 0) times Dual<1>'s, so are the exact derivative and
    # its bound, exactly
    # (composed sinh / cosh beyond SINH_FAR: the components with a seed of +-1 alone, 32 g' leaves the range)
    for k in range(12):
        rk = reg & (np.abs(P[:, 1]) <= SINH_FAR) if op in COMPOSED and abs(SEED[k]) != 1. else reg
        err = np.abs((d12[rk, k] - SEED[k] * R['d_hi'][rk]) - SEED[k] * R['d_lo'][rk])
        bad = ~(err <= abs(SEED[k]) * R['d_allow'][rk])
        assert not bad.any(), (f"{where} {op}: Dual<12>.d[{k}] = {d12[rk, k][bad][0]!r} at {P[rk][bad][0, 1:].tolist()}, exact "
                               f"{SEED[k] * R['d_hi'][rk][bad][0]!r}")
    # the named edges: non-finite derivative components, stated per case in EDGES, and the plain double value IEEE gives there
    for i in np.flatnonzero(edge):
        what = EDGES[op][edge[i] - 1][1]
        comp = np.concatenate([[d1[i]], d12[i, SEED != 0], [ja[i], jb[i]]])
        assert not np.isfinite(comp).any(), f"{where} {op} at {P[i, 1:3]} ({what}): a finite derivative {comp}"
        want = edge_value(op, P[i, 1], P[i, 2])
        assert same_bits(plain[i], want) or abs(plain[i] - want) <= ulp_f(want), f"{where} {op} at {P[i, 1:3]} ({what}): value {plain[i]!r}, {want!r} wanted"
    return info


# ---- the postfix interpreter (csrc/hilo_expr.h): an expression tree of hilo_mpc_amd.expr in exact second-order Taylor arithmetic ----
def _jmul(x, y):
    return (x[0] * y[0], x[1] * y[0] + x[0] * y[1], x[2] * y[0] + 2 * x[1] * y[1] + x[0] * y[2])


def _jrecip(y):
    i = 1 / y[0]
    return (i, -y[1] * i * i, 2 * y[1] * y[1] * i ** 3 - y[2] * i * i)


def _jchain(x, g, g1, g2):
    return (g, g1 * x[1], g2 * x[1] * x[1] + g1 * x[2])


def jet_eval(e, x, u, p):
    """(v, a, b) of the expression e; x, u: lists of (v, a, b) triples of mpf, p: list of mpf.  Raises ZeroDivisionError /
    ValueError where the expression is undefined."""
    val = {}
    zero = mpf(0)
    for n in sorted(e.nodes().values(), key=lambda q: q.serial):
        a = [val[id(c)] for c in n.args]
        op = n.op
        if op == 'const':
            r = (mpf(n.value), zero, zero)
        elif op == 'x':
            r = x[int(n.value)]
        elif op == 'u':
            r = u[int(n.value)]
        elif op == 'p':
            r = (p[int(n.value)], zero, zero)
        elif op == 'add':
            r = tuple(s + t for s, t in zip(a[0], a[1]))
        elif op == 'sub':
            r = tuple(s - t for s, t in zip(a[0], a[1]))
        elif op == 'neg':
            r = tuple(-s for s in a[0])
        elif op == 'mul':
            r = _jmul(a[0], a[1])
        elif op == 'div':
            r = _jmul(a[0], _jrecip(a[1]))
        elif op == 'powi':
            k = int(n.value)
            r = (mpf(1), zero, zero)
            for _ in range(abs(k)):
                r = _jmul(r, a[0])
            if k < 0:
                r = _jrecip(r)
        else:
            g, g1, g2 = _unary(op, a[0][0])
            r = _jchain(a[0], g, g1, M.fsum(g2))
        val[id(n)] = r
    return val[id(e)]
