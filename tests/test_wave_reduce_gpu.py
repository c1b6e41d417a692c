"""GPU: the n-value wave reduction of the interior-point engine (csrc/hilo_ocp.h::WaveReduceN) in its transposing form against its
plain form and against a numpy restatement of the documented pairing tree, through the debug entry hilo_ocp_reduce_selftest (one wave,
64 x n lane values in, both results out).

The tree: lane l combines with lane l ^ 1, then l ^ 2, l ^ 4, l ^ 8 inside its row of 16 (the two mirror levels of the plain form pair
equal partials, so they are xor 4 and xor 8 in value), then (r0 o r16) o (r32 o r48) over the four row totals.  Both forms walk this tree;
they differ in which lane holds a partial.  Every comparison is BIT FOR BIT - there is no tolerance in this file - except that a NaN is
compared as a NaN where numpy's and the hardware's default NaN differ in sign (inf - inf).  Zero signs follow the hardware: a maximum
of +0 and -0 is +0, a minimum -0, whichever side they come from.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

SUM, MAX, MIN, MAX2 = 0, 1, 2, 3
# the mixes compiled into the entry: the call sites' (three sums of eval_values_call; maximum, maximum, sum of the step lengths; the
# seven of kkt_pass; the single reductions) and further ones for every n
MIXES = [(SUM,), (MAX,), (MIN,), (MAX2,),
         (SUM, SUM), (MAX, MAX), (MIN, MAX), (SUM, MAX2),
         (SUM, SUM, SUM), (MAX, MAX, SUM), (MIN, SUM, MAX2),
         (SUM, SUM, SUM, SUM), (MAX2, MIN, MAX, MAX), (SUM, MAX, MIN, MAX2),
         (SUM, MAX2, MIN, MAX, MAX, SUM, SUM), (SUM,) * 7,
         (SUM,) * 8, (SUM, MAX2, MIN, MAX, MAX, SUM, SUM, MAX), (MAX, MAX2, MAX, MIN, MAX2, MAX, MIN, MAX)]
NAN_LANES = list(range(16, 32)) + [5, 40, 63]      # every lane of one row, one lane of each other row


def _run(ops, lanes):
    from hilo_mpc_amd import _lib
    n = len(ops)
    assert lanes.shape == (64, n)
    dev = torch.as_tensor(np.ascontiguousarray(lanes), device='cuda')
    new = torch.zeros(n, dtype=torch.float64, device='cuda')
    plain = torch.zeros(n, dtype=torch.float64, device='cuda')
    _lib.check(_lib.lib().hilo_ocp_reduce_selftest(n, (C.c_int * n)(*ops), dev.data_ptr(), new.data_ptr(), plain.data_ptr(), None))
    return new.cpu().numpy(), plain.cpu().numpy()


def _hw_max(a, b):
    r = np.fmax(a, b)
    zz = (a == 0) & (b == 0)
    return np.where(zz, np.where(np.signbit(a) & np.signbit(b), -0.0, 0.0), r)


def _hw_min(a, b):
    r = np.fmin(a, b)
    zz = (a == 0) & (b == 0)
    return np.where(zz, np.where(np.signbit(a) | np.signbit(b), -0.0, 0.0), r)


def _tree(col, op):
    f = {SUM: np.add, MAX: _hw_max, MAX2: _hw_max, MIN: _hw_min}[op]
    lane = np.arange(64)
    with np.errstate(all='ignore'):
        a = col.copy()
        for s in (1, 2, 4, 8):
            a = f(a, a[lane ^ s])
        r = f(f(a[0], a[16]), f(a[32], a[48]))
    if op == MAX and np.isnan(col).any():
        return np.nan
    return float(r)


def _datasets(n, rng):
    """name -> [64, n] lane values"""
    def decades():
        return rng.choice([-1., 1.], (64, n)) * 10. ** rng.uniform(-15., 15., (64, n))
    out = {'decades': decades(), 'decades2': decades()}
    z = rng.choice([0., -0.], (64, n))
    z[:, 0] = -0.                                        # a column of negative zeros only
    out['zeros'] = z
    zm = decades()
    zm[rng.uniform(size=(64, n)) < .7] = 0.
    zm[rng.uniform(size=(64, n)) < .3] = -0.
    out['zeros among magnitudes'] = -np.abs(zm)          # maxima decided between -0 and negative numbers
    for name, vals in (('+inf', [np.inf]), ('-inf', [-np.inf]), ('both inf', [np.inf, -np.inf])):
        d = decades()
        for j in range(n):
            for v, ln in zip(vals, rng.choice(64, len(vals), replace=False)):
                d[ln, j] = v
        out[name] = d
    out['denormals'] = rng.choice([-1., 1.], (64, n)) * rng.integers(1, 2 ** 40, (64, n)) * 5e-324
    dm = decades() * 1e-300
    out['around the denormal threshold'] = dm
    base = decades()
    for ln in NAN_LANES:
        d = base.copy()
        d[ln, :] = np.nan
        out[f'nan in lane {ln}'] = d
    d = base.copy()
    d[7, 0] = np.nan                                     # a NaN in one value only: its neighbours must not see it
    out['nan in one value'] = d
    return out


def _same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


@pytest.mark.parametrize('ops', MIXES, ids=lambda m: ''.join('SXNP'[o] for o in m))
def test_transposing_reduction_equals_plain_form_and_documented_tree(ops):
    rng = np.random.default_rng(20261020 + 97 * len(ops) + sum(o << (2 * j) for j, o in enumerate(ops)))
    n = len(ops)
    for name, lanes in _datasets(n, rng).items():
        new, plain = _run(ops, lanes)
        want = np.array([_tree(lanes[:, j], ops[j]) for j in range(n)])
        print(name, 'new', new.tolist(), 'plain', plain.tolist(), 'tree', want.tolist())
        assert _same_bits(new, plain), (name, new.tolist(), plain.tolist())
        for j in range(n):
            if np.isnan(want[j]):
                assert np.isnan(new[j]), (name, j, new[j])
            else:
                assert _same_bits(new[j:j + 1], want[j:j + 1]), (name, j, float(new[j]).hex(), float(want[j]).hex())
            if ops[j] == MAX and np.isnan(lanes[:, j]).any():
                assert np.isnan(new[j]) and np.isnan(plain[j]), (name, j)      # NaN in, NaN out


def test_a_mix_that_is_not_compiled_in_is_an_error():
    from hilo_mpc_amd import _lib
    buf = torch.zeros(64 * 2, dtype=torch.float64, device='cuda')
    out = torch.zeros(4, dtype=torch.float64, device='cuda')
    rc = _lib.lib().hilo_ocp_reduce_selftest(2, (C.c_int * 2)(MIN, MIN), buf.data_ptr(), out.data_ptr(), out.data_ptr() + 16, None)
    assert rc != 0 and b'not compiled in' in _lib.lib().hilo_last_error()
