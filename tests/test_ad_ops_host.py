"""CPU: the derivative arithmetic of csrc/hilo_ad.h compiled for the HOST (the header is `__host__ __device__`) and compared with a
60-digit reference, operation by operation and scalar type by scalar type - the statements the device self-test runs
(csrc/hilo_ad_selftest.h, tests/test_ad_ops_gpu.py), here with the host's math library and rcp_fast's host branch 1 / x.

Bounds and points: tests/ad_reference.py.  The plain double values are asserted within twice the figure measured on the HOST
(tests/ad_reference_ulp.py: HOST_ULP -> VALUE_ULPS_HOST, floor 1 ulp); the device test asserts twice the device figure.  The two
differ: glibc's acosh at 1.40 ulp would not pass twice the device's 0.61."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import ad_reference as ar
from tests.ad_reference_ulp import VALUE_ULPS_HOST as VALUE_ULPS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'hilo_mpc_amd', 'csrc')

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include "hilo_ad_selftest.h"
using namespace hilo;

// argv: points (binary doubles [n][7]), results (binary doubles [n][20])
int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  fseek(f, 0, SEEK_END);
  const long bytes = ftell(f);
  fseek(f, 0, SEEK_SET);
  const long n = bytes / (7 * sizeof(double));
  double* in = (double*)malloc(bytes);
  double* out = (double*)malloc(n * AD_OUT * sizeof(double));
  if (!in || !out || (long)fread(in, 7 * sizeof(double), n, f) != n) return 2;
  fclose(f);
  for (long i = 0; i < n; ++i) ad_selftest_point((int)in[7 * i], in[7 * i + 1], in[7 * i + 2], in[7 * i + 3], in[7 * i + 4],
                                                 in[7 * i + 5], in[7 * i + 6], out + AD_OUT * i);
  f = fopen(argv[2], "wb");
  if (!f || (long)fwrite(out, AD_OUT * sizeof(double), n, f) != n) return 2;
  fclose(f);
  free(in);
  free(out);
  return 0;
}
"""


def _hipcc():
    for c in (os.environ.get('HIPCC'), '/opt/rocm/bin/hipcc', shutil.which('hipcc')):
        if c and os.path.exists(c):
            return c
    return None


@pytest.fixture(scope='module')
def host_out(tmp_path_factory):
    """{op: out[n][20]} of the host-compiled driver at the points of every operation, one run."""
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip('hipcc not available')
    d = tmp_path_factory.mktemp('ad_ops_host')
    (d / 'driver.hip').write_text(DRIVER)
    subprocess.check_call([hipcc, '-x', 'hip', '--cuda-host-only', '-std=c++17', '-O2', '-I', CSRC, str(d / 'driver.hip'), '-o',
                           str(d / 'driver')])
    P = np.concatenate([ar.points(op)[0] for op in ar.OPS])
    P.tofile(str(d / 'in.bin'))
    subprocess.check_call([str(d / 'driver'), str(d / 'in.bin'), str(d / 'out.bin')])
    out = np.fromfile(str(d / 'out.bin')).reshape(len(P), ar.OUT)
    res, q = {}, 0
    for op in ar.OPS:
        n = len(ar.points(op)[0])
        res[op] = out[q:q + n]
        q += n
    return res


@pytest.mark.parametrize('op', ar.OPS)
def test_reference_is_finite_outside_the_named_edges(op):
    """No failing point can hide among the 'expected non-finite' ones: mpmath is finite and real at every point that is not in the
    operation's named edge set (ad_reference.reference raises otherwise), and every bound is a finite positive number."""
    R = ar.reference(op)
    reg = R['edge'] == 0
    assert reg.sum() >= len(reg) - len(ar.EDGES.get(op, []))
    if op in ('rcp', 'valof'):
        assert np.all(np.isfinite(R['v_hi'][reg])) or op == 'valof'
        return
    for k in ('v_hi', 'd_hi', 'jb_hi', 'd_allow', 'jb_allow', 'v_ulp'):
        assert np.all(np.isfinite(R[k][reg])), (op, k)
    assert np.all(R['d_allow'][reg] > 0) and np.all(R['jb_allow'][reg] > 0)


@pytest.mark.parametrize('op', [o for o in ar.OPS if o not in ('rcp', 'valof')])
def test_host_operation_against_the_reference(host_out, op):
    info = ar.check(op, host_out[op], VALUE_ULPS.get(op.split('_')[0] if op.startswith('atan2') else op, 0.5), 'host')
    print(op, info)


def test_host_valof_and_reciprocal(host_out):
    """valof / value return the value component of every type unchanged; rcp_fast's host branch is the IEEE reciprocal."""
    P, _ = ar.points('valof')
    o = host_out['valof']
    for c in (0, 1, 2, 3, 4, 5, 17, 18, 19):
        assert ar.same_bits(o[:, c], P[:, 1]).all(), c
    R = ar.reference('rcp')
    assert np.array_equal(host_out['rcp'][:, 0], 1. / R['in'][:, 1])
    err = np.abs((host_out['rcp'][:, 0] - R['v_hi']) - R['v_lo']) / R['v_ulp']
    assert err.max() <= 0.5


def test_tanh_is_finite_and_exact_far_out(host_out):
    """tanh composed of exp(2a) was inf / inf = NaN beyond |a| = 354.9, value and derivatives: at every |a| <= 1e4 (a = +-0 included)
    value, first and second derivative are finite in all four scalar types (the bound itself: the parametrised test above)."""
    P, _ = ar.points('tanh')
    o = host_out['tanh']
    assert np.abs(P[:, 1]).max() == 1e4 and np.isfinite(o).all()
    far = np.abs(P[:, 1]) >= 400.
    unit = far & (P[:, 3] == 1.) & (P[:, 5] == 0.)
    assert far.sum() >= 6 and unit.any()
    assert np.array_equal(o[far, 0], np.sign(P[far, 1])) and np.all(o[unit][:, [3, 18, 19]] == 0.)
