"""CPU: the structural-zero masks XMASK / JMASK / HMASK of the generated derivative code (hilo_mpc_amd/symdiff.py::sym_source)
against sympy, for the three models of tests/model_probe_reference.py.  The derivative phase skips every product whose bit is clear,
so a bit that is clear on an entry that is not identically zero is a wrong Hessian."""
import re

import pytest

from tests import model_probe_reference as mr


def _is_zero(e, syms):
    """Identically zero: literally 0 after differentiation, or 0 at three generic points at 30 digits (an expression of these
    analytic functions that vanishes at three generic points vanishes everywhere; nothing here is simplified symbolically)."""
    if e == 0:
        return True
    pts = ((.37, -.61, .83, 1.21, -.47, .29), (-.91, .53, .22, -.75, 1.3, .68), (.14, .95, -.58, .41, .77, -1.1))
    return all(abs(e.evalf(30, subs=dict(zip(syms, pt)))) < 1e-25 for pt in pts)


@pytest.mark.parametrize('name', sorted(mr.MODELS))
def test_structural_zero_masks_against_sympy(name):
    """Every entry whose bit is clear is identically zero in the sympy derivative, and every identically zero entry has its bit
    clear (H: for every row m, since the adjoint weights kb are free) - the hash-consed DAG folds exactly the zeros sympy finds in
    these three models, so no bit may stay set on a zero."""
    m = mr.MODELS[name][0]()
    src = m.user_source()
    assert 'HAS_MASKS = true' in src
    xmask, jmask, hmask = (int(v, 16) for v in re.search(r'XMASK = 0x([0-9a-f]+)ull, JMASK = 0x([0-9a-f]+)ull, HMASK = 0x([0-9a-f]+)ull',
                                                         src).groups())
    xs, us, ps, f, h, Jf, Jh, Hf, Hh = mr.symbolic(name)
    nx, nz = len(xs), len(xs) + len(us)
    syms = xs + us + ps
    assert (m.n_x, m.n_u) == (nx, len(us))
    for r in range(nx):
        for j in range(nz):
            zero = _is_zero(Jf[r][j], syms)
            assert bool(jmask >> (r * nz + j) & 1) == (not zero), ('JMASK', r, j, Jf[r][j])
            if j < nx:
                assert bool(xmask >> (r * nx + j) & 1) == (not zero), ('XMASK', r, j, Jf[r][j])
    q = 0
    for i in range(nz):
        for j in range(i + 1):
            zero = all(_is_zero(Hf[r][i][j], syms) for r in range(nx))
            assert bool(hmask >> q & 1) == (not zero), ('HMASK', i, j, [Hf[r][i][j] for r in range(nx)])
            q += 1
    assert hmask >> q == 0 and jmask >> (nx * nz) == 0 and xmask >> (nx * nx) == 0
