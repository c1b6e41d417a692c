"""GPU: the reference's whole function table through the public API, with no test-only device code: the table model written as a
DISCRETE model x+ = f(x, u), so that Model.linearization returns A = df/dx, B = df/du, C = dh/dx exactly and Model.step the values,
against sympy -> mpmath at 50 digits (tests/model_probe_reference.py; its tolerance: the host test's bounds times the measured
device-over-host factor 2.4 - values rtol 2.4e-14, first derivatives rtol 2.4e-12 + 2.4e-14).  67 operating points: one wave and
three lanes of the next."""
import numpy as np
import pytest

from tests import model_probe_reference as mr

pytestmark = pytest.mark.gpu


def test_table_model_linearisation_and_step_against_sympy():
    m = mr.table_model(discrete=True)
    m.setup(dt=1.)
    assert (m.n_x, m.n_u, m.n_y) == (2, 1, 1) and m.discrete
    X, U, p = mr.points('table', n=67)
    R = mr.reference('table', X, U, p)
    A, B, C = m.linearization(X, U)
    xn, _ = m.step(X, U)
    EJ = mr.J_RTOL * np.abs(R['Jf']) + mr.J_ATOL
    for what, got, ref, bound in (('A', A, R['Jf'][:, :, :2], EJ[:, :, :2]), ('B', B, R['Jf'][:, :, 2:], EJ[:, :, 2:]),
                                  ('C', C, R['Jy'][:, :, :2], mr.J_RTOL * np.abs(R['Jy'][:, :, :2]) + mr.J_ATOL),
                                  ('step', xn, R['f'], mr.V_RTOL * np.abs(R['f']))):
        err = np.abs(np.asarray(got) - ref)
        print(what, 'max error / bound', (err / bound).max())
        assert np.all(err <= bound), f"{what}: error {err.max():.3e} at point {np.unravel_index(np.argmax(err - bound), err.shape)}"
