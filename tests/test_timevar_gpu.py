"""GPU: time-variant models written as text through `Model.step` / `rollout` / `simulate` - the fixed-step maps, `solver='dopri5'`
and `solver='bdf'` - against the references and bounds of tests/timevar_reference.py.

Batches: forced2 with 130 instances (two full waves and two lanes: the tail block, and lanes that finish at different times), the
initial state, the input and the forcing frequency w varied by +-30 % per instance; prothero1 with 70 instances, lam between 1e3
and 1e5.  Every instance is compared with its own references, which worker processes that never open the GPU compute once per
module.  Each test prints the figures it asserts on."""
import numpy as np
import pytest

from hilo_mpc_amd import Model
from tests import sim_reference as sr
from tests import stiff_reference as st
from tests import timevar_reference as tv

pytestmark = pytest.mark.gpu

B, BS, STEPS = 130, 70, 10
FORCED2_TEXT = """
dx_1/dt = x_2(t)
dx_2/dt = -k*x_1(t) - c*x_2(t) + u(k)*sin(w*t)
y(k) = x_1(t) + cos(t)
"""


def _forced2(**setup):
    m = Model(name='forced2')
    m.set_parameters(['k', 'c', 'w'])
    m.set_equations(FORCED2_TEXT)
    return m.setup(dt=.5, **setup)


def _prothero(**setup):
    m = Model(name='prothero1')
    m.set_equations("dx/dt = -lam*(x(t) - cos(t)) - sin(t)\ny(k) = x(t)")
    return m.setup(dt=1., **setup)


def _forced2_batch(n=B, seed=21):
    x0, u, p, dt, steps, _ = tv.CASES['forced2']
    rng = np.random.default_rng(seed)
    X0 = np.asarray(x0) * (1 + .3 * rng.uniform(-1, 1, (n, 2))) + [0., .3] * rng.uniform(-1, 1, (n, 2))
    U = np.asarray(u) * (1 + .3 * rng.uniform(-1, 1, (n, 1)))
    P = np.tile(p, (n, 1))
    P[:, 2] *= 1 + .3 * rng.uniform(-1, 1, n)
    Useq = U[None] * (1 + .5 * rng.uniform(-1, 1, (STEPS, n, 1)))
    return X0, U, Useq, P


def _prothero_batch(n=BS, seed=22):
    x0, _, _, dt, steps, t0 = tv.CASES['prothero1']
    rng = np.random.default_rng(seed)
    X0 = np.tile(x0, (n, 1))
    P = 10. ** rng.uniform(3., 5., (n, 1))
    Pseq = np.clip(P[None] * rng.uniform(.5, 2., (STEPS, n, 1)), 1e3, 1e5)
    return X0, P, Pseq


@pytest.fixture(scope='module')
def forced2_refs():
    """(t0 = 2.5, an input sequence) and (t0 = 0, inputs held), each at both tolerances: results of timevar_reference.bounds_batch."""
    X0, U, Useq, P = _forced2_batch()
    return {'seq': tv.bounds_batch('explicit', 'forced2', X0, Useq, P, .5, STEPS, 2.5, tv.TOLS_EXPLICIT),
            'held': tv.bounds_batch('explicit', 'forced2', X0, U, P, .5, STEPS, 0., tv.TOLS_EXPLICIT)}


@pytest.fixture(scope='module')
def prothero_refs():
    X0, P, Pseq = _prothero_batch()
    U = np.zeros((BS, 0))
    return {'held': tv.bounds_batch('stiff', 'prothero1', X0, U, P, 1., STEPS, 1., tv.TOLS_STIFF),
            'seq': tv.bounds_batch('stiff', 'prothero1', X0, U, Pseq, 1., STEPS, 1., tv.TOLS_STIFF)}


def _within(tag, x, ref, admissible, e_cmp, e_tight, rtol, atol):
    worst = 0.
    for i in range(ref.shape[1]):
        err = sr.rel_err(x[:, i], ref[:, i], rtol, atol)
        worst = max(worst, err / max(e_cmp[i], e_tight[i]))
        assert err <= admissible[i], (tag, i, err, admissible[i])
    print(f"{tag}: largest error / max(comparator's error, tight solutions' disagreement) over {ref.shape[1]} instances: {worst:.2f} "
          f"(comparator {e_cmp.min():.2e} .. {e_cmp.max():.2e}, tight {e_tight.max():.2e})")


def _forced2_y(x, t0, dt):
    tk = t0 + dt * np.arange(x.shape[0] - 1)
    return x[1:, :, :1] + np.cos(tk + dt)[:, None, None]


# ---- 4: forced2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i_tol', [0, 1])
@pytest.mark.parametrize('inputs,t0', [('seq', 2.5), ('held', 0.)])
def test_forced2_under_dopri5(forced2_refs, inputs, t0, i_tol):
    rtol, atol = tv.TOLS_EXPLICIT[i_tol]
    X0, U, Useq, P = _forced2_batch()
    m = _forced2(solver='dopri5', solver_options={'reltol': rtol, 'abstol': atol})
    x, y, stats = m.rollout(X0, Useq if inputs == 'seq' else U, P, steps=STEPS, return_stats=True, t0=t0)
    ref, admissible, e45, e_tight = forced2_refs[inputs][i_tol]
    assert not stats['status'].any()
    _within(f"forced2 dopri5 {inputs} t0={t0} rtol={rtol:g}", x, ref, admissible, e45, e_tight, rtol, atol)
    np.testing.assert_allclose(y, _forced2_y(x, t0, .5), rtol=1e-14, atol=1e-14)          # Y[k] = h(t_k + dt, x[k + 1])


@pytest.mark.parametrize('t0', [2.5, 0.])
@pytest.mark.parametrize('inputs', ['held', 'seq'])
@pytest.mark.parametrize('recipe', ['default', 'erk2'])
def test_forced2_through_the_fixed_step_maps(recipe, inputs, t0):
    """The default map (eight classic Runge-Kutta sub-steps) and `discretize('erk', 2)` against the same recipe with stage times
    written out in numpy, to 1e-12 of the largest state."""
    X0, U, Useq, P = _forced2_batch()
    m = _forced2() if recipe == 'default' else _forced2().discretize('erk', 2).setup(dt=.5)
    Uin = Useq if inputs == 'seq' else U
    x, y = m.rollout(X0, Uin, P, steps=STEPS, t0=t0)
    order, n_sub = (4, 8) if recipe == 'default' else (2, 1)
    ref = tv.erk_rollout(tv.forced2_batch, X0, Uin, P, .5, STEPS, t0, order, n_sub)
    err = np.max(np.abs(x - ref)) / np.max(np.abs(ref))
    print(f"forced2 {recipe} {inputs} t0={t0}: {err:.2e} of the largest state")
    assert err <= 1e-12
    np.testing.assert_allclose(y, _forced2_y(x, t0, .5), rtol=1e-14, atol=1e-14)


# ---- 5: prothero1 under bdf -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i_tol', [0, 1])
@pytest.mark.parametrize('inputs', ['held', 'seq'])
def test_prothero1_under_bdf(prothero_refs, inputs, i_tol):
    rtol, atol = tv.TOLS_STIFF[i_tol]
    X0, P, Pseq = _prothero_batch()
    t0 = tv.CASES['prothero1'][5]
    m = _prothero(solver='bdf', solver_options={'reltol': rtol, 'abstol': atol})
    x, y, stats = m.rollout(X0, None, Pseq if inputs == 'seq' else P, steps=STEPS, return_stats=True, t0=t0)
    ref, admissible, e_bdf, e_tight, counts = prothero_refs[inputs][i_tol]
    assert not stats['status'].any()
    _within(f"prothero1 bdf {inputs} rtol={rtol:g}", x, ref, admissible, e_bdf, e_tight, rtol, atol)
    r_acc, r_rhs = stats['n_accepted'] / counts[:, 0], stats['n_rhs'] / counts[:, 1]
    print(f"   accepted steps / scipy's {r_acc.min():.3f} .. {r_acc.max():.3f}, right-hand sides / scipy's {r_rhs.min():.3f} .. {r_rhs.max():.3f}")
    assert np.all(stats['n_accepted'] <= st.COST_MARGIN * counts[:, 0]) and np.all(stats['n_rhs'] <= st.COST_MARGIN * counts[:, 1])
    np.testing.assert_array_equal(y, x[1:])
    if inputs == 'held':
        t = t0 + np.arange(STEPS + 1)
        exact = tv.prothero_exact(t[:, None], X0[None, :, 0], P[None, :, 0], t0)
        e_exact = np.max(np.abs(x[:, :, 0] - exact) / np.abs(exact))
        print(f"   against the exact solution {e_exact:.3e}")
        assert e_exact <= 10. * sr.FACTOR * rtol


# ---- 6: polynomials in t through the maps ----------------------------------------------------------------------------------------
def _poly(m_exp):
    m = Model(name=f'poly{m_exp}')
    m.set_equations(f"dx/dt = t^{m_exp}\ny(k) = x(t)")
    return m


def test_poly_on_the_device():
    """A Runge-Kutta method of order s integrates t^(s-1) exactly when its stages are evaluated at the right times: to 4 ulp."""
    t0, dt, steps = 1.5, .25, 4
    X0 = np.zeros((3, 1))
    for order, n_sub in ((1, 1), (2, 1), (3, 1), (4, 1), (4, 8)):
        m_exp = order - 1
        m = _poly(m_exp)
        m = m.setup(dt=dt) if n_sub == 8 else m.discretize('erk', order).setup(dt=dt)     # (8: the default map of a continuous model)
        x, _ = m.rollout(X0, steps=steps, t0=t0)
        exact = ((t0 + steps * dt) ** (m_exp + 1) - t0 ** (m_exp + 1)) / (m_exp + 1)
        print(f"order {order} x {n_sub}, t^{m_exp}: {x[-1, 0, 0]!r} vs {exact!r}")
        assert np.all(np.abs(x[-1, :, 0] - exact) <= 4. * np.spacing(exact))
    x, _ = _poly(4).discretize('erk', 4).setup(dt=dt).rollout(X0, steps=steps, t0=t0)
    exact = ((t0 + steps * dt) ** 5 - t0 ** 5) / 5
    assert np.all(np.abs(x[-1, :, 0] - exact) > 1e3 * np.spacing(exact))                    # t^4 is beyond order 4


# ---- 7: a discrete model ---------------------------------------------------------------------------------------------------------------
def test_discrete_model_sees_the_time_of_the_call():
    """x(k+1) = a x(k) + sin(t_k), y(k) = x(k+1) + t_k with t_k = t0 + k dt: the map and the measurement of call k are handed the
    same time (the reference's discrete function takes one time value per call, modules/base.py:1785-1795, :1882-1895)."""
    m = Model(name='disc', discrete=True)
    m.set_equations("x(k+1) = a*x(k) + sin(t)\ny(k) = x(k) + t")
    m.setup(dt=.5)
    t0, steps = 2.5, 5
    X0 = np.array([[1.], [-2.], [.25]])
    a = np.array([[.9], [.5], [-.7]])
    x, y = m.rollout(X0, None, a, steps=steps, t0=t0)
    ref = [X0]
    for k in range(steps):
        ref.append(a * ref[-1] + np.sin(t0 + k * .5))
    ref = np.array(ref)
    np.testing.assert_allclose(x, ref, rtol=1e-14)
    np.testing.assert_allclose(y, ref[1:] + (t0 + .5 * np.arange(steps))[:, None, None], rtol=1e-14)
    xn, yn = m.step(X0, None, a, t0=t0 + .5)                  # one call at t_1
    np.testing.assert_allclose(xn, a * X0 + np.sin(t0 + .5), rtol=1e-14)


# ---- 8: no value crosses lanes -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('solver', ['dopri5', 'bdf'])
def test_an_instance_does_not_depend_on_its_neighbours(solver):
    X0, U, Useq, P = _forced2_batch()
    m = _forced2(solver=solver, solver_options={'reltol': 1e-8, 'abstol': 1e-10})
    x, y = m.rollout(X0, U, P, steps=STEPS, t0=2.5)
    x1, y1 = m.rollout(X0[:1], U[:1], P[:1], steps=STEPS, t0=2.5)
    assert np.array_equal(x[:, 0], x1[:, 0]) and np.array_equal(y[:, 0], y1[:, 0])
    assert not np.array_equal(x[:, 0], x[:, 1])


# ---- 9: simulate continues the clock -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('solver', [None, 'dopri5', 'bdf'])
def test_simulate_in_two_calls_equals_one_rollout(solver):
    """`simulate` of 5 + 5 intervals from t0 = 2.5 against one `rollout` of 10: bit for bit under the map and 'dopri5'; under 'bdf'
    with held inputs the second call restarts the integrator, so both are held to the bound of the stiff tests instead.

    Under 'dopri5' one roll-out carries each instance's step-size proposal across every sampling instant; `simulate` keeps the
    proposals its call ended with and hands them to the next (`hilo_model_rollout_resume`), and the slope at the start is
    evaluated again at the same time and state - without that the two differ by about 1e-10 here."""
    rtol, atol = 1e-8, 1e-10
    X0, U, _, P = _forced2_batch(8)
    m = _forced2(**({'solver': solver, 'solver_options': {'reltol': rtol, 'abstol': atol}} if solver else {}))
    x, y = m.rollout(X0, U, P, steps=STEPS, t0=2.5)
    m.set_initial_conditions(X0, t0=2.5)
    m.simulate(u=U, p=P, steps=5)
    assert float(np.ravel(m.solution['t:f'])[0]) == 5.
    m.simulate(u=U, p=P, steps=5)
    xs, ys = m.solution['x'], m.solution['y']
    diff = float(np.max(np.abs(xs - x)))
    print(f"simulate 5 + 5 vs rollout 10 ({solver}): largest difference {diff:.3e}")
    if solver == 'bdf':
        ref, admissible, e_bdf, e_tight, _ = tv.bounds_batch('stiff', 'forced2', X0, U, P, .5, STEPS, 2.5, [(rtol, atol)])[0]
        _within("simulate 5 + 5 under bdf", xs, ref, admissible, e_bdf, e_tight, rtol, atol)
        _within("rollout 10 under bdf", x, ref, admissible, e_bdf, e_tight, rtol, atol)
    else:
        assert np.array_equal(xs, x) and np.array_equal(ys, y)


# ---- the failure exits of the explicit pair on a time-variant model -----------------------------------------------------------------------
def test_dopri5_failure_ends_the_instance_and_no_other():
    """prothero1 under 'dopri5' with 2000 attempted steps per interval: the explicit pair is bound by stability to steps of about
    3.3 / lam, so lam >= 3e4 (about 9000 steps per interval) ends with 'max_num_steps reached' and NaN rows, lam <= 1e3 (about 300)
    reaches the end within 10 FACTOR rtol of the exact solution, and a finished lane next to a failed one equals its own B = 1 run
    bit for bit."""
    rtol, atol = 1e-8, 1e-10
    x0, _, _, dt, steps, t0 = tv.CASES['prothero1']
    rng = np.random.default_rng(23)
    P = 10. ** rng.uniform(1., 5., (BS, 1))
    P[:4, 0] = [1e2, 1e5, 5e1, 5e4]
    X0 = np.tile(x0, (BS, 1))
    m = _prothero(solver='dopri5', solver_options={'reltol': rtol, 'abstol': atol, 'max_num_steps': 2000})
    x, y, stats = m.rollout(X0, None, P, steps=STEPS, return_stats=True, t0=t0)
    stiff, mild = P[:, 0] >= 3e4, P[:, 0] <= 1e3
    print(f"{int(stiff.sum())} stiff, {int(mild.sum())} mild of {BS}; status counts {np.bincount(stats['status'], minlength=3)}")
    assert np.all(stats['status'][stiff] == 1) and np.all(np.isnan(x[1:, stiff]))
    assert np.all(stats['status'][mild] == 0)
    ok = stats['status'] == 0
    t = t0 + np.arange(STEPS + 1)
    exact = tv.prothero_exact(t[:, None], X0[None, ok, 0], P[None, ok, 0], t0)
    e_exact = np.max(np.abs(x[:, ok, 0] - exact) / np.abs(exact))
    print(f"   finished instances against the exact solution {e_exact:.3e}")
    assert e_exact <= 10. * sr.FACTOR * rtol
    x1, _ = m.rollout(X0[:1], None, P[:1], steps=STEPS, t0=t0)
    assert np.array_equal(x[:, 0], x1[:, 0])
