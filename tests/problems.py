"""Shared plain problem specs (SURVEY.md 8d synthetic configurations), buildable as oracle or product objects."""
import numpy as np

SEED = 20260926

C2 = dict(                       # tracking NMPC on the CSTR-sized chemostat (nx=4, nu=2, N=20)
    model='chemostat4', dt=1., N=20, order=4,
    stage_states=[([2], [10.], [2.])],           # P -> 2, weight 10 (nmpc_hybrid_bio.ipynb cell 16 pattern)
    stage_inputs=[([0, 1], [.1, .1], None)],
    terminal_states=[([2], [10.], [2.])],
    x_lb=[0., 0., 0., 0.], u_lb=[0., 0.], u_ub=[1., 1.],
    x_guess=[.1, 40., 0., 0.], u_guess=[0., 0.],
    p=[100., 4., 1., 0.],
)


def c2_x0(B, seed=SEED):
    rng = np.random.default_rng(seed)
    return np.array([.1, 40., 0., 0.]) * (1 + .1 * rng.uniform(-1, 1, (B, 4)))


def oracle_problem(spec):
    from oracle import models
    from oracle.nmpc import NmpcProblem
    kw = {k: v for k, v in spec.items() if k not in ('model', 'p')}
    return NmpcProblem(models.get(spec['model']), **kw)


def symbolic_model(name):
    """The zoo models written as expressions - what a reference user does with `Model.set_dynamical_equations`
    (dynamic_model.py:1293-1553).  Each statement mirrors the compiled functor of csrc/hilo_models.h term by term, so that the
    emitted code and the hand-written one are the same expression tree."""
    from hilo_mpc_amd import Model
    from hilo_mpc_amd.expr import cos, exp, sin
    m = Model(name=name + '_expr')
    if name in ('chemostat4', 'pendulum4', 'cstr3'):
        from hilo_mpc_amd import zoo_expr
        return zoo_expr.define(m, name)
    if name == 'chemostat4_dae':
        # oracle/models.py::chemostat4_dae: the growth rate as algebraic state that feeds back into the balances
        x = m.set_dynamical_states(['X', 'S', 'P', 'I'])
        u = m.set_inputs(['DS', 'DI'])
        p = m.set_parameters(['Sf', 'If', 'ISF', 'IRF'])
        z = m.set_algebraic_states(['mu'])
        X, S, Pr, I = x
        phi = 0.407 * S / (0.108 + S + S * S / 14814.0)
        Rfp = phi * (0.0005 + I) / (0.022 + I)
        D = u[0] + u[1]
        m.set_dynamical_equations([z[0] * X - D * X, -(2.0 * z[0] * X) - D * S + u[0] * p[0], Rfp * X - D * Pr,
                                   -(D * I) + u[1] * p[1]])
        m.set_algebraic_equations([z[0] - phi * (p[2] + 0.22 * p[3] / (0.22 + I))])
        m.set_measurement_equations([X, Pr])
    elif name == 'pendulum4_dae':
        # the reference's DAE test model (tests/test_NMPC.py:1866-1911): height of the pendulum tip as algebraic state
        x = m.set_dynamical_states(['x', 'v', 'theta', 'omega'])
        u = m.set_inputs(['F'])
        z = m.set_algebraic_states(['y'])
        M, mm, l, g, h = 5.0, 1.0, 1.0, 9.81, .5
        s, c = sin(x[2]), cos(x[2])
        dv = 1.0 / (M + mm - mm * c) * (mm * g * s - mm * l * s * x[3] * x[3] + u[0])
        m.set_dynamical_equations([x[1], dv, x[3], 1.0 / l * (dv * c + g * s)])
        m.set_algebraic_equations([h + l * c - z[0]])
        m.set_measurement_equations([x[0], x[1], x[2], x[3]])
    elif name in ('robot6', 'robot6_dae'):
        # C5's robot (oracle/models.py::robot6) and its DAE variant: the squared speed as algebraic state, 0 = z - (vx^2 + vy^2)
        x = m.set_dynamical_states(['px', 'vx', 'py', 'vy', 'psi', 'omega'])
        u = m.set_inputs(['a', 'alpha'])
        m.set_dynamical_equations([x[1], u[0] * cos(x[4]), x[3], u[0] * sin(x[4]), x[5], u[1]])
        if name == 'robot6_dae':
            z = m.set_algebraic_states(['z'])
            m.set_algebraic_equations([z[0] - (x[1] * x[1] + x[3] * x[3])])
        m.set_measurement_equations([x[0], x[2]])
    elif name == 'chemostat4_mu':
        # the chemostat whose growth rate of the biomass balance is a parameter `mu` - to be replaced by a learned model
        # (`model.substitute_from(gp)`, nmpc_hybrid_bio.ipynb); the other rates keep their closed forms
        x = m.set_dynamical_states(['X', 'S', 'P', 'I'])
        u = m.set_inputs(['DS', 'DI'])
        p = m.set_parameters(['Sf', 'If', 'ISF', 'IRF', 'mu'])
        X, S, Pr, I = x
        phi = 0.407 * S / (0.108 + S + S * S / 14814.0)
        Rs = 2.0 * (phi * (p[2] + 0.22 * p[3] / (0.22 + I)))
        Rfp = phi * (0.0005 + I) / (0.022 + I)
        D = u[0] + u[1]
        m.set_dynamical_equations([p['mu'] * X - D * X, -(Rs * X) - D * S + u[0] * p[0], Rfp * X - D * Pr,
                                   -(D * I) + u[1] * p[1]])
        m.set_measurement_equations([X, Pr])
    else:
        raise ValueError(name)
    return m


def product_nmpc(spec, gp=None, model=None, **solver_options):
    """Build the product NMPC for a plain spec through the reference-style API."""
    from hilo_mpc_amd import NMPC, Model
    if model is not None:
        m = model
    elif spec['model'] == 'chemostat4_gp':
        m = Model('chemostat4')
        m.substitute_from(gp if gp is not None else product_gp())                 # dynamic_model.py:3040-3125
    else:
        m = Model(spec['model'])
    m = m.discretize('erk', order=spec.get('order', 4)).setup(dt=spec['dt'])
    nmpc = NMPC(m)
    xs, us = m.dynamical_state_names, m.input_names
    for ind, W, ref in spec.get('stage_states', []):
        nmpc.quad_stage_cost.add_states(names=[xs[i] for i in ind], weights=list(W), ref=ref)
    for ind, W, ref in spec.get('stage_inputs', []):
        nmpc.quad_stage_cost.add_inputs(names=[us[i] for i in ind], weights=list(W), ref=ref)
    if spec.get('Nc'):
        nmpc.prediction_horizon, nmpc.control_horizon = spec['N'], spec['Nc']
    if spec.get('input_change'):
        ind, W = spec['input_change']
        nmpc.quad_stage_cost.add_inputs_change(names=[us[i] for i in ind], weights=list(W))
    for ind, W, ref in spec.get('terminal_states', []):
        nmpc.quad_terminal_cost.add_states(names=[xs[i] for i in ind], weights=list(W), ref=ref)
    if not spec.get('Nc'):
        nmpc.horizon = spec['N']
    nmpc.set_box_constraints(x_ub=spec.get('x_ub'), x_lb=spec.get('x_lb'), u_ub=spec.get('u_ub'), u_lb=spec.get('u_lb'))
    nmpc.set_initial_guess(x_guess=spec.get('x_guess'), u_guess=spec.get('u_guess'))
    if spec.get('x_scaling') or spec.get('u_scaling'):
        nmpc.set_scaling(x_scaling=spec.get('x_scaling'), u_scaling=spec.get('u_scaling'))
    nmpc.setup(options={'integration_method': 'discrete'}, solver_options=solver_options or None)
    return nmpc


# ---- the reference's only published NMPC result: docs/docsource/examples/CSTR_Example.ipynb ---------------------------------
# cell 4 constants; cell 6 `true_plant_model`; cell 14 controller; cell 16 printed output after 1000 closed-loop steps
CSTR = dict(T_0=400., tau=60., k_A=5000., k_B=1e6, E_A=1e4, E_B=1.5e4, R=1.987, dH=-5000., rho=1., Cp=1000., C_A_0=1., V=100.,
            x_lb=[0., 0., 400.], x_ub=[1., 1., 500.], u_lb=[0.], u_ub=[1e5], x_scaling=[1., 1., 1e2], u_scaling=[1e5],
            x_guess=[0.4912, 0.5088, 438.47], u_guess=[59881.84], heat_price=7e-7, N=10, dt=1., x0=[1., 0., 400.])
CSTR_PRINTED = ('59882.1817', '0.4912', '0.5088', '438.4732')        # Q, C_A, C_B, T of the line "True: ..."


def cstr_equations(x, u, lib=None):
    from hilo_mpc_amd.zoo_expr import cstr_equations as f
    return f(x, u, lib)


def cstr_nmpc(heat_price=None, **solver_options):
    """Cell 14, statement by statement, on the product API."""
    from hilo_mpc_amd import NMPC, Model
    c = CSTR
    plant = Model(name='plant')
    x = plant.set_dynamical_states(['C_A', 'C_B', 'T'])
    u = plant.set_inputs(['Q'])
    ode, r = cstr_equations(x, u)
    plant.set_dynamical_equations(ode)
    plant.set_measurement_equations([r])
    plant.setup(dt=c['dt'])
    nmpc = NMPC(plant)
    nmpc.set_scaling(x_scaling=c['x_scaling'], u_scaling=c['u_scaling'])
    nmpc.stage_cost.cost = plant.x[0] / c['C_A_0'] + plant.u[0] * (c['heat_price'] if heat_price is None else heat_price)
    nmpc.horizon = c['N']
    nmpc.set_box_constraints(x_lb=c['x_lb'], x_ub=c['x_ub'], u_lb=c['u_lb'], u_ub=c['u_ub'])
    nmpc.set_initial_guess(x_guess=c['x_guess'], u_guess=c['u_guess'])
    nmpc.setup(options={'print_level': 0}, solver_options=solver_options or None)
    return nmpc


def cstr_oracle(**ipm_options):
    from oracle import models
    from oracle.nmpc import IpmOptions
    from oracle.nmpc_coll import CollIpm, CollNmpcProblem
    c = CSTR
    m = models.get('cstr3')
    pb = CollNmpcProblem(m, dt=c['dt'], N=c['N'], degree=3, objective='continuous',
                         generic_stage=m.x[0] / c['C_A_0'] + m.u[0] * c['heat_price'],
                         x_lb=c['x_lb'], x_ub=c['x_ub'], u_lb=c['u_lb'], u_ub=c['u_ub'], x_scaling=c['x_scaling'],
                         u_scaling=c['u_scaling'], x_guess=c['x_guess'], u_guess=c['u_guess'])
    return pb, CollIpm(pb, IpmOptions(**ipm_options))


def cstr_plant(x, u, n_sub=50):
    """One sampling interval of the true plant: classic RK4 with `n_sub` sub-steps (numpy; test harness, stands in for the
    reference's CVODES call `plant.simulate(u=u)`)."""
    import numpy as _np

    class L:
        exp = staticmethod(_np.exp)
    x = _np.array(x, dtype=float)
    u = _np.asarray(u, dtype=float).reshape(x.shape[0], 1)
    h = CSTR['dt'] / n_sub

    def f(z):
        d, _ = cstr_equations([z[:, 0], z[:, 1], z[:, 2]], [u[:, 0]], lib=L)
        return _np.stack(d, axis=1)
    for _ in range(n_sub):
        k1 = f(x)
        k2 = f(x + .5 * h * k1)
        k3 = f(x + .5 * h * k2)
        k4 = f(x + h * k3)
        x = x + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
    return x


# ---- C3: MHE on the chemostat (nx=4, ny=2, N=30), SURVEY.md 8d ------------------------------------------------
C3 = dict(model='chemostat4', dt=.25, N=30, order=4, Wx=[4.] * 4, Wy=[16.] * 2, Ww=[1e6] * 4,
          x_lb=[0., 0., 0., 0.], x_guess=[.1, 40., 0., 0.], p=[100., 4., 1., 0.])


# C3 with the process noise boxed: in the reference's formulation w_0 carries no cost (mhe.py:742-748), so x_1 is free
# and the weakly observable states S, I make the plain C3 NLP degenerate (several KKT points); the box ties x_1 to
# Phi(x_0) and makes the minimiser unique - used for the tight parity comparison
C3B = dict(C3, w_lb=[-1e-3] * 4, w_ub=[1e-3] * 4)


def chemostat4_rk4(x, u, p, dt):
    """One classic Runge-Kutta step of the benchmark's chemostat (`ecoli_D1210_conti('simple')` with the rates of the
    'complex' variant, library/models.py:143-198) in plain numpy - the synthetic truth of the estimator workloads.  (Plain numpy so
    that building a workload needs nothing of `oracle/`; the same right-hand side as oracle/models.py::chemostat4 and the product's
    zoo functor, which tests/test_oracle_mhe.py checks.)"""
    Sf, If, ISF, IRF = (np.asarray(p, dtype=float) + np.zeros((x.shape[0], 4))).T

    def f(x):
        X, S, P, I = x.T
        DS, DI = u.T
        phi = 0.407 * S / (0.108 + S + S ** 2 / 14814.0)
        mu = phi * (ISF + 0.22 * IRF / (0.22 + I))
        Rfp = phi * (0.0005 + I) / (0.022 + I)
        D = DS + DI
        return np.stack([mu * X - D * X, -2 * mu * X - D * S + DS * Sf, Rfp * X - D * P, -D * I + DI * If], axis=1)
    k1 = f(x)
    k2 = f(x + .5 * dt * k1)
    k3 = f(x + .5 * dt * k2)
    k4 = f(x + dt * k3)
    return x + dt / 6. * (k1 + 2 * k2 + 2 * k3 + k4)


def product_mhe(spec, **solver_options):
    """The product's moving-horizon estimator for a spec of this module (C3 / C3B) through the reference-style API
    (the pattern of tests/test_MHE.py:403-409)."""
    from hilo_mpc_amd import MHE, Model
    m = Model(spec['model']).discretize('erk', order=spec.get('order', 4)).setup(dt=spec['dt'])
    mhe = MHE(m)
    mhe.quad_arrival_cost.add_states(weights=list(spec['Wx']), guess=spec['x_guess'])
    mhe.quad_stage_cost.add_measurements(weights=list(spec['Wy']))
    mhe.quad_stage_cost.add_state_noise(weights=list(spec['Ww']))
    mhe.horizon = spec['N']
    mhe.set_box_constraints(x_lb=spec.get('x_lb'), x_ub=spec.get('x_ub'), w_lb=spec.get('w_lb'), w_ub=spec.get('w_ub'),
                            p_lb=spec['p'], p_ub=spec['p'])
    mhe.set_initial_guess(x_guess=spec['x_guess'])
    if spec.get('x_scaling') or spec.get('w_scaling') or spec.get('u_scaling'):
        mhe.set_scaling(x_scaling=spec.get('x_scaling'), w_scaling=spec.get('w_scaling'), u_scaling=spec.get('u_scaling'))
    mhe.setup(options={'integration_method': 'discrete'}, nlp_opts=solver_options or None)
    return mhe


# ---- C1: LMPC on the discrete double integrator (tests/test_LMPC.py:8-33), SURVEY.md 8d ---------------------------------------
LMPC_DT = .5
LMPC_A = np.array([[1., LMPC_DT], [0., 1.]])                 # tests/test_LMPC.py:14-15
LMPC_B = np.array([[LMPC_DT ** 2 / 2], [LMPC_DT]])
C1 = dict(A=LMPC_A, B=LMPC_B, N=10, Q=np.eye(2), R=[[1.]], x_lb=[-5, -5], x_ub=[5, 5], u_lb=[-1], u_ub=[1])


def product_lmpc(kron_variant, N=10, Q=None):
    from hilo_mpc_amd import LMPC, Model
    m = Model('lti', A=LMPC_A, B=LMPC_B).setup(dt=LMPC_DT)     # tests/test_LMPC.py:8-19
    mpc = LMPC(m)
    mpc.Q = np.eye(2) if Q is None else Q
    mpc.R = 1
    mpc.horizon = N
    mpc.set_box_constraints(x_lb=[-5, -5], x_ub=[5, 5], u_lb=[-1], u_ub=[1])
    mpc.setup(kron_variant=kron_variant)
    return mpc


def c3_data(B, N=30, seed=SEED):
    """Truth simulated with the RK4 map from perturbed initial states under slowly varying inputs, measurements
    y = (X, P) + N(0, 1e-2).  Returns x_arrival [B,4], u_meas [B,N,2], y_meas [B,N,2], x_true [B,N+1,4]."""
    rng = np.random.default_rng(seed)
    x = np.array([.1, 40., 0.05, 0.05]) * (1 + .1 * rng.uniform(-1, 1, (B, 4)))
    xs = [x]
    u = np.empty((B, N, 2))
    for k in range(N):
        u[:, k, 0] = .05 + .03 * np.sin(.3 * k + rng.uniform(0, 6.28, B))
        u[:, k, 1] = .02 + .01 * np.cos(.2 * k + rng.uniform(0, 6.28, B))
        x = chemostat4_rk4(x, u[:, k], C3['p'], C3['dt'])
        xs.append(x)
    xt = np.stack(xs, axis=1)
    y = xt[:, :N][:, :, [0, 2]] + .01 * rng.normal(size=(B, N, 2))
    xa = xt[:, 0] * (1 + .05 * rng.normal(size=(B, 4)))
    return xa, u, y, xt


def oracle_mhe(spec):
    from oracle import models
    from oracle.mhe import MheProblem
    kw = {k: v for k, v in spec.items() if k not in ('model', 'p')}
    return MheProblem(models.get(spec['model']), **kw)


# ---- C4: GP-hybrid NMPC: chemostat4 whose biomass growth rate `mu` comes from a GP over (S, I) ----------
C4_GP = dict(length_scales=[10., 1.], signal_variance=1., noise_variance=1e-4)
C4 = dict(C2, model='chemostat4_gp')


def c4_training_data(seed=SEED):
    """200 points on a 20 x 10 grid of S in [0, 40], I in [0, 4]; targets = the closed-form rate (ISF = 1, IRF = 0:
    the parameter values of C2) + N(0, 1e-4).  Returns X (2 x 200), y (1 x 200)."""
    S, I = np.meshgrid(np.linspace(0., 40., 20), np.linspace(0., 4., 10), indexing='ij')
    S, I = S.ravel(), I.ravel()
    phi = 0.407 * S / (0.108 + S + S ** 2 / 14814.0)
    mu = phi * (1. + 0.22 * 0. / (0.22 + I))
    rng = np.random.default_rng(seed + 4)
    return np.stack([S, I]), (mu + 1e-2 * rng.standard_normal(mu.size))[None, :]


def oracle_c4(spec=C4):
    from oracle import gp as ogp, models
    from oracle.nmpc import NmpcProblem
    X, y = c4_training_data()
    post = ogp.Posterior({'type': 'squared_exponential',
                          'kwargs': dict(active_dims=[0, 1], length_scales=C4_GP['length_scales'], ard=True,
                                         signal_variance=C4_GP['signal_variance'])},
                         {'type': 'zero'}, X, y, C4_GP['noise_variance'])
    model = models.chemostat4_gp(X, post.alpha, C4_GP['length_scales'], C4_GP['signal_variance'])
    kw = {k: v for k, v in spec.items() if k not in ('model', 'p')}
    return NmpcProblem(model, **kw), post


def product_gp(X=None, y=None):
    from hilo_mpc_amd import GP, Kernel
    if X is None:
        X, y = c4_training_data()
    gp = GP(['S', 'I'], ['mu'], kernel=Kernel.squared_exponential(active_dims=[0, 1], length_scales=C4_GP['length_scales'],
                                                                  ard=True, signal_variance=C4_GP['signal_variance']),
            noise_variance=C4_GP['noise_variance'])
    gp.set_training_data(X, y)
    gp.setup()
    return gp


# ---- general NMPC: nonlinear stage constraints and path following -----------------
C2H = dict(C2, constraint=dict(expr=['X * S'], lb=[-np.inf], ub=[60.]))                      # hard, one-sided
C2S = dict(C2, constraint=dict(expr=['X * S'], lb=[-np.inf], ub=[60.], soft=True))           # soft, default W = 1e4
C5 = dict(                       # path-following NMPC, mobile robot nx=6 (+theta), nu=2 (+u_theta), soft speed limit
    model='robot6', dt=.1, N=50, order=4,
    stage_inputs=[([0, 1], [.1, .1], None)],
    path=dict(theta_guess=0., theta_lb=0., theta_ub=np.inf, u_pf_lb=1e-4, u_pf_ub=1.,
              stage=[([0, 2], [10., 10.], ['sin(theta)', 'sin(2*theta)'])],
              terminal=[([0, 2], [10., 10.], ['sin(theta)', 'sin(2*theta)'])]),
    constraint=dict(expr=['vx**2 + vy**2'], lb=[-np.inf], ub=[4.], soft=True),
    u_lb=[-5., -5.], u_ub=[5., 5.],
    x_guess=[0., 1.5, 0., 1.3, .6, 0.], u_guess=[0., 0.],      # guess = nominal initial state (tiled over the horizon)
    p=[],
)
C5S = dict(C5, N=10)             # short horizon for oracle-sized tests


def c5_x0(B, seed=SEED):
    rng = np.random.default_rng(seed + 5)
    return np.array([0., 1.5, 0., 1.3, .6, 0.]) + .1 * rng.uniform(-1, 1, (B, 6))   # |v|^2 ~ 3.9 +- 0.4 around the limit 4


def oracle_gen(spec):
    from oracle import models
    from oracle.nmpc_gen import GenNmpcProblem
    kw = {k: v for k, v in spec.items() if k not in ('model', 'p')}
    return GenNmpcProblem(models.get(spec['model']), **kw)


def product_gen(spec, **solver_options):
    """Product NMPC for a general spec (path following / stage constraints) through the reference-style API; the
    expression strings of the spec are evaluated on the model's symbols.  spec['collocation'] = dict(degree=, points=, objective=):
    the continuous model (written as expressions; DAE models too) under the reference's default integration method."""
    from hilo_mpc_amd import NMPC, Model, expr
    coll = spec.get('collocation')
    if coll is not None:
        m = symbolic_model(spec['model']).setup(dt=spec['dt'])
    else:
        m = Model(spec['model']).discretize('erk', order=spec.get('order', 4)).setup(dt=spec['dt'])
    nmpc = NMPC(m)
    xs, us = m.dynamical_state_names, m.input_names
    ns = {'sin': expr.sin, 'cos': expr.cos, 'exp': expr.exp, 'log': expr.log, 'sqrt': expr.sqrt}
    ns.update({n: m.x[n] for n in xs})
    ns.update({n: m.u[n] for n in us})
    if getattr(m, 'n_z', 0):
        ns.update({n: m.z[n] for n in m.algebraic_state_names})
    for ind, W, ref in spec.get('stage_states', []):
        nmpc.quad_stage_cost.add_states(names=[xs[i] for i in ind], weights=list(W), ref=ref)
    for ind, W, ref in spec.get('stage_inputs', []):
        nmpc.quad_stage_cost.add_inputs(names=[us[i] for i in ind], weights=list(W), ref=ref)
    for ind, W, ref in spec.get('terminal_states', []):
        nmpc.quad_terminal_cost.add_states(names=[xs[i] for i in ind], weights=list(W), ref=ref)
    if spec.get('path'):
        pa = dict(spec['path'])
        theta = nmpc.create_path_variable(**{k: v for k, v in pa.items() if k not in ('stage', 'terminal')})
        ns[pa.get('name', 'theta')] = theta
        for ind, W, refs in pa.get('stage', []):
            nmpc.quad_stage_cost.add_states(names=[xs[i] for i in ind], weights=list(W), path_following=True,
                                            ref=[eval(r, dict(ns)) for r in refs])
        for ind, W, refs in pa.get('terminal', []):
            nmpc.quad_terminal_cost.add_states(names=[xs[i] for i in ind], weights=list(W), path_following=True,
                                               ref=[eval(r, dict(ns)) for r in refs])
    if spec.get('constraint'):
        co = spec['constraint']
        nmpc.stage_constraint.constraint = [eval(e, dict(ns)) for e in co['expr']]
        nmpc.stage_constraint.lb, nmpc.stage_constraint.ub = list(co['lb']), list(co['ub'])
        nmpc.stage_constraint.is_soft = bool(co.get('soft', False))
        if co.get('weight') is not None:
            nmpc.stage_constraint.weight = co['weight']
        if co.get('max_violation') is not None:
            nmpc.stage_constraint.max_violation = co['max_violation']
    if spec.get('terminal_constraint'):
        tc = spec['terminal_constraint']
        nmpc.terminal_constraint.constraint = [eval(e, dict(ns)) for e in tc['expr']]
        nmpc.terminal_constraint.lb, nmpc.terminal_constraint.ub = list(tc['lb']), list(tc['ub'])
        nmpc.terminal_constraint.is_soft = bool(tc.get('soft', False))
        if tc.get('weight') is not None:
            nmpc.terminal_constraint.weight = tc['weight']
        if tc.get('max_violation') is not None:
            nmpc.terminal_constraint.max_violation = tc['max_violation']
    nmpc.horizon = spec['N']
    nmpc.set_box_constraints(x_ub=spec.get('x_ub'), x_lb=spec.get('x_lb'), u_ub=spec.get('u_ub'), u_lb=spec.get('u_lb'))
    nmpc.set_initial_guess(x_guess=spec.get('x_guess'), u_guess=spec.get('u_guess'), z_guess=spec.get('z_guess'))
    if spec.get('custom'):
        cu = spec['custom']
        nmpc.set_custom_constraints_function(cu['fun'], lb=cu.get('lb'), ub=cu.get('ub'), **(
            dict(soft=True, max_violation=cu.get('max_violation', np.inf)) if cu.get('soft') else {}))
    if spec.get('x_scaling') or spec.get('u_scaling'):
        nmpc.set_scaling(x_scaling=spec.get('x_scaling'), u_scaling=spec.get('u_scaling'))
    if coll is not None:
        opts = {'integration_method': 'collocation', 'degree': coll.get('degree', 3), 'collocation_points': coll.get('points', 'radau'),
                'objective_function': coll.get('objective', 'continuous')}
    else:
        opts = {'integration_method': 'discrete'}
    nmpc.setup(options=opts, solver_options=solver_options or None)
    return nmpc


# BASELINE configuration 5 as it is written: path following on the robot's DAE (squared speed as algebraic state) with the soft
# speed limit on that algebraic state, the reference's default transcription (collocation, Radau 3, continuous objective)
C5D = dict(C5, model='robot6_dae', constraint=dict(expr=['z'], lb=[-np.inf], ub=[4.], soft=True), z_guess=[3.94],
           collocation=dict(degree=3))
C5DS = dict(C5D, N=10)


def oracle_coll_gen(spec):
    from oracle import models
    from oracle.nmpc_coll_gen import GenCollProblem
    kw = {k: v for k, v in spec.items() if k not in ('model', 'p', 'order', 'collocation', 'terminal_constraint')}
    co = spec.get('collocation', {})
    return GenCollProblem(models.get(spec['model']), degree=co.get('degree', 3), points=co.get('points', 'radau'),
                          objective=co.get('objective', 'continuous'), terminal=spec.get('terminal_constraint'), **kw)


# ---- stochastic NMPC: the reference's own test systems (tests/test_SMPC.py) and a nonlinear one -------------
SMPC_GP = dict(length_scales=[.5], signal_variance=1., noise_variance=1e-2)


def smpc_training_data():
    """tests/test_SMPC.py:38-39."""
    X = np.array([[0., .5, 1. / np.sqrt(2.), np.sqrt(3.) / 2., 1., 0.]])
    y = np.array([[0., np.pi / 6., np.pi / 4., np.pi / 3., np.pi / 2., np.pi]])
    return X, y


SMPC_CASES = {
    # tests/test_SMPC.py:8-44: a single integrator, explicit Euler with dt = 1, B = [[1]]; input weight and terminal cost added so
    # that the problem is regular (the reference's smoke configuration leaves the last input undetermined)
    'siso': dict(order=1, features=[0], Bw=[[1.]], N=10, x0=[15.], cov0=[[0.]], K=[[0.]],
                 stage_states=[([0], [10.], [1.])], stage_inputs=[([0], [.1], None)], terminal_states=[([0], [10.], [1.])],
                 x_lb=[10.], x_lb_p=[.9]),
    # tests/test_SMPC.py:132-170: two integrators, B = [[1], [1]], bounds on both sides.  Map checks and smoke runs only: the
    # terminal rows take sqrt(Kx_ii) of the INTEGRATED end state, which is negative at trial points with an indefinite Kx
    # (its off-diagonal entries are free variables) - every solver's path through those NaN rejections is its own
    'mimo': dict(solve=False, order=1, features=[0], Bw=[[1.], [1.]], N=8, x0=[15., 10.], cov0=[[.01, 0.], [0., .02]],
                 K=[[-.2, 0.], [0., -.1]],
                 stage_states=[([0, 1], [10., 10.], [1., 1.])], stage_inputs=[([0, 1], [.1, .1], None)],
                 terminal_states=[([0, 1], [10., 10.], [1., 1.])],
                 x_lb=[-100., 0.], x_lb_p=[.95, .95], x_ub=[100., 30.], x_ub_p=[.95, .95]),
    # a nonlinear plant (pendulum-like, Heun's method): the Jacobian of the known part depends on the state; the learned
    # term acts on the velocity and reads the angle
    'pend': dict(order=2, features=[0], Bw=[[0.], [.1]], N=8, x0=[.9, 0.], cov0=[[1e-3, 0.], [0., 1e-3]], K=[[-.5, -.3]],
                 stage_states=[([0, 1], [10., 1.], [0., 0.])], stage_inputs=[([0], [.1], None)],
                 terminal_states=[([0, 1], [10., 1.], [0., 0.])],
                 x_lb=[-1.2, -2.], x_lb_p=[.95, .95], x_ub=[1.2, 2.], x_ub_p=[.95, .95], u_lb=[-3.], u_ub=[3.]),
}


def smpc_models(name):
    """(product model written as expressions, oracle model), both discretised like the case says (dt = 1)."""
    import sympy as sp
    from hilo_mpc_amd import Model
    from hilo_mpc_amd.expr import sin
    from oracle.models import OracleModel
    c = SMPC_CASES[name]
    m = Model(name=f'smpc_{name}')
    dt = sp.Symbol('dt')
    if name == 'siso':
        x, u = m.set_dynamical_states(['px']), m.set_inputs(['a'])
        m.set_dynamical_equations([u[0]])
        px, a = sp.symbols('px a')
        om = OracleModel(name, -1, [px], [a], [], [a], dt=dt)
    elif name == 'mimo':
        x, u = m.set_dynamical_states(['px', 'py']), m.set_inputs(['ax', 'ay'])
        m.set_dynamical_equations([u[0], u[1]])
        px, py, ax, ay = sp.symbols('px py ax ay')
        om = OracleModel(name, -1, [px, py], [ax, ay], [], [ax, ay], dt=dt)
    else:
        x, u = m.set_dynamical_states(['th', 'om']), m.set_inputs(['tau'])
        m.set_dynamical_equations([.3 * x[1], -.3 * sin(x[0]) - .05 * x[1] + .2 * u[0]])
        th, w, tau = sp.symbols('th om tau')
        om = OracleModel(name, -1, [th, w], [tau], [], [.3 * w, -.3 * sp.sin(th) - .05 * w + .2 * tau], dt=dt)
    m.discretize('erk', order=c['order'], inplace=True)
    m.setup(dt=1.)
    return m, om.discretize(c['order'])


def smpc_oracle_post():
    from oracle import gp as ogp
    X, y = smpc_training_data()
    return ogp.Posterior({'type': 'squared_exponential', 'kwargs': dict(active_dims=[0], length_scales=SMPC_GP['length_scales'],
                                                                        signal_variance=SMPC_GP['signal_variance'])},
                         {'type': 'zero'}, X, y, SMPC_GP['noise_variance'])


def smpc_product_gp(feature):
    """GP(['px'], 'z') of tests/test_SMPC.py:37-43 with FIXED hyper-parameters (the parity tests do not depend on a fit)."""
    from hilo_mpc_amd import GP, Kernel
    X, y = smpc_training_data()
    gp = GP([feature], ['z'], kernel=Kernel.squared_exponential(active_dims=[0], length_scales=SMPC_GP['length_scales'],
                                                                signal_variance=SMPC_GP['signal_variance']),
            noise_variance=SMPC_GP['noise_variance'])
    gp.set_training_data(X, y)
    gp.setup()
    return gp


def smpc_oracle_problem(name, Kgain_is_parameter=True, **kw):
    from oracle import smpc as osmpc
    c = SMPC_CASES[name]
    _, om = smpc_models(name)
    keys = ('stage_states', 'stage_inputs', 'terminal_states', 'x_lb', 'x_ub', 'x_lb_p', 'x_ub_p', 'u_lb', 'u_ub')
    return osmpc.smpc_problem(om, [smpc_oracle_post()], [c['features']], c['Bw'], c['N'], c['K'],
                              Kgain_is_parameter=Kgain_is_parameter, **{k: c[k] for k in keys if k in c}, **kw)


def smpc_product(name, gp, Kgain=None, **solver_options):
    """The same problem through the reference's interface (tests/test_SMPC.py:104-110)."""
    from hilo_mpc_amd import SMPC
    c = SMPC_CASES[name]
    m, _ = smpc_models(name)
    smpc = SMPC(m, gp, np.asarray(c['Bw']), Kgain=Kgain)
    smpc.horizon = c['N']
    xs, us = m.dynamical_state_names, m.input_names
    for ind, W, ref in c.get('stage_states', []):
        smpc.quad_stage_cost.add_states(names=[xs[i] for i in ind], weights=list(W), ref=ref)
    for ind, W, ref in c.get('stage_inputs', []):
        smpc.quad_stage_cost.add_inputs(names=[us[i] for i in ind], weights=list(W), ref=ref)
    for ind, W, ref in c.get('terminal_states', []):
        smpc.quad_terminal_cost.add_states(names=[xs[i] for i in ind], weights=list(W), ref=ref)
    kw = {k: c[k] for k in ('x_lb', 'x_ub', 'u_lb', 'u_ub', 'x_lb_p', 'x_ub_p') if k in c}
    smpc.set_box_chance_constraints(**kw)
    smpc.setup(options={'chance_constraints': 'prs', 'print_level': 0},
               solver_options={f'ipopt.{k}': v for k, v in solver_options.items()} or None)
    return smpc


def eval_exprs(exprs, x, u, p, gps=()):
    """Numeric value of expression trees (hilo_mpc_amd/expr.py) at one point - test helper: the product never evaluates its
    expressions on the host.  gps[k] = dict(mean=f(feats), var=f(feats), dmean=f(feats, j)) for the learned-term nodes."""
    import math
    from hilo_mpc_amd.expr import Expr
    allnodes = {}
    for e in exprs:
        Expr.wrap(e).nodes(allnodes)
    val = {}
    fn = {'sin': math.sin, 'cos': math.cos, 'exp': math.exp, 'log': math.log, 'sqrt': math.sqrt, 'log10': math.log10,
          'fabs': math.fabs, 'sign': lambda v: float((v > 0) - (v < 0)), 'asin': math.asin, 'acos': math.acos, 'atan': math.atan,
          'asinh': math.asinh, 'acosh': math.acosh, 'atanh': math.atanh, 'tanh': math.tanh,
          'sech2': lambda v: 4.0 * math.exp(-2.0 * abs(v)) / (1.0 + math.exp(-2.0 * abs(v))) ** 2}
    for n in sorted(allnodes.values(), key=lambda q: q.serial):
        a = [val[id(c)] for c in n.args]
        op = n.op
        if op == 'const':
            r = n.value
        elif op in ('x', 'u', 'p'):
            r = float({'x': x, 'u': u, 'p': p}[op][int(n.value)])
        elif op == 'add':
            r = a[0] + a[1]
        elif op == 'sub':
            r = a[0] - a[1]
        elif op == 'mul':
            r = a[0] * a[1]
        elif op == 'div':
            r = a[0] / a[1]
        elif op == 'neg':
            r = -a[0]
        elif op == 'sq':
            r = a[0] * a[0]
        elif op == 'powi':
            r = a[0] ** int(n.value)
        elif op == 'atan2':
            r = math.atan2(a[0], a[1])
        elif op in fn:
            r = fn[op](a[0])
        elif op == 'gp':
            r = gps[int(n.value)]['mean'](a)
        elif op == 'gpvar':
            r = gps[int(n.value)]['var'](a)
        elif op == 'gpd':
            r = gps[int(n.value[0])]['dmean'](a, int(n.value[1]))
        else:
            raise NotImplementedError(op)
        val[id(n)] = r
    return np.array([val[id(Expr.wrap(e))] for e in exprs])
