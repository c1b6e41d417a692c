"""Model descriptions: the zoo of device functors (hilo_mpc_amd/csrc/hilo_models.h) and models written as expressions
(`set_dynamical_states / set_inputs / set_parameters / set_algebraic_states`, `set_dynamical_equations`,
`set_algebraic_equations`, `set_measurement_equations`, `substitute_from`), which hilo_mpc_amd/codegen.py turns into a functor of
the same shape for the run-time compiler.

The reference's `Model` (hilo_mpc/modules/dynamic_model/dynamic_model.py) is a symbolic CasADi container; the
hot path only needs its *description*: dimensions, whether it is discrete, the discretisation recipe and the
sampling interval.  Method names follow the reference (`discretize`, `setup`, `is_linear`).
"""
import copy

import numpy as np

from . import expr as _expr
from .expr import Expr, SymVector


# name -> (model id, is_linear, state names, input names, parameter names, measurement names)
ZOO = {
    'lti': (0, True, None, None, None, None),
    'toy1d': (1, False, ['x'], [], [], ['y']),
    'bioreactor3': (2, False, ['T', 'cB', 'cS'], ['D'], ['alpha', 'T_amb', 'mu_0', 'mu_1', 'K', 'Y'],
                    ['y_0', 'y_1']),
    'chemostat4': (3, False, ['X', 'S', 'P', 'I'], ['DS', 'DI'], ['Sf', 'If', 'ISF', 'IRF'], ['yX', 'yP']),
    'pendulum4': (4, False, ['x', 'v', 'theta', 'omega'], ['F'], [], ['yx', 'yv', 'ytheta', 'tomega']),
    'robot6': (5, False, ['px', 'vx', 'py', 'vy', 'psi', 'omega'], ['a', 'alpha'], [], ['ypx', 'ypy']),
    'cstr3': (6, False, ['C_A', 'C_B', 'T'], ['Q'], [], ['r']),           # CSTR_Example.ipynb cell 6
    'linear2': (7, True, ['x_1', 'x_2'], ['u'], ['k_1', 'k_2'], ['y']),
    'chemostat4_gp': (8, False, ['X', 'S', 'P', 'I'], ['DS', 'DI'], ['Sf', 'If', 'ISF', 'IRF'], ['yX', 'yP']),
}
# zoo models whose right-hand side has a slot for a learned term: base name -> (label, features, hybrid functor)
LEARNABLE = {'chemostat4': ('mu', ['S', 'I'], 'chemostat4_gp')}
NATIVE_DISCRETE = {'toy1d', 'lti'}
# device functor of each zoo model (csrc/hilo_models.h): what a run-time compiled problem aliases as `UserModel`
ZOO_FUNCTOR = {'toy1d': 'Toy1D', 'bioreactor3': 'Bioreactor3', 'chemostat4': 'Chemostat4', 'pendulum4': 'Pendulum4',
               'robot6': 'Robot6', 'linear2': 'Linear2', 'cstr3': 'Cstr3'}
MODEL_USER = 100    # HILO_MODEL_USER: the model is defined by expressions and compiled at setup (csrc/hilo_jit.hip)
# `Model.setup(solver=...)`: integrators with error control and their options under CasADi's names (what the reference's
# `solver_options` carries to `ca.integrator`), with CasADi's defaults for CVODES
SOLVERS = {'dopri5': 1, 'bdf': 2, 'idas': 3}  # name -> hilo_sim_opts.method (HILO_SIM_DOPRI5, HILO_SIM_BDF, HILO_SIM_IDAS)
IDAS_MAX_STATES = 8  # n_x + n_z of a model under 'idas' (HILO_SIM_BDF_MAX_NX: the store of the method in the LDS of one workgroup)
SENS_MAX_NX = 4   # HILO_SIM_SENS_MAX_NX: the widest model the sensitivity roll-out is built for
SOLVER_OPTIONS = {'reltol': 1e-6, 'abstol': 1e-8, 'max_num_steps': 10000, 'first_step': 0.}
SIM_STATUS = {0: 'ok', 1: 'max_num_steps reached', 2: 'step size too small'}     # HILO_SIM_STATUS_*


class Model:
    """Zoo model: `Model('chemostat4').discretize('rk4').setup(dt=1.)`, or a model defined by expressions like the reference's
    (`Model.set_dynamical_states / set_inputs / set_parameters / set_dynamical_equations / set_measurement_equations`,
    hilo_mpc/modules/dynamic_model/dynamic_model.py:1293-1553):

        m = Model(name='plant')
        x = m.set_dynamical_states(['C_A', 'C_B', 'T']); u = m.set_inputs(['Q'])
        r = 5000 * exp(-1e4 / (1.987 * x[2])) * x[0] - 1e6 * exp(-1.5e4 / (1.987 * x[2])) * x[1]
        m.set_dynamical_equations([(1 - x[0]) / 60 - r, -x[1] / 60 + r, 5 * r + (400 - x[2]) / 60 + u[0] / 1e5])
        m.setup(dt=1.)

    Such a model is emitted as a device functor (hilo_mpc_amd/codegen.py) and compiled with hiprtc at `NMPC.setup()`.

    For `Model('lti', A=..., B=..., C=...)` the matrices define a discrete LTI system
    (`x+ = A x + B u`, `y = C x`, cf. tests/test_LMPC.py:8-19)."""

    _solver = None              # `setup(solver=...)`: None = the fixed-step maps, 'dopri5' / 'bdf' / 'idas' = integration with error control
    _solver_options = None

    def __init__(self, name=None, A=None, B=None, C=None, discrete=None, id=None, plot_backend=None, **kwargs):
        if name == 'chemostat4_gp':
            raise ValueError("build the hybrid model with Model('chemostat4').substitute_from(gp)")
        if name not in ZOO:
            # a model defined by expressions
            self.name = name
            self._symbolic = True
            self.model_id, self._linear = MODEL_USER, False
            self.dt, self.erk_order, self.n_sub, self._is_setup = None, 0, 1, False
            self._native_discrete = bool(discrete)
            self.dynamical_state_names, self.input_names, self.parameter_names, self.measurement_names = [], [], [], []
            self.n_x = self.n_u = self.n_p = self.n_y = 0
            self._ode, self._meas = None, []
            self.learned = None
            self._gps = []              # trained GPs substituted into the equations (substitute_from)
            self.algebraic_state_names, self.n_z, self._alg = [], 0, []    # semi-explicit DAE: 0 = g(x, z, u, p)
            return
        self._symbolic = False
        self.name = name
        self.model_id, self._linear, xs, us, ps, ys = ZOO[name]
        self.dt = None
        self.erk_order = 0          # 0: not discretised
        self.n_sub = 1
        self._is_setup = False
        if name == 'lti':
            A = np.atleast_2d(np.asarray(A, dtype=float))
            B = np.atleast_2d(np.asarray(B, dtype=float))
            if B.shape[0] != A.shape[0]:
                B = B.T
            C = np.eye(A.shape[0]) if C is None else np.atleast_2d(np.asarray(C, dtype=float))
            self.A, self.B, self.C = A, B, C
            self.n_x, self.n_u, self.n_y = A.shape[0], B.shape[1], C.shape[0]
            self.n_p = A.size + B.size + C.size
            self._native_discrete = True
            xs = [f'x_{i}' for i in range(self.n_x)]
            us = [f'u_{i}' for i in range(self.n_u)]
            ps, ys = [], [f'y_{i}' for i in range(self.n_y)]
        else:
            # dimensions are those of the device functor; tests/test_abi.py checks this table against
            # hilo_model_dims() of the built library
            self.n_x, self.n_u, self.n_p, self.n_y = len(xs), len(us), len(ps), len(ys)
            self._native_discrete = name in NATIVE_DISCRETE if discrete is None else bool(discrete)
        self.dynamical_state_names, self.input_names = list(xs), list(us)
        self.parameter_names, self.measurement_names = list(ps), list(ys)
        self.learned = None         # trained GaussianProcess substituted into the right-hand side

    # -- reference-like surface ---------------------------------------------------------------
    # symbols for expressions (the reference's `model.x`, `model.u`, `model.p` SX vectors)
    x = property(lambda s: SymVector('x', s.dynamical_state_names))
    u = property(lambda s: SymVector('u', s.input_names))
    p = property(lambda s: SymVector('p', s.parameter_names))
    z = property(lambda s: SymVector('z', getattr(s, 'algebraic_state_names', [])))
    t = property(lambda s: Expr('t', name='t'))     # the time, for equations written as expressions (`u[0] * sin(w * m.t)`)
    time = t

    @property
    def discrete(self):
        return self._native_discrete or self.erk_order > 0

    # -- models defined by expressions ----------------------------------------------------------------
    def _declare(self, attr, names, kind):
        if not self._symbolic:
            raise RuntimeError(f"'{self.name}' is a model of the device zoo; its variables are fixed")
        names = [names] if isinstance(names, str) else list(names)
        if len(set(names)) != len(names):
            raise ValueError(f"duplicate names in {names}")
        setattr(self, attr, names)
        self.n_x, self.n_u, self.n_p = len(self.dynamical_state_names), len(self.input_names), len(self.parameter_names)
        self.n_z = len(self.algebraic_state_names)
        return SymVector(kind, names)

    def set_dynamical_states(self, *names):
        """dynamic_model.py `set_dynamical_states`: returns the symbols of the states."""
        return self._declare('dynamical_state_names', names[0] if len(names) == 1 and not isinstance(names[0], str) else names, 'x')

    def set_inputs(self, *names):
        return self._declare('input_names', names[0] if len(names) == 1 and not isinstance(names[0], str) else names, 'u')

    def set_parameters(self, *names):
        return self._declare('parameter_names', names[0] if len(names) == 1 and not isinstance(names[0], str) else names, 'p')

    def set_measurements(self, *names):
        """dynamic_model.py `set_measurements`: names of the measurements (their equations follow with
        `set_measurement_equations`)."""
        if not self._symbolic:
            raise RuntimeError(f"'{self.name}' is a model of the device zoo; its variables are fixed")
        names = names[0] if len(names) == 1 and not isinstance(names[0], str) else names
        names = [names] if isinstance(names, str) else list(names)
        if len(set(names)) != len(names):
            raise ValueError(f"duplicate names in {names}")
        self._declared_measurements = names
        return SymVector('y', names)

    def set_algebraic_states(self, *names):
        """dynamic_model.py `set_algebraic_states`: the z of a semi-explicit DAE  dx/dt = f(x, z, u, p),  0 = g(x, z, u, p)."""
        return self._declare('algebraic_state_names', names[0] if len(names) == 1 and not isinstance(names[0], str) else names, 'z')

    def set_algebraic_equations(self, equations):
        """dynamic_model.py `set_algebraic_equations`: one residual per algebraic state (index 1: dg/dz regular)."""
        if not self._symbolic:
            raise RuntimeError(f"'{self.name}' is a model of the device zoo; its equations are fixed")
        eqs = self._parse(equations)
        if len(eqs) != self.n_z:
            raise ValueError(f"the model has {self.n_z} algebraic states but {len(eqs)} algebraic equations were supplied")
        self._alg = eqs

    def _parse(self, eqs):
        """Expressions, or strings of the model's variable names with the functions of the reference's table (the right-hand side of
        an optional `... = ` is taken, like the reference's equation strings, util/parsing.py)."""
        from .parsing import FUNCTIONS
        ns = dict(FUNCTIONS)                        # the reference's function table (util/parsing.py:36-58)
        ns['dt'] = Expr('dt', name='dt')            # the sampling interval inside the equations of a discrete model
        ns['t'] = Expr('t', name='t')               # the time: a time-variant model (is_time_variant)
        for vec in (self.x, self.u, self.p, self.z):
            ns.update({n: vec[n] for n in vec._names})
        out = []
        for e in ([eqs] if isinstance(eqs, (Expr, str, int, float)) else list(eqs)):
            if isinstance(e, str):
                e = eval(e.split('=')[-1].replace('^', '**'), {'__builtins__': {}}, dict(ns))
            out.append(Expr.wrap(e))
        return out

    def set_dynamical_equations(self, equations):
        """dynamic_model.py:1293-1405: one right-hand side per state (dx/dt for a continuous model, x+ for a discrete one)."""
        if not self._symbolic:
            raise RuntimeError(f"'{self.name}' is a model of the device zoo; its equations are fixed")
        eqs = self._parse(equations)
        if len(eqs) != self.n_x:
            raise ValueError(f"the model has {self.n_x} dynamical states but {len(eqs)} equations were supplied")
        self._ode = eqs
        self._linear = self._check_linearity()

    def set_measurement_equations(self, equations):
        """dynamic_model.py:1407-1460; the measurements carry the names given to `set_measurements`, y_0, y_1, ... otherwise (the
        reference's defaults)."""
        if not self._symbolic:
            raise RuntimeError(f"'{self.name}' is a model of the device zoo; its equations are fixed")
        self._meas = self._parse(equations)
        named = getattr(self, '_declared_measurements', None)
        self.measurement_names = list(named) if named and len(named) == len(self._meas) else [f'y_{i}' for i in range(len(self._meas))]
        self.n_y = len(self._meas)
        self._linear = self._check_linearity()

    def set_equations(self, equations=None, ode=None, meas=None, alg=None, **kwargs):
        """dynamic_model.py:1508-1553: `equations` as text (one string with line breaks, or a list of lines; grammar in
        hilo_mpc_amd/parsing.py) declares states, measurements, algebraic states, inputs and parameters by the way they appear;
        or the equation groups separately (`ode=`, `alg=`, `meas=`)."""
        if equations is not None:
            if not self._symbolic:
                raise RuntimeError(f"'{self.name}' is a model of the device zoo; its equations are fixed")
            if not (isinstance(equations, str) or (isinstance(equations, (list, tuple)) and all(isinstance(q, str) for q in equations))):
                raise TypeError("equations must be a string or a list of strings")
            from .parsing import parse_dynamic_equations
            pm = parse_dynamic_equations(equations, discrete=self._native_discrete, x=self.dynamical_state_names,
                                         y=self.measurement_names if self._meas else (), z=self.algebraic_state_names,
                                         u=self.input_names, p=self.parameter_names)
            if any(e is None for e in pm.ode):
                missing = [n for n, e in zip(pm.x, pm.ode) if e is None]
                raise ValueError(f"no dynamical equation for the state(s) {missing}")
            self.dynamical_state_names, self.input_names, self.parameter_names = pm.x, pm.u, pm.p
            self.algebraic_state_names = pm.z
            self.n_x, self.n_u, self.n_p, self.n_z = len(pm.x), len(pm.u), len(pm.p), len(pm.z)
            if len(pm.alg) != len(pm.z):
                raise ValueError(f"the model has {len(pm.z)} algebraic states but {len(pm.alg)} algebraic equations were supplied")
            self._ode, self._alg = pm.ode, pm.alg
            self._meas, self.measurement_names, self.n_y = pm.meas, list(pm.y), len(pm.meas)
            self._equation_notes = pm.notes
            self._is_setup = False
            self._linear = self._check_linearity()
            return
        if ode is not None:
            self.set_dynamical_equations(ode)
        if alg is not None:
            self.set_algebraic_equations(alg)
        if meas is not None:
            self.set_measurement_equations(meas)

    def _check_linearity(self):
        """dynamic_model.py `_check_linearity`: the right-hand sides are linear in (x, z, u) when no entry of their Jacobian depends
        on these variables (parameters may appear in the matrices)."""
        if not self._symbolic or self._ode is None:
            return self._linear
        from .expr import jacobian
        rows = list(self._ode) + list(self._alg) + list(self._meas)
        w = list(self.x) + list(self.z) + list(self.u)
        try:
            J = jacobian(rows, w)
        except NotImplementedError:
            return False
        return not any(n.op in ('x', 'z', 'u') for r in J for e in r for n in e.nodes().values())

    def is_time_variant(self):
        """dynamic_model.py:2480-2486: an equation names the time t explicitly.  Such a model is simulated as a plant (`step`,
        `rollout`, `simulate`, the plant of a `SimpleControlLoop`); controllers, estimators and the linearisations refuse it."""
        if not self._symbolic or self._ode is None:
            return False
        return any(e.depends_on('t') for e in list(self._ode) + list(self._meas) + list(self._alg))

    def is_autonomous(self):
        """dynamic_model.py:2458-2463: the model has no inputs (the reference's meaning of the word; time dependence is
        `is_time_variant`)."""
        return self.n_u == 0

    def _refuse_time_variant(self, who, instead="simulate it as a plant (Model.step, rollout, simulate, the plant of a SimpleControlLoop)"):
        if self.is_time_variant():
            raise NotImplementedError(f"model '{self.name}' depends on time explicitly; {who} takes autonomous models only: write the "
                                      f"time dependence as an input or a time-varying parameter of the {who} model, or {instead}")

    def user_source(self, z_guess=None, alg_at_slope=False):
        """HIP source that defines `UserModel` for the run-time compiled path: the emitted functor, or the alias of the
        zoo functor.  z_guess: start of the Newton iteration on the algebraic equations of a DAE (`set_initial_guess(z_guess=)`)."""
        from . import codegen
        if getattr(self, '_linearized', False):
            # linearize() keeps the nonlinear equations and only marks the copy (the matrices come from system_matrices()); kernels
            # compiled from it would run the NONLINEAR dynamics in absolute coordinates (the reference rewrites the equations in
            # deviation variables, dynamic_model.py:2488-2612)
            raise NotImplementedError("a linearised model (Model.linearize) is offloaded for the linear MPC and system_matrices() only; "
                                      "filters, NMPC and simulation need the model itself")
        if self._symbolic:
            if self._ode is None:
                raise RuntimeError("Model is not set up: no dynamical equations (set_dynamical_equations)")
            for e in self._ode + self._meas + self._alg:
                if e.depends_on('theta'):
                    raise ValueError("a path variable cannot appear in the model equations")
            if any(e.depends_on('dt') for e in self._ode + self._meas + self._alg):
                # the sampling interval written into the equations of a discrete model (`25*dt*x/(1 + x^2)`): a number once the
                # model is set up
                if self.dt is None:
                    raise RuntimeError("Model is not set up: the equations use the sampling interval dt (Model.setup(dt=...))")
                dtc = Expr.wrap(float(self.dt))
                n1, n2 = len(self._ode), len(self._ode) + len(self._meas)
                sub = Expr.substitute(self._ode + self._meas + self._alg, lambda n: dtc if n.op == 'dt' else None)
                m = copy.copy(self)
                m._ode, m._meas, m._alg = sub[:n1], sub[n1:n2], sub[n2:]
                return m.user_source(z_guess, alg_at_slope)
            if self.n_z and len(self._alg) != self.n_z:
                raise RuntimeError("Model is not set up: algebraic states without algebraic equations (set_algebraic_equations)")
            if self.n_z:
                if self._native_discrete:
                    raise NotImplementedError("algebraic states of a discrete model are not built")
                # a network inside a model with algebraic states: the symbolic source and the LQR_CHUNK hint of the branch below are
                # not passed on - `linearization` / LQR differentiate such a model in one pass
                return codegen.dae_model_source(self.n_x, self.n_u, self.n_p, self.n_z, self._ode, self._alg, self._meas,
                                                z_guess if z_guess is not None else [0.] * self.n_z, alg_at_slope=alg_at_slope)
            helpers = [src for _, src in sorted(getattr(self, '_gp_helpers', {}).items())]
            ann_nodes = sum(a.n_nodes() for a in getattr(self, '_anns', None) or [])
            return codegen.model_source(self.n_x, self.n_u, self.n_p, self._ode, self._meas, self._native_discrete, helpers=helpers,
                                        symbolic=ann_nodes <= self.ANN_SYM_NODES, lqr_chunk=self.ANN_LQR_CHUNK if ann_nodes else None)
        if self.name == 'lti':
            return codegen.zoo_alias(f"Lti<{self.n_x}, {self.n_u}, {self.n_y}>")
        if self.name not in ZOO_FUNCTOR:
            raise NotImplementedError(f"model '{self.name}' cannot be used in a run-time compiled problem")
        return codegen.zoo_alias(ZOO_FUNCTOR[self.name])

    def is_linear(self):
        """dynamic_model.py `is_linear`: a model of the zoo by its table; a model written as expressions when it was linearised or
        when the Jacobian of its equations with respect to states and inputs holds neither."""
        if not self._symbolic:
            return self._linear
        if getattr(self, '_linearized', False):
            return True
        if self._ode is None or self.n_z:
            return False
        from .expr import jacobian
        try:
            J = jacobian(list(self._ode) + list(self._meas), list(self.x) + list(self.u))
        except NotImplementedError:          # a node without a derivative rule (a learned term, ...): not known to be linear
            return False
        return not any(e.depends_on('x') or e.depends_on('u') for row in J for e in row)

    # ---- linearisation (dynamic_model.py:2488-2612, :3670-3684) and the matrices the linear MPC reads (mpc.py:2183-2184) -----------
    def linearize(self, name=None, trajectory=None):
        """The model linearised about its equilibrium point (`set_equilibrium_point`, default: the origin): a copy that reports
        `is_linear()` and hands out `state_matrix`, `input_matrix`, `output_matrix` - the Jacobians of the equations (of the
        explicit Runge-Kutta step when the model was discretised first, like in tests/test_LMPC.py:82-85) with respect to states
        and inputs, in deviation variables."""
        if not self._symbolic:
            if self._linear:
                print("Model is already linear. Linearization is not necessary. Nothing to be done.")
                return self
            raise NotImplementedError("the models of the device zoo carry no expressions to linearise")
        self._refuse_time_variant('linearize')
        if trajectory is not None:
            raise NotImplementedError("linearisation along a trajectory is not built")
        if self._ode is None:
            print("Model is empty. Nothing to be done.")
            return self
        if getattr(self, '_linearized', False):
            print("Model is already linearized. Nothing to be done.")
            return self
        if self.is_linear():
            print("Model is already linear. Linearization is not necessary. Nothing to be done.")
            return self
        if self.n_z:
            raise NotImplementedError("linearisation of a model with algebraic states is not built")
        m = self.copy()
        if name is not None:
            m.name = name
        m._linearized = True
        m._x_eq = m._u_eq = None
        return m

    def set_equilibrium_point(self, x_eq=None, u_eq=None, z_eq=None):
        """dynamic_model.py `set_equilibrium_point`: where the Jacobians of a linearised model are taken."""
        def chk(v, n, what):
            if v is None:
                return None
            v = np.asarray(v, dtype=float).ravel()
            if v.size != n:
                raise ValueError(f"Dimension mismatch: the equilibrium point of the {what} has {v.size} entries, the model {n}")
            return v
        self._x_eq, self._u_eq = chk(x_eq, self.n_x, 'states'), chk(u_eq, self.n_u, 'inputs')

    def set_initial_parameter_values(self, p=None):
        """dynamic_model.py `set_initial_parameter_values` (here: the values the system matrices are evaluated with when none
        are handed over)."""
        p = np.asarray([] if p is None else p, dtype=float).ravel()
        if p.size != self.n_p:
            raise ValueError(f"Dimension mismatch: {p.size} parameter values for {self.n_p} parameters")
        self._p_init = p

    def _jacobian_program(self):
        """(dag, nodes of d rows / d (x, u), number of rows): rows = x+ (or dx/dt) and the measurement equations."""
        from .smpc import SMPC
        from .symdiff import Dag
        fx = SMPC._discrete_map(self, self.dt) if self.discrete else list(self._ode)
        rows = list(fx) + list(self._meas)
        if any(e.depends_on('t') for e in rows):
            raise NotImplementedError(f"model '{self.name}' depends on time explicitly; system matrices are those of autonomous models: "
                                      f"write the time dependence as an input or a parameter, or simulate the model as a plant")
        if any(e.depends_on('dt') for e in rows):      # the sampling interval written into the equations (tests/test_LMPC.py:12-13)
            if self.dt is None:
                raise RuntimeError("Model is not set up. Run Model.setup(dt=...) first: the equations hold the sampling interval.")
            rows = Expr.substitute(rows, lambda n: Expr.wrap(float(self.dt)) if n.op == 'dt' else None)
        g, memo = Dag(), {}
        rows = [g.from_expr(e, memo) for e in rows]
        w = [g.var('x', i) for i in range(self.n_x)] + [g.var('u', i) for i in range(self.n_u)]
        jac = [g.diff(r, v) for r in rows for v in w]
        return g, jac, len(rows)

    def system_matrices(self, p=None):
        """(A, B, C) of a linear (or linearised) model: numeric Jacobians of x+ = f(x, u, p) (a discrete or discretised model) or
        dx/dt = f (a continuous one that was not discretised) and of y = h(x, u, p) at the equilibrium point."""
        if not self._symbolic:
            if self.name == 'lti':
                return self.A, self.B, self.C
            raise NotImplementedError("the models of the device zoo carry no expressions to differentiate")
        if not self.is_linear():
            raise RuntimeError("The model is nonlinear: linearize it first (Model.linearize)")
        if self.discrete and not self._native_discrete and self.dt is None:
            raise RuntimeError("Model is not set up. Run Model.setup(dt=...) before asking for the matrices of a discretised model.")
        if self.n_p:
            p = getattr(self, '_p_init', None) if p is None else np.asarray(p, dtype=float).ravel()
            if p is None or p.size != self.n_p:
                raise ValueError(f"The model has {self.n_p} parameter(s): {self.parameter_names}. Their values are needed for "
                                 f"the system matrices (argument `p` / set_initial_parameter_values).")
        else:
            p = np.zeros(0)
        # the Jacobian as a straight-line program, built once per (equations, discretisation, sampling interval) and evaluated per
        # call (the linear MPC asks for one pair of matrices per stage when parameters vary along the horizon)
        # (the equation lists themselves are kept in the cache entry: an id is only unique among live objects)
        stamp = (id(self._ode), id(self._meas), self.erk_order, self.n_sub, self.dt, self.discrete)
        cache = getattr(self, '_sysmat_cache', None)
        if cache is None or cache[0] != stamp or cache[4] is not self._ode or cache[5] is not self._meas:
            g, jac, n_rows = self._jacobian_program()
            self._sysmat_cache = cache = (stamp, g, jac, n_rows, self._ode, self._meas)
        _, g, jac, n_rows = cache[:4]
        xe = getattr(self, '_x_eq', None)
        ue = getattr(self, '_u_eq', None)
        xe = np.zeros(self.n_x) if xe is None else xe
        ue = np.zeros(self.n_u) if ue is None else ue
        J = np.array(g.evaluate(jac, xe, ue, p), dtype=float).reshape(n_rows, self.n_x + self.n_u)
        nx = self.n_x
        C = J[nx:, :nx] if len(self._meas) else np.eye(nx)
        return J[:nx, :nx], J[:nx, nx:], C

    state_matrix = property(lambda s: s.system_matrices()[0])
    input_matrix = property(lambda s: s.system_matrices()[1])
    output_matrix = property(lambda s: s.system_matrices()[2])

    def _linearization_handle(self, device_index=None):
        """The filter handle whose map `linearization` and the LQR differentiate on the device.  A linearised copy (`linearize`)
        carries the nonlinear equations and a mark; its handle is built from a private copy without the mark (`user_source` keeps
        refusing the marked one: filters, NMPC and simulation need the model itself).  A model without measurement equations
        gets y = x in that private copy (`system_matrices` hands out C = I for it)."""
        stamp = (self.dt, self.erk_order, self.n_sub, id(self._ode) if self._symbolic else None, id(self._meas) if self._symbolic else None)
        h = getattr(self, '_lin_plant', None)
        if h is None or h._model_stamp != stamp:
            from .estimator import ExtendedKalmanFilter
            pm = self
            if self._symbolic and (getattr(self, '_linearized', False) or not self._meas):
                pm = copy.copy(self)
                pm._linearized = False
                if not pm._meas:
                    pm._meas, pm.n_y = list(pm.x), pm.n_x
                    pm.measurement_names = [f'y_{i}' for i in range(pm.n_x)]
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')          # ("the supplied model is linear": the filter is only the handle's carrier)
                h = ExtendedKalmanFilter(pm, device_index=device_index)
            h.setup()
            h._model_stamp = stamp
            self._lin_plant = h
        return h

    def linearization(self, x=None, u=None, p=None, device_index=None):
        """(A, B, C) = (dPhi/dx, dPhi/du, dh/dx) of the discrete-time map x+ = Phi(x, u, p) - the map of `step`, `rollout` and the
        extended Kalman filter - for a batch of operating points, on the device in forward mode (`hilo_model_linearize`): the
        device sibling of `system_matrices`.  x [n_x] or [B, n_x] (default: the equilibrium point, else the origin), u and p
        likewise (p default: `set_initial_parameter_values`); a leading axis of 1 is shared by the batch.  Returns [B, n_x, n_x],
        [B, n_x, n_u], [B, n_y, n_x] (without the batch axis when no argument had one) - device tensors for device tensors, numpy
        otherwise.  A continuous model has to be discretised first."""
        import torch
        from . import _lib
        from ._device import ptr, stream_ptr, to_dev
        self._refuse_time_variant('linearization')
        if not self._is_setup:
            raise RuntimeError("Model is not set up. Run Model.setup() before asking for its linearisation.")
        if not self.discrete:
            raise NotImplementedError("the Jacobians are those of the discrete-time map: discretize the model first (Model.discretize)")
        if getattr(self, 'n_z', 0):
            raise NotImplementedError("linearisation of a model with algebraic states is not built")
        if self.n_u == 0:
            raise RuntimeError("The model is autonomous: there is no input matrix.")
        h = self._linearization_handle(device_index)
        dev = h._dev
        tensors = any(isinstance(v, torch.Tensor) for v in (x, u, p))
        x = getattr(self, '_x_eq', None) if x is None else x
        u = getattr(self, '_u_eq', None) if u is None else u
        x = np.zeros(self.n_x) if x is None else x
        u = np.zeros(self.n_u) if u is None else u
        if self.name == 'lti':
            p = self.lti_parameters()
        elif h._n_p:
            p = getattr(self, '_p_init', None) if p is None else p
            if p is None:
                raise ValueError(f"The model has {self.n_p} parameter(s): {self.parameter_names}. Their values are needed for "
                                 f"the system matrices (argument `p` / set_initial_parameter_values).")
        rows, batched = [], False
        for v, n, what in ((x, self.n_x, 'states'), (u, self.n_u, 'inputs'), (p, h._n_p, 'parameters')):
            if n == 0:
                rows.append(None)
                continue
            t = to_dev(v, dev)
            if t.dim() > 2 or (t.dim() == 2 and t.shape[1] != n) or (t.dim() <= 1 and t.numel() != n):
                raise ValueError(f"{what}: expected [{n}] or [B, {n}], got {list(t.shape)}")
            batched = batched or t.dim() == 2
            rows.append(t.reshape(-1, n))
        B = max(t.shape[0] for t in rows if t is not None)
        for t, what in zip(rows, ('states', 'inputs', 'parameters')):
            if t is not None and t.shape[0] not in (1, B):
                raise ValueError(f"{what}: batch {t.shape[0]} does not match {B}")
        xt = rows[0].expand(B, -1).contiguous()
        up = torch.cat([t.expand(B, -1) for t in rows[1:] if t is not None], dim=1).contiguous()
        ny = h._n_y
        A = torch.empty(B, self.n_x, self.n_x, dtype=torch.float64, device=dev)
        Bm = torch.empty(B, self.n_x, self.n_u, dtype=torch.float64, device=dev)
        Cm = torch.empty(B, ny, self.n_x, dtype=torch.float64, device=dev)
        _lib.check(_lib.lib().hilo_model_linearize(h._handle, B, ptr(xt), ptr(up), up.shape[1], ptr(A), ptr(Bm), ptr(Cm), stream_ptr(dev)))
        out = (A, Bm, Cm) if batched else (A[0], Bm[0], Cm[0])
        return out if tensors else tuple(t.cpu().numpy() for t in out)

    def lti_parameters(self):
        return np.concatenate([self.A.ravel(), self.B.ravel(), self.C.ravel()])

    def discretize(self, method='rk4', order=None, inplace=False, n_sub=1):
        """`Model.discretize` (dynamic_model.py:2113-2456): 'rk4' = classic order 4, 'erk' with order 1..4
        (modeling.py:1239-1250)."""
        if method == 'rk4':
            order = 4
        elif method == 'erk':
            order = 1 if order is None else order
        else:
            raise ValueError(f"discretisation method '{method}' is not available on the device "
                             f"(explicit Runge-Kutta 'erk'/'rk4' only)")
        if order not in (1, 2, 3, 4):
            raise NotImplementedError(f"Explicit Runge-Kutta discretization for order {order} is not yet "
                                      f"implemented.")
        m = self if inplace else copy.copy(self)
        if not m._native_discrete:
            m.erk_order = order
            m.n_sub = n_sub
            m._solver = m._solver_options = None      # a map needs no integrator
        return m

    def setup(self, dt=None, solver=None, solver_options=None):
        """dynamic_model.py `setup`: fixes the sampling interval (default 1).

        solver: None keeps the fixed-step maps (a continuous model that was not discretised is simulated with eight classic
        Runge-Kutta steps per interval, no error control).  'dopri5' integrates a continuous model with the Dormand-Prince 5(4)
        pair under step-size control (csrc/hilo_integrate.h) wherever the model is simulated - `step`, `rollout`, `simulate`, the
        plant of a `SimpleControlLoop` - where the reference integrates with CVODES.  'bdf' integrates it with variable-order
        (1..5) backward differentiation formulas, a Newton iteration on the exact Jacobian and step size and order chosen per
        instance (scipy's `BDF` restated on the device): the method for a stiff model, on which the explicit pair is bound by
        stability and takes thousands of steps per interval or ends with 'max_num_steps reached'.  With inputs held over a
        `rollout` the integrator's state is carried across the sampling instants (their states are interpolated, only the end
        clips a step); with an input sequence every interval starts afresh.  Models of up to 8 states.
        'idas' is the same method for a model WITH algebraic states, dx/dt = f(x, z, u, p), 0 = g(x, z, u, p), where the reference
        integrates with IDAS: the formulas are applied to the combined vector [x; z] (the algebraic equations are rows of the Newton
        system, not a nested iteration per evaluation; the error test sees z as well), z is made consistent at the start and
        whenever the inputs jump, and `rollout(..., return_z=True)` / `solution['z']` give the algebraic states at the sampling
        instants.  Models of up to 8 differential and algebraic states together.
        solver_options, under CasADi's names (defaults: CasADi's for CVODES): reltol 1e-6, abstol 1e-8, max_num_steps 10000
        (attempted steps per sampling interval), first_step 0 (estimated)."""
        if self._symbolic and self._ode is None:
            raise RuntimeError("Model is not set up: no dynamical equations (set_dynamical_equations)")
        if getattr(self, 'n_z', 0) and self.is_time_variant():
            raise NotImplementedError(f"model '{self.name}' has algebraic states and depends on time explicitly: time-variant models are "
                                      f"ordinary differential (or difference) equations; eliminate the algebraic states or write the "
                                      f"time dependence as an input")
        if solver is None and solver_options is not None:
            raise ValueError("solver_options without a solver")
        if solver is not None:
            # dynamic_model.py `check_solver` (:1958-1993); what the reference warns about and then fails on is an error here
            if not isinstance(solver, str):
                raise TypeError("Solver type must be a string")
            if self.discrete:
                raise RuntimeError("Model is discrete. No solver is required.")
            if solver not in SOLVERS:
                raise ValueError(f"Solver '{solver}' is not available on your system. Use 'dopri5' instead, or 'bdf' for a stiff model")
            if solver == 'idas':
                if not getattr(self, 'n_z', 0):
                    raise RuntimeError(f"Solver 'idas' integrates a model with algebraic states; model '{self.name}' has none. Use "
                                       f"'bdf' for a stiff model, or 'dopri5'")
                if self.n_x + self.n_z > IDAS_MAX_STATES:
                    raise NotImplementedError(f"Solver 'idas' is built for at most {IDAS_MAX_STATES} differential and algebraic states "
                                              f"together; model '{self.name}' has {self.n_x} + {self.n_z}")
            elif getattr(self, 'n_z', 0):
                raise RuntimeError(f"Solver '{solver}' is not suitable for DAE systems. Use 'idas' or 'collocation' instead")
            opts = dict(SOLVER_OPTIONS)
            for k, v in (solver_options or {}).items():
                if k not in SOLVER_OPTIONS:
                    raise ValueError(f"Unknown option '{k}' for solver '{solver}'. Available options: {sorted(SOLVER_OPTIONS)}")
                opts[k] = type(SOLVER_OPTIONS[k])(v)
            if not (opts['reltol'] > 0. and opts['abstol'] > 0.):
                raise ValueError("reltol and abstol must be positive")
            if opts['max_num_steps'] < 1 or opts['first_step'] < 0.:
                raise ValueError("max_num_steps must be at least 1 and first_step non-negative")
            self._solver, self._solver_options = solver, opts
        if dt is not None:
            self.dt = float(dt)
        if self.dt is None:
            self.dt = 1.
        self._is_setup = True
        return self

    def substitute_from(self, obj):
        """`Model.substitute_from(gp)` (dynamic_model.py:3040-3125): the quantity named by `gp.labels` is replaced
        by the GP's posterior mean `gp.predict(features)[0]`, the features being looked up by name among the model's
        variables (:3056-3061).  The device zoo offers this for the growth rate `mu` of 'chemostat4' over the
        features (S, I) (`nmpc_hybrid_bio.ipynb`); the GP must be trained (`setup` + `fit_model` or `set_training_data`
        + `setup`) with a squared-exponential kernel and a constant/zero mean."""
        from .gp import GPArray
        if isinstance(obj, GPArray):                     # like the list of its members
            obj = list(obj._members())
        if isinstance(obj, (list, tuple, set)):
            for o in obj:
                self.substitute_from(o)
            return self
        from .ann import ArtificialNeuralNetwork
        if self._symbolic:
            if isinstance(obj, ArtificialNeuralNetwork):
                return self._substitute_ann(obj)
            return self._substitute_symbolic(obj)
        if isinstance(obj, ArtificialNeuralNetwork):
            raise NotImplementedError(f"model '{self.name}' is a model of the device zoo: a neural network is substituted into models "
                                      f"written as expressions (Model.set_dynamical_equations)")
        if self.name not in LEARNABLE:
            raise NotImplementedError(f"model '{self.name}' has no learnable term in the device zoo "
                                      f"(available: {sorted(LEARNABLE)})")
        label, features, hybrid = LEARNABLE[self.name]
        if list(getattr(obj, 'labels', [])) != [label] or list(getattr(obj, 'features', [])) != features:
            raise ValueError(f"model '{self.name}' takes a learned model with labels ['{label}'] and features "
                             f"{features}; got labels {getattr(obj, 'labels', None)}, features "
                             f"{getattr(obj, 'features', None)}")
        if getattr(obj, '_handle', None) is None:
            raise RuntimeError("The GP has not been set up (trained) yet. Run GaussianProcess.setup() first.")
        m = self
        m.name = hybrid
        m.model_id = ZOO[hybrid][0]
        m.learned = obj
        return m

    def _substitute_symbolic(self, gp):
        """The general case for a model written as expressions: the label must be a parameter (the reference only handles
        parameters either, dynamic_model.py:3000-3004 `self._p.remove`), which leaves the parameter vector; the features are
        states, inputs or remaining parameters, looked up by name (:3056-3061).  In the compiled right-hand side the
        parameter becomes `gp_se_mean(<packed GP>, features)` (csrc/hilo_models.h), differentiated like any other
        operation by the scalar type it is evaluated with."""
        labels, features = list(getattr(gp, 'labels', [])), list(getattr(gp, 'features', []))
        if len(labels) != 1 or not callable(getattr(gp, 'predict', None)):
            raise ValueError("substitute_from takes a learned model with exactly one label")
        if getattr(gp, '_handle', None) is None:
            raise RuntimeError("The GP has not been set up (trained) yet. Run GaussianProcess.setup() first.")
        if self._ode is None:
            raise RuntimeError("set the model equations before substituting a learned term")
        if labels[0] not in self.parameter_names:
            raise ValueError(f"label '{labels[0]}' is not a parameter of model '{self.name}' (parameters: "
                             f"{self.parameter_names})")
        if len(self._gps) >= 4:
            raise NotImplementedError("at most 4 learned terms per model")
        ip = self.parameter_names.index(labels[0])
        keep = [n for n in self.parameter_names if n != labels[0]]
        newp = SymVector('p', keep)
        feats = []
        for f in features:
            if f == labels[0]:
                raise ValueError(f"feature '{f}' is the label itself")
            for vec in (self.x, self.u, newp):
                if f in vec._names:
                    feats.append(vec[f])
                    break
            else:
                raise ValueError(f"feature '{f}' is not a state, input or parameter of model '{self.name}'")
        # the plain squared-exponential kernel has a device function of its own (gp_se_mean, also the variance and the mean's
        # Jacobian of the stochastic NMPC); any other stationary kernel / sum / product is compiled into the model source
        from .gp import is_plain_se, kernel_expr
        from . import codegen
        kern = getattr(gp, 'kernel', None)       # (an object without one is taken to the device function: the library checks its kernel)
        kprog = list(kern.program(len(features))) if kern is not None else None
        k = len(self._gps)
        if kprog is None or is_plain_se(kprog):
            node = Expr('gp', feats, value=k, name=labels[0])
        else:
            if len(features) > 8:
                raise NotImplementedError("a learned term inside a model takes at most 8 features")
            fe = [Expr('x', value=q, name=f"f{q}") for q in range(len(features))]
            te = [Expr('p', value=q, name=f"t{q}") for q in range(len(features))]
            if not hasattr(self, '_gp_helpers') or self._gp_helpers is None:
                self._gp_helpers = {}
            self._gp_helpers = dict(self._gp_helpers)
            self._gp_helpers[k] = codegen.gp_helper_source(k, len(features), kernel_expr(kprog, fe, te))
            node = Expr('gpk', feats, value=k, name=labels[0])

        def leaf(n):
            if n.op != 'p':
                return None
            i = int(n.value)
            return node if i == ip else (newp[i - 1] if i > ip else None)

        # every equation list that can hold a parameter leaf is re-indexed together (the algebraic equations too)
        alg = list(getattr(self, '_alg', None) or [])
        neq, nalg = len(self._ode), len(alg)
        out = Expr.substitute(self._ode + alg + self._meas, leaf)
        self._ode, self._meas = out[:neq], out[neq + nalg:]
        if nalg:
            self._alg = out[neq:neq + nalg]
        self.parameter_names, self.n_p = keep, len(keep)
        self._gps.append(gp)
        self._is_setup = False
        return self

    # Size limits of a network written into a model as expressions, in neurons (hidden nodes + labels; DESIGN.md 5.3b has the
    # compile measurements behind them): above ANN_SYM_NODES the symbolic first / second derivative source is left out and the
    # engine keeps its Taylor sweeps (as for GP terms); above ANN_MAX_NODES the substitution is refused.  Both count the neurons of
    # all networks of the model together, as `user_source` emits them together.
    ANN_SYM_NODES = 24
    ANN_LQR_CHUNK = 3           # forward-mode directions per pass of `linearization` / LQR on a model that carries a network
    ANN_MAX_NODES = 56

    def _substitute_ann(self, ann):
        """A neural network as a learned term (dynamic_model.py:3040-3125 with util/machine_learning.py:521-578
        `net_to_casadi_graph`): every label must be a parameter, all of them leave the parameter vector; the features are states,
        inputs or remaining parameters, looked up by name.  The network becomes part of the expressions - weights as numbers,
        hidden activations shared between the labels - so the model stays an ordinary expression model for every consumer."""
        labels, features = list(ann.labels), list(ann.features)
        if not ann.is_trained():
            raise RuntimeError("The ANN has not been trained yet. Hand the weights over with load_torch() or set_weights().")
        if self._ode is None:
            raise RuntimeError("set the model equations before substituting a learned term")
        if len(set(labels)) != len(labels):
            raise ValueError(f"duplicate labels in {labels}")
        for lb in labels:
            if lb not in self.parameter_names:
                raise ValueError(f"label '{lb}' is not a parameter of model '{self.name}' (parameters: "
                                 f"{self.parameter_names})")
        have = sum(a.n_nodes() for a in getattr(self, '_anns', None) or [])
        if have + ann.n_nodes() > self.ANN_MAX_NODES:
            raise NotImplementedError(f"a network of {ann.n_nodes()} neurons (hidden nodes + labels) inside a model" +
                                      (f" that already holds {have}" if have else "") +
                                      f": at most {self.ANN_MAX_NODES} are compiled into the model's right-hand side")
        keep = [n for n in self.parameter_names if n not in labels]
        newp = SymVector('p', keep)
        feats = []
        for f in features:
            if f in labels:
                raise ValueError(f"feature '{f}' is the label itself")
            for vec in (self.x, self.u, newp):
                if f in vec._names:
                    feats.append(vec[f])
                    break
            else:
                raise ValueError(f"feature '{f}' is not a state, input or parameter of model '{self.name}'")
        out_exprs = ann.expressions(feats)
        old = list(self.parameter_names)
        repl = {old.index(lb): e for lb, e in zip(labels, out_exprs)}
        newidx = {old.index(n): newp[q] for q, n in enumerate(keep)}

        def leaf(n):
            if n.op != 'p':
                return None
            i = int(n.value)
            if i in repl:
                return repl[i]
            return newidx[i] if int(newidx[i].value) != i else None

        # every equation list that can hold a parameter leaf is re-indexed together (the algebraic equations too).  The network's
        # nodes are younger than the user's statements; Expr.substitute rebuilds in creation order, so they must be passed through
        # as they are: the rebuilt equations only refer to them.
        alg = list(getattr(self, '_alg', None) or [])
        neq, nalg = len(self._ode), len(alg)
        out = Expr.substitute(self._ode + alg + self._meas, leaf)
        self._ode, self._meas = out[:neq], out[neq + nalg:]
        if nalg:
            self._alg = out[neq:neq + nalg]
        self.parameter_names, self.n_p = keep, len(keep)
        self._anns = list(getattr(self, '_anns', None) or []) + [ann]
        self._is_setup = False
        self._linear = self._check_linearity()
        return self

    def copy(self, setup=True):
        m = copy.copy(self)
        m._sim = None              # the copy simulates its own trajectory
        m._rollout_up = None       # ... with its own buffer for the packed inputs and parameters
        m._lin_plant = None        # ... and its own handle for `linearization`
        if hasattr(self, '_gps'):
            m._gps = list(self._gps)    # learned terms substituted into the copy later must not appear in the original
        if getattr(self, '_gp_helpers', None):
            m._gp_helpers = dict(self._gp_helpers)
        if getattr(self, '_anns', None):
            m._anns = list(self._anns)
        return m

    # ---- the model as a PLANT: one sampling interval for a batch of states (dynamic_model.py:3360-3400, :3911-4000) -----------------
    def _plant_handle(self, device_index=None):
        """A filter handle of the library carries exactly what a plant step needs - the model functor (zoo, or compiled from the
        expressions), the sampling interval and the discretisation - and `hilo_pf_function` with one particle per instance and
        zero noise IS that step: x+ = Phi(x, u, p), y = h(x+, u, p) (a continuous model is integrated with eight classic
        Runge-Kutta steps per interval and no error control; `setup(solver='dopri5')` integrates it with step-size control like the
        reference's CVODES, through `hilo_model_rollout` on the same handle)."""
        h = getattr(self, '_plant', None)
        if h is None or h._model_stamp != (self.dt, self.erk_order, self.n_sub, id(self._ode) if self._symbolic else None):
            from .estimator import ExtendedKalmanFilter
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter('ignore')
                h = ExtendedKalmanFilter(self, device_index=device_index, _as_plant=True)
            h.setup()
            h._model_stamp = (self.dt, self.erk_order, self.n_sub, id(self._ode) if self._symbolic else None)
            self._plant = h
        return h

    def step(self, x, u=None, p=None, device_index=None, t0=0., sensitivities=None):
        """x [B, n_x] -> (x_next [B, n_x], y [B, n_y]) after one sampling interval, on the device (numpy in -> numpy out).
        t0: the time at which the interval starts, one value for the batch (read by a time-variant model only).
        sensitivities (under `setup(solver='dopri5')`; see `rollout`): a further output `sens` with the derivatives of x_next and y at
        the end of the interval, `sens['x']['p']` [B, n_x, n_p] and so on - row 1 of the one-interval roll-out."""
        import torch
        from . import _lib
        from ._device import ptr, stream_ptr, to_dev
        if not self._is_setup:
            raise RuntimeError("Model is not set up. Run Model.setup() before running simulations.")
        if sensitivities is not None:
            xs, ys, sens = self.rollout(x, u, p, steps=1, device_index=device_index, t0=t0, sensitivities=sensitivities)
            sens['x'] = {g: v[1] for g, v in sens['x'].items()}
            if 'y' in sens:
                sens['y'] = {g: v[0] for g, v in sens['y'].items()}
            return xs[1], ys[0], sens
        if self._solver is not None or self.is_time_variant():   # one sampling interval under error control / with the time
            xs, ys = self.rollout(x, u, p, steps=1, device_index=device_index, t0=t0)
            return xs[1], ys[0]
        h = self._plant_handle(device_index)
        dev = h._dev
        host = not isinstance(x, torch.Tensor)
        xt = to_dev(x, dev).reshape(-1, self.n_x).contiguous()
        B = xt.shape[0]
        parts = []
        for v, n, what in ((u, self.n_u, 'inputs'), (self.lti_parameters() if self.name == 'lti' else p, h._n_p, 'parameters')):
            if n:
                if v is None:
                    raise RuntimeError(f"The model has {n} {what}; pass them to step() / simulate().")
                t = to_dev(v, dev).reshape(-1, n)
                if t.shape[0] not in (1, B):
                    raise ValueError(f"{what}: batch {t.shape[0]} does not match {B} states")
                parts.append(t.expand(B, -1))
        up = torch.cat(parts, dim=1).contiguous() if parts else None
        ny = h._n_y
        zeros_x = torch.zeros(B, 1, self.n_x, dtype=torch.float64, device=dev)
        zeros_y = torch.zeros(B, 1, ny, dtype=torch.float64, device=dev)
        R = torch.eye(ny, dtype=torch.float64, device=dev)
        xn, y = torch.empty(B, 1, self.n_x, dtype=torch.float64, device=dev), torch.empty(B, 1, ny, dtype=torch.float64, device=dev)
        q = torch.empty(B, 1, dtype=torch.float64, device=dev)
        _lib.check(_lib.lib().hilo_pf_function(h._handle, B, 1, ptr(xt), ptr(zeros_y), ptr(up), (up.shape[1] if up is not None else 0),
                                               ptr(zeros_x), ptr(zeros_y), ptr(R), 0, ptr(xn), ptr(y), ptr(q), stream_ptr(dev)))
        xn, y = xn[:, 0], y[:, 0]
        return (xn.cpu().numpy(), y.cpu().numpy()) if host else (xn, y)

    def _sensitivity_groups(self, sensitivities, n_p, is_sequence):
        """The groups of `sensitivities=` in the order of the kernel's columns (x0, u, p) with their widths, after the refusals."""
        have = {'x0': self.n_x, 'u': self.n_u, 'p': n_p}
        if self._solver != 'dopri5':
            if self._solver is None:
                raise NotImplementedError("sensitivities are integrated next to the states by the explicit pair: the fixed-step maps "
                                          "carry none. Set the model up with Model.setup(solver='dopri5') (a discrete or discretised "
                                          "model: Model.linearization gives the Jacobians of its map)")
            raise NotImplementedError(f"sensitivities under solver '{self._solver}' are not implemented (its difference tables leave no "
                                      f"room for a second table per column). Use Model.setup(solver='dopri5'), or central differences "
                                      f"through Model.rollout for a stiff model")
        if sensitivities is True:
            groups = tuple(g for g in ('x0', 'u', 'p') if have[g])
        else:
            if isinstance(sensitivities, str):
                sensitivities = (sensitivities,)
            groups = tuple(sensitivities)
            for g in groups:
                if g not in have:
                    raise ValueError(f"sensitivities: unknown group '{g}'. Choose out of ('x0', 'u', 'p'), or pass True for every group "
                                     f"the model has")
                if not have[g]:
                    raise ValueError(f"sensitivities: the model has no {'inputs' if g == 'u' else 'parameters'}, so there is no group "
                                     f"'{g}'. Leave it out (True selects every group the model has)")
            groups = tuple(g for g in ('x0', 'u', 'p') if g in groups)
        if not groups:
            raise ValueError("sensitivities: no group selected. Pass True or a tuple out of ('x0', 'u', 'p')")
        if 'u' in groups and (is_sequence['inputs'] or is_sequence['parameters']):
            raise ValueError("sensitivities: with an input sequence every sampling interval's input is a parameter of its own, so there "
                             "is no one column per input. Select ('x0', 'p'), or hold the inputs (and parameters) over the roll-out "
                             "(u [B, n_u])")
        if 'p' in groups and is_sequence['parameters']:
            raise ValueError("sensitivities: with a parameter sequence every sampling interval's parameters are parameters of their own. "
                             "Select ('x0',), or hold the parameters over the roll-out (p [B, n_p])")
        if self.n_x > SENS_MAX_NX:
            raise NotImplementedError(f"sensitivities: the kernel keeps the pair's vectors twice as wide as the plain roll-out and is built "
                                      f"for up to {SENS_MAX_NX} states; the model has {self.n_x}. Use central differences through "
                                      f"Model.rollout")
        ns = sum(have[g] for g in groups)
        if ns > 64:
            raise NotImplementedError(f"sensitivities: {ns} columns; an instance's columns are spread over the lanes of one wave, at "
                                      f"most 64. Select fewer groups per call")
        return [(g, have[g]) for g in groups]

    def rollout(self, x0, u=None, p=None, steps=1, return_stats=False, device_index=None, t0=0., _h=None, z0=None, return_z=False,
                sensitivities=None):
        """The many-interval sibling of `step`: `steps` sampling intervals for a batch of states in ONE launch
        (`hilo_model_rollout`), with the model's own map or, after `setup(solver='dopri5')` or `'bdf'`, under error control.

        x0 [B, n_x]; u [B, n_u] held over the roll-out or [steps, B, n_u] one row per sampling interval, p likewise; a batch axis
        of 1 is shared by the batch.  Returns x [steps + 1, B, n_x] (x[0] = x0) and y [steps, B, n_y] with y[k] = h(x[k + 1], u[k], p)
        - device tensors for device tensors (no host copy), numpy for numpy - and with return_stats a dict of per-instance arrays
        'status' (0 ok, 1 max_num_steps reached, 2 step size too small, 3 - 'idas' alone - no consistent algebraic states found: the
        Newton iteration on g = 0 did not converge, dg/dz is singular or a value is not finite; at the start, at a jump of the inputs
        or at any sampling instant, where the interpolated z is corrected onto g = 0), 'n_accepted', 'n_rejected', 'n_rhs'.
        Under `setup(solver='idas')`: z0 [B, n_z], or one row for the batch, is where the Newton iteration for the consistent initial
        algebraic states starts (None: the guess compiled into the model, `user_source(z_guess=)`; zeros unless one was given); with return_z a further output z [steps + 1, B, n_z] follows y - the algebraic states at
        the sampling instants, z[0] the consistent initial values - and y[k] = h(x[k + 1], z[k + 1], u[k], p).  Either with another
        solver is a ValueError.  The rows of an instance
        whose integration failed are NaN from the sampling instant it did not reach.  Allocates its outputs; inputs AND
        parameters together are packed into one buffer that is kept for the next call - calls on one model must therefore be
        ordered on one stream (the current stream of the device at the time of the call): a second call rewrites the buffer.

        t0: the time of x0, one value for the batch (a per-instance phase belongs in a parameter); read by a time-variant model only.
        Sampling interval k starts at t_k = t0 + k dt.  Over it a continuous model's right-hand side is f(t_k + tau, x, u[k], p),
        tau in [0, dt] - the inputs are held, time is not - and y[k] = h(t_k + dt, x[k + 1], u[k], p); a discrete model's map and
        measurement both see t_k: x[k + 1] = f(t_k, x[k], u[k], p), y[k] = h(t_k, x[k + 1], u[k], p).

        sensitivities (under `setup(solver='dopri5')`): None - every return value as above; True - the forward sensitivities of the
        trajectory with respect to every group the model has out of the initial state, the inputs and the parameters; a tuple out of
        ('x0', 'u', 'p') - those groups.  The result gains a LAST element `sens = {'x': {...}, 'y': {...}}` with one entry per selected
        group: `sens['x']['p']` [steps + 1, B, n_x, n_p] = dx[k] / dp (row 0 the seed: the identity for 'x0', zeros otherwise),
        `sens['y']['p']` [steps, B, n_y, n_p] = h_x dx[k + 1]/dp + h_p, the others likewise ('y' only when the model has measurement
        equations) - device tensors for device tensors, numpy otherwise; permuted views of the kernel's buffers [.., columns, n_x],
        not copies.  The kernel (`hilo_model_rollout_sens`) integrates the augmented system dS/dt = f_x S + f_theta next to the state
        with the same pair, the error norm over ALL components - what scipy's RK45 does on [x; vec S], what a CasADi integrator's
        forward sensitivities are - so its step sequence, and x within the tolerance, differ from the roll-out without; one instance
        runs on a team of lanes, one column per lane.  A failed instance gets NaN in sens wherever it gets NaN in x.  Refused: no
        solver, 'bdf' or 'idas' (NotImplementedError); 'u' together with an input sequence and a group the model does not have
        (ValueError); more than 4 states, more than 64 columns, a learned term, algebraic states.  Out of scope: sensitivities under
        'bdf' / 'idas', of the fixed-step maps, in `simulate`, `Model.linearization` / `LQR` on continuous models, adjoint
        (reverse) sensitivities.

        _h (what `simulate` keeps between its calls): a one-element list holding the 'dopri5' step-size proposals [B] that the previous
        roll-out ended with (None: none yet); they are this one's first steps and are replaced by the ones it ends with
        (`hilo_model_rollout_resume`)."""
        import ctypes
        import torch
        from . import _lib
        from ._device import ptr, stream_ptr, to_dev
        if not self._is_setup:
            raise RuntimeError("Model is not set up. Run Model.setup() before running simulations.")
        steps = int(steps)
        if steps < 1:
            raise ValueError(f"steps must be at least 1, got {steps}")
        idas = self._solver == 'idas'
        if (z0 is not None or return_z) and not idas:
            raise ValueError("z0 and return_z belong to solver='idas' (Model.setup); this model is simulated " +
                             (f"with solver '{self._solver}'" if self._solver else "with its fixed-step map"))
        h = self._plant_handle(device_index)
        dev = h._dev
        host = not isinstance(x0, torch.Tensor)
        xt = to_dev(x0, dev).reshape(-1, self.n_x).contiguous()
        B = xt.shape[0]
        parts, is_sequence = [], {'inputs': False, 'parameters': False}
        for v, n, what in ((u, self.n_u, 'inputs'), (self.lti_parameters() if self.name == 'lti' else p, h._n_p, 'parameters')):
            if n:
                if v is None:
                    raise RuntimeError(f"The model has {n} {what}; pass them to step() / simulate().")
                t = to_dev(v, dev)
                if t.dim() > 3 or (t.dim() == 3 and t.shape[-1] != n):
                    raise ValueError(f"{what}: expected [B, {n}] or [steps, B, {n}], got {list(t.shape)}")
                t = t.reshape(1, -1, n) if t.dim() < 3 else t
                if t.shape[0] not in (1, steps):
                    raise ValueError(f"{what}: a sequence of {t.shape[0]} rows for {steps} sampling intervals")
                if t.shape[1] not in (1, B):
                    raise ValueError(f"{what}: batch {t.shape[1]} does not match {B} states")
                parts.append(t)
                is_sequence[what] = t.shape[0] > 1
        if len(parts) == 2:
            S, Bb = max(q.shape[0] for q in parts), max(q.shape[1] for q in parts)
            up = getattr(self, '_rollout_up', None)
            if up is None or up.shape != (S, Bb, self.n_u + h._n_p) or up.device != xt.device:
                up = self._rollout_up = torch.empty(S, Bb, self.n_u + h._n_p, dtype=torch.float64, device=dev)
            up[:, :, :self.n_u] = parts[0]
            up[:, :, self.n_u:] = parts[1]
        else:
            up = parts[0].contiguous() if parts else None
        nup = up.shape[2] if up is not None else 0
        up_stride = nup if up is not None and up.shape[1] == B else 0
        up_step = up.shape[1] * nup if up is not None and up.shape[0] > 1 else 0
        ny = h._n_y
        X = torch.empty(steps + 1, B, self.n_x, dtype=torch.float64, device=dev)
        Y = torch.empty(steps, B, ny, dtype=torch.float64, device=dev)
        stats = torch.empty(B, 4, dtype=torch.int32, device=dev) if return_stats else None
        sens_groups = None if sensitivities is None else self._sensitivity_groups(sensitivities, h._n_p, is_sequence)
        opts = _lib.SimOpts()
        opts.t0 = float(t0)
        if self._solver is not None:
            o = self._solver_options
            opts.method, opts.max_steps = SOLVERS[self._solver], o['max_num_steps']
            opts.rtol, opts.atol, opts.h0 = o['reltol'], o['abstol'], o['first_step']
        if idas:
            zt = None
            if z0 is not None:
                zt = to_dev(z0, dev).reshape(-1, self.n_z)
                if zt.shape[0] not in (1, B):
                    raise ValueError(f"a z0 of {zt.shape[0]} rows does not match {B} states")
                zt = zt.expand(B, -1).contiguous()
            Z = torch.empty(steps + 1, B, self.n_z, dtype=torch.float64, device=dev) if return_z else None
            _lib.check(_lib.lib().hilo_model_rollout_dae(h._handle, ctypes.byref(opts), B, steps, ptr(xt), ptr(zt), ptr(up), up_stride,
                                                         up_step, ptr(X), ptr(Z), ptr(Y), ptr(stats), stream_ptr(dev)))
        elif sens_groups is not None:
            ns = sum(n for _, n in sens_groups)
            wrt = sum({'x0': 1, 'u': 2, 'p': 4}[g] for g, _ in sens_groups)
            SX = torch.empty(steps + 1, B, ns, self.n_x, dtype=torch.float64, device=dev)
            SY = torch.empty(steps, B, ns, ny, dtype=torch.float64, device=dev) if ny else None
            _lib.check(_lib.lib().hilo_model_rollout_sens(h._handle, ctypes.byref(opts), B, steps, ptr(xt), ptr(up), up_stride, up_step, wrt,
                                                          ptr(X), ptr(Y), ptr(SX), ptr(SY), ptr(stats), stream_ptr(dev)))
        elif _h is not None and self._solver == 'dopri5':
            if _h[0] is None or _h[0].shape != (B,) or _h[0].device != xt.device:
                _h[0] = torch.zeros(B, dtype=torch.float64, device=dev)
            _lib.check(_lib.lib().hilo_model_rollout_resume(h._handle, ctypes.byref(opts), B, steps, ptr(xt), ptr(up), up_stride, up_step,
                                                            ptr(X), ptr(Y), ptr(stats), ptr(_h[0]), stream_ptr(dev)))
        else:
            _lib.check(_lib.lib().hilo_model_rollout(h._handle, ctypes.byref(opts), B, steps, ptr(xt), ptr(up), up_stride, up_step, ptr(X),
                                                     ptr(Y), ptr(stats), stream_ptr(dev)))
        out = (X.cpu().numpy(), Y.cpu().numpy()) if host else (X, Y)
        if return_z:
            out += (Z.cpu().numpy() if host else Z,)
        if return_stats:
            st = stats.cpu().numpy() if host else stats
            out += ({'status': st[:, 0], 'n_accepted': st[:, 1], 'n_rejected': st[:, 2], 'n_rhs': st[:, 3]},)
        if sens_groups is not None:
            out += (self._sensitivity_views(sens_groups, SX.cpu().numpy() if host else SX,
                                            None if SY is None else (SY.cpu().numpy() if host else SY)),)
        return out

    @staticmethod
    def _sensitivity_views(sens_groups, SX, SY):
        """The kernel's buffers [rows, B, columns, n] cut into the groups' columns and turned to [rows, B, n, n_group]: views."""
        def cut(S):
            res, at = {}, 0
            for g, n in sens_groups:
                v = S[:, :, at:at + n]
                res[g] = v.permute(0, 1, 3, 2) if hasattr(v, 'permute') else v.transpose(0, 1, 3, 2)
                at += n
            return res
        sens = {'x': cut(SX)}
        if SY is not None:
            sens['y'] = cut(SY)
        return sens

    def set_initial_conditions(self, x0, t0=0., z0=None):
        """dynamic_model.py:3360-3400 (a batch of states is allowed: [B, n_x])."""
        if not self._is_setup:
            raise RuntimeError("Model is not set up. Run Model.setup() before setting the initial conditions.")
        x = np.atleast_2d(np.asarray(x0.cpu() if hasattr(x0, 'cpu') else x0, dtype=float))
        if x.shape[1] != self.n_x:
            x = x.T
        if x.shape[1] != self.n_x:
            raise ValueError(f"Dimension mismatch. Supplied dimension for the initial states is {x.shape[1]}, but required "
                             f"dimension is {self.n_x}.")
        self._sim = {'t': [float(t0)], 'x': [x], 'y': [], 'u': [], 'status': [], 'n_accepted': [], 'n_rejected': []}
        if z0 is not None and getattr(self, 'n_z', 0):
            # where `simulate` under solver='idas' starts the Newton iteration for the consistent algebraic states of the first call
            z = np.atleast_2d(np.asarray(z0.cpu() if hasattr(z0, 'cpu') else z0, dtype=float))
            if z.shape[1] != self.n_z:
                z = z.T
            if z.shape[1] != self.n_z or z.shape[0] not in (1, x.shape[0]):
                raise ValueError(f"Dimension mismatch. Supplied dimension for the initial algebraic states is {z.shape[1]}, but "
                                 f"required dimension is {self.n_z}.")
            self._sim['_z0'] = z

    def simulate(self, u=None, p=None, steps=1, tf=None, **kwargs):
        """dynamic_model.py:3911-4000: advance the stored state by `steps` sampling intervals (or up to `tf`: int(tf / dt) of them,
        :3937-3941 - truncated, so a `tf` that floating-point division leaves just below a multiple of dt loses an interval, and tf < dt
        does nothing) with the inputs held; results in `model.solution` (`solution['x:f']` the last state, `solution['x']` the
        trajectory).  A time-variant model starts each call at `solution['t:f']` (`set_initial_conditions(x0, t0)` sets the first)
        and is always ONE `rollout`; under 'dopri5' it also starts with the step sizes the last call ended with, so that calls in a row
        give what one `rollout` over all of them gives.  Without a solver and with inputs / parameters of at most two dimensions this is a loop over `step`.  With
        `setup(solver=...)`, or with a sequence u [steps, B, n_u] (p likewise; `steps` is then taken from it), it is ONE `rollout`;
        `solution['status']`, `['n_accepted']`, `['n_rejected']` hold the integrator's per-instance status and step counts of each
        call.  Under 'idas' `solution['z']` / `['z:f']` hold the algebraic states, shaped like x; the first call starts the Newton
        iteration for the consistent initial values at the z0 of `set_initial_conditions`, every later one at the stored z."""
        if not self._is_setup:
            raise RuntimeError("Model is not set up. Run Model.setup() before running simulations.")
        if getattr(self, '_sim', None) is None:
            raise RuntimeError("No initial dynamical states found. Please set initial conditions before simulating the model.")
        if tf is not None:
            steps = int(tf / self.dt)             # truncated like the reference's: tf = .3 at dt = .1 is 2 intervals
        if int(steps) == 0 and not [v for v in (u, p) if v is not None and getattr(v, 'ndim', np.ndim(v)) == 3]:
            return                                # (tf < dt: nothing to do, on either path)
        seq = [v for v in (u, p) if v is not None and getattr(v, 'ndim', np.ndim(v)) == 3]
        if self._solver is not None or seq or self.is_time_variant():
            for v in seq:
                steps = int(v.shape[0] if hasattr(v, 'shape') else len(v))
            host = lambda v: None if v is None else np.asarray(v.cpu() if hasattr(v, 'cpu') else v, dtype=float)
            u, p = host(u), host(p)
            if u is not None and u.ndim < 3:
                u = u.reshape(1, -1) if u.size == self.n_u else (u.T if u.ndim == 2 and u.shape[0] == self.n_u and u.shape[1] != self.n_u else u)
            # a time-variant model goes on with the step sizes of its last call: two calls equal one roll-out over both stretches
            # (an autonomous model's calls each estimate their first step, as they always did)
            keep = self._sim.setdefault('_h', [None]) if self.is_time_variant() else None
            if self._solver == 'idas':
                # from the stored z of the last call, else the caller's z0; the first call records the consistent initial values
                zs = self._sim.setdefault('z', [])
                x, y, z, st = self.rollout(self._sim['x'][-1], u, p, steps=steps, return_stats=True, t0=self._sim['t'][-1],
                                           z0=zs[-1] if zs else self._sim.get('_z0'), return_z=True)
                zs[:] = zs or [z[0]]
                zs.extend(z[1:])
            else:
                x, y, st = self.rollout(self._sim['x'][-1], u, p, steps=steps, return_stats=True, t0=self._sim['t'][-1], _h=keep)
            for k in range(int(steps)):
                self._sim['x'].append(x[k + 1]), self._sim['y'].append(y[k])
                self._sim['u'].append(u if u is None or u.ndim < 3 else u[k])
                self._sim['t'].append(self._sim['t'][-1] + self.dt)
            for key in ('status', 'n_accepted', 'n_rejected'):
                self._sim.setdefault(key, []).append(st[key])
            return
        if u is not None:
            u = np.asarray(u.cpu() if hasattr(u, 'cpu') else u, dtype=float)
            u = u.reshape(1, -1) if u.size == self.n_u else (u.T if u.ndim == 2 and u.shape[0] == self.n_u and u.shape[1] != self.n_u else u)
        for _ in range(int(steps)):
            x, y = self.step(self._sim['x'][-1], u, p)
            self._sim['x'].append(x), self._sim['y'].append(y), self._sim['u'].append(u)
            self._sim['t'].append(self._sim['t'][-1] + self.dt)

    def generate_data(self, signal_type, *args, output='absolute', shift=0, add_noise=None, n_samples=None, steps=None, bounds=None,
                      mean=None, variance=None, seed=None, chirps=None, skip=None, **kwargs):
        """dynamic_model.py:4214-4369: excite this model with a 'random_uniform' / 'random_normal' staircase or with 'chirp' signals
        and return the `DataSet` of features and labels - for a batch of experiments (x0 [B, n_x], p0 [B, n_p] in **kwargs, which
        go to `DataGenerator`) in ONE launch.  bounds {input: {'lb': .., 'ub': ..}} (default 0 and 1); mean / variance {input: value}
        default to the middle of the bounds and to a third of their half width as standard deviation; chirps {input: {'type',
        'amplitude', 'length', 'mean', 'chirp_rate', 'initial_phase', 'initial_frequency', 'initial_frequency_ratio'}}; skip: names
        or indices of states left out.  'closed_loop' is not built."""
        from .data import DataGenerator
        data_generator = DataGenerator(self, **kwargs)
        signal_type = signal_type.replace(' ', '_').lower()
        if signal_type in ['random_uniform', 'random_normal']:
            if n_samples is None:
                raise ValueError(f"Generating data using the {signal_type.replace('_', ' ')} signal requires "
                                 f"information about the number of samples by supplying the keyword 'n_samples'")
            if steps is None:
                raise ValueError(f"Generating data using the {signal_type.replace('_', ' ')} signal requires "
                                 f"information about the number of steps by supplying the keyword 'steps'")
            lbs, ubs = [], []
            for k in self.input_names:
                name = (bounds or {}).get(k)
                lb = ub = None
                if name is not None:
                    lb = name.get('lb')
                    if lb is None:
                        lb = name.get('lower_bound')
                    ub = name.get('ub')
                    if ub is None:
                        ub = name.get('upper_bound')
                lbs.append(0. if lb is None else lb)
                ubs.append(1. if ub is None else ub)
            if signal_type == 'random_uniform':
                data_generator.random_uniform(n_samples, steps, lbs, ubs, seed=seed)
            else:
                mus = [None if mean is None else mean.get(k) for k in self.input_names]
                sigmas = [None if variance is None else variance.get(k) for k in self.input_names]
                for k in range(self.n_u):
                    if mus[k] is None:
                        mus[k] = lbs[k] + (ubs[k] - lbs[k]) / 2
                    if sigmas[k] is None:
                        sigmas[k] = (1. / 3. * (ubs[k] - lbs[k]) / 2) ** 2  # 99.7% lie between lb and ub
                data_generator.random_normal(n_samples, steps, mus, sigmas, seed=seed)
        elif signal_type == 'chirp':
            cols = [[] for _ in range(8)]
            for k in self.input_names:
                chirp = (chirps or {}).get(k)
                if chirp is None:
                    raise ValueError(f"No chirp signals supplied for input'{k}'")
                if chirp.get('length') is None:
                    raise ValueError(f"No length(s) supplied for input '{k}'")
                if chirp.get('chirp_rate') is None:
                    raise ValueError(f"No chirp rate(s) supplied for input '{k}'")
                cols[0].append('linear' if chirp.get('type') is None else chirp.get('type'))
                cols[1].append(1. if chirp.get('amplitude') is None else chirp.get('amplitude'))
                cols[2].append(chirp.get('length'))
                cols[3].append(0. if chirp.get('mean') is None else chirp.get('mean'))
                cols[4].append(chirp.get('chirp_rate'))
                cols[5].append(chirp.get('initial_phase'))
                cols[6].append(chirp.get('initial_frequency'))
                cols[7].append(chirp.get('initial_frequency_ratio'))
            data_generator.chirp(*cols[:5], initial_phase=cols[5], initial_frequency=cols[6], initial_frequency_ratio=cols[7])
        elif signal_type == 'closed_loop':
            if not args:
                raise ValueError(f"No controller supplied for {signal_type.replace('_', ' ')} setup")
            if steps is None:
                raise ValueError(f"Generating data using the {signal_type.replace('_', ' ')} setup requires "
                                 f"information about the number of steps by supplying the keyword 'steps'")
            data_generator.closed_loop(*args, steps)
        else:
            raise ValueError(f"Signal type '{signal_type}' not recognized. Choose 'random_uniform', 'random_normal' or 'chirp'")
        if add_noise is not None and 'seed' not in add_noise and seed is not None:
            add_noise = add_noise.copy()
            add_noise['seed'] = seed
        if skip is not None:
            if all(isinstance(k, str) for k in skip):
                missing = [k for k in skip if k not in self.dynamical_state_names]
                if missing:
                    raise ValueError(f"skip: the model has no dynamical states {missing}. Choose out of {self.dynamical_state_names}")
                skip = [self.dynamical_state_names.index(k) for k in skip]
            elif any(isinstance(k, str) for k in skip):
                raise ValueError("Mixed iterables for the keyword argument 'skip' are not allowed. Either use only "
                                 "strings or only indices (integers) in your iterable.")
        data_generator.run(output, skip=skip, shift=shift, add_noise=add_noise)
        return data_generator.data

    @property
    def solution(self):
        """`model.solution['x:f']`, `['y:f']`, `['t:f']`, `['x']` ... (the key language of base.py:2426-2470 for the last value /
        the whole series; single instance: column vectors like the reference's)."""
        sim = getattr(self, '_sim', None)

        class _View:
            def __getitem__(_, key):
                if sim is None:
                    raise KeyError(key)
                name, _, sel = key.partition(':')
                series = sim[name]
                if not series:
                    raise KeyError(key)
                if sel in ('f', '-1'):
                    v = np.asarray(series[-1])
                    return v.T if (v.ndim == 2 and v.shape[0] == 1) else v
                if sel == '0':
                    v = np.asarray(series[0])
                    return v.T if (v.ndim == 2 and v.shape[0] == 1) else v
                a = np.asarray(series)
                return a[:, 0].T if (a.ndim == 3 and a.shape[1] == 1) else a

            get_by_id = __getitem__
        return _View()
