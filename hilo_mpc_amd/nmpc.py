"""Batched nonlinear MPC on the GPU.

API mirror of `hilo_mpc.NMPC` (hilo_mpc/modules/controller/mpc.py) for the hot path: constructor, `quad_stage_cost`
/ `quad_terminal_cost` (`add_states`, `add_inputs`, `add_inputs_change`, util/modeling.py:364-450), `horizon`,
`set_box_constraints` (mpc.py:619-710), `set_initial_guess`, `set_scaling` (optimizer.py:1476-1506),
`set_nlp_options` (optimizer.py:1388-1474), `setup` (mpc.py:1789-1801), `optimize` (mpc.py:744-857) and
`return_prediction` (mpc.py:1803-1827) - with a leading batch axis on `x0`, `cp`, `v0`.

Scope of this backend: models of the device zoo or written as expressions (`Model.set_dynamical_equations`, compiled at
`setup()`, csrc/hilo_jit.hip), pre-discretised with `model.discretize('rk4'|'erk')` + `integration_method='discrete'` (SURVEY.md
Q18), or continuous with the reference's default collocation / explicit Runge-Kutta inside the NLP (continuous objective);
quadratic costs on states / inputs / input changes / measurements with constant, path-following or trajectory references,
generic costs (`stage_cost.cost = ...`), nonlinear stage / terminal constraints (hard or soft), control horizon, algebraic
states (collocation), learned terms (`substitute_from(gp)`), box constraints, scaling, multi-start.  Everything numeric is done
by `hilo_nmpc_solve` in libhilo_hip.so; what is not offloaded raises NotImplementedError, nothing falls back to the CPU.
"""
import ctypes as C
import os
import time
import warnings

import numpy as np
import torch

from . import _lib
from ._device import device, to_dev, ptr, stream_ptr
from .expr import Expr, compile_block as _compile_block
from .model import ZOO_FUNCTOR as ZOO_FUNCTOR_NAMES

STATUS_TEXT = {1: 'solve_succeeded', 2: 'solved_to_acceptable_level', 3: 'infeasible_problem_detected',
               4: 'restoration_failed', 5: 'maximum_iterations_exceeded', -1: 'other'}


def _eval_time(e, t):
    """Value of an expression of the time variable at time t (reference trajectories given as functions, mpc.py:1847)."""
    import math
    from .symdiff import _NUMERIC as fn
    val = {}
    for n in sorted(Expr.wrap(e).nodes().values(), key=lambda q: q.serial):
        a = [val[id(c)] for c in n.args]
        op = n.op
        if op == 'const':
            r = n.value
        elif op == 't':
            r = float(t)
        elif op in ('add', 'sub', 'mul', 'div'):
            r = a[0] + a[1] if op == 'add' else a[0] - a[1] if op == 'sub' else a[0] * a[1] if op == 'mul' else a[0] / a[1]
        elif op == 'neg':
            r = -a[0]
        elif op == 'sq':
            r = a[0] * a[0]
        elif op == 'powi':
            r = a[0] ** int(n.value)
        elif op in fn:
            r = fn[op](a[0])
        elif op == 'atan2':
            r = math.atan2(a[0], a[1])
        else:
            raise ValueError(f"a trajectory reference can only be a function of the time variable (found '{op}')")
        val[id(n)] = r
    return val[id(Expr.wrap(e))]


def _wrap_list(v):
    if v is None:
        return None
    if isinstance(v, (int, float)):
        return [float(v)]
    return [float(a) for a in np.asarray(v, dtype=float).ravel()]


def _weight_matrix(arg, n, name):
    """QuadraticCost._create_weight_matrix (modeling.py:164-185)."""
    if isinstance(arg, np.ndarray):
        if arg.ndim == 2 and arg.shape[0] == arg.shape[1]:
            W = arg
        elif arg.ndim == 1:
            W = np.diag(arg)
        else:
            raise TypeError(f"{name} must be a square matrix,a 1-D array or a list of real numbers.")
    elif isinstance(arg, list):
        W = np.diag(arg)
    elif isinstance(arg, (float, int)):
        W = np.diag([arg])
    else:
        raise TypeError(f"The {name} must be a list of floats, numpy array or casadi DM.")
    W = np.asarray(W, dtype=float)
    if W.shape[0] != n:
        raise ValueError(f"states and weights dimensions must be compatible. The states vector you passed me is"
                         f" {n} long while cost {W.shape}.")
    return W


def _constraint_weight(arg, n, name):
    """The weight of a soft constraint is used as it is given, `e^T weight e` (modeling.py:870, :878): a matrix.  A scalar weighs
    every slack alike, a vector is taken as a diagonal."""
    W = np.asarray(arg, dtype=float)
    if W.ndim == 0:
        W = float(W) * np.eye(n)
    elif W.ndim == 1:
        W = np.diag(W)
    if W.ndim != 2 or W.shape != (n, n):
        raise ValueError(f"The weight of the soft {name} must be a {n} x {n} matrix, it is {W.shape}.")
    return np.ascontiguousarray(W)


def _collocation_basis(degree, points='radau'):
    """`RungeKutta._construct_polynomial_basis` (hilo_mpc/util/modeling.py:1091-1127) for tau = [0] +
    collocation_points(degree, points): D_i = L_i(1), C[i, j] = L_i'(tau_j); plus the Runge-Kutta matrix of the method,
    A = (C[1:, 1:]^T)^-1, which is the form the device solves the collocation equations in (csrc/hilo_colloc.h)."""
    from numpy.polynomial import legendre
    c = np.zeros(degree + 1)
    if points == 'radau':                      # roots of P_{d-1} - P_d: Gauss-Radau with the right end point
        c[degree - 1], c[degree] = 1., -1.
    else:                                      # 'legendre': Gauss points
        c[degree] = 1.
    tau = [0.] + list((np.sort(np.real(legendre.legroots(c))) + 1.) / 2.)
    Cm, D, Bq = np.zeros((degree + 1, degree + 1)), np.zeros(degree + 1), np.zeros(degree + 1)
    for i in range(degree + 1):
        L = np.poly1d([1.])
        for j in range(degree + 1):
            if j != i:
                L *= np.poly1d([1., -tau[j]]) / (tau[i] - tau[j])
        D[i] = L(1.)
        Ld = np.polyder(L)
        for j in range(degree + 1):
            Cm[i, j] = Ld(tau[j])
        Bq[i] = np.polyint(L)(1.)                # quadrature weights of the continuous objective (modeling.py:1124)
    return {'d': degree, 'tau': np.array(tau), 'C': Cm, 'D': D, 'B': Bq, 'A': np.linalg.inv(Cm[1:, 1:].T)}


class QuadraticCost:
    """`util/modeling.py:89-531` restricted to what the device solver evaluates."""

    def __init__(self, model):
        self._model = model
        self._terms = []          # (type, indices, W, ref)
        self._paths = []          # (state indices, W, [expression of theta])
        self._trajectories = []   # (kind, names, indices): references supplied per call or as functions of time
        self._traj_funs = {}      # name -> expression of the time variable (modeling.py:262-283 with `ref` given)
        self._meas_terms = []     # (measurement indices, W, ref): costs on y = h(x, u) (modeling.py:385-408)
        self._is_set = False

    def _add(self, kind, names, pool, weights, ref, path_following, trajectory_tracking):
        names = [names] if isinstance(names, str) else list(names)
        if trajectory_tracking:
            # modeling.py:262-283: the reference is a placeholder - filled per call from `optimize(ref_sc=..., ref_tc=...)`
            # (mpc.py:365-463), or a FUNCTION OF TIME (`ref=sin(nmpc.get_time_variable())`) substituted into the cost
            # (mpc.py:232-246) and evaluated at the time of each stage, t_0 + k dt (mpc.py:1649, :1727).  Both arrive at the
            # device as the per-stage reference table of a solve (`_stage_table`).
            funs = None
            if ref is not None:
                funs = [ref] if isinstance(ref, (Expr, int, float)) else list(ref)
                if len(funs) != len(names):
                    raise ValueError(f"{kind} and reference dimensions must be compatible. The states vector you passed me "
                                     f"is {len(names)} long while cost {len(funs)}.")
                funs = [Expr.wrap(f) for f in funs]
                for f in funs:
                    if any(n.op in ('x', 'u', 'p', 'z', 'theta', 'gp', 'gpd', 'gpvar', 'gpk') for n in f.nodes().values()):
                        raise ValueError("a trajectory reference can only be a function of the time variable "
                                         "(nmpc.get_time_variable())")
            ind = []
            for n in names:
                if n not in pool:
                    raise ValueError(f"The state {n} does not exist. The available states are {pool}")
                ind.append(pool.index(n))
            self._terms.append((kind, ind, _weight_matrix(weights, len(names), 'weights'), None))
            self._trajectories.append((kind, names, ind))
            for k_, n in enumerate(names):
                if n in self._traj_funs or (funs is None and n in [q for _, nn, _ in self._trajectories[:-1] for q in nn]):
                    raise TypeError("Two different varying trajectory for the same states are not allowed.")
                if funs is not None:
                    self._traj_funs[n] = funs[k_]
            self._is_set = True
            return
        if path_following:
            # modeling.py:252-261: the reference is an expression of the path variable, substituted into the cost
            if kind != 'states':
                raise NotImplementedError("path references are offloaded for states")
            ref = [ref] if isinstance(ref, Expr) else list(ref or [])
            if len(ref) != len(names) or not all(isinstance(r, (Expr, int, float)) for r in ref):
                raise ValueError("path following needs one expression of the path variable per name")
            ind = []
            for n in names:
                if n not in pool:
                    raise ValueError(f"The state {n} does not exist. The available states are {pool}")
                ind.append(pool.index(n))
            self._paths.append((ind, _weight_matrix(weights, len(names), 'weights'), [Expr.wrap(r) for r in ref]))
            self._is_set = True
            return
        ind = []
        for n in names:
            if n not in pool:
                raise ValueError(f"The state {n} does not exist. The available states are {pool}")
            ind.append(pool.index(n))
        if weights is None:
            raise ValueError(f"You passed the following {kind}: {names} to the cost function, but I do not have any "
                             f"weights for it/them. Please pass me the weights.")
        W = _weight_matrix(weights, len(names), 'weights')
        ref = _wrap_list(ref)
        if ref is not None and len(ref) != len(names):
            raise ValueError(f"{kind} and reference dimensions must be compatible. The states vector you passed me "
                             f"is {len(names)} long while cost {len(ref)}.")
        self._terms.append((kind, ind, W, ref))
        self._is_set = True

    def add_states(self, names, weights, ref=None, path_following=False, trajectory_tracking=False):
        self._add('states', names, self._model.dynamical_state_names, weights, ref, path_following, trajectory_tracking)

    def add_inputs(self, names, weights, ref=None, path_following=False, trajectory_tracking=False):
        self._add('inputs', names, self._model.input_names, weights, ref, path_following, trajectory_tracking)

    def add_inputs_change(self, names, weights):
        self._add('inputs_change', names, self._model.input_names, weights, None, False, False)

    @property
    def name_open_varying_trajectories(self):
        return [n for _, names, _ in self._trajectories for n in names if n not in self._traj_funs]   # modeling.py:485-490

    _has_trajectory_following = property(lambda s: bool(s._trajectories))

    def add_measurements(self, names, weights, ref=None, path_following=False, trajectory_tracking=False):
        """modeling.py:385-408: (h(x, u) - ref)^T W (h(x, u) - ref) on the model's measurement equations; the reference (a
        constant here) is divided by the measurement scaling at setup (modeling.py:310)."""
        if path_following or trajectory_tracking:
            raise NotImplementedError("measurement costs with path / trajectory references are not offloaded")
        names = [names] if isinstance(names, str) else list(names)
        ind = []
        for n in names:
            if n not in self._model.measurement_names:
                raise ValueError(f"The measurement {n} does not exist. The available measurements are "
                                 f"{self._model.measurement_names}")
            ind.append(self._model.measurement_names.index(n))
        W = _weight_matrix(weights, len(ind), 'weights')
        r = np.zeros(len(ind)) if ref is None else np.asarray(_wrap_list(ref), dtype=float)
        if r.size != len(ind):
            raise ValueError("the reference must have one entry per measurement")
        self._meas_terms.append((ind, W, r))
        self._is_set = True

    def _measurement_cost(self, y_scaling):
        """The measurement terms as ONE expression of the model symbols (run-time compiled like a GenericCost; evaluated on the
        scaled variables like every cost of the reference), or None."""
        if not self._meas_terms:
            return None
        m = self._model
        if getattr(m, '_symbolic', False):
            meas = m._meas
        else:
            from . import zoo_expr
            from .model import Model
            if m.name not in zoo_expr.FUNCTOR:
                raise NotImplementedError(f"measurement costs need the measurement equations as expressions; model '{m.name}' "
                                          f"of the device zoo has none (available: {sorted(zoo_expr.FUNCTOR)})")
            meas = zoo_expr.define(Model(name=m.name + '_expr'), m.name)._meas
        sy = np.ones(len(meas)) if y_scaling is None else np.asarray(y_scaling, dtype=float)
        total = None
        for ind, W, r in self._meas_terms:
            e = [meas[i] - float(r[q] / sy[i]) for q, i in enumerate(ind)]
            for a in range(len(ind)):
                for b in range(len(ind)):
                    if W[a, b] != 0.0:
                        t = float(W[a, b]) * (e[a] * e[b])
                        total = t if total is None else total + t
        return total


class GenericCost:
    """`util/modeling.py:38-87`: a free-form cost, `nmpc.stage_cost.cost = expression of model.x / model.u / model.p`
    (assignments accumulate, like the reference's `self._cost += arg`).

    Restated quirk of the reference: the expression is attached to the model after the model has been scaled
    (mpc.py:1210 then :1283; `Model.scale` only substitutes inside the model's own equations, base.py:1169-1179), so its
    symbols are the scaled NLP variables - with `set_scaling(x_scaling=s)` the cost sees x / s."""

    def __init__(self, model):
        self._model = model
        self._cost = None
        self._is_set = False

    @property
    def cost(self):
        return 0 if self._cost is None else self._cost

    @cost.setter
    def cost(self, arg):
        if not isinstance(arg, Expr):
            raise TypeError('The cost function must be an expression of the model symbols (model.x, model.u, model.p).')
        self._cost = arg if self._cost is None else self._cost + arg
        self._is_set = True


class GenericConstraint:
    """`util/modeling.py:820-1005`: lb <= constraint(x, u) <= ub per stage; soft: one slack shared by all stages with the
    penalty e^T weight e per stage (default weight 1e4 I, modeling.py:875)."""

    def __init__(self, model, name='constraint'):
        self._model, self._name = model, name
        self._function = None
        self._lb = self._ub = None
        self._is_soft = False
        self._weight = None
        self._max_violation = None
        self.e_soft_value = 0

    @property
    def constraint(self):
        return self._function

    @constraint.setter
    def constraint(self, arg):
        if arg is not None:
            arg = [arg] if isinstance(arg, Expr) else list(arg)
            if not all(isinstance(a, Expr) for a in arg):
                raise TypeError(f"The {self._name} must be an expression of the model symbols (model.x, model.u, "
                                f"model.p) or None.")
        self._function = arg

    lb = property(lambda s: s._lb, lambda s, v: setattr(s, '_lb', None if v is None else _wrap_list(v)))
    ub = property(lambda s: s._ub, lambda s, v: setattr(s, '_ub', None if v is None else _wrap_list(v)))
    max_violation = property(lambda s: s._max_violation,
                             lambda s, v: setattr(s, '_max_violation', None if v is None else _wrap_list(v)))
    weight = property(lambda s: s._weight, lambda s, v: setattr(s, '_weight', v))

    @property
    def is_soft(self):
        return self._is_soft

    @is_soft.setter
    def is_soft(self, arg):
        if not isinstance(arg, bool):
            raise TypeError("is_soft must be of type bool")
        self._is_soft = arg

    @property
    def size(self):
        return 0 if self._function is None else len(self._function)

    @property
    def is_set(self):
        return self._function is not None


class NMPC:
    _solver_name_list_nlp = ['ipopt', 'hip_ipm']

    def __init__(self, model, id=None, name=None, plot_backend=None, use_sx=True, stats=False, device_index=None):
        # a continuous model is transcribed at setup() by `integration_method`: 'collocation' (the reference's default,
        # optimizer.py:1410-1418) or explicit Runge-Kutta ('rk4' / 'erk'); a discrete(-ised) model uses 'discrete'
        model._refuse_time_variant(getattr(self, 'type', None) or 'NMPC')
        if not model._is_setup:
            model.setup()
        self._model = model
        self.name = name
        self._stats = stats
        self._n_x, self._n_u, self._n_p = model.n_x, model.n_u, model.n_p
        self.quad_stage_cost = QuadraticCost(model)
        self.quad_terminal_cost = QuadraticCost(model)
        self.stage_cost = GenericCost(model)
        self.terminal_cost = GenericCost(model)
        self.stage_constraint = GenericConstraint(model, name='stage constraint')
        self.terminal_constraint = GenericConstraint(model, name='terminal constraint')
        self._paths_var_list = []
        self._time_varying_parameters = []
        self._time_varying_parameters_values = None
        self._prediction_horizon = self._control_horizon = None
        self._x_lb = self._x_ub = self._u_lb = self._u_ub = None
        self._x_guess = self._u_guess = None
        self._x_scaling = self._u_scaling = None
        self._nlp_options = None
        self._solver_options = {}
        self._handle = None
        self._dev_index = device_index
        self._nlp_setup_done = False
        self._time = 0.
        self._n_iterations = 0
        self._nlp_solution = None
        self._sampling_interval = model.dt
        self._u_prev = None
        self._full_solution = False   # keep_full_solution: also return the solver result's `g` and `lam_x`

    type = 'NMPC'

    # ---- horizons (optimizer.py:1730-1768) ------------------------------------------------------------------
    @property
    def horizon(self):
        return self._prediction_horizon

    @horizon.setter
    def horizon(self, n):
        self.prediction_horizon = n
        self.control_horizon = n

    @property
    def prediction_horizon(self):
        return self._prediction_horizon

    @prediction_horizon.setter
    def prediction_horizon(self, n):
        if not isinstance(n, (int, np.integer)) or n <= 0:
            raise ValueError("The prediction horizon must be a positive integer")
        self._prediction_horizon = int(n)

    @property
    def control_horizon(self):
        return self._control_horizon

    @control_horizon.setter
    def control_horizon(self, n):
        if not isinstance(n, (int, np.integer)) or n <= 0:
            raise ValueError("The control horizon must be a positive integer")
        self._control_horizon = int(n)

    @property
    def sampling_interval(self):
        return self._sampling_interval

    n_iterations = property(lambda s: s._n_iterations)
    n_of_path_vars = property(lambda s: len(s._paths_var_list))

    def set_time_varying_parameters(self, names=None, values=None):
        """optimizer.py:1519-1560: model parameters whose value changes along the horizon; `values` {name: sequence} may be
        given here (then the horizon window advances with the iteration counter, mpc.py:292-333) or to optimize(tvp=...)."""
        if names is None:
            self._time_varying_parameters = []
        else:
            if not (isinstance(names, (list, tuple)) and all(isinstance(n, str) for n in names)):
                raise ValueError('Tvp must be a list of strings with the paramers name that are time varying')
            for tvp in names:
                if tvp not in self._model.parameter_names:
                    raise ValueError(f"I could not find the parameter {tvp} in the model. The models parameters are "
                                     f"{self._model.parameter_names}.")
            self._time_varying_parameters = list(names)
        if values is not None:
            if not isinstance(values, dict):
                raise TypeError("The values parameter must be a dictionary.")
            for key in values:
                if key not in (names or []):
                    raise ValueError(f"The key {key} is not in the name vector: {names}. You need to pass a dictionary "
                                     f"where the keys are the name of the time varying parameters.")
        self._time_varying_parameters_values = values
        self._n_tvp = len(self._time_varying_parameters)

    # ---- small accessors of the reference's controller base (optimizer.py:1508-1768, mpc.py:1926-1931) -----------------------
    current_time = property(lambda s: s._time)
    initial_time = property(lambda s: s._time)
    n_tvp = property(lambda s: len(s._time_varying_parameters))
    x_lb = property(lambda s: s._x_lb)
    x_ub = property(lambda s: s._x_ub)
    u_lb = property(lambda s: s._u_lb)
    u_ub = property(lambda s: s._u_ub)
    time_var = property(lambda s: getattr(s, '_time_var', []))

    def is_setup(self):
        return bool(self._nlp_setup_done)

    def set_sampling_interval(self, dt=None):
        """optimizer.py `set_sampling_interval`: the interval the controller's clock advances by per optimize()."""
        if dt is not None:
            if isinstance(dt, (float, int)):
                self._sampling_interval = dt
            else:
                raise TypeError("Sampling interval must be a float.")

    def set_nlp_solver(self, solver):
        """optimizer.py:1372-1385; the name is checked by `set_nlp_options` ('ipopt' = the interior point of the device)."""
        self._solver_name = solver
        self._nlp_solver_is_set = True

    def reset_solution(self):
        """Forget the last solve: result, warm start, clock and iteration counter."""
        self._nlp_solution, self._u_prev = None, None
        self._time, self._n_iterations = 0., 0
        if self._handle is not None:
            _lib.check(_lib.lib().hilo_nmpc_reset_warm_start(self._handle))
        if getattr(self, '_mt', None) is not None:       # minimum-time problems: the solve lives in the inner controller
            self._mt.reset_solution()

    SUNDIALS_SUBSTEPS = 64    # Runge-Kutta sub-steps per interval behind integration_method 'cvodes' / 'idas'

    def minimize_final_time(self, weight=1):
        """mpc.py:859-866: the N sampling intervals become decision variables (the last block of `v`, bounds [0, inf), guess dt;
        forced equal by N - 1 rows at the end of `g`, mpc.py:1746-1751) and J += weight * sum(dt) (:1754)."""
        self._minimize_final_time_flag = True
        self._minimize_final_time_weight = float(weight)

    # ---- minimum-time problems ---------------------------------------------------------------------------------------------
    # All intervals are forced equal, so the problem has ONE more degree of freedom: the common interval.  It is carried as an extra
    # STATE r with r' = 0 and dt = r^2, on a normalised time axis - the model becomes x' = r^2 f(x, u, p) with sampling interval 1
    # (identical collocation / Runge-Kutta equations: dt f = r^2 f), the reference's N - 1 equality rows ARE the continuity rows of
    # r, the objective weight * dt_k is the quadratic stage cost weight * r^2 (integrated over an interval of length 1), and dt >= 0
    # holds by construction.  r_0 is a variable (desc.x0_free_mask).  Same minimiser and multipliers as the reference's NLP - the
    # multipliers of its dt rows follow from the continuity multipliers of r, eta_k = -lambda^r_k / (2 r) - different iterates.
    def _setup_min_time(self, options, solver_options):
        from .model import Model
        m = self._model
        if not getattr(m, '_symbolic', False) or m.discrete or getattr(m, 'n_z', 0):
            raise NotImplementedError("minimize_final_time needs a continuous model written as expressions without algebraic states")
        if self.quad_stage_cost._is_set or self.stage_cost._is_set or self.terminal_cost._is_set or self._paths_var_list:
            raise NotImplementedError("minimize_final_time together with further stage-cost terms or a path variable is not built "
                                      "(their integrals would scale with the interval)")
        if self._control_horizon != self._prediction_horizon or self._time_varying_parameters:
            raise NotImplementedError("minimize_final_time with a shorter control horizon or time-varying parameters is not built")
        rname = '_dt_root'
        aug = Model(name=(m.name or 'model') + '_min_time')
        xa = aug.set_dynamical_states(list(m.dynamical_state_names) + [rname])
        aug.set_inputs(list(m.input_names))
        aug.set_parameters(list(m.parameter_names))
        r = xa[len(m.dynamical_state_names)]
        aug.set_dynamical_equations([r * r * e for e in m._ode] + [0.0 * r])
        if m._meas:
            aug.set_measurement_equations(list(m._meas))
        aug.setup(dt=1.0)
        inner = NMPC(aug, device_index=self._dev_index)
        inner.horizon = self._prediction_horizon
        inner.quad_stage_cost.add_states(names=[rname], weights=[self._minimize_final_time_weight], ref=[0.])
        for kind, ind, W, ref in self.quad_terminal_cost._terms:
            if kind != 'states':
                raise NotImplementedError("minimize_final_time: the terminal cost may contain states only")
            inner.quad_terminal_cost.add_states(names=[m.dynamical_state_names[i] for i in ind], weights=W, ref=ref)
        for mine, theirs in ((self.stage_constraint, inner.stage_constraint), (self.terminal_constraint, inner.terminal_constraint)):
            if mine.is_set:
                theirs.constraint, theirs.lb, theirs.ub = mine.constraint, mine.lb, mine.ub
                theirs.is_soft, theirs.weight, theirs.max_violation = mine.is_soft, mine.weight, mine.max_violation
        nx, dt = self._n_x, float(m.dt)
        box = lambda v, fill, last: (list(np.full(nx, fill)) if v is None else list(v)) + [last]      # noqa: E731
        inner.set_box_constraints(x_lb=box(self._x_lb, -np.inf, 0.), x_ub=box(self._x_ub, np.inf, np.inf), u_lb=self._u_lb, u_ub=self._u_ub)
        inner.set_initial_guess(x_guess=box(self._x_guess, 0., np.sqrt(dt)), u_guess=self._u_guess)
        if self._x_scaling is not None or self._u_scaling is not None:
            inner.set_scaling(x_scaling=None if self._x_scaling is None else list(self._x_scaling) + [1.], u_scaling=self._u_scaling)
        inner._x0_free_mask = 1 << nx
        inner.setup(options=options, solver_options=solver_options)
        if os.environ.get('HILO_JIT_COMPILE_ONLY'):
            return
        self._mt = inner
        N, nu, na = self._prediction_horizon, self._n_u, nx + 1
        d = 0 if inner._ip_ind == [] else len(inner._ip_ind[0]) // na
        ne = len(getattr(inner, '_e_soft_stage_ind', []) or [])
        # index maps of the reference's layout (mpc.py:1462-1548; the dt block last, :1606-1617)
        self._x_ind = [list(range(k * nx, (k + 1) * nx)) for k in range(N + 1)]
        off = (N + 1) * nx
        self._u_ind = [list(range(off + k * nu, off + (k + 1) * nu)) for k in range(N)]
        off += N * nu
        self._ip_ind = [list(range(off + k * d * nx, off + (k + 1) * d * nx)) for k in range(N)] if d else []
        off += N * d * nx
        self._e_soft_stage_ind = list(range(off, off + ne))
        off += ne
        self._dt_ind = list(range(off, off + N))
        self._n_v = off + N
        # columns of the inner v that survive, in the reference's order
        keep = [i for k in range(N + 1) for i in inner._x_ind[k][:nx]] + [i for k in range(N) for i in inner._u_ind[k]]
        for k in range(N):
            blk = inner._ip_ind[k] if d else []
            keep += [blk[i * na + a] for i in range(d) for a in range(nx)]
        keep += list(getattr(inner, '_e_soft_stage_ind', []) or [])
        self._mt_keep = keep
        self._mt_r = [inner._x_ind[k][nx] for k in range(N)]
        # rows of the inner lam_g: per interval [d R | d na collocation | na continuity | (terminal, last) | R]
        R = (inner._n_g - N * (d * na + na) - (self.terminal_constraint.size * (2 if self.terminal_constraint.is_soft else 1)
                                                 if self.terminal_constraint.is_set else 0)) // (N * (d + 1)) if N else 0
        TR = (self.terminal_constraint.size * (2 if self.terminal_constraint.is_soft else 1)) if self.terminal_constraint.is_set else 0
        rows, rrow, pos = [], [], 0
        for k in range(N):
            rows += list(range(pos, pos + d * R))
            pos += d * R
            for i in range(d):
                rows += list(range(pos, pos + nx))
                pos += na
            rows += list(range(pos, pos + nx))
            rrow.append(pos + nx)
            pos += na
            if k == N - 1:
                rows += list(range(pos, pos + TR))
                pos += TR
            rows += list(range(pos, pos + R))
            pos += R
        assert pos == inner._n_g, (pos, inner._n_g)
        self._mt_rows, self._mt_rrow = rows, rrow
        self._n_g = len(rows) + max(0, N - 1)
        self._nlp_setup_done = True
        self._dev = inner._dev
        self._sx, self._su = inner._sx[:nx], inner._su
        self._nth = 0

    def _optimize_min_time(self, x0, cp, kwargs):
        inner = self._mt
        host = not isinstance(x0, torch.Tensor)
        x = to_dev(x0, inner._dev)
        single = x.ndim <= 1 or (x.ndim == 2 and x.shape[1] == 1 and x.shape[0] == self._n_x and self._n_x != 1)
        x = x.reshape(1, -1) if single else x
        if x.shape[1] != self._n_x:
            raise ValueError(f"We have an issue mate, the x0 you supplied has dimension {x.shape[1]} but the model has "
                             f"{self._n_x} states.")
        xa = torch.cat([x, torch.full((x.shape[0], 1), float(np.sqrt(self._model.dt)), dtype=torch.float64, device=x.device)], dim=1)
        u = inner.optimize(xa, cp=cp)
        s = inner._nlp_solution
        v = s['x']
        r = v[:, self._mt_r]
        lam = s['lam_g']
        eta = -lam[:, self._mt_rrow[:-1]] / (2.0 * r[:, :-1])
        self._nlp_solution = {'x': torch.cat([v[:, self._mt_keep], r * r], dim=1), 'f': s['f'],
                              'lam_g': torch.cat([lam[:, self._mt_rows], eta], dim=1), 'status': s['status'],
                              'iter_count': s['iter_count'], 'kkt_error': s.get('kkt_error')}
        self._time += self._sampling_interval
        self._n_iterations += 1
        if host:                                         # the regular path's conventions: (nu x 1) for a single host state
            u = u if isinstance(u, np.ndarray) else u.cpu().numpy()
            return u.reshape(-1, 1) if single else u.reshape(-1, self._n_u)
        u = u.reshape(-1, self._n_u)
        return u[0] if single else u

    def set_custom_constraints_function(self, fun=None, lb=None, ub=None, soft=False, max_violation=np.inf):
        """optimizer.py:1180-1208: `lb <= fun(v, x_ind, u_ind) <= ub`, appended at the end of g (mpc.py:1729-1745); `v` is the
        (scaled) decision vector, `x_ind` / `u_ind` the index lists of the nodes.  Offloaded for functions that are SUMS OVER THE
        STAGES of single-stage terms (integrals, budgets, averages - the reference's own use, tests/test_NMPC.py:519-552): each
        row rides on an accumulator state of the stage-structured problem (hilo_mpc_amd/custom.py); the function is called once at
        setup() with a vector of symbols.  soft=True (mpc.py:1551-1556, :1731-1740): one slack `e_cus` per row behind the other slacks
        in v, in [0, max_violation], penalised by 1e4 e_cus^T e_cus, and TWO rows per function in g - fun - e_cus <= ub, then
        fun + e_cus >= lb."""
        if fun is None or not callable(fun):
            raise TypeError("The custom constraint must be a function fun(v, x_ind, u_ind).")
        lb = [-np.inf] if lb is None else _wrap_list(lb)                 # optimizer.py:1195-1200
        ub = [np.inf] if ub is None else _wrap_list(ub)
        if len(lb) != len(ub):
            raise ValueError("The custom constraint needs as many lower as upper bounds.")
        self._custom_constraint_fun = fun
        self._custom_constraint_fun_lb, self._custom_constraint_fun_ub = [float(v) for v in lb], [float(v) for v in ub]
        self._custom_constraint_size = len(lb)
        self._custom_constraint_is_soft_flag = bool(soft)
        mv = np.broadcast_to(np.asarray(max_violation, dtype=float).ravel(), (len(lb),)) if np.size(max_violation) in (1, len(lb)) else None
        if mv is None:
            raise ValueError("max_violation must be one value or one per custom constraint row.")
        self._custom_constraint_maximum_violation = mv.copy()
        self._custom_constraint_flag = True
        self._nlp_setup_done = False

    def get_time_variable(self):
        """mpc.py:1055-1062: the time symbol for trajectory references given as functions, `ref=[sin(t), ...]`."""
        self._time_var = Expr('t', name='t')
        return self._time_var

    def create_path_variable(self, name='theta', u_pf_lb=0.0001, u_pf_ub=1, u_pf_ref=None, u_pf_weight=10,
                             theta_guess=0, theta_lb=0, theta_ub=np.inf):
        """mpc.py:1025-1053: returns the symbol to build path references with."""
        if self._paths_var_list:
            raise NotImplementedError("one path variable per controller is offloaded")
        self._paths_var_list.append({'name': name, 'u_pf_lb': u_pf_lb, 'u_pf_ub': u_pf_ub, 'u_pf_ref': u_pf_ref,
                                     'u_pf_weight': u_pf_weight, 'theta_guess': theta_guess, 'theta_lb': theta_lb,
                                     'theta_ub': theta_ub})
        return Expr('theta', value=0, name=name)

    # ---- problem data ---------------------------------------------------------------------------------------
    def set_box_constraints(self, x_ub=None, x_lb=None, u_ub=None, u_lb=None, y_ub=None, y_lb=None, z_ub=None, z_lb=None):
        """mpc.py:619-710."""
        def chk(v, n, what):
            if v is None:
                return None
            v = _wrap_list(v)
            if len(v) != n:
                raise TypeError(f"The model has {n} {what}. You need to pass the same number of bounds.")
            return v
        self._x_ub, self._x_lb = chk(x_ub, self._n_x, 'states'), chk(x_lb, self._n_x, 'states')
        self._u_ub, self._u_lb = chk(u_ub, self._n_u, 'inputs'), chk(u_lb, self._n_u, 'inputs')
        if y_ub is not None or y_lb is not None:
            # mpc.py:703-708: measurement box constraints ARE an extra stage and terminal constraint on the measurement
            # equations (they replace whatever stage / terminal constraint was set before, like there)
            meas = self._meas_exprs()
            for b in (y_ub, y_lb):
                if b is not None and len(_wrap_list(b)) != len(meas):
                    raise TypeError(f"The model has {len(meas)} measurements. You need to pass the same number of bounds.")
            self.set_stage_constraints(stage_constraint=meas, ub=y_ub, lb=y_lb, name='measurement_constraint')
            self.set_terminal_constraints(terminal_constraint=meas, ub=y_ub, lb=y_lb, name='measurement_constraint')
        # the algebraic states are eliminated through their equations: a finite box on them (mpc.py:645-701, the box of
        # the zp blocks of v, :1512-1518) becomes hard rows on z(x_{k,i}, u_k) at the collocation points
        nza = getattr(self._model, 'n_z', 0)
        self._z_lb = None if z_lb is None else chk(np.broadcast_to(np.asarray(_wrap_list(z_lb), dtype=float), (nza,)) if np.size(z_lb) == 1
                                                   else z_lb, nza, 'algebraic states')
        self._z_ub = None if z_ub is None else chk(np.broadcast_to(np.asarray(_wrap_list(z_ub), dtype=float), (nza,)) if np.size(z_ub) == 1
                                                   else z_ub, nza, 'algebraic states')

    def _meas_exprs(self):
        """The model's measurement equations as expressions (models written as expressions; zoo models held as expressions)."""
        m = self._model
        if getattr(m, '_symbolic', False):
            if not m._meas:
                raise RuntimeError("The model has no measurement equations (set_measurement_equations)")
            return list(m._meas)
        from . import zoo_expr
        from .model import Model
        if m.name not in zoo_expr.FUNCTOR:
            raise NotImplementedError(f"measurement constraints need the measurement equations as expressions; model '{m.name}' "
                                      f"of the device zoo has none (available: {sorted(zoo_expr.FUNCTOR)})")
        return list(zoo_expr.define(Model(name=m.name + '_expr'), m.name)._meas)

    def set_initial_guess(self, x_guess=None, u_guess=None, z_guess=None):
        def chk(v, n, what):
            if v is None:
                return None
            v = _wrap_list(v)
            if len(v) != n:
                raise ValueError(f"x_guess dimension and model dimension do not match. Model {what} has dimension "
                                 f"{n} while x_guess has dimension {len(v)}")
            return v
        self._x_guess, self._u_guess = chk(x_guess, self._n_x, 'x'), chk(u_guess, self._n_u, 'u')
        self._z_guess = chk(z_guess, getattr(self._model, 'n_z', 0), 'z')

    def set_scaling(self, x_scaling=None, u_scaling=None, y_scaling=None):
        """optimizer.py:1476-1506."""
        def chk(v, n, what):
            if v is None:
                return None
            v = _wrap_list(v)
            if len(v) != n:
                raise ValueError(f"{what} scaling dimension does not match the model")
            return v
        self._x_scaling, self._u_scaling = chk(x_scaling, self._n_x, 'x'), chk(u_scaling, self._n_u, 'u')
        self._y_scaling = chk(y_scaling, getattr(self._model, 'n_y', 0), 'y')

    # ---- compact setters of the reference (same names, argument order and meaning) -------------------------------------
    def set_quadratic_stage_cost(self, states=None, cost_states=None, states_references=None, inputs=None, cost_inputs=None,
                                 inputs_references=None):
        """mpc.py:1064-1084: set-point tracking in one call."""
        if states is not None:
            self.quad_stage_cost.add_states(names=states, weights=cost_states, ref=states_references)
        if inputs is not None:
            self.quad_stage_cost.add_inputs(names=inputs, weights=cost_inputs, ref=inputs_references)

    def set_quadratic_terminal_cost(self, states=None, cost=None, references=None):
        """mpc.py:1086-1100."""
        self.quad_terminal_cost.add_states(names=states, weights=cost, ref=references)

    @staticmethod
    def _set_constraint(c, function, lb, ub, is_soft, max_violation, weight, name):
        c.constraint = function
        c.lb, c.ub = lb, ub
        c.is_soft = is_soft
        c.max_violation = None if max_violation is None or np.all(np.isinf(np.atleast_1d(max_violation))) else max_violation
        c.weight = weight
        c._name = name

    def set_stage_constraints(self, stage_constraint=None, lb=None, ub=None, is_soft=False, max_violation=np.inf, weight=None,
                              name='stage_constraint'):
        """optimizer.py:1154-1178: lb <= stage_constraint(x, u) <= ub in every stage."""
        self._set_constraint(self.stage_constraint, stage_constraint, lb, ub, is_soft, max_violation, weight, name)

    def set_terminal_constraints(self, terminal_constraint, name='terminal_constraint', lb=None, ub=None, is_soft=False,
                                 max_violation=np.inf, weight=None):
        """mpc.py:1102-1131 (note the reference's argument order: name before the bounds)."""
        self._set_constraint(self.terminal_constraint, terminal_constraint, lb, ub, is_soft, max_violation, weight, name)

    def set_nlp_options(self, *args, **kwargs):
        """optimizer.py:1388-1474 (same keys, same allow-lists, same defaults)."""
        possible = {'integration_method': ['collocation', 'rk4', 'erk', 'discrete', 'idas', 'cvodes'],
                    'solver': self._solver_name_list_nlp, 'collocation_points': ['radau', 'legendre'],
                    'objective_function': ['discrete', 'continuous'], 'warm_start': [True, False], 'degree': None,
                    'print_level': [0, 1], 'ipopt_debugger': [True, False]}
        # optimizer.py:1423-1426: the objective is the integral of the Lagrange term for a continuous model, the sum for a
        # discrete one
        opts = {'integration_method': 'collocation', 'collocation_points': 'radau', 'degree': 3, 'print_level': 1,
                'warm_start': True, 'solver': 'ipopt', 'ipopt_debugger': False,
                'objective_function': 'discrete' if self._model.discrete else 'continuous'}
        given = args[0] if (args and isinstance(args[0], dict)) else kwargs
        for k, v in (given or {}).items():
            if k not in opts:
                raise ValueError(f"The option named {k} does not exist. Possible options are {list(opts)}.")
            if possible[k] is not None and v not in possible[k]:
                raise ValueError(f"The option {k} is set to value {v} but the only allowed values are {possible[k]}.")
            opts[k] = v
        if self._model.discrete:
            if opts['integration_method'] != 'discrete':
                if given and 'integration_method' in given:
                    warnings.warn(f"The integration method is set to {opts['integration_method']} but I notice that the "
                                  f"model is in discrete time. I am overwriting and using discrete mode.")
                opts['integration_method'] = 'discrete'                      # optimizer.py:1441-1447
        else:
            if opts['integration_method'] == 'discrete':
                raise ValueError("The integration method is 'discrete' but the model is in continuous time.")
            if opts['integration_method'] in ('idas', 'cvodes'):
                # mpc.py:1421-1434 embeds SUNDIALS' adaptive integrator (CasADi's defaults: reltol 1e-6, abstol 1e-8) in the shooting
                # map.  The stand-in here is a FIXED-step map - classic Runge-Kutta with 64 sub-steps per interval (1e-8 relative per
                # interval on the benchmark's chemostat, whose RK4 error only falls below 1e-6 beyond 16 sub-steps) - with exact first
                # and second derivatives of THAT map.  No error control: a stiff model needs 'collocation' (DESIGN.md 7).
                if getattr(self._model, 'n_z', 0):
                    raise NotImplementedError("'idas' on a model with algebraic states is not offloaded: use 'collocation'")
                warnings.warn(f"integration_method '{opts['integration_method']}': SUNDIALS' adaptive integrator is replaced by a "
                              f"fixed-step Runge-Kutta map of order 4 with {self.SUNDIALS_SUBSTEPS} sub-steps per sampling interval")
            if opts['integration_method'] == 'collocation' and opts['degree'] not in (1, 2, 3, 4):
                raise NotImplementedError("collocation is built for degrees 1 to 4 (the reference's default is 3)")
        if opts['ipopt_debugger']:
            raise NotImplementedError("the IPOPT iteration callback has no device counterpart")
        self._nlp_options = opts

    def set_solver_opts(self, options=None):
        """optimizer.py:1342-1370: keys understood here: 'ipopt.tol', 'ipopt.max_iter', 'ipopt.acceptable_tol',
        'ipopt.acceptable_iter', 'ipopt.mu_init', 'ipopt.bound_relax_factor' (with or without the prefix)."""
        self._solver_options = {}
        for k, v in (options or {}).items():
            self._solver_options[k.split('.')[-1]] = v

    # ---- setup (mpc.py:1133-1801) ---------------------------------------------------------------------------
    def setup(self, options=None, solver_options=None):
        if self._prediction_horizon is None:
            raise ValueError("You must set a prediction horizon length before")
        if self._control_horizon is None:
            raise ValueError("You must set a control horizon length before.")
        if getattr(self, '_minimize_final_time_flag', False):
            return self._setup_min_time(options, solver_options)
        if not (self.quad_stage_cost._is_set or self.quad_terminal_cost._is_set or self.stage_cost._is_set or
                self.terminal_cost._is_set):
            raise ValueError("You need to define a cost function before setting up the mpc.")
        if self._control_horizon > self._prediction_horizon:
            raise ValueError("The control horizon must be smaller or equal to the prediction horizon")
        if self._nlp_options is None or options is not None:
            self.set_nlp_options(options or {})
        if solver_options is not None:
            self.set_solver_opts(solver_options)
        m = self._model
        coll = None
        if not m.discrete:
            if self._nlp_options['integration_method'] == 'collocation':
                coll = _collocation_basis(self._nlp_options['degree'], self._nlp_options['collocation_points'])
            elif self._nlp_options['integration_method'] in ('cvodes', 'idas'):
                m = m.discretize('rk4', n_sub=self.SUNDIALS_SUBSTEPS)     # the stand-in for the adaptive integrator (set_nlp_options)
            else:   # 'rk4' / 'erk': one explicit Runge-Kutta step per interval (modeling.py:1213-1281)
                m = m.discretize('rk4' if self._nlp_options['integration_method'] == 'rk4' else 'erk',
                                 order=None if self._nlp_options['integration_method'] == 'rk4' else 1)
        nx, nu = self._n_x, self._n_u
        nz = nx + nu
        sx = np.ones(nx) if self._x_scaling is None else np.asarray(self._x_scaling)
        su = np.ones(nu) if self._u_scaling is None else np.asarray(self._u_scaling)
        Wz, zref = np.zeros((nz, nz)), np.zeros(nz)
        Wdu, has_du = np.zeros((nu, nu)), False
        for kind, ind, W, ref in self.quad_stage_cost._terms:
            if kind == 'states':
                Wz[np.ix_(ind, ind)] += W
                if ref is not None:
                    zref[ind] = np.asarray(ref) / sx[ind]             # modeling.py:310
            elif kind == 'inputs':
                jj = [nx + i for i in ind]
                Wz[np.ix_(jj, jj)] += W
                if ref is not None:
                    zref[jj] = np.asarray(ref) / su[ind]
            else:
                Wdu[np.ix_(ind, ind)] += W
                has_du = True
        WN, xrefN = np.zeros((nx, nx)), np.zeros(nx)
        for kind, ind, W, ref in self.quad_terminal_cost._terms:
            if kind != 'states':
                raise TypeError("The terminal cost can only contain states")
            WN[np.ix_(ind, ind)] += W
            if ref is not None:
                xrefN[ind] = np.asarray(ref) / sx[ind]
        self._has_du = has_du
        keep = []                                                   # keep numpy buffers alive during the call

        def hp(a):
            if a is None:
                return None
            a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
            keep.append(a)
            return a.ctypes.data

        prog_fail = []

        def compile_block(exprs, theta_index=None):
            # postfix programs for the precompiled policies' interpreter; an expression it cannot hold (too deep) sends the
            # problem to the run-time compiled policy, where expressions are compiled
            try:
                return _compile_block(exprs, theta_index=theta_index)
            except (ValueError, NotImplementedError) as err:
                prog_fail.append(str(err))
                return [0.]

        d = _lib.NmpcDesc()
        d.model_id, d.N, d.Nc = m.model_id, self._prediction_horizon, self._control_horizon
        d.erk_order = m.erk_order if m.erk_order else 4
        d.n_sub = m.n_sub
        so = self._solver_options
        d.max_iter = int(so.get('max_iter', 0))
        d.acceptable_iter = int(so.get('acceptable_iter', 0))
        d.dt = m.dt
        d.tol = float(so.get('tol', 0.))
        d.acceptable_tol = float(so.get('acceptable_tol', 0.))
        d.mu_init = float(so.get('mu_init', 0.))
        d.bound_relax_factor = float(so.get('bound_relax_factor', -1.))
        d.max_hessian_perturbation = float(so.get('max_hessian_perturbation', 0.))
        d.Wz, d.zref, d.WN, d.xrefN = hp(Wz), hp(zref), hp(WN), hp(xrefN)
        d.Wdu = hp(Wdu) if has_du else None
        d.x_lb, d.x_ub, d.u_lb, d.u_ub = hp(self._x_lb), hp(self._x_ub), hp(self._u_lb), hp(self._u_ub)
        d.x_scaling, d.u_scaling = hp(self._x_scaling), hp(self._u_scaling)
        d.x_guess, d.u_guess = hp(self._x_guess), hp(self._u_guess)
        learned = getattr(m, 'learned', None)
        d.learned = learned._handle if learned is not None else None
        # ---- path following (mpc.py:1173-1204) ----
        nth = len(self._paths_var_list)
        if (self.quad_stage_cost._paths or self.quad_terminal_cost._paths) and not nth:
            raise ValueError("path references need a path variable: call create_path_variable() first")

        def hi(a):
            a = np.ascontiguousarray(np.asarray(a, dtype=np.int32))
            keep.append(a)
            return a.ctypes.data

        def path_terms(cost):
            ind, refs = [], []
            for i, W, r in cost._paths:
                ind += i
                refs += r
            n = len(ind)
            Wp = np.zeros((n, n))
            o = 0
            for i, W, r in cost._paths:
                Wp[o:o + len(i), o:o + len(i)] = W
                o += len(i)
            return ind, Wp, refs
        if nth:
            pv = self._paths_var_list[0]
            d.n_path_var = 1
            d.theta_guess, d.theta_lb, d.theta_ub = float(pv['theta_guess']), float(pv['theta_lb']), float(pv['theta_ub'])
            d.u_pf_lb, d.u_pf_ub = float(pv['u_pf_lb']), float(pv['u_pf_ub'])
            d.has_u_pf_ref = int(pv['u_pf_ref'] is not None)
            d.u_pf_ref = float(pv['u_pf_ref'] or 0.)
            d.u_pf_weight = float(pv['u_pf_weight'])
            si, sW, sr = path_terms(self.quad_stage_cost)
            ti, tW, tr = path_terms(self.quad_terminal_cost)
            d.n_path_stage, d.n_path_term = len(si), len(ti)
            d.path_stage_idx, d.path_stage_W, d.path_term_idx, d.path_term_W = hi(si), hp(sW), hi(ti), hp(tW)
            prog = compile_block(sr + tr, theta_index=nx)           # theta is state index nx (mpc.py:1181)
            d.path_prog, d.path_prog_len = hp(prog), len(prog)
        # ---- nonlinear stage constraint (modeling.py:820-1005) ----
        tc = self.terminal_constraint
        if tc.is_set:
            # hard: lb <= c_T(x_end) <= ub on the integrated end state (mpc.py:1693-1700); soft: on x_{N-1} with the slack
            # e_soft_term behind the stage slack in v (mpc.py:1540-1548, :1684-1692)
            for e in tc.constraint:
                if e.depends_on('theta') or e.depends_on('u'):
                    raise ValueError("The terminal constraint is a function of the states (and parameters) only")
            nt = tc.size
            tlb = [-np.inf] * nt if tc.lb is None else tc.lb
            tub = [np.inf] * nt if tc.ub is None else tc.ub
            if len(tlb) != nt or len(tub) != nt:
                raise ValueError("The dimensions of the terminal constraint function and its bounds are not compatible.")
            prog = compile_block(tc.constraint)
            d.n_tcon, d.tcon_prog, d.tcon_prog_len = nt, hp(prog), len(prog)
            d.tcon_lb, d.tcon_ub = hp(tlb), hp(tub)
            if tc.is_soft:
                d.tcon_soft = 1
                d.tcon_weight = hp(_constraint_weight(tc.weight, nt, 'terminal constraint')) if tc.weight is not None else None
                d.tcon_max_violation = hp(tc.max_violation) if tc.max_violation is not None else None
        sc = self.stage_constraint
        ne = 0
        if sc.is_set:
            nc = sc.size
            lb = [-np.inf] * nc if sc.lb is None else sc.lb                  # modeling.py:878-881
            ub = [np.inf] * nc if sc.ub is None else sc.ub
            if len(lb) != nc or len(ub) != nc:
                raise ValueError("The dimensions of the stage constraint function and its bounds are not compatible.")
            if any(e.depends_on('theta') for e in sc.constraint):
                # a constraint on the path variable (a state of the augmented model, mpc.py:1181-1191): the expression interpreter of
                # the precompiled variants has no slot for it - the run-time compiled policy compiles the expression in
                prog_fail.append("constraint on the path variable")
                prog = [0.]
            else:
                prog = compile_block(sc.constraint)
            d.n_con, d.con_soft = nc, int(sc.is_soft)
            d.con_prog, d.con_prog_len = hp(prog), len(prog)
            d.con_lb, d.con_ub = hp(lb), hp(ub)
            if sc.is_soft:
                ne = nc
                d.con_weight = hp(_constraint_weight(sc.weight, nc, 'stage constraint')) if sc.weight is not None else None
                d.con_max_violation = hp(sc.max_violation) if sc.max_violation is not None else None
        ne_term = tc.size if tc.is_set and tc.is_soft else 0
        self._nth, self._ne, self._ne_term = nth, ne, ne_term
        self._tv = bool(self._time_varying_parameters or self.quad_stage_cost._trajectories or
                        self.quad_terminal_cost._trajectories)
        d.time_varying = int(self._tv)
        self._zref_const, self._xrefN_const = zref.copy(), xrefN.copy()
        if coll is not None:
            d.collocation_degree = coll['d']
            d.coll_A, d.coll_D = hp(coll['A']), hp(coll['D'])
        self._coll = coll
        # HILO_JIT_COMPILE_ONLY=1 (image builds on machines without a GPU): setup() compiles the problem's kernels into the cache
        # (<library dir>/jit_cache or HILO_JIT_CACHE) and stops; the controller cannot optimize
        compile_only = bool(os.environ.get('HILO_JIT_COMPILE_ONLY'))
        self._dev = None if compile_only else device(self._dev_index)
        dev_index = 0 if compile_only else self._dev.index
        # ---- route: precompiled zoo variant, or compiled at run time (csrc/hilo_jit.hip) ----
        N, Nc = self._prediction_horizon, self._control_horizon
        cont = (not self._model.discrete) and self._nlp_options['objective_function'] == 'continuous'
        if cont and (self.quad_stage_cost._traj_funs or self.quad_terminal_cost._traj_funs):
            # the reference integrates r(t) inside the interval then; here references are per-stage data
            raise NotImplementedError("trajectory references as functions of time are offloaded for the discrete objective; pass "
                                      "options={'objective_function': 'discrete'}")
        ys = getattr(self, '_y_scaling', None)
        meas_stage, meas_term = self.quad_stage_cost._measurement_cost(ys), self.quad_terminal_cost._measurement_cost(ys)
        gen_stage = self.stage_cost._cost if meas_stage is None else \
            (meas_stage if self.stage_cost._cost is None else self.stage_cost._cost + meas_stage)
        gen_term = self.terminal_cost._cost if meas_term is None else \
            (meas_term if self.terminal_cost._cost is None else self.terminal_cost._cost + meas_term)
        generic = gen_stage is not None or gen_term is not None
        general = bool(nth or sc.is_set or tc.is_set)
        need_user = generic or Nc < N or cont or (coll is not None and (general or self._tv)) or (self._tv and general) or \
            bool(prog_fail) or bool(getattr(m, 'n_z', 0))         # (algebraic states: the general policy owns their output passes)
        sym = getattr(m, '_symbolic', False)
        if coll is not None:
            d.coll_B = hp(coll['B'])
        d.objective_continuous = int(cont)
        # ---- custom constraint function over the whole decision vector (hilo_mpc_amd/custom.py): accumulator states + terminal rows
        acc_psi, acc_term, self._nq, self._custom_const = (), (), 0, None
        if getattr(self, '_custom_constraint_flag', False):
            from .custom import decompose
            if getattr(self, '_minimize_final_time_flag', False):
                raise NotImplementedError("a custom constraint together with minimize_final_time is not offloaded")
            nxa_, nua_ = nx + nth, nu + nth
            nza_ = getattr(m, 'n_z', 0) if coll is not None else 0
            dn_ = coll['d'] * (nxa_ + nza_) if coll is not None else 0
            xi = [list(range(k * nxa_, (k + 1) * nxa_)) for k in range(N + 1)]
            ui = [list(range((N + 1) * nxa_ + k * nua_, (N + 1) * nxa_ + (k + 1) * nua_)) for k in range(Nc)]
            mc = self._custom_constraint_size
            csoft = bool(getattr(self, '_custom_constraint_is_soft_flag', False))
            if csoft and ne_term:
                raise NotImplementedError("soft custom constraints together with a soft terminal constraint are not offloaded")
            n_v_ref = (N + 1) * nxa_ + Nc * nua_ + (N + 1) * nza_ + N * dn_ + ne + ne_term + (mc if csoft else 0)
            acc_psi, coef, const = decompose(self._custom_constraint_fun, xi, ui, n_v_ref, m, mc)
            if Nc < N:
                raise NotImplementedError("a custom constraint together with a control horizon Nc < N is not offloaded")
            if any(e.depends_on('theta') for e in acc_psi):
                raise NotImplementedError("a custom constraint on the path variable is not offloaded")
            self._nq, self._custom_const = mc, const
            # stage expressions with a coefficient at stage N act on the integrated END state x_N = F(x_{N-1}, u_{N-1}): their second
            # derivatives reach the last interval's Hessian through the dynamics (J_F^T psi'' J_F)
            acc_term = tuple(acc_psi[j] for j in range(len(acc_psi)) if np.any(np.asarray(coef)[:, N, j] != 0.))
            d.n_acc, d.n_acc_expr = mc, len(acc_psi)
            d.acc_coef = hp(np.ascontiguousarray(coef, dtype=np.float64).ravel())
            d.acc_lb = hp(np.asarray(self._custom_constraint_fun_lb) - const)
            d.acc_ub = hp(np.asarray(self._custom_constraint_fun_ub) - const)
            if csoft:
                d.acc_soft = 1
                d.acc_max_violation = hp(self._custom_constraint_maximum_violation)
            need_user = True

        def jit_desc(policy):
            from . import codegen
            nza = getattr(m, 'n_z', 0)
            if nza:
                if tc.is_set:
                    raise NotImplementedError("a nonlinear terminal constraint on a DAE model is not offloaded")
                if coll is None and self._model.discrete:
                    raise NotImplementedError("algebraic states of a pre-discretised model are not offloaded: hand the continuous model "
                                              "over and use 'collocation' (the reference's default) or 'rk4' / 'erk'")
                if coll is None:
                    # explicit Runge-Kutta ('rk4' / 'erk', mpc.py:1375-1412): a block of algebraic variables per STAGE, whose equations
                    # the reference evaluates at the stage's slope (modeling.py:1268) - restated as it is (codegen.py, alg_at_slope);
                    # built for the shape of the reference's own case (tests/test_NMPC.py:1950-1975): quadratic costs and boxes
                    if sc.is_set or nth or getattr(self, '_custom_constraint_flag', False) or self._control_horizon < self._prediction_horizon:
                        raise NotImplementedError("algebraic states under an explicit Runge-Kutta transcription are offloaded for quadratic "
                                                  "costs and box constraints; use 'collocation' (the reference's default) for the rest")
                    zl = getattr(self, '_z_lb', None)
                    zu = getattr(self, '_z_ub', None)
                    if (zl is not None and np.any(np.isfinite(zl))) or (zu is not None and np.any(np.isfinite(zu))):
                        warnings.warn("bounds on algebraic states under an explicit Runge-Kutta transcription are not enforced by the "
                                      "device solver (the stage variables are eliminated); check the returned zp values")
                src = m.user_source(z_guess=getattr(self, '_z_guess', None), alg_at_slope=coll is None)
                d.user_nz = nza
            else:
                src = m.user_source()
            if policy == 2:
                zb = []                      # bounded algebraic states: expressions behind the constraint's, rows at the collocation points
                if nza and coll is not None:
                    zl = [-np.inf] * nza if getattr(self, '_z_lb', None) is None else list(self._z_lb)
                    zu = [np.inf] * nza if getattr(self, '_z_ub', None) is None else list(self._z_ub)
                    zb = [a for a in range(nza) if np.isfinite(zl[a]) or np.isfinite(zu[a])]
                    if zb:
                        d.n_zbound = len(zb)
                        d.zb_lb, d.zb_ub = hp([zl[a] for a in zb]), hp([zu[a] for a in zb])
                src += codegen.fun_source(
                    nx, stage=gen_stage, term=gen_term,
                    con=(list(sc.constraint) if sc.is_set else []) + [m.z[a] for a in zb], tcon=tc.constraint if tc.is_set else (),
                    path_stage=[r for _, _, rr in self.quad_stage_cost._paths for r in rr],
                    path_term=[r for _, _, rr in self.quad_terminal_cost._paths for r in rr], acc=list(acc_psi))
                d.user_has_fun = 1
                d.path_prog, d.path_prog_len = None, 0          # expressions are compiled in, not interpreted
                d.con_prog, d.con_prog_len, d.tcon_prog, d.tcon_prog_len = None, 0, None, 0
                pat = self._hessian_pattern(m, nx, nu, nth, Wz, Wdu if has_du else None, gen_stage, sc, tc,
                                            composed=bool(cont or coll is not None), extra=[m.z[a] for a in zb] + list(acc_psi),
                                            extra_composed=list(acc_term))
                if pat is not None:
                    pat = np.ascontiguousarray(pat, dtype=np.uint8)
                    keep.append(pat)
                    d.hess_pattern = pat.ctypes.data
                self._hess_pattern = pat
            self._user_source = src
            d.user_source = src.encode()
            d.x0_free_mask = int(getattr(self, '_x0_free_mask', 0))
            d.user_policy = policy
            d.user_nx, d.user_nu, d.user_np, d.user_ny = m.n_x, m.n_u, m.n_p, m.n_y
            d.user_discrete = int(getattr(m, '_native_discrete', False))
            gps = list(getattr(m, '_gps', []))
            d.n_user_gp = len(gps)
            for k, g in enumerate(gps):
                # (compile-only mode never dereferences the handles: any non-NULL value)
                d.user_gp[k] = 1 if os.environ.get('HILO_JIT_COMPILE_ONLY') else \
                    (g._handle.value if hasattr(g._handle, 'value') else g._handle)

        h = C.c_void_p()
        # Problems with a path variable or nonlinear constraints: the run-time compiled general policy (expressions compiled
        # in, horizon a compile-time constant) is the default - measured 1.8x faster than the precompiled variants with their
        # expression interpreter on C5 (218 vs 392 ms per 8192-instance step) at the price of seconds of hiprtc at the first
        # setup() of a problem structure (cached on disk afterwards).  HILO_NMPC_BACKEND=precompiled keeps the library's variants.
        backend = os.environ.get('HILO_NMPC_BACKEND', 'auto')
        if backend not in ('auto', 'precompiled', 'runtime'):
            raise ValueError(f"HILO_NMPC_BACKEND must be auto, precompiled or runtime (got '{backend}')")
        if getattr(m, 'learned', None) is None and not sym and m.name in ZOO_FUNCTOR_NAMES and \
                (backend == 'runtime' or (backend == 'auto' and general and not prog_fail)):
            need_user = True
        if sym or need_user:
            if getattr(m, 'learned', None) is not None:
                raise NotImplementedError("a learned term inside a run-time compiled problem is not offloaded")
            jit_desc(2 if (need_user or general or coll is not None or self._tv) else 0)
            rc = _lib.lib().hilo_nmpc_create(C.byref(d), dev_index, C.byref(h))
        else:
            rc = _lib.lib().hilo_nmpc_create(C.byref(d), dev_index, C.byref(h))
            if rc == -4 and getattr(m, 'learned', None) is None:
                # no precompiled variant for this combination of features: compile the general policy for the zoo functor
                jit_desc(2)
                rc = _lib.lib().hilo_nmpc_create(C.byref(d), dev_index, C.byref(h))
        self._jit = bool(d.user_source)
        if compile_only:
            if rc not in (0, _lib.COMPILED_ONLY) and self._jit:
                _lib.check(rc)
            if rc == 0:                                    # (a machine WITH a GPU and a precompiled variant: nothing to compile)
                _lib.lib().hilo_nmpc_destroy(h)
            self._nlp_setup_done = False
            self._sx, self._su = sx, su
            return
        _lib.check(rc)
        self._destroy()
        self._handle = h
        dims = [C.c_int() for _ in range(5)]
        _lib.check(_lib.lib().hilo_nmpc_dims(h, *[C.byref(v) for v in dims]))
        # (with a custom constraint the engine's rows of v end with its hidden accumulator values; `_n_v` is the reference's n_v)
        self._n_v_eng = dims[0].value
        self._n_v, self._n_g = dims[0].value - self._nq, dims[1].value
        self._g_order = None
        if self._nq:
            # the engine's lam_g / g carry the custom rows as the last terminal rows, in front of the last node's stage rows; the
            # reference appends them to g (mpc.py:1729-1745)
            R = (2 * sc.size if sc.is_soft else sc.size) if sc.is_set else 0
            nqr = self._nq_rows = (2 if getattr(self, '_custom_constraint_is_soft_flag', False) else 1) * self._nq    # mpc.py:1733-1739
            cus = list(range(self._n_g - R - nqr, self._n_g - R))
            self._g_order = [i for i in range(self._n_g) if i not in set(cus)] + cus
        N, Nc = self._prediction_horizon, self._control_horizon
        # integer bookkeeping of mpc.py:1464-1537 (bit-exact index maps); a path variable is a state + an input;
        # the control horizon holds Nc input blocks (mpc.py:1476-1485)
        nxa, nua = nx + nth, nu + nth
        self._x_ind = [list(range(k * nxa, (k + 1) * nxa)) for k in range(N + 1)]
        self._u_ind = [list(range((N + 1) * nxa + k * nua, (N + 1) * nxa + (k + 1) * nua)) for k in range(Nc)]
        dn = coll['d'] * nxa if coll is not None else 0
        nza = getattr(m, 'n_z', 0) if (coll is not None or getattr(m, '_symbolic', False)) else 0
        # algebraic variables per interval: one block per collocation point, or per stage of the explicit Runge-Kutta scheme (mpc.py:1322, :1394)
        zblocks = coll['d'] if coll is not None else (m.erk_order if m.erk_order else 4)
        off = (N + 1) * nxa + Nc * nua
        # the slacks of the soft constraints come LAST in v (mpc.py:1529-1548 follows the algebraic and collocation blocks, :1488-1527)
        eoff = off + (N + 1) * nza + N * (dn + zblocks * nza)
        self._e_soft_stage_ind = list(range(eoff, eoff + ne))
        self._e_soft_term_ind = list(range(eoff + ne, eoff + ne + ne_term))                               # mpc.py:1542-1543
        ne_cus = self._nq if (self._nq and getattr(self, '_custom_constraint_is_soft_flag', False)) else 0
        self._e_cus_ind = list(range(eoff + ne + ne_term, eoff + ne + ne_term + ne_cus))                    # mpc.py:1551-1556
        # algebraic states: node blocks z_0..z_N behind the slacks' predecessors, then per interval [ip_k | zp_k] (mpc.py:1488-1518)
        self._z_ind = [list(range(off + k * nza, off + (k + 1) * nza)) for k in range(N + 1)] if nza else []
        off += (N + 1) * nza
        dz = zblocks * nza
        self._ip_ind = [list(range(off + k * (dn + dz), off + k * (dn + dz) + dn)) for k in range(N)] if dn else []   # mpc.py:1501-1509
        self._zp_ind = [list(range(off + k * (dn + dz) + dn, off + (k + 1) * (dn + dz))) for k in range(N)] if dz else []
        self._sx, self._su = sx, su
        self._nlp_setup_done = True

    def _destroy(self):
        if self._handle is not None:
            _lib.lib().hilo_nmpc_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass

    # ---- optimize (mpc.py:744-857) --------------------------------------------------------------------------
    def optimize(self, x0, cp=None, tvp=None, v0=None, runs=0, fix_x0=True, **kwargs):
        if not self._nlp_setup_done:
            raise ValueError("Howdy! You need to setup the MPC before optimizing. Run .setup() on the MPC object.")
        if getattr(self, '_mt', None) is not None:
            if v0 is not None or runs != 0 or not fix_x0 or tvp is not None:
                raise NotImplementedError("minimize_final_time: v0 / runs / fix_x0=False / tvp are not built")
            return self._optimize_min_time(x0, cp, kwargs)
        if runs != 0:
            return self._multi_start(x0, cp, tvp, v0, int(runs), fix_x0, kwargs)
        box = None
        if not fix_x0 and (kwargs.get('x0_lb') is not None or kwargs.get('x0_ub') is not None):
            # mpc.py:803-807: x_0 is a variable inside its own box instead of the state box
            box = [None if kwargs.get(k) is None else np.ascontiguousarray(_wrap_list(kwargs[k]), dtype=np.float64)
                   for k in ('x0_lb', 'x0_ub')]
            for b in box:
                if b is not None and b.size != self._n_x:
                    raise ValueError(f"x0_lb / x0_ub must have {self._n_x} entries")
        _lib.check(_lib.lib().hilo_nmpc_set_x0_box(self._handle, *[None if (box is None or b is None) else b.ctypes.data
                                                                    for b in (box or [None, None])]))
        _lib.check(_lib.lib().hilo_nmpc_set_fix_x0(self._handle, int(bool(fix_x0))))     # mpc.py:797-807
        if tvp is not None and not self._time_varying_parameters:
            raise ValueError("tvp values were passed but no parameter was declared time varying "
                             "(set_time_varying_parameters)")
        host = not isinstance(x0, torch.Tensor)
        x = to_dev(x0, self._dev)
        single = x.ndim <= 1 or (x.ndim == 2 and x.shape[1] == 1 and x.shape[0] == self._n_x and self._n_x != 1)
        x = x.reshape(1, -1) if single else x
        if x.shape[1] != self._n_x:
            raise ValueError(f"We have an issue mate, the x0 you supplied has dimension {x.shape[1]} but the model has "
                             f"{self._n_x} states.")
        B = x.shape[0]
        sd = None
        if getattr(self, '_tv', False):
            sd = to_dev(self._stage_table(cp, tvp, kwargs), self._dev).contiguous()
            p, ps = None, 0
        elif self._n_p != 0:
            if cp is None:
                raise ValueError(f"The model has {self._n_p} constant parameter(s): {self._model.parameter_names}. "
                                 f"You must pass me the value of these before running the optimization to the 'cp' "
                                 f"parameter.")
            p = to_dev(cp, self._dev)
            p = p.reshape(1, -1) if p.ndim <= 1 else p
            if p.shape[1] != self._n_p or p.shape[0] not in (1, B):
                raise ValueError(f"The model has {self._n_p} constant parameter(s): {self._model.parameter_names}. "
                                 f"You must pass me the value of these before running the optimization to the 'cp' "
                                 f"parameter.")
            ps = 0 if p.shape[0] == 1 else self._n_p
        else:
            if cp is not None:
                warnings.warn("You are passing a parameter vector in the optimizer, but the model has no defined "
                              "parameters. I am ignoring the vector.")
            p, ps = None, 0
        pt = getattr(self, '_plant_table', None)
        if pt is not None:
            # the solve advances the attached plant state in place (set_plant_buffer): only the loop that attached it may call
            rows = pt.reshape(-1, self._n_x).shape[0]
            if rows != B:
                raise ValueError(f"optimize() for {B} instance(s) while a plant buffer of {rows} row(s) is attached "
                                 f"(set_plant_buffer): the solve would write x+ of instance b to row b of that buffer. Detach it "
                                 f"with set_plant_buffer(None) first.")
            if kwargs.get('_in_multi_start'):
                raise ValueError("optimize(runs > 0) solves several times and would advance the attached plant state (set_plant_buffer) "
                                 "once per run. Detach it with set_plant_buffer(None) first.")
        v0t = None
        wo = getattr(self, '_warm_override', None)          # best run of a multi-start call: the next call's start vector
        self._warm_override = None
        if v0 is None and wo is not None and wo.shape[0] == B and self._nlp_options['warm_start'] and not kwargs.get('_in_multi_start'):
            v0 = wo
        if v0 is not None:
            v0t = to_dev(v0, self._dev).reshape(-1, self._n_v)
            if v0t.shape[0] == 1 and B > 1:
                v0t = v0t.expand(B, -1).contiguous()
            if self._nq:                                   # hidden accumulator entries of the engine's rows: they start at zero
                v0t = torch.cat([v0t, torch.zeros(v0t.shape[0], self._nq, dtype=torch.float64, device=v0t.device)], dim=1).contiguous()
        elif not self._nlp_options['warm_start']:
            _lib.check(_lib.lib().hilo_nmpc_reset_warm_start(self._handle))
        u_old = None
        if self._has_du:
            # mpc.py:488-493: previous first input, or the guess on the very first call (scaled);
            # `u_old=` (scaled, [B, nu]) overrides the internal memory (batched drivers that re-order instances)
            if kwargs.get('u_old') is not None:
                u_old = to_dev(kwargs['u_old'], self._dev).reshape(-1, self._n_u)
                u_old = (u_old.expand(B, -1) if u_old.shape[0] == 1 else u_old).contiguous()
            elif self._u_prev is not None and self._u_prev.shape[0] == B:
                u_old = self._u_prev
            else:
                g = np.zeros(self._n_u) if self._u_guess is None else np.asarray(self._u_guess) / self._su
                u_old = to_dev(np.tile(g, (B, 1)), self._dev)
        dev = self._dev
        v_opt = torch.empty(B, self._n_v_eng, dtype=torch.float64, device=dev)
        f_opt = torch.empty(B, dtype=torch.float64, device=dev)
        lam_g = torch.empty(B, self._n_g, dtype=torch.float64, device=dev)
        u0 = torch.empty(B, self._n_u, dtype=torch.float64, device=dev)
        status = torch.empty(B, dtype=torch.int32, device=dev)
        iters = torch.empty(B, dtype=torch.int32, device=dev)
        kkt = torch.empty(B, dtype=torch.float64, device=dev)
        # the reference keeps the whole solver result (mpc.py:722-723): constraint values g and bound multipliers lam_x too.
        # Opt-in here (`keep_full_solution = True`): two more result vectors per instance that a control loop never reads.
        # Layouts with a collocation output pass return them as zeros.
        # lbx / ubx of THIS call (`v_lb=` / `v_ub=`: [n_v] or [B, n_v], scaled like v) - the reference passes its bound vectors
        # with every solver call (mpc.py:722) and moves entries between calls (mpc.py:797-807); None keeps the setup's bounds
        vlb, vub = kwargs.get('v_lb'), kwargs.get('v_ub')
        if (vlb is None) != (vub is None):
            raise ValueError("pass both v_lb and v_ub (the solver call's lbx and ubx) or neither")
        if vlb is not None:
            vlb = to_dev(vlb, self._dev).reshape(-1, self._n_v)
            vub = to_dev(vub, self._dev).reshape(-1, self._n_v)
            vlb = (vlb.expand(B, -1) if vlb.shape[0] == 1 else vlb).contiguous()
            vub = (vub.expand(B, -1) if vub.shape[0] == 1 else vub).contiguous()
            if vlb.shape[0] != B or vub.shape[0] != B:
                raise ValueError(f"v_lb / v_ub need one row or {B} rows of {self._n_v} entries")
            if self._nq:
                inf = torch.full((B, self._nq), float('inf'), dtype=torch.float64, device=vlb.device)
                vlb, vub = torch.cat([vlb, -inf], dim=1).contiguous(), torch.cat([vub, inf], dim=1).contiguous()
        _lib.check(_lib.lib().hilo_nmpc_set_var_bounds(self._handle, ptr(vlb), ptr(vub)))
        g_val = lam_x = None
        if self._full_solution:
            g_val = torch.zeros(B, self._n_g, dtype=torch.float64, device=dev)
            lam_x = torch.zeros(B, self._n_v_eng, dtype=torch.float64, device=dev)
        _lib.check(_lib.lib().hilo_nmpc_set_aux_outputs(self._handle, ptr(g_val), ptr(lam_x)))
        t0 = time.time() if self._stats else None
        if sd is not None:
            _lib.check(_lib.lib().hilo_nmpc_solve_tv(self._handle, B, ptr(x.contiguous()), ptr(sd), 0, ptr(v0t), ptr(u_old),
                                                     ptr(v_opt), ptr(f_opt), ptr(lam_g), ptr(u0), ptr(status), ptr(iters),
                                                     ptr(kkt), stream_ptr(dev)))
        else:
            _lib.check(_lib.lib().hilo_nmpc_solve(self._handle, B, ptr(x.contiguous()), ptr(p), ps, ptr(v0t), ptr(u_old),
                                                  ptr(v_opt), ptr(f_opt), ptr(lam_g), ptr(u0), ptr(status), ptr(iters),
                                                  ptr(kkt), stream_ptr(dev)))
        if self._nq:       # the reference's layouts: no accumulator entries in v, the custom rows at the end of g (+ their constant parts)
            v_opt, lam_g = v_opt[:, :self._n_v], lam_g[:, self._g_order]
            soft_rows = self._nq_rows - self._nq          # the engine's row -(fun + e_cus) <= -lb is the reference's fun + e_cus >= lb
            if soft_rows:
                lam_g[:, -soft_rows:] = -lam_g[:, -soft_rows:]
            if self._full_solution:
                g_val, lam_x = g_val[:, self._g_order].clone(), lam_x[:, :self._n_v]
                if soft_rows:
                    g_val[:, -soft_rows:] = -g_val[:, -soft_rows:]
                g_val[:, -self._nq_rows:] += torch.as_tensor(np.tile(self._custom_const, self._nq_rows // self._nq), dtype=torch.float64,
                                                             device=dev)
        self._nlp_solution = {'x': v_opt, 'f': f_opt, 'lam_g': lam_g, 'status': status, 'iter_count': iters, 'kkt_error': kkt}
        if self._full_solution:
            self._nlp_solution.update(g=g_val, lam_x=lam_x)
        if self._has_du:
            self._u_prev = v_opt[:, self._u_ind[0][:self._n_u]].contiguous()
        if self._ne:
            self.stage_constraint.e_soft_value = v_opt[:, self._e_soft_stage_ind]        # mpc.py:833-834
        if self._ne_term:
            self.terminal_constraint.e_soft_value = v_opt[:, self._e_soft_term_ind]      # mpc.py:840-841
        if self._stats:
            torch.cuda.synchronize(dev)
            self._extime = time.time() - t0
        self._time += self._sampling_interval            # mpc.py:850
        self._n_iterations += 1                          # mpc.py:853
        if host:
            u = u0.cpu().numpy()
            return u.reshape(-1, 1) if single else u     # single instance: (nu x 1) like the reference's DM
        return u0[0] if single else u0

    def _hessian_pattern(self, m, nx, nu, nth, Wz, Wdu, gen_stage, sc, tc, composed=False, extra=(), extra_composed=()):
        """Structural sparsity of the interval Hessian over the augmented z = [x, theta | u, u_theta] (hilo_mpc_amd/sparsity.py),
        or None (dense) when the model has no expression form."""
        from . import zoo_expr
        from .model import Model
        from .sparsity import stage_hessian_pattern
        if getattr(m, '_gps', None):
            return None
        elim = None
        if getattr(m, '_symbolic', False):
            ode = m._ode
            if getattr(m, 'n_z', 0):
                # algebraic states are eliminated through their equations, z = zeta(x, u): for the structure every one of them
                # stands for a generic nonlinear function of the states and inputs ANY algebraic equation names (conservative)
                from .expr import hessian_structure
                dep = set()
                for e in m._alg:
                    dep |= {k for k in hessian_structure(e)[0] if k[0] in ('x', 'u')}
                if not dep:
                    return None
                tot = None
                for kind, i in sorted(dep):
                    leaf = (m.x if kind == 'x' else m.u)[i]
                    tot = leaf if tot is None else tot + leaf
                surrogate = tot * tot
                elim = lambda n: surrogate if n.op == 'z' else None        # noqa: E731
                ode = Expr.substitute(list(ode), elim)
        elif m.name in zoo_expr.FUNCTOR or m.name in zoo_expr.STRUCTURE_ONLY:
            ode = zoo_expr.define(Model(name=m.name + '_structure'), m.name)._ode
        else:
            return None
        mza = nx + nth + nu + nth
        az = lambda i: i if i < nx else nx + nth + (i - nx)            # noqa: E731  model z -> augmented z
        Wa = np.zeros((mza, mza))
        W = np.asarray(Wz, dtype=float).reshape(nx + nu, nx + nu)
        for i in range(nx + nu):
            for j in range(nx + nu):
                Wa[az(i), az(j)] = W[i, j]
        # stage constraints act at the node (mpc.py:1700-1725; with collocation also at the collocation states: composed);
        # a hard terminal constraint on the integrated end state (mpc.py:1693-1700), a soft one at the node x_{N-1}
        # (`extra`: the rows of bounded algebraic states - z itself, i.e. after the elimination the surrogate of every z: their
        # multiplier-weighted second derivatives belong to the interval Hessian like those of any other row)
        exprs = [gen_stage] + (list(sc.constraint) if sc.is_set else []) + (list(tc.constraint) if tc.is_set and tc.is_soft else []) + \
            list(extra)
        exprs_c = (list(tc.constraint) if tc.is_set and not tc.is_soft else []) + list(extra_composed)
        if elim is not None:
            exprs = [None if e is None else Expr.substitute([Expr.wrap(e)], elim)[0] for e in exprs]
            exprs_c = [Expr.substitute([Expr.wrap(e)], elim)[0] for e in exprs_c]
        terms, o, Wp = [], 0, None
        if nth:
            ind, refs = [], []
            for i, W_, r in self.quad_stage_cost._paths:
                ind += list(i)
                refs += list(r)
            Wp = np.zeros((len(ind), len(ind)))
            for i, W_, r in self.quad_stage_cost._paths:
                Wp[o:o + len(i), o:o + len(i)] = W_
                o += len(i)
            terms = list(zip(ind, refs))
        return stage_hessian_pattern(ode, nx, nu, nth, discrete=bool(getattr(m, '_native_discrete', False)), Wz=Wa, Wdu=Wdu,
                                     exprs=exprs, path_terms=terms, path_weights=Wp, composed=composed, exprs_composed=exprs_c)

    def _multi_start(self, x0, cp, tvp, v0, runs, fix_x0, kwargs):
        """mpc.py:727-741: `runs` solves, the first from the given start, the following from `v0 (1 + (1 - 2 rand) pert_factor)`
        clipped to the bounds; per instance the best objective among the solves that ended with status 1 or 2 is kept.  The
        reference draws from the unseeded numpy generator; here `seed=` (default 0) makes the draws reproducible."""
        pert = float(kwargs.get('pert_factor', 0.1))
        prev = self._nlp_solution
        warm = prev['x'].clone() if (prev is not None and self._nlp_options.get('warm_start', True)) else None
        gen = torch.Generator(device='cpu').manual_seed(int(kwargs.get('seed', 0)))
        kw = {k: v for k, v in kwargs.items() if k not in ('pert_factor', 'seed')}
        n_it, t_it = self._n_iterations, self._time
        u_prev = self._u_prev           # every run solves the SAME problem: the previous input of the change penalty is fixed
        best = None
        start = v0
        for r in range(runs):
            self._n_iterations, self._time = n_it, t_it               # one optimize() as far as the counters go
            self._u_prev = u_prev
            u = self.optimize(x0, cp=cp, tvp=tvp, v0=start, runs=0, fix_x0=fix_x0, _in_multi_start=True, **kw)
            sol = self._nlp_solution
            ok = (sol['status'] == 1) | (sol['status'] == 2)
            if best is None:
                best = {k: v.clone() for k, v in sol.items()}
                best['u0'] = torch.as_tensor(np.asarray(u).reshape(len(ok), -1), device=self._dev) if not isinstance(u, torch.Tensor) else u.reshape(len(ok), -1).clone()
                # perturbation base (mpc.py:735): the start vector of the first run - the caller's v0, else the warm start of
                # the previous call, else the initial guess
                if v0 is not None:
                    base = to_dev(v0, self._dev).reshape(-1, self._n_v).clone()
                elif warm is not None and warm.shape[0] == len(ok):
                    base = warm
                else:
                    base = self._guess_vector(len(ok))
                best_ok = ok.clone()
                take = torch.zeros_like(ok)
            else:
                take = ok & (~best_ok | (sol['f'] < best['f']))
                un = torch.as_tensor(np.asarray(u).reshape(len(ok), -1), device=self._dev) if not isinstance(u, torch.Tensor) else u.reshape(len(ok), -1)
                for k in sol:
                    best[k][take] = sol[k][take]
                best['u0'][take] = un[take]
                best_ok |= ok
            lb, ub = self._v_bounds()
            rnd = torch.rand(base.shape, generator=gen, dtype=torch.float64).to(self._dev)
            start = torch.minimum(torch.maximum(base + base * (1 - 2 * rnd) * pert, lb), ub)
        u0 = best.pop('u0')
        self._nlp_solution = best
        # the memory of the next call belongs to the BEST run (mpc.py:739-741 sets `_v0` from it): previous input and warm start
        if self._has_du:
            self._u_prev = best['x'][:, self._u_ind[0][:self._n_u]].contiguous()
        self._warm_override = best['x']
        host = not isinstance(x0, torch.Tensor)
        single = u0.shape[0] == 1 and np.ndim(x0) <= 1
        if host:
            un = u0.cpu().numpy()
            return un.reshape(-1, 1) if single else un
        return u0[0] if single else u0

    def _guess_vector(self, B):
        """The tiled initial guess in the reference's v layout (mpc.py:1468-1482), scaled."""
        N, Nc, nx, nu, nth = self._prediction_horizon, self._control_horizon, self._n_x, self._n_u, self._nth
        xg = np.zeros(nx) if self._x_guess is None else np.asarray(self._x_guess) / self._sx
        ug = np.zeros(nu) if self._u_guess is None else np.asarray(self._u_guess) / self._su
        pv = self._paths_var_list[0] if nth else None
        xa = np.concatenate([xg, [pv['theta_guess']] if nth else []])
        ua = np.concatenate([ug, [pv['u_pf_lb'] + 0.0001] if nth else []])
        v = np.zeros(self._n_v)
        v[:(N + 1) * (nx + nth)] = np.tile(xa, N + 1)
        v[(N + 1) * (nx + nth):(N + 1) * (nx + nth) + Nc * (nu + nth)] = np.tile(ua, Nc)
        for ind in self._ip_ind:
            v[ind] = np.tile(xa, len(ind) // (nx + nth))
        zg = getattr(self, '_z_guess', None)
        if zg is not None:
            for ind in getattr(self, '_z_ind', []) + getattr(self, '_zp_ind', []):
                v[ind] = np.tile(np.asarray(zg, dtype=float), len(ind) // len(zg))
        if getattr(self, '_e_cus_ind', []):
            v[self._e_cus_ind] = len(self._e_cus_ind)                      # mpc.py:1555: the size where the other slacks get zeros
        return to_dev(np.tile(v, (B, 1)), self._dev)

    def _v_bounds(self):
        """lbx / ubx of the reference's solver call (mpc.py:722) as device vectors [n_v] (scaled)."""
        N, Nc, nx, nu, nth = self._prediction_horizon, self._control_horizon, self._n_x, self._n_u, self._nth
        inf = np.inf
        xl = np.full(nx, -inf) if self._x_lb is None else np.asarray(self._x_lb) / self._sx
        xu = np.full(nx, inf) if self._x_ub is None else np.asarray(self._x_ub) / self._sx
        ul = np.full(nu, -inf) if self._u_lb is None else np.asarray(self._u_lb) / self._su
        uu = np.full(nu, inf) if self._u_ub is None else np.asarray(self._u_ub) / self._su
        pv = self._paths_var_list[0] if nth else None
        xl, xu = np.concatenate([xl, [pv['theta_lb']] if nth else []]), np.concatenate([xu, [pv['theta_ub']] if nth else []])
        ul, uu = np.concatenate([ul, [pv['u_pf_lb']] if nth else []]), np.concatenate([uu, [pv['u_pf_ub']] if nth else []])
        lb, ub = np.full(self._n_v, -inf), np.full(self._n_v, inf)
        nxa, nua = nx + nth, nu + nth
        lb[:(N + 1) * nxa], ub[:(N + 1) * nxa] = np.tile(xl, N + 1), np.tile(xu, N + 1)
        lb[(N + 1) * nxa:(N + 1) * nxa + Nc * nua], ub[(N + 1) * nxa:(N + 1) * nxa + Nc * nua] = np.tile(ul, Nc), np.tile(uu, Nc)
        for ind in (self._e_soft_stage_ind, self._e_soft_term_ind, getattr(self, '_e_cus_ind', [])):
            lb[ind] = 0.
        if getattr(self, '_e_cus_ind', []):
            ub[self._e_cus_ind] = self._custom_constraint_maximum_violation
        for ind in self._ip_ind:
            lb[ind], ub[ind] = np.tile(xl, len(ind) // nxa), np.tile(xu, len(ind) // nxa)
        return to_dev(lb, self._dev), to_dev(ub, self._dev)

    def _stage_table(self, cp, tvp, kwargs):
        """[(N+1), nz + np]: per stage [zref_k / scaling | p_k]; row N = terminal reference (first nx entries).
        References: mpc.py:365-463 (`ref_sc` / `ref_tc`: one value = constant, else the window
        [n_iterations, n_iterations + N) and the terminal sample n_iterations + N), divided by the scaling like
        modeling.py:329.  Parameters: mpc.py:335-364 + optimizer.py:905-929 (`cp` holds the NON time-varying parameters in
        model order; the rows of the tvp window are consumed in model order)."""
        N, nx, nu, npar = self._prediction_horizon, self._n_x, self._n_u, self._n_p
        nz = nx + nu
        tab = np.zeros((N + 1, nz + npar))
        tab[:N, :nz] = self._zref_const
        tab[N, :nx] = self._xrefN_const
        ci = self._n_iterations

        def window(traj, name, terminal):
            t = _wrap_list(traj)
            if len(t) == 1:
                return t[0] if terminal else np.full(N, t[0])
            if ci + N >= len(t):
                raise ValueError(f"The length of the varying reference must be one or longer than than the simulation time "
                                 f"plus the prediction horizon. Please supply data points. The trajectory is long {len(t)} "
                                 f"but I am predicting at least up to the {ci + N + 1} step.")
            return t[ci + N] if terminal else np.asarray(t[ci:ci + N])
        for cost, key, terminal in ((self.quad_stage_cost, 'ref_sc', False), (self.quad_terminal_cost, 'ref_tc', True)):
            if not cost._trajectories:
                continue
            ref = kwargs.get(key)
            if ref is None:
                if cost.name_open_varying_trajectories:
                    raise ValueError(f"Mate, it looks like the variable(s) {cost.name_open_varying_trajectories} must follow "
                                     f"a reference, but you did not pass any. Please pass a reference as a function in the "
                                     f"cost or as values in optimize({key}=...).")
                ref = {}
            if not isinstance(ref, dict):
                raise TypeError("The trajectory must be a dict with as key the name of the variables that have a trajectory.")
            for k_ in ref:
                if k_ not in cost.name_open_varying_trajectories:
                    raise ValueError(f"I cannot find the variable {k_} in the variables with varying trajectory. The "
                                     f"trajectories without reference are {', '.join(cost.name_open_varying_trajectories)}")
            for kind, names, ind in cost._trajectories:
                for name, i in zip(names, ind):
                    col = i if kind == 'states' else nx + i
                    sc = self._sx[i] if kind == 'states' else self._su[i]
                    if name in cost._traj_funs:
                        # function of time: stage k sees r(t_0 + k dt), the terminal term r(t_0 + N dt) (mpc.py:1649-1727: `time`
                        # starts at the controller's clock and advances by the sampling interval per stage)
                        f, dt = cost._traj_funs[name], self._sampling_interval
                        if terminal:
                            tab[N, col] = _eval_time(f, self._time + N * dt) / sc
                        else:
                            tab[:N, col] = [_eval_time(f, self._time + k_ * dt) / sc for k_ in range(N)]
                        continue
                    if terminal:
                        tab[N, col] = window(ref[name], name, True) / sc
                    else:
                        tab[:N, col] = window(ref[name], name, False) / sc
        if npar:
            names = self._model.parameter_names
            n_tvp = len(self._time_varying_parameters)
            cpv = np.zeros(0) if cp is None else np.asarray(cp.cpu() if isinstance(cp, torch.Tensor) else cp, dtype=float).ravel()
            if cpv.size != npar - n_tvp:
                raise ValueError(f"The model has {npar - n_tvp} constant parameter(s): "
                                 f"{[n for n in names if n not in self._time_varying_parameters]}. You must pass me the "
                                 f"value of these before running the optimization to the 'cp' parameter.")
            win = np.zeros((n_tvp, N))
            if n_tvp:
                if tvp is not None:                                              # mpc.py:341-354
                    for r, (key, value) in enumerate(tvp.items()):
                        if len(value) < N:
                            raise TypeError(f"When passing time-varying parameters, you need to pass a number of values at "
                                            f"least as long as the prediction horizon. The parameter {key} has {len(value)} "
                                            f"values but the MPC has a prediction horizon length of {N}.")
                        win[r] = np.asarray(value[0:N], dtype=float)
                elif self._time_varying_parameters_values is not None:           # mpc.py:292-333
                    vals = self._time_varying_parameters_values
                    if ci == 0 or getattr(self, '_tvp_window', None) is None:
                        for r, (key, value) in enumerate(vals.items()):
                            if len(value) < N:
                                raise TypeError(f"The parameter {key} has {len(value)} values but the MPC has a prediction "
                                                f"horizon length of {N}.")
                            win[r] = np.asarray(value[0:N], dtype=float)
                    else:
                        win = self._tvp_window.copy()
                        win[:, :-1] = win[:, 1:]
                        for r, name in enumerate(self._time_varying_parameters):
                            value = vals[name]
                            if ci + N > len(value):
                                warnings.warn("The prediction horizon is predicting outside the values of the time varying "
                                              "parameters. I am now taking looping back the values and start from there.")
                                win[r, -1] = value[ci - N * int(np.floor(ci / N))]
                            else:
                                win[r, -1] = value[ci + N - 1]
                    self._tvp_window = win
                else:
                    raise ValueError(f"Mate, I know there are {n_tvp} time varying parameters but you did not pass me any."
                                     f"Please provide me with the values of the parameters, either to the optimize() "
                                     f"method or to the set_time_varying_parameters() method.")
            for k in range(N):                                                   # optimizer.py:905-929
                it, ic = 0, 0
                for j, name in enumerate(names):
                    if name in self._time_varying_parameters:
                        tab[k, nz + j] = win[it, k]
                        it += 1
                    else:
                        tab[k, nz + j] = cpv[ic]
                        ic += 1
            tab[N, nz:] = tab[N - 1, nz:]
        return tab

    # ---- results --------------------------------------------------------------------------------------------
    @property
    def solver_status_code(self):
        """optimizer.py:1085-1104 codes, one per instance."""
        return None if self._nlp_solution is None else self._nlp_solution['status'].cpu().numpy()

    def stats(self):
        s = self._nlp_solution
        if s is None:
            return {}
        st = s['status'].cpu().numpy()
        return {'return_status': [STATUS_TEXT.get(int(c), 'other') for c in st], 'success': (st == 1) | (st == 2),
                'iter_count': s['iter_count'].cpu().numpy(), 'kkt_error': s['kkt_error'].cpu().numpy()}

    def return_prediction(self):
        """mpc.py:1803-1827: (x_pred [B, nx, N+1], u_pred [B, nu, N], None), un-scaled."""
        if self._nlp_solution is None:
            warnings.warn("There is still no mpc solution available. Run mpc.optimize() to get one.")
            return None, None, None
        v = self._nlp_solution['x'].cpu().numpy()
        if getattr(self, '_mt', None) is not None:                    # mpc.py:1818-1820: the sampling intervals as third value
            N, nx, nu = self._prediction_horizon, self._n_x, self._n_u
            X = v[:, :(N + 1) * nx].reshape(-1, N + 1, nx) * np.asarray(self._sx)
            U = v[:, (N + 1) * nx:(N + 1) * nx + N * nu].reshape(-1, N, nu) * np.asarray(self._su)
            return np.swapaxes(X, 1, 2), np.swapaxes(U, 1, 2), v[:, self._dt_ind]
        N, Nc, nx, nu, nth = self._prediction_horizon, self._control_horizon, self._n_x, self._n_u, self._nth
        nxa, nua = nx + nth, nu + nth
        X = v[:, :(N + 1) * nxa].reshape(-1, N + 1, nxa) * np.concatenate([self._sx, np.ones(nth)])
        U = v[:, (N + 1) * nxa:(N + 1) * nxa + Nc * nua].reshape(-1, Nc, nua) * np.concatenate([self._su, np.ones(nth)])
        return np.swapaxes(X, 1, 2), np.swapaxes(U, 1, 2), None

    def phase_profile(self, enable=True):
        """Developer aid (hilo_nmpc_profile): shader-clock cycles instance 0 spent per solver phase in the launches
        since the last call.  Returns a dict or None when collection was just switched on."""
        names = ['derivatives', 'errors', 'riccati', 'step', 'line_search', 'update', 'n_factorizations', 'n_trial_points']
        buf = (C.c_longlong * 10)()
        had = getattr(self, '_prof_on', False)
        _lib.check(_lib.lib().hilo_nmpc_profile(self._handle, int(bool(enable)), buf if had else None))
        self._prof_on = bool(enable)
        self._prof_ends = dict(setup=buf[8], finish=buf[9]) if had else None
        return dict(zip(names, list(buf)[:8])) if had else None

    def phase_profile_ends(self):
        """The two per-LAUNCH slots that came with the last `phase_profile()` read-out: shader-clock cycles of instance 0 in front of
        the first iteration ('setup': constants, parameter row and warm start into LDS, bounds, start point) and behind the last
        ('finish': the write-back) of the most recent launch.  None before the first read-out."""
        return getattr(self, '_prof_ends', None)

    @property
    def keep_full_solution(self):
        """True: `_nlp_solution` also carries the constraint values `g` and the bound multipliers `lam_x` of the reference's solver
        result (mpc.py:722-723).  Off by default: a control loop reads neither, and they double the bytes a solve writes."""
        return self._full_solution

    @keep_full_solution.setter
    def keep_full_solution(self, arg):
        self._full_solution = bool(arg)

    def set_gather_buffer(self, table):
        """Sharded batches: the solve writes [u0 | status | iterations] rows (fp64) into `table` ([B, >= nu + 2], device) itself
        (hilo_nmpc_set_gather).  Returns False for problem kinds whose solve does not offer it (the caller then packs)."""
        if table is None:
            _lib.check(_lib.lib().hilo_nmpc_set_gather(self._handle, None, 0))
            return False
        if not table.is_contiguous():
            return False
        try:
            _lib.check(_lib.lib().hilo_nmpc_set_gather(self._handle, ptr(table), int(table.shape[1])))
        except _lib.HiloError as err:
            if err.code != -4:
                raise
            return False
        self._gather_table = table
        return True

    def set_plant_buffer(self, x_next):
        """Closed loops whose plant is the controller's own model: every solve writes x+ = Phi(x0, u_0, p) of its instances into
        `x_next` ([B, n_x], contiguous, device; may be the x0 tensor of the call itself) - the plant step of `plant_step` fused
        into the solve's launch (hilo_nmpc_set_plant_out).  None switches it off.  Returns False for problem kinds whose kernel
        does not offer it (the caller then calls `plant_step`)."""
        if x_next is None:
            _lib.check(_lib.lib().hilo_nmpc_set_plant_out(self._handle, None))
            self._plant_table = None
            return False
        if not (x_next.is_cuda and x_next.device == self._dev and x_next.is_contiguous() and x_next.dtype == torch.float64 and
                x_next.shape[-1] == self._n_x):
            return False
        try:
            _lib.check(_lib.lib().hilo_nmpc_set_plant_out(self._handle, ptr(x_next)))
        except _lib.HiloError as err:
            if err.code != -4:
                raise
            return False
        self._plant_table = x_next
        return True

    def plant_step(self, x, u, cp=None):
        """Closed-loop helper: x+ = Phi(x, u, p) with the controller's shooting map, on the device."""
        if getattr(self, '_mt', None) is not None:
            # (the inner problem's map advances by ITS sampling interval, a state of that problem: not the plant's clock)
            raise NotImplementedError("plant_step of a minimum-time controller: simulate the plant with Model.step / Model.simulate")
        x = to_dev(x, self._dev).reshape(-1, self._n_x).contiguous()
        u = to_dev(u, self._dev).reshape(-1, self._n_u).contiguous()
        B = x.shape[0]
        p, ps = None, 0
        if self._n_p:
            p = to_dev(cp, self._dev)
            p = p.reshape(1, -1) if p.ndim <= 1 else p
            ps = 0 if p.shape[0] == 1 else self._n_p
        xn = torch.empty_like(x)
        _lib.check(_lib.lib().hilo_nmpc_plant_step(self._handle, B, ptr(x), ptr(u), ptr(p), ps, ptr(xn),
                                                   stream_ptr(self._dev)))
        return xn
