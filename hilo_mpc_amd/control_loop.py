"""`SimpleControlLoop` (hilo_mpc/modules/control_loop.py:41-431) for batches: controller step -> plant step -> observer step,
`steps` times, for every instance of the batch at once.

What the reference's `_run` does per iteration (control_loop.py:343-397): `u = controller.optimize(x0[states of the
controller's model], cp=p)`, `plant.simulate(u=u, p=p)`, `observer.estimate()` - the controller is fed the PLANT state, the
observer runs alongside.  Here the plant is advanced on the device: with the controller's shooting map when it is the
controller's own model (`NMPC.plant_step`), with `Model.step` for a plant model of its own (a continuous plant is integrated with
eight classic Runge-Kutta steps per interval, or - set up with `Model.setup(solver='dopri5')` - under error control like the
reference's CVODES; a plant with algebraic states set up with `solver='idas'` like its IDAS: the loop keeps the plant's algebraic
states and starts the Newton iteration for the consistent start of each interval at those of the previous instant - the first
interval of a `run` at the model's guess - so that z stays on its branch where g has several roots), or by a callable
`(x, u, p) -> x+`.  A time-variant plant (`Model.is_time_variant`) is advanced with `plant.simulate`, like the reference's, so that it keeps its clock: `run` starts it from x0 at the time of the plant's stored
solution (`plant.set_initial_conditions(x0, t0=...)` beforehand chooses it; 0 otherwise).  A controller without `optimize` but with `call` (the LQR) is asked
`u = controller.call(x=x, p=p)` (control_loop.py:377).  A `PID` (`controller.type == 'PID'`) around a `Model` plant without an observer is
ONE launch, `PID.closed_loop`; with an observer, or around a callable plant, it is asked `u = controller.call(pv=...)` step by step."""
import numpy as np
import torch


class SimpleControlLoop:
    def __init__(self, plant, controller, observer=None):
        if not hasattr(controller, 'optimize') and not hasattr(controller, 'call'):
            raise TypeError("the controller must offer optimize() (NMPC / LMPC)")
        self._controller, self._observer = controller, observer
        if callable(plant) and not hasattr(plant, 'dynamical_state_names'):
            self._plant_fun, self._plant = plant, None
        else:
            cm = getattr(controller, '_model', None)
            if plant is cm and hasattr(controller, 'plant_step'):
                self._plant_fun, self._plant = None, plant          # the controller's own shooting map
            else:
                # a plant of its own (other parameters, discretisation or equations than the controller's model): advanced
                # on the device by `Model.step` (hilo_pf_function with one particle per instance, no noise)
                if not hasattr(plant, 'step'):
                    raise TypeError("the plant must be a Model or a callable (x, u, p) -> x_next")
                if len(plant.input_names) != len(getattr(cm, 'input_names', plant.input_names)):
                    raise ValueError("plant and controller model have different numbers of inputs")
                self._plant_fun, self._plant = (lambda x, u, p: plant.step(x, u, p)[0]), plant
                if getattr(plant, 'is_time_variant', lambda: False)():
                    self._plant_fun = self._simulate_plant
                elif getattr(plant, '_solver', None) == 'idas':
                    self._plant_fun = self._idas_plant
        self._plant_z = None
        self.solution = None

    def _simulate_plant(self, x, u, p):
        """One sampling interval of a time-variant plant through `simulate`, which holds the plant's time and advances it."""
        plant = self._plant
        plant.simulate(u=u, p=p, steps=1)
        xn = plant._sim['x'][-1]
        return torch.as_tensor(xn, device=x.device) if isinstance(x, torch.Tensor) else xn

    def _idas_plant(self, x, u, p):
        """One sampling interval of a plant with algebraic states; its z at the end is where the next interval's Newton iteration starts."""
        xs, _, zs = self._plant.rollout(x, u, p, steps=1, z0=self._plant_z, return_z=True)
        self._plant_z = zs[1]
        return xs[1]

    def _measure(self, x):
        obs = self._observer
        names = list(getattr(obs._model, 'measurement_names', []))
        states = list(obs._model.dynamical_state_names)
        mnames = getattr(obs, '_measured_states', None)
        if mnames is None:
            raise NotImplementedError("pass `measure=` to run(): a callable x -> y for the observer")
        return x[:, [states.index(n) for n in mnames]]

    def run(self, steps, x0, p=None, measure=None, **kwargs):
        """x0 [B, nx] (numpy or device tensor).  Returns (and stores as `.solution`) a dict with the closed-loop trajectories
        x [steps + 1, B, nx], u [steps, B, nu], the solver status per step and, with an observer, its estimates."""
        c = self._controller
        if getattr(c, 'type', None) == 'PID':
            return self._run_pid(int(steps), x0, p, measure, **kwargs)
        tensor = isinstance(x0, torch.Tensor)
        x = x0 if tensor else np.atleast_2d(np.asarray(x0, dtype=float))
        X, U, S, E = [x], [], [], []
        self._plant_z = None                               # an 'idas' plant starts this run at the model's guess
        if self._plant_fun == self._simulate_plant:        # the plant starts from x0 and goes on with its own clock
            sim = getattr(self._plant, '_sim', None)
            self._plant.set_initial_conditions(x, t0=sim['t'][-1] if sim else 0.)
        for _ in range(int(steps)):
            if hasattr(c, 'optimize'):
                u = c.optimize(x, cp=p, **kwargs) if p is not None else c.optimize(x, **kwargs)   # control_loop.py:362
            else:
                u = c.call(x=x, p=p)                                                              # control_loop.py:377 (LQR)
            st = getattr(c, 'solver_status_code', None)
            S.append(None if st is None else np.asarray(st).copy())
            if self._plant_fun is not None:
                x = self._plant_fun(x, u, p)                                                        # control_loop.py:385
            else:
                xn = c.plant_step(x, u, cp=p)
                x = xn if tensor else xn.cpu().numpy()
            if self._observer is not None:                                                          # control_loop.py:388-397
                y = (measure or self._measure)(x)
                E.append(self._observer.estimate(y=y, u=u))
            X.append(x)
            U.append(u)
        stack = (lambda a: torch.stack(list(a))) if tensor else (lambda a: np.stack([np.asarray(q) for q in a]))
        self.solution = {'x': stack(X), 'u': stack([torch.as_tensor(q, device=x.device) if tensor and not isinstance(q, torch.Tensor)
                                                    else q for q in U]),
                         'status': S, 'estimates': E}
        return self.solution

    def _run_pid(self, steps, x0, p, measure, u=None, set_point=None, process_values=None, outputs=None, **kwargs):
        """A PID controller.  u: the held inputs [B, n_u] (read for the inputs no loop drives; None: zeros); set_point,
        process_values, outputs as for `PID.closed_loop`.  The solution's 'u' holds the controller outputs [steps, B, nsp]; 'indices'
        are those of `PID.closed_loop` on the one-launch path and None step by step (nothing is summed on the host)."""
        c, plant = self._controller, self._plant
        if kwargs:
            raise TypeError(f"run() got unexpected arguments {sorted(kwargs)} for a PID controller")
        if plant is not None and hasattr(plant, 'rollout') and self._observer is None:
            r = c.closed_loop(plant, x0, u=u, p=p, steps=steps, set_point=set_point, process_values=process_values, outputs=outputs,
                              return_stats=True, t0=(plant._sim['t'][-1] if plant.is_time_variant() and getattr(plant, '_sim', None) else 0.))
            self.solution = {'x': r['x'], 'u': r['u'], 'y': r['y'], 'status': [r['stats']['status']], 'estimates': [],
                             'indices': r['indices']}
            return self.solution
        if plant is None:
            raise NotImplementedError("a PID around a callable plant: the loop cannot tell which of its values the controller sees. Pass "
                                      "a Model as the plant")
        if set_point is not None:
            c.set_point = set_point
        pv_sel, out_sel = c._resolve(plant, process_values, outputs)
        if any(not is_state for _, is_state in pv_sel) and measure is None:
            raise NotImplementedError("step by step the controller is fed from the plant state: name states in process_values=[...], or "
                                      "pass `measure=`, a callable x -> y [B, n_y] for the controller and the observer")
        tensor = isinstance(x0, torch.Tensor)
        x = x0 if tensor else np.atleast_2d(np.asarray(x0, dtype=float))
        B = x.shape[0]
        new = (lambda a: torch.as_tensor(a, dtype=torch.float64, device=x.device)) if tensor else (lambda a: np.array(a, dtype=float))
        uf = new(np.zeros((B, plant.n_u))) if u is None else new(u).reshape(-1, plant.n_u)
        uf = (uf.expand(B, -1).clone() if tensor else np.tile(uf, (B // uf.shape[0], 1)))
        X, U, E = [x], [], []
        self._plant_z = None
        if self._plant_fun == self._simulate_plant:
            sim = getattr(plant, '_sim', None)
            plant.set_initial_conditions(x, t0=sim['t'][-1] if sim else 0.)
        for _ in range(steps):
            y = measure(x) if measure is not None else None
            cols = [x[:, i] if is_state else y[:, i] for i, is_state in pv_sel]
            pv = torch.stack(cols, dim=1) if tensor else np.stack(cols, axis=1)
            uo = c.call(pv=pv)
            uf = uf.clone() if tensor else uf.copy()
            uf[:, out_sel] = uo
            x = self._plant_fun(x, uf, p)
            if self._observer is not None:
                E.append(self._observer.estimate(y=(measure or self._measure)(x), u=uf, **({} if p is None else {'p': p})))
            X.append(x)
            U.append(uo)
        stack = torch.stack if tensor else np.stack
        self.solution = {'x': stack(X), 'u': stack(U), 'status': steps * [None], 'estimates': E, 'indices': None}
        return self.solution
