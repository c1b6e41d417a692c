"""PID controllers for batches of loops, and closed loops of controller and plant in one launch.

API mirror of `hilo_mpc/modules/controller/pid.py` (`PID`: `k_p` / `t_i` / `t_d` with their diagonal-matrix getters, `k_i`, `k_d`,
`set_point`, `setup(dt=)`, `call(pv=)`) with a leading batch axis.  The law is the reference's velocity form (csrc/hilo_pid.h) and
runs in libhilo_hip.so: `call` is one `hilo_pid_call`, nothing is computed on the host.  Beyond the reference:

  * `k_p`, `t_i`, `t_d` and `set_point` also take [B, n_set_points]: one controller per instance, held on the device (host data of
    shape [n_set_points, n_set_points] is the reference's matrix of ONE controller and has to be diagonal; a device tensor of
    two dimensions is always one row per instance);
  * `output_limits=(lo, hi)` clamps u, and the clamped value is what the controller remembers - the anti-windup of the velocity
    form (the reference: "TODO: Add anti-windup");
  * `closed_loop(plant, x0, ...)` runs controller AND plant for `steps` sampling intervals in one launch (`hilo_pid_loop`): the
    roll-out of `Model.rollout` with the input computed inside the kernel, plus the indices ISE, IAE, ITAE and the total
    variation of u per loop.  With `store=False` only those and the final state leave the device - a gain study is "simulate
    10^5 loops and rank them", `torch.argmin(result['indices']['ise'][:, 0])`.

Out of scope: plants under 'bdf' / 'idas', coupled (non-diagonal) gains, the proportional band, a derivative filter.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from ._device import device, ptr, stream_ptr, to_dev

MAX_LOOPS = 4   # HILO_PID_MAX_LOOPS
_MEM = 5        # HILO_PID_MEM
_LABEL = {'k_p': 'K_P', 't_i': 'T_I', 't_d': 'T_D'}


class PID:
    """`pid = PID(k_p=8., t_i=1.); pid.setup(dt=.01); pid.set_point = 1.; u = pid.call(pv=y)`."""

    def __init__(self, n_set_points=1, k_p=None, t_i=None, t_d=None, proportional_on_process_value=False,
                 derivative_on_process_value=False, output_limits=None, id=None, name=None, plot_backend=None, device_index=None):
        self.id, self.name, self.type = id, name, 'PID'
        self._n_set_points = int(n_set_points)
        if self._n_set_points < 1:
            raise ValueError(f"n_set_points must be at least 1, got {n_set_points}")
        self._dev_index, self._dev = device_index, None
        self._gains = {}            # 'k_p' / 't_i' / 't_d' -> [nsp] on the host, or [B, nsp] (numpy or device tensor)
        self._packed = None         # the three as one device tensor [1 or B, 3, nsp]
        n = self._n_set_points
        self._set_tuning_parameter('k_p', n * [1.] if k_p is None else k_p)
        self._set_tuning_parameter('t_i', n * [np.inf] if t_i is None else t_i)
        self._set_tuning_parameter('t_d', n * [0.] if t_d is None else t_d)
        self._proportional_on_process_value = bool(proportional_on_process_value)
        self._derivative_on_process_value = bool(derivative_on_process_value)
        self._p_band = False
        self.output_limits = output_limits
        self._set_point = np.zeros((n, 1))
        self._dt = None
        self._mem = None            # [B, nsp, 5] on the device: pv[-2], pv[-1], sp[-2], sp[-1], u_prev
        self._hc = None             # ('dopri5' plants given as expressions) the step-size proposals the last closed loop ended with

    # ---- tuning ------------------------------------------------------------------------------
    def _set_tuning_parameter(self, which, value):
        n = self._n_set_points
        tensor = isinstance(value, torch.Tensor)
        a = value if tensor else np.asarray(value, dtype=float)
        if a.ndim == 2 and a.shape[1] == n and (tensor or a.shape[0] != n):
            # one controller per instance ([n, n] on the host is the reference's matrix of one controller)
            self._gains[which] = a if tensor else a.copy()
            self._packed = None
            return
        if tensor:
            a = a.detach().cpu().numpy().astype(float)
        if a.ndim == 0 or a.size == 1 and n > 1:
            a = np.full((n, n), float(a.reshape(-1)[0]))     # what the reference's `convert` makes of a scalar
        elif a.ndim == 1 or (a.ndim == 2 and 1 in a.shape and a.shape != (n, n)):
            if a.size != n:
                raise ValueError(f"Dimension mismatch. Supplied dimension for {_LABEL[which]} is {a.size}, but required dimension is "
                                 f"{n} (one value per set point), {n}x{n} (a diagonal matrix) or Bx{n} (one row per instance).")
            a = np.diag(a.ravel())
        if a.shape != (n, n):
            raise ValueError(f"Dimension mismatch. Supplied dimension for {_LABEL[which]} is {'x'.join(map(str, a.shape))}, but "
                             f"required dimension is {n} (one value per set point), {n}x{n} (a diagonal matrix) or Bx{n} (one row "
                             f"per instance).")
        if not _is_diagonal(a):
            raise ValueError(f"The number of set points is greater than 1, but the supplied matrix for {_LABEL[which]} is not a "
                             f"diagonal matrix. Coupled multi-variable control is not supported at the moment.")
        self._gains[which] = np.diag(a).copy()
        self._packed = None

    def _get(self, which):
        g = self._gains[which]
        return np.diag(g) if isinstance(g, np.ndarray) and g.ndim == 1 else g

    proportional_gain = k_p = property(lambda s: s._get('k_p'), lambda s, v: s._set_tuning_parameter('k_p', v))
    integral_time = t_i = property(lambda s: s._get('t_i'), lambda s, v: s._set_tuning_parameter('t_i', v))
    derivative_time = t_d = property(lambda s: s._get('t_d'), lambda s, v: s._set_tuning_parameter('t_d', v))

    def _derived(self, f):
        kp, other = self._gains['k_p'], self._gains['t_i' if f == 'i' else 't_d']
        batched = any(not (isinstance(g, np.ndarray) and g.ndim == 1) for g in (kp, other))
        if batched:
            kp, other = (torch.as_tensor(g) if not isinstance(g, torch.Tensor) else g for g in (kp, other))
            if kp.device != other.device:
                kp, other = kp.cpu(), other.cpu()
        v = kp / other if f == 'i' else kp * other
        return v if batched else np.diag(v)

    integral_gain = k_i = property(lambda s: s._derived('i'))
    derivative_gain = k_d = property(lambda s: s._derived('d'))

    @property
    def set_point(self):
        return self._set_point

    @set_point.setter
    def set_point(self, value):
        n = self._n_set_points
        if isinstance(value, torch.Tensor) and value.dim() == 2 and value.shape[1] == n:
            self._set_point = value
            return
        a = np.asarray(value.detach().cpu() if isinstance(value, torch.Tensor) else value, dtype=float)
        if a.ndim == 2 and a.shape[1] == n and not (a.shape == (n, 1)):
            self._set_point = a.copy()                   # [B, nsp]: one row per instance
            return
        a = a.reshape(-1, 1) if a.ndim < 2 else a
        if n > 1:
            if a.shape[0] == 1:
                a = np.tile(a, (n, 1))
            elif a.shape[0] != n:
                raise ValueError(f"Dimension mismatch. Supplied dimension for the set point is {a.shape[0]}x{a.shape[1]}, but "
                                 f"required dimension is {n}x1.")
        self._set_point = a

    s_p = set_point

    @property
    def output_limits(self):
        return self._limits

    @output_limits.setter
    def output_limits(self, limits):
        n = self._n_set_points
        if limits is None:
            self._limits = None
            return
        if len(limits) != 2:
            raise ValueError("output_limits must be None or a pair (lo, hi), each a number or one value per set point")
        lo, hi = (np.broadcast_to(np.asarray(v, dtype=float).ravel(), (n,)).copy() if np.size(v) in (1, n) else None for v in limits)
        if lo is None or hi is None:
            raise ValueError(f"output_limits: lo and hi are numbers or hold one value per set point ({n})")
        if not np.all(lo <= hi):
            raise ValueError(f"output_limits: lo {lo.tolist()} must not exceed hi {hi.tolist()}")
        self._limits = (lo, hi)

    # ---- setup -------------------------------------------------------------------------------
    def setup(self, **kwargs):
        dt = kwargs.get('dt')
        if dt is None:
            dt = 1.
        if self._p_band:
            raise NotImplementedError("The use of the proportional band has not been implemented yet.")
        dt = float(dt)
        if not (dt > 0. and np.isfinite(dt)):
            raise ValueError(f"The sampling interval dt must be positive and finite, got {dt}")
        self._dt = dt
        return self

    def is_setup(self):
        return self._dt is not None

    def reset(self):
        """Forget the process-value and set-point history and the last output: the next call is a first call."""
        if self._mem is not None:
            self._mem.zero_()
        self._hc = None

    # ---- device state ------------------------------------------------------------------------
    def _device(self, *args):
        for a in args:
            if isinstance(a, torch.Tensor) and a.is_cuda:
                return a.device
        if self._dev is None:
            self._dev = device(self._dev_index)
        return self._dev

    def _opts(self):
        o = _lib.PidOpts()
        o.nsp = self._n_set_points
        o.flags = (1 if self._proportional_on_process_value else 0) | (2 if self._derivative_on_process_value else 0) | \
                  (4 if self._limits is not None else 0)
        if self._limits is not None:
            for j in range(min(self._n_set_points, MAX_LOOPS)):
                o.lo[j], o.hi[j] = self._limits[0][j], self._limits[1][j]
        return o

    def _batch_of_gains(self):
        return max([g.shape[0] for g in self._gains.values() if not (isinstance(g, np.ndarray) and g.ndim == 1)], default=1)

    def _pack_gains(self, dev):
        """[1 or B, 3, nsp] on the device, rebuilt when a gain was set (element-wise copies; no arithmetic)."""
        if self._packed is None or self._packed.device != dev:
            Bg, n = self._batch_of_gains(), self._n_set_points
            t = torch.empty(Bg, 3, n, dtype=torch.float64, device=dev)
            for r, which in enumerate(('k_p', 't_i', 't_d')):
                g = to_dev(self._gains[which], dev).reshape(-1, n)
                if g.shape[0] not in (1, Bg):
                    raise ValueError(f"{_LABEL[which]} holds {g.shape[0]} rows, another gain {Bg}: per-instance gains must agree in "
                                     f"their batch")
                t[:, r] = g
            self._packed = t
        return self._packed

    def _batched_inputs(self, B, dev, set_point=None):
        """(gains, gain_stride, sp, sp_stride) for a batch of B."""
        n = self._n_set_points
        g = self._pack_gains(dev)
        if g.shape[0] not in (1, B):
            raise ValueError(f"the gains are given for {g.shape[0]} instances, the call is for {B}")
        sp = self._set_point if set_point is None else set_point
        sp = to_dev(sp, dev)
        sp = sp.reshape(1, n) if sp.numel() == n else sp
        if sp.dim() != 2 or sp.shape[1] != n or sp.shape[0] not in (1, B):
            raise ValueError(f"the set point holds {list(sp.shape)} values; expected [{n}] or [{B}, {n}]")
        return g, (3 * n if g.shape[0] == B else 0), sp.contiguous(), (n if sp.shape[0] == B else 0)

    def _memory(self, B, dev):
        if self._mem is None or self._mem.shape[0] != B or self._mem.device != dev:
            self._mem = torch.zeros(B, self._n_set_points, _MEM, dtype=torch.float64, device=dev)
            self._hc = None
        return self._mem

    # ---- the law -----------------------------------------------------------------------------
    def _type_letters(self):
        t = 'P'

        def any_ne(g, v):
            g = g.detach().cpu().numpy() if isinstance(g, torch.Tensor) else g
            return bool(np.any(g != v))
        if any_ne(self._gains['t_i'], np.inf):
            t += 'I'
        if any_ne(self._gains['t_d'], 0.):
            t += 'D'
        return t

    def call(self, *args, **kwargs):
        """pv [nsp], [B, nsp] or missing (zeros) -> u [nsp, 1] like the reference's column, or [B, nsp]; numpy in gives numpy
        out, a device tensor in gives a device tensor out.  One `hilo_pid_call`."""
        if self._dt is None:
            t = self._type_letters()
            raise RuntimeError(f"{t} controller is not set up. Run PID.setup() before calling the {t} controller")
        n = self._n_set_points
        if n > MAX_LOOPS:
            raise NotImplementedError(f"the kernels are built for up to {MAX_LOOPS} set points per controller; this one has {n}. "
                                      f"Use several controllers")
        pv = kwargs.get('pv')
        tensor = isinstance(pv, torch.Tensor)
        dev = self._device(pv)
        Bg = self._batch_of_gains()
        sp_rows = self._set_point.shape[0] if (self._set_point.ndim == 2 and self._set_point.shape[1] == n and
                                               self._set_point.shape != (n, 1)) else 1
        if pv is None:
            B, pvt, single = max(Bg, sp_rows, self._mem.shape[0] if self._mem is not None else 1), None, False
            single = B == 1 and Bg == 1 and sp_rows == 1
        else:
            pvt = to_dev(pv, dev)
            if n == 1 and pvt.dim() == 1 and pvt.numel() > 1:
                pvt = pvt.reshape(-1, 1)
            batched = pvt.dim() == 2 and pvt.shape[1] == n and tuple(pvt.shape) != (n, 1)
            if not batched:                                     # one process value per set point (a single value serves all)
                if pvt.numel() not in (1, n):
                    raise ValueError(f"Dimension mismatch. Supplied dimension for the process value is {pvt.numel()}, but required "
                                     f"dimension is {n}x1 (or Bx{n}: one row per instance).")
                pvt = pvt.reshape(1, -1).expand(1, n)
            B = pvt.shape[0] if batched else max(Bg, sp_rows)
            pvt = pvt.expand(B, n).contiguous()
            single = not batched and B == 1
        g, gs, sp, ss = self._batched_inputs(B, dev)
        mem = self._memory(B, dev)
        u = torch.empty(B, n, dtype=torch.float64, device=dev)
        opts = self._opts()
        _lib.check(_lib.lib().hilo_pid_call(C.byref(opts), B, self._dt, ptr(pvt), ptr(sp), ss, ptr(g), gs, ptr(mem), ptr(u),
                                            stream_ptr(dev)))
        if tensor:
            return u[0] if single else u
        u = u.cpu().numpy()
        return u[0].reshape(n, 1) if single else u

    # ---- controller and plant in one launch ----------------------------------------------------
    def _resolve(self, plant, process_values, outputs):
        n = self._n_set_points
        ys, xs, us = list(plant.measurement_names), list(plant.dynamical_state_names), list(plant.input_names)
        if n > min(len(us), MAX_LOOPS):
            raise ValueError(f"the controller has {n} set points, the plant {len(us)} inputs and the kernel is built for up to "
                             f"{MAX_LOOPS} loops: every loop drives an input of its own. Use a PID with at most "
                             f"{min(len(us), MAX_LOOPS)} set points")
        if process_values is None:
            if len(ys) == n:
                process_values = ys
            elif len(xs) == n:
                process_values = xs
            else:
                raise ValueError(f"the controller has {n} set points, the plant {len(ys)} measurements {ys} and {len(xs)} states "
                                 f"{xs}: name the {n} controlled ones with process_values=[...]")
        if outputs is None:
            if len(us) != n:
                raise ValueError(f"the controller has {n} set points, the plant {len(us)} inputs {us}: name the {n} driven ones with "
                                 f"outputs=[...]")
            outputs = us
        process_values = [process_values] if isinstance(process_values, str) else list(process_values)
        outputs = [outputs] if isinstance(outputs, str) else list(outputs)
        for what, names in (('process_values', process_values), ('outputs', outputs)):
            if len(names) != n:
                raise ValueError(f"{what} names {len(names)} quantities for {n} set points; give one per set point")
            twice = sorted({v for v in names if names.count(v) > 1})
            if twice:
                raise ValueError(f"{what}: {twice} used twice; every loop needs a quantity of its own")
        pv = []
        for v in process_values:
            if v in ys:
                pv.append((ys.index(v), 0))
            elif v in xs:
                pv.append((xs.index(v), 1))
            else:
                raise ValueError(f"process_values: the plant has no measurement or state '{v}'. Choose out of the measurements {ys} or "
                                 f"the states {xs}")
        out = []
        for v in outputs:
            if v not in us:
                raise ValueError(f"outputs: the plant has no input '{v}'. Choose out of {us}")
            out.append(us.index(v))
        return pv, out

    def closed_loop(self, plant, x0, u=None, p=None, steps=1, set_point=None, process_values=None, outputs=None, store=True,
                    return_stats=False, t0=0.):
        """`steps` sampling intervals of this controller around `plant` (a Model) for a batch of loops, in ONE launch.

        x0 [B, n_x]; u [B, n_u] (or one row) the held inputs - read for the inputs no loop drives, None: zeros; p like
        `Model.rollout`; set_point None (the controller's), [nsp], [B, nsp], or a schedule [steps, B, nsp] / [steps, 1, nsp];
        process_values: names of plant measurements or states, one per loop; outputs: names of plant inputs, one per loop.
        Per interval k: pv = the selected h(t_k, x[k], u[k-1], p) or states, the law, the driven inputs overwritten, the plant
        advanced with its map or under 'dopri5'.  Returns a dict: 'x' [steps + 1, B, n_x], 'u' [steps, B, nsp] (the controller
        outputs), 'y' [steps, B, n_y] (absent with store=False), 'x_final' [B, n_x], 'indices' {'ise', 'iae', 'itae', 'tvu'} each
        [B, nsp] (sums of e^2 dt, |e| dt, (k dt) |e| dt and |u_k - u_{k-1}| over the intervals of THIS call), with return_stats
        'stats' as `Model.rollout` gives them.  The controller's memory is left where the loop ended: a second call goes on.
        An instance whose integration fails gets NaN rows from the instant it did not reach and NaN indices."""
        from .model import Model, SOLVERS
        if self._dt is None:
            t = self._type_letters()
            raise RuntimeError(f"{t} controller is not set up. Run PID.setup() before calling the {t} controller")
        if not isinstance(plant, Model):
            raise TypeError("closed_loop runs the controller around a Model; for another plant call the controller step by step "
                            "(PID.call) or use SimpleControlLoop")
        if not plant._is_setup:
            raise RuntimeError("Model is not set up. Run Model.setup() before closing a loop around it.")
        if plant.dt is None or abs(plant.dt - self._dt) > 1e-12 * abs(self._dt):
            raise ValueError(f"the controller is set up with dt = {self._dt}, the plant with dt = {plant.dt}: one sampling interval "
                             f"serves both. Run PID.setup(dt={plant.dt}) or set the plant up with dt={self._dt}")
        if plant._solver in ('bdf', 'idas'):
            raise NotImplementedError(f"closed_loop under solver '{plant._solver}' is not built: the input jumps at every sampling "
                                      f"instant, so the implicit method would restart every interval. Set the plant up with "
                                      f"Model.setup(solver='dopri5') or without a solver, or run the loop step by step "
                                      f"(SimpleControlLoop with an observer, or PID.call + Model.step)")
        if getattr(plant, 'n_z', 0):
            raise NotImplementedError("closed_loop is built for plants without algebraic states; run the loop step by step "
                                      "(PID.call + Model.rollout(steps=1))")
        pv_sel, out_sel = self._resolve(plant, process_values, outputs)
        steps = int(steps)
        if steps < 1:
            raise ValueError(f"steps must be at least 1, got {steps}")
        n = self._n_set_points
        sched = None
        if set_point is not None:
            s = set_point if isinstance(set_point, torch.Tensor) else np.asarray(set_point, dtype=float)
            if s.ndim == 3:
                if s.shape[0] != steps or s.shape[2] != n:
                    raise ValueError(f"the set-point schedule holds {list(s.shape)} values for {steps} sampling intervals and {n} set "
                                     f"points: pass [steps, B, {n}] (or [steps, 1, {n}]) with one row per interval, or a held set "
                                     f"point [{n}] / [B, {n}]")
                sched = s
        h = plant._plant_handle(self._dev_index)
        dev = h._dev
        host = not isinstance(x0, torch.Tensor)
        xt = to_dev(x0, dev).reshape(-1, plant.n_x).contiguous()
        B = xt.shape[0]
        parts = []
        for v, m, what in ((u, plant.n_u, 'inputs'), (plant.lti_parameters() if plant.name == 'lti' else p, h._n_p, 'parameters')):
            if m:
                if v is None:
                    if what == 'parameters':
                        raise RuntimeError(f"The model has {m} parameters; pass them to closed_loop().")
                    t = torch.zeros(1, m, dtype=torch.float64, device=dev)
                else:
                    t = to_dev(v, dev).reshape(-1, m)
                if t.shape[0] not in (1, B):
                    raise ValueError(f"{what}: batch {t.shape[0]} does not match {B} states")
                parts.append(t)
        Bu = max(t.shape[0] for t in parts)
        up = torch.cat([t.expand(Bu, -1) for t in parts], dim=1).contiguous()
        up_stride = up.shape[1] if Bu == B else 0
        if sched is not None:
            spt = to_dev(sched, dev)
            if spt.shape[1] not in (1, B):
                raise ValueError(f"the set-point schedule is given for {spt.shape[1]} instances, the loop has {B}")
            g, gs, _, _ = self._batched_inputs(B, dev)
            ss, sstep = (n if spt.shape[1] == B else 0), spt.shape[1] * n
        else:
            g, gs, spt, ss = self._batched_inputs(B, dev, set_point)
            sstep = 0
        mem = self._memory(B, dev)
        opts = self._opts()
        for j, ((i, is_state), o) in enumerate(zip(pv_sel, out_sel)):
            opts.pv_index[j], opts.pv_is_state[j], opts.out_index[j] = i, is_state, o
        sim = _lib.SimOpts()
        sim.t0 = float(t0)
        hc = None
        if plant._solver is not None:
            o = plant._solver_options
            sim.method, sim.max_steps = SOLVERS[plant._solver], o['max_num_steps']
            sim.rtol, sim.atol, sim.h0 = o['reltol'], o['abstol'], o['first_step']
            if plant._symbolic:       # the kernel of a model given as expressions hands the step-size proposal on
                key = (id(plant), B)
                if self._hc is None or self._hc[0] != key or self._hc[1].device != dev:
                    self._hc = (key, torch.zeros(B, dtype=torch.float64, device=dev))
                hc = self._hc[1]
        ny = h._n_y
        X = torch.empty(steps + 1, B, plant.n_x, dtype=torch.float64, device=dev) if store else None
        U = torch.empty(steps, B, n, dtype=torch.float64, device=dev) if store else None
        Y = torch.empty(steps, B, ny, dtype=torch.float64, device=dev) if store else None
        J = torch.empty(B, n, 4, dtype=torch.float64, device=dev)
        xf = torch.empty(B, plant.n_x, dtype=torch.float64, device=dev)
        stats = torch.empty(B, 4, dtype=torch.int32, device=dev) if return_stats else None
        _lib.check(_lib.lib().hilo_pid_loop(h._handle, C.byref(sim), C.byref(opts), B, steps, ptr(xt), ptr(up), up_stride, ptr(spt), ss,
                                            sstep, ptr(g), gs, ptr(mem), ptr(X), ptr(U), ptr(Y), ptr(J), ptr(xf), ptr(stats), ptr(hc),
                                            stream_ptr(dev)))
        out_ = (lambda t: t.cpu().numpy()) if host else (lambda t: t)
        res = {}
        if store:
            res.update(x=out_(X), u=out_(U), y=out_(Y))
        J = out_(J)
        res['x_final'] = out_(xf)
        res['indices'] = {'ise': J[:, :, 0], 'iae': J[:, :, 1], 'itae': J[:, :, 2], 'tvu': J[:, :, 3]}
        if return_stats:
            st = out_(stats)
            res['stats'] = {'status': st[:, 0], 'n_accepted': st[:, 1], 'n_rejected': st[:, 2], 'n_rhs': st[:, 3]}
        return res


def _is_diagonal(a):
    return a.ndim == 2 and a.shape[0] == a.shape[1] and not np.any(a[~np.eye(a.shape[0], dtype=bool)])


__all__ = ['PID']
