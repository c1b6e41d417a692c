"""Linear-quadratic regulator for batches of plants, each with its own parameters and operating point.

API mirror of `hilo_mpc/modules/controller/lqr.py` (`LinearQuadraticRegulator`: constructor checks, `Q` / `R` setters, `horizon`,
`setup()`, `call(x=, p=)`, `K` / `feedback_gain`) with a leading batch axis.  The arithmetic runs in libhilo_hip.so
(csrc/hilo_lqr.h): the Jacobians of the model's discrete-time map at each instance's operating point in forward mode, the Riccati
recursion of lqr.py:236-245 from P = Q (`horizon` steps), and the feedback - one launch (`hilo_lqr_call`).  Beyond the reference:
`horizon = None` is the stationary gain (the reference raises NotImplementedError, "future releases"), from the discrete algebraic
Riccati equation by the structure-preserving doubling algorithm; `P` hands out the Riccati solution (what a terminal cost needs);
`call(x_eq=, u_eq=)` takes per-instance operating points (gain scheduling).  Nothing is computed on the host.
"""
import ctypes as C
import os
import warnings

import numpy as np
import torch

from . import _lib
from ._device import ptr, stream_ptr, to_dev
from .model import Model

LQR_STATUS = {0: 'ok', 1: 'max_iter reached', 2: 'not finite, singular, or R + B\'PB not positive definite'}     # HILO_LQR_STATUS_*


def _square(arg, what):
    """lqr.py:108-112: real-valued; a vector becomes a diagonal."""
    a = arg.detach().cpu().numpy() if isinstance(arg, torch.Tensor) else np.asarray(arg)
    if a.dtype == object or np.iscomplexobj(a) or not np.issubdtype(a.dtype, np.number):
        raise ValueError(f"LQR matrix {what} needs to be real-valued")
    a = a.astype(float)
    if a.ndim == 0:
        a = a.reshape(1, 1)
    if a.ndim == 1 or (a.ndim == 2 and a.shape[0] != a.shape[1] and 1 in a.shape):
        a = np.diag(a.ravel())
    if a.ndim != 2:
        raise ValueError(f"LQR matrix {what} needs to be a vector or a matrix")
    return a


class _Key:
    """What one argument of `call` was at the last solve: a device tensor by identity and version counter (no copy, no
    synchronisation), host data by value."""

    def __init__(self, v):
        self.tensor = isinstance(v, torch.Tensor)
        self.obj = v if self.tensor else None
        self.version = v._version if self.tensor else None
        self.value = None if (v is None or self.tensor) else np.array(v, dtype=float, copy=True)
        self.none = v is None

    def matches(self, v):
        if v is None or self.none:
            return v is None and self.none
        if isinstance(v, torch.Tensor) or self.tensor:
            return v is self.obj and v._version == self.version
        w = np.asarray(v, dtype=float)
        return w.shape == self.value.shape and np.array_equal(w, self.value)


class LinearQuadraticRegulator:
    """`LQR(model)`; `lqr.horizon = 5` (or None: stationary); `lqr.setup()`; `lqr.Q = ...; lqr.R = ...`; `u = lqr.call(x=x, p=p)`."""

    def __init__(self, model, id=None, name=None, discrete=True, plot_backend=None, device_index=None):
        if not isinstance(model, Model):
            raise TypeError("The model must be an object of the Model class.")
        model._refuse_time_variant('LQR')
        if not model._is_setup:
            raise RuntimeError("Model is not set up. Run Model.setup() before passing it to the controller.")
        if discrete and not model.discrete:
            raise RuntimeError("The model used for the LQR needs to be discrete. Use Model.discretize() to obtain a "
                               "discrete model.")
        if not discrete and model.discrete:
            raise RuntimeError("The model used for the LQR needs to be continuous.")
        if not model.is_linear():
            raise RuntimeError("The model used for the LQR needs to be linear. Use Model.linearize() to obtain a "
                               "linearized model.")
        if model.n_u == 0:
            raise RuntimeError("The model used for the LQR is autonomous.")
        self.id, self.name, self.type = id, name, 'LQR'
        self._discrete = bool(discrete)
        self._model = model.copy(setup=True)
        self._model._lin_plant = None               # the copy gets a handle of its own
        self._dev_index, self._dev, self._eq = device_index, None, (None, None)
        self._Q = self._R = self._N = self._K = self._P = None
        self._n_x = self._n_u = self._n_p = 0
        self._horizon = None
        self._is_setup = False
        self._max_iter, self._tol = 50, 1e-12
        self._stats = None
        self._keys = None
        self._host = True
        self._batched = False
        self._checked = True

    # ---- tuning ------------------------------------------------------------------------------
    def _weight(self, arg, what, n, definite):
        a = _square(arg, what)
        if a.shape != (n, n):
            raise ValueError(f"Dimension mismatch. Supplied dimension is {a.shape[0]}x{a.shape[1]}, but required "
                             f"dimension is {n}x{n}")
        if not np.allclose(a, a.T, rtol=1e-12, atol=1e-14):
            raise ValueError(f"LQR matrix {what} needs to be symmetric")
        ev = np.linalg.eigvalsh(.5 * (a + a.T)) if n else np.zeros(0)
        if definite and not np.all(ev > 0.):
            raise ValueError(f"LQR matrix {what} needs to be positive definite")
        if not definite and not np.all(ev >= -1e-12 * max(1., np.abs(ev).max(initial=0.))):
            raise ValueError(f"LQR matrix {what} needs to be positive semidefinite")
        return a

    @property
    def Q(self):
        return self._Q

    @Q.setter
    def Q(self, arg):
        self._Q = self._weight(arg, 'Q', self._n_x, False)
        self._Qd = to_dev(self._Q, self._dev)
        self._K = self._P = self._keys = None

    @property
    def R(self):
        return self._R

    @R.setter
    def R(self, arg):
        self._R = self._weight(arg, 'R', self._n_u, True)
        self._Rd = to_dev(self._R, self._dev)
        self._K = self._P = self._keys = None

    @property
    def N(self):
        return self._N

    @property
    def horizon(self):
        return self._horizon

    @horizon.setter
    def horizon(self, arg):
        if arg is not None and int(arg) < 1:
            raise ValueError("The horizon needs to be a positive integer (or None for the stationary gain)")
        self._horizon = None if arg is None else int(arg)
        self._K = self._P = self._keys = None

    n_x = property(lambda s: s._n_x)
    n_u = property(lambda s: s._n_u)
    n_p = property(lambda s: s._n_p)

    def _out(self, t):
        """The result of the last solve the way its inputs came: numpy for host data, [n, m] without a batch axis."""
        if t is None:
            return None
        self._check_status()
        t = t if self._batched else t[0]
        return t.cpu().numpy() if self._host else t

    @property
    def feedback_gain(self):
        return self._out(self._K)

    K = feedback_gain

    @property
    def P(self):
        """The Riccati solution behind the gain: after `horizon` backward steps from Q, or the stationary one."""
        return self._out(self._P)

    @property
    def status(self):
        """HILO_LQR_STATUS_* of the last solve per instance: 0 ok, 1 max_iter reached, 2 failed (rows of K, P, u are NaN)."""
        if self._stats is None:
            return None
        self._check_status()
        s = self._stats[:, 0] if self._batched else self._stats[0, 0]
        return s.cpu().numpy() if self._host else s

    @property
    def iterations(self):
        """Backward steps / doubling steps of the last solve per instance."""
        if self._stats is None:
            return None
        s = self._stats[:, 1] if self._batched else self._stats[0, 1]
        return s.cpu().numpy() if self._host else s

    def _check_status(self):
        if self._checked or self._stats is None:
            return
        self._checked = True
        st = self._stats[:, 0].cpu().numpy()
        if np.any(st != 0):
            bad = np.flatnonzero(st != 0)
            warnings.warn(f"LQR: the Riccati equation was not solved for {bad.size} of {st.size} instance(s) (first: instance {bad[0]}, "
                          f"status {st[bad[0]]}: {LQR_STATUS.get(int(st[bad[0]]), '?')}); their rows of K, P and u are NaN", RuntimeWarning)

    # ---- set-up ------------------------------------------------------------------------------
    def setup(self, max_iter=50, tol=1e-12, **kwargs):
        """lqr.py:204-258.  Creates the device handle of the model's map (a model written as expressions is compiled here, or, with
        HILO_JIT_COMPILE_ONLY, only compiled into the cache); `Model('lti', A, B)` needs none.  Resets Q, R and K like the
        reference.  max_iter, tol: the doubling iteration of the stationary gain."""
        if not self._discrete:
            raise NotImplementedError("Continuous-time LQR is not built: only discrete formulations are supported (lqr.py:217)")
        m = self._model
        self._max_iter, self._tol = int(max_iter), float(tol)
        self._plant = None
        compile_only = bool(os.environ.get('HILO_JIT_COMPILE_ONLY'))
        if m.name == 'lti':
            from ._device import device
            self._dev = None if compile_only else device(self._dev_index)
        else:
            self._plant = m._linearization_handle(self._dev_index)
            self._dev = self._plant._dev
        self._n_x, self._n_u, self._n_p = m.n_x, m.n_u, m.n_p
        self._Q = self._R = self._K = self._P = self._keys = None
        self._N = np.zeros((self._n_x, self._n_u))
        self._is_setup = True

    def _opts(self):
        o = _lib.LqrOpts()
        o.horizon, o.max_iter, o.tol = (0 if self._horizon is None else self._horizon), self._max_iter, self._tol
        return o

    # ---- the controller ------------------------------------------------------------------------
    def _rows(self, v, n, what):
        """[n] or [B, n] -> device tensor [B, n] and whether a batch axis came with it"""
        t = to_dev(v, self._dev)
        batched = t.dim() >= 2
        if t.dim() > 2 or t.numel() % max(n, 1) or (t.dim() == 2 and t.shape[1] != n) or (t.dim() <= 1 and t.numel() != n):
            raise ValueError(f"Dimension mismatch. Supplied dimension for the {what} is {list(t.shape)}, but required dimension is "
                             f"[{n}] or [B, {n}].")
        return t.reshape(-1, n).contiguous(), batched

    def call(self, *args, x=None, p=None, x_eq=None, u_eq=None, **kwargs):
        """u = -K x (lqr.py:262-306), or u = u_eq - K (x - x_eq) with the Jacobians taken at (x_eq, u_eq) per instance.

        x [n_x] or [B, n_x]; p, x_eq, u_eq likewise with their widths, a leading axis of 1 (or none) shared by the batch; a missing p
        means zeros.  numpy in -> numpy out; device tensors in -> device tensors out without a host copy (the status of the solve is
        then looked at when `status`, `K` or `P` are read).  Without x_eq / u_eq the Jacobians are those at the model's equilibrium
        point (`set_equilibrium_point`, default the origin) and u = -K x: the reference's deviation variables.  The gain is kept
        while p, x_eq and u_eq are what they were at the previous call (host data: the same values; a device tensor: the same
        object, not written since) - `call` is then `hilo_lqr_apply` alone; otherwise one `hilo_lqr_call` when the operating data
        come per instance, and a gain for the one operating point followed by `hilo_lqr_apply` when they are shared."""
        if not self._is_setup:
            raise RuntimeError("LQR is not set up. Run LQR.setup(...) before calling the LQR.")
        if self._Q is None:
            raise RuntimeError("Matrix Q is not set properly. To ensure that a unique solution exists, the matrix Q "
                               "needs to be symmetric, real-valued and positive semidefinite.")
        if self._R is None:
            raise RuntimeError("Matrix R is not set properly. To ensure that a unique solutions exists, the matrix R "
                               "needs to be symmetric, real-valued and positive definite.")
        if x is None:
            raise ValueError("No state information was supplied to the LQR!")
        lib, dev = _lib.lib(), self._dev
        nx, nu, n_p = self._n_x, self._n_u, self._n_p
        host = not isinstance(x, torch.Tensor)
        xt, x_batched = self._rows(x, nx, 'states')
        B = xt.shape[0]
        lti = self._model.name == 'lti'
        # (the model's own equilibrium point is part of the operating data: `set_equilibrium_point` on the private copy after a solve)
        operating = (p, x_eq, u_eq, getattr(self._model, '_x_eq', None), getattr(self._model, '_u_eq', None))
        hit = self._K is not None and self._keys is not None and all(k.matches(v) for k, v in zip(self._keys, operating))
        if hit:
            xe, ue, Bop = self._eq[0], self._eq[1], self._bop
        else:
            ops = {}
            if n_p and not lti:
                ops['p'] = self._rows(np.zeros(n_p) if p is None else p, n_p, 'parameters')
            if x_eq is not None:
                ops['x_eq'] = self._rows(x_eq, nx, 'equilibrium states')
            if u_eq is not None:
                ops['u_eq'] = self._rows(u_eq, nu, 'equilibrium inputs')
            Bop = max([t.shape[0] for t, _ in ops.values()] + [1])
            for name, (t, _) in ops.items():
                if t.shape[0] not in (1, Bop):
                    raise ValueError(f"{name}: batch {t.shape[0]} does not match {Bop}")
            # (an LTI model has ONE gain whatever the set-points are: K and P without a batch axis)
            self._batched = not lti and any(b for _, b in ops.values())
            pt = ops['p'][0] if 'p' in ops else None
            xe = ops['x_eq'][0].expand(Bop, -1).contiguous() if 'x_eq' in ops else None
            ue = ops['u_eq'][0].expand(Bop, -1).contiguous() if 'u_eq' in ops else None
        if B not in (1, Bop) and Bop != 1:
            raise ValueError(f"states: batch {B} does not match {Bop} operating points")
        if B == 1 and Bop > 1:
            xt = xt.expand(Bop, -1).contiguous()
            B = Bop
        u = torch.empty(B, nu, dtype=torch.float64, device=dev)
        fused = False
        if not hit:
            nk = 1 if lti else Bop                      # gains solved for: every row of K, P and stats is written by the launch below
            K = torch.empty(nk, nu, nx, dtype=torch.float64, device=dev)
            P = torch.empty(nk, nx, nx, dtype=torch.float64, device=dev)
            stats = torch.empty(nk, 2, dtype=torch.int32, device=dev)
            opts = self._opts()
            if lti:
                A, Bm = to_dev(self._model.A, dev), to_dev(self._model.B, dev)
                _lib.check(lib.hilo_lqr_gain(nx, nu, 1, ptr(A), 0, ptr(Bm), 0, ptr(self._Qd), 0, ptr(self._Rd), 0, None, 0, C.byref(opts),
                                             ptr(K), ptr(P), ptr(stats), stream_ptr(dev)))
            else:
                # the Jacobians at the operating point handed over, else at the model's equilibrium point (the feedback then stays
                # u = -K x: only the gains are computed there)
                m = self._model
                lin_x, lin_u = xe, ue
                own_eq = x_eq is None and u_eq is None and (getattr(m, '_x_eq', None) is not None or getattr(m, '_u_eq', None) is not None)
                if own_eq:
                    lin_x = None if m._x_eq is None else to_dev(m._x_eq, dev).reshape(1, nx).expand(Bop, -1).contiguous()
                    lin_u = None if m._u_eq is None else to_dev(m._u_eq, dev).reshape(1, nu).expand(Bop, -1).contiguous()
                fused = Bop == B and not own_eq
                _lib.check(lib.hilo_lqr_call(self._plant._handle, C.byref(opts), Bop, ptr(xt) if fused else None, ptr(lin_x), ptr(lin_u),
                                             ptr(pt), (n_p if pt is not None and pt.shape[0] == Bop and Bop > 1 else 0), ptr(self._Qd),
                                             ptr(self._Rd), None, ptr(K), ptr(P), ptr(u) if fused else None, ptr(stats), stream_ptr(dev)))
            self._K, self._P, self._stats, self._eq, self._bop = K, P, stats, (xe, ue), Bop
            self._keys = [_Key(v) for v in operating]
            self._checked = False
        self._host = host
        if not fused:
            _lib.check(lib.hilo_lqr_apply(nx, nu, B, ptr(self._K), (nu * nx if self._K.shape[0] > 1 else 0), ptr(xt), ptr(xe), ptr(ue), ptr(u),
                                          stream_ptr(dev)))
        if host and not hit:
            self._check_status()
        out = u if (x_batched or B > 1) else u[0]
        return out.cpu().numpy() if host else out


LQR = LinearQuadraticRegulator

__all__ = ['LinearQuadraticRegulator', 'LQR']
