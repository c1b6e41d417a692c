"""Data generation for learning a model term: `DataGenerator`, `DataSet` (hilo_mpc/util/data.py:80-1209) and what
`Model.generate_data` needs (dynamic_model.py:4214 onwards), for a BATCH of experiments in ONE launch (`hilo_datagen_run`,
csrc/hilo_datagen.h).

The reference excites one plant with a signal drawn by numpy's global generator, simulates it, and slices the trajectory into
features and labels on the host.  Here B plants - each with its own initial state, parameters and random stream - run over
`n_samples * steps` sampling intervals without leaving the device: the signal is evaluated inside the kernel, the features and
labels are written in training layout, the measurement noise is added there.  Every random number is a pure function of
(seed, instance number, index) - Philox4x32-10, the particle filter's generator - so a row depends neither on the batch it was
drawn in nor on any generator state of the host.

Deviations from the reference: the draws are not numpy's; the noise entry of state k acts on state k also when
`skip` is not empty (the reference indexes its noise array with the state number, data.py:776); an unknown `output` is refused
instead of read as 'absolute'; inputs whose chirps have different total lengths and a hyperbolic chirp whose logarithm leaves
its domain are refused.  Not built: `closed_loop` (and with it `use_input_as_label`), plants under 'bdf' / 'idas', algebraic
states and parameters as features, `DataSet.append / sort / copy / plot*`, the euclidean-distance selection."""
import ctypes as C
import secrets
import warnings

import numpy as np

MAX_NU, MAX_NX, MAX_SEG = 4, 12, 8                       # HILO_DATAGEN_MAX_NU / _NX / _SEG
UNIFORM, NORMAL, CHIRP = 0, 1, 2                         # HILO_DATAGEN_*
CHIRP_TYPES = {'linear': 0, 'exponential': 1, 'hyperbolic': 2}
NOISE_NONE, NOISE_UNIFORM, NOISE_NORMAL = 0, 1, 2
_MASK64 = (1 << 64) - 1


def is_list_like(v):
    return isinstance(v, (list, tuple, set, np.ndarray))


def _get_distribution_information(**kwargs):
    """data.py:1170-1209, defaults and warnings included."""
    distribution = kwargs.get('distribution')
    if distribution is None:
        distribution = 'random_normal'
    seed = kwargs.get('seed')
    info = None
    if distribution == 'random_uniform':
        lb = kwargs.get('lb')
        if lb is None:
            lb = kwargs.get('lower_bound')
        ub = kwargs.get('ub')
        if ub is None:
            ub = kwargs.get('upper_bound')
        if lb is None:
            warnings.warn("No lower bound was supplied for random uniform distribution. Assuming lower bound of 0.")
            lb = 0.
        if ub is None:
            warnings.warn("No upper bound was supplied for random uniform distribution. Assuming upper bound of 1.")
            ub = 1.
        info = [lb, ub]
    elif distribution == 'random_normal':
        std = kwargs.get('std')
        if std is None:
            var = kwargs.get('var')
            if var is not None:
                std = np.sqrt(var)
        if std is None:
            warnings.warn("No standard deviation was supplied for random normal distribution. Assuming a standard "
                          "deviation of 1.")
            std = 1.
        info = std
    return distribution, seed, info


def feature_label_names(state_names, input_names, keep, output, shift):
    """The names of data.py:1060-1131: features [x_k-shift .. x_k-1, x_k, u], labels x_k+1 or delta_x."""
    kept = [n for i, n in enumerate(state_names) if i in keep]
    if output == 'difference':
        features = [n + '_k' if shift > 0 else n for n in kept] + list(input_names)
        labels = ['delta_' + n for n in kept]
    else:
        features = [n + '_k' for n in kept] + list(input_names)
        labels = [n + '_k+1' for n in kept]
    for k in range(shift):
        features = [n + f'_k-{k + 1}' for n in kept] + features
    return features, labels


class DataSet:
    """What a run leaves: a small holder (not the reference's TimeSeries machinery).

    features / labels   the reference's names (`x_k-1`, `x_k`, `u`, `x_k+1` / `delta_x`)
    raw_data            (features [n_f, N * B], labels [n_l, N * B]) in the reference's orientation, column r * B + b for row r of
                        instance b: transposed VIEWS of the kernel's buffers (device tensors for device input, numpy otherwise)
    time [N]            t0 + (r + shift + 1) dt, the time of the label of row r
    status [B]          the integrator's status per instance (0: ok), x [T + 1, B, n_x] / u [T, B, n_u] the clean trajectories"""

    def __init__(self, features, labels, F, L, time, status, x, u, dt, stats=None):
        self._features, self._labels = list(features), list(labels)
        self._F, self._L = F, L                     # [N, B, n_f], [N, B, n_l]
        self.time, self.status, self.x, self.u, self.stats = time, status, x, u, stats
        self._dt = dt
        self._train_index = []
        self._test_index = []

    def __len__(self):
        return self._F.shape[0] * self._F.shape[1]

    features = property(lambda s: list(s._features))
    labels = property(lambda s: list(s._labels))
    sampling_time = property(lambda s: s._dt)
    dt = sampling_time
    n_rows = property(lambda s: s._F.shape[0])
    n_instances = property(lambda s: s._F.shape[1])

    @property
    def raw_data(self):
        n = len(self)
        return self._F.reshape(n, self._F.shape[2]).T, self._L.reshape(n, self._L.shape[2]).T

    def finite_rows(self):
        """Index of the columns of raw_data without NaN (an instance whose integration failed has some)."""
        f, l = self.raw_data
        if isinstance(f, np.ndarray):
            return np.flatnonzero(~(np.isnan(f).any(axis=0) | np.isnan(l).any(axis=0)))
        import torch
        return torch.nonzero(~(torch.isnan(f).any(dim=0) | torch.isnan(l).any(dim=0))).reshape(-1)

    def _reduce_data(self, method, distance_threshold=None, downsample_factor=None):
        if method == 'downsample':
            if downsample_factor is None or int(downsample_factor) < 1:
                raise ValueError(f"the method 'downsample' needs a downsample_factor of at least 1, got {downsample_factor}")
            return len(self), np.arange(0, len(self), int(downsample_factor))
        if method == 'euclidean_distance':
            raise NotImplementedError("Data selection method 'euclidean_distance' is sequential host work and not built; select "
                                      "with 'downsample' or index raw_data yourself")
        raise NotImplementedError(f"Data selection method '{method}' not implemented or recognized")

    def select_train_data(self, method, distance_threshold=None, downsample_factor=None):
        dim, self._train_index = self._reduce_data(method, distance_threshold, downsample_factor)
        print(f"{len(self._train_index)}/{dim} data points selected for training")

    def select_test_data(self, method, distance_threshold=None, downsample_factor=None):
        dim, self._test_index = self._reduce_data(method, distance_threshold, downsample_factor)
        print(f"{len(self._test_index)}/{dim} data points selected for testing")

    def _take(self, index):
        f, l = self.raw_data
        if isinstance(f, np.ndarray):
            index = np.asarray(index, dtype=np.int64)
        else:
            import torch
            index = torch.as_tensor(np.asarray(index, dtype=np.int64), device=f.device)
        return f[:, index], l[:, index]

    train_data = property(lambda s: s._take(s._train_index))
    test_data = property(lambda s: s._take(s._test_index))


class DataGenerator:
    """`DataGenerator(model, x0, p0)`, one of `random_uniform` / `random_normal` / `chirp`, then `run`; the result is `.data`.

    x0 [B, n_x] or one row (None: the model's initial conditions), p0 [B, n_p] or one row (None: the model's initial parameter
    values): instance b of the batch is experiment number `instance_offset + b` - its draws are those of that number whatever the
    batch.  Device tensors in give device tensors out, numpy in gives numpy out."""

    def __init__(self, model, x0=None, p0=None, use_input_as_label=False, instance_offset=0, z0=None):
        from .model import Model
        if not isinstance(model, Model):
            raise TypeError("DataGenerator excites a Model")
        if not model._is_setup:
            raise RuntimeError("Model is not set up. Run Model.setup() before generating data.")
        if x0 is None:
            sim = getattr(model, '_sim', None)
            x0 = sim['x'][0] if sim else None
            if x0 is None:
                raise RuntimeError("No initial dynamical states found. Please supply initial dynamical states or set "
                                   "initial conditions of the model before generating data!")
        n_z = getattr(model, 'n_z', 0)
        if n_z > 0:
            if z0 is None and (getattr(model, '_sim', None) or {}).get('_z0') is None:
                raise RuntimeError("No initial algebraic states found. Please supply initial algebraic states or set "
                                   "initial conditions of the model before generating data!")
            raise NotImplementedError("data generation is built for models without algebraic states")
        if model.name == 'lti':
            p0 = model.lti_parameters()
        elif p0 is None:
            p0 = getattr(model, '_p_init', None)
            if model.n_p > 0 and p0 is None:
                raise RuntimeError("No parameter values found. Please supply parameter values or set values for the "
                                   "parameters of the model before generating data!")
        if use_input_as_label:
            raise NotImplementedError("use_input_as_label=True belongs to closed_loop data generation, which is not built")
        if model.n_u < 1:
            raise ValueError("the model has no inputs to excite")
        if model.n_u > MAX_NU or model.n_x > MAX_NX:
            raise NotImplementedError(f"the kernel holds the signal parameters of up to {MAX_NU} inputs and the noise parameters of up "
                                      f"to {MAX_NX} states; the model has {model.n_u} inputs and {model.n_x} states")
        if model._solver in ('bdf', 'idas'):
            raise NotImplementedError(f"data generation under solver '{model._solver}' is not built: the input jumps at the sampling "
                                      f"instants, so the implicit method would restart every interval. Set the plant up with "
                                      f"Model.setup(solver='dopri5') or without a solver")
        self._model = model
        self._x0, self._p0 = x0, p0
        self._n_inputs = model.n_u
        self._instance_offset = int(instance_offset)
        if self._instance_offset < 0:
            raise ValueError(f"instance_offset must not be negative, got {instance_offset}")
        self._use_input_as_label = False
        self._signal = None
        self._data_set = None
        self.seed = None

    @property
    def data(self):
        return self._data_set

    def _fresh_seed(self, seed):
        self.seed = secrets.randbits(64) if seed is None else int(seed) & _MASK64
        return self.seed

    def _per_input(self, v, what):
        a = np.asarray(v, dtype=float)
        try:
            return np.broadcast_to(a, (self._n_inputs,)).copy()
        except ValueError:
            raise ValueError(f"Dimension mismatch. Supplied dimension for the {what} is {a.size}, but required dimension is "
                             f"{self._n_inputs} (one per input) or 1.") from None

    def _staircase(self, kind, n_samples, steps, a, b, seed):
        n_samples, steps = int(n_samples), int(steps)
        if n_samples < 1 or steps < 1:
            raise ValueError(f"n_samples and steps must be at least 1, got {n_samples} and {steps}")
        self._fresh_seed(seed)
        self._signal = dict(kind=kind, hold=steps, T=n_samples * steps, a=a, b=b, table=None)

    def random_uniform(self, n_samples, steps, lower_bound, upper_bound, seed=None):
        """data.py:806: n_samples values per input, uniform in [lower_bound, upper_bound), each held for `steps` sampling intervals."""
        self._staircase(UNIFORM, n_samples, steps, self._per_input(lower_bound, 'lower bound'),
                        self._per_input(upper_bound, 'upper bound'), seed)

    def random_normal(self, n_samples, steps, mean, variance, seed=None):
        """data.py:831: the same with normal values."""
        var = self._per_input(variance, 'variance')
        if np.any(var < 0.):
            raise ValueError(f"the variance must not be negative, got {var.tolist()}")
        self._staircase(NORMAL, n_samples, steps, self._per_input(mean, 'mean'), var, seed)

    def chirp(self, type_, amplitude, length, mean, chirp_rate, initial_phase=None, initial_frequency=None,
              initial_frequency_ratio=None):
        """data.py:856-993: per input a sequence of chirp segments mean + amplitude sin(phase(t)), t = 0, dt, .. < length:
          linear       phase = initial_phase + 2 pi (chirp_rate / 2 t + initial_frequency) t
          exponential  phase = initial_phase + 2 pi initial_frequency (chirp_rate^t - 1) / log(chirp_rate)
          hyperbolic   phase = initial_phase - 2 pi dt initial_frequency / f log(1 - f / dt t), f = 1 - 1 / initial_frequency_ratio
        with the defaults initial_phase = pi / 2 and initial_frequency = 1e-4.  Every argument: a scalar (all inputs, one segment), or
        one entry per input, itself a scalar or one entry per segment."""
        n_u = self._n_inputs
        args = [type_, amplitude, length, mean, chirp_rate, initial_phase, initial_frequency, initial_frequency_ratio]
        args = [a if is_list_like(a) else [[a] for _ in range(n_u)] for a in args]
        dt = self._model.dt
        table = np.zeros((n_u, MAX_SEG, 8))
        totals = []
        for i in range(n_u):
            ti, ai, li, mi, ci, phi, fri, rati = [list(a[i]) if is_list_like(a[i]) else [a[i]] for a in args]
            lens = [len(ti), len(ai), len(li), len(mi), len(ci), len(phi), len(fri), len(rati)]
            n_chirps = max(lens)
            if any(k != n_chirps and k != 1 for k in lens):
                what = ['types', 'amplitudes', 'lengths', 'means', 'chirp rates', 'initial phases', 'initial frequencies',
                        'initial frequency ratios']
                mismatch = [f'{w} ({k})' for w, k in zip(what, lens) if k != 1]
                raise ValueError(f"Dimension mismatch between {', '.join(mismatch[:-1])} and {mismatch[-1]}")
            ti, ai, li, mi, ci, phi, fri, rati = [v * n_chirps if len(v) != n_chirps else v
                                                  for v in (ti, ai, li, mi, ci, phi, fri, rati)]
            if n_chirps > MAX_SEG:
                raise NotImplementedError(f"the kernel's table holds up to {MAX_SEG} chirp segments per input; input {i} has {n_chirps}")
            total = 0
            for j in range(n_chirps):
                t = np.arange(0., li[j], dt)                 # the reference's grid, so the reference's point count
                tij = str(ti[j]).lower()
                if tij not in CHIRP_TYPES:
                    raise ValueError(f"Type '{ti[j]}' not recognized for chirp signal")
                phase = np.pi / 2. if phi[j] is None else float(phi[j])
                f0 = .0001 if fri[j] is None else float(fri[j])
                ratio = 0.
                if tij == 'hyperbolic':
                    if rati[j] is None:
                        raise ValueError("Initial frequency ratio for hyperbolic chirp signal was not supplied")
                    ratio = float(rati[j])
                    fraction = 1. - 1. / ratio
                    if t.size and not np.all(1. - fraction / dt * t > 0.):
                        raise ValueError(f"hyperbolic chirp {j} of input {i}: 1 - (1 - 1 / initial_frequency_ratio) t / dt is not "
                                         f"positive on the whole segment (its logarithm would hand NaN to the plant); shorten the "
                                         f"segment or choose a ratio closer to 1")
                table[i, j] = [CHIRP_TYPES[tij], t.size, float(ai[j]), float(mi[j]), float(ci[j]), phase, f0, ratio]
                total += t.size
            totals.append(total)
        if len(set(totals)) != 1:
            raise ValueError(f"the chirp signals of the inputs have different lengths: {totals} points; every input needs a value "
                             f"for every sampling interval")
        if totals[0] < 1:
            raise ValueError("the chirp signals hold no point (length < dt?)")
        self._signal = dict(kind=CHIRP, hold=0, T=totals[0], a=np.zeros(n_u), b=np.zeros(n_u), table=table)

    def closed_loop(self, controller, steps):
        raise NotImplementedError("closed_loop data generation is not built; run the loop (PID.closed_loop, SimpleControlLoop) and "
                                  "assemble the data from its trajectories")

    def _noise(self, add_noise, keep):
        """Per state (kind, seed, a, b) from the reference's two dict shapes (data.py:757-796)."""
        names = self._model.dynamical_state_names
        out = {}
        if add_noise is None:
            return out

        def entry(spec):
            distribution, seed, info = _get_distribution_information(**spec)
            seed = self.seed if seed is None else int(seed) & _MASK64
            if distribution == 'random_uniform':
                return NOISE_UNIFORM, seed, float(info[0]), float(info[1])
            if distribution == 'random_normal':
                return NOISE_NORMAL, seed, float(info), 0.
            raise ValueError(f"Distribution '{distribution}' not available/recognized for adding noise to generated data")
        for k, name in enumerate(names):
            if k in keep and isinstance(add_noise.get(name), dict):
                out[k] = entry(add_noise[name])        # the entry of state k acts on state k
        if not out:
            e = entry(add_noise)
            out = {k: e for k in keep}
        return out

    def run(self, output, skip=None, shift=0, add_noise=None, t0=0.):
        """data.py:1024-1167 for a batch, in ONE launch.  output 'absolute' (labels x_k+1) or 'difference' (x_k+1 - x_k); skip: states
        (indices or names) left out of features and labels; shift: that many past states in every feature row; add_noise: one
        distribution for all kept states - {'distribution': 'random_normal', 'std': .01, 'seed': 1} - or one such dict per state
        name.  The data set is `.data`."""
        import torch
        from . import _lib
        from ._device import ptr, stream_ptr, to_dev
        from .model import SOLVERS
        m = self._model
        if self._signal is None:
            raise RuntimeError("No excitation signal set. Run one of DataGenerator.random_uniform(), random_normal() or chirp() "
                               "before running the data generation")
        if output not in ('absolute', 'difference'):
            raise ValueError(f"Output '{output}' not recognized. Choose 'absolute' or 'difference'")
        names = m.dynamical_state_names
        skip_idx = set()
        for s in ([] if skip is None else ([skip] if isinstance(skip, (str, int)) else skip)):
            if isinstance(s, str):
                if s not in names:
                    raise ValueError(f"skip: the model has no dynamical state '{s}'. Choose out of {names}")
                s = names.index(s)
            if not 0 <= int(s) < m.n_x:
                raise ValueError(f"skip: state index {s} out of range for {m.n_x} states")
            skip_idx.add(int(s))
        keep = [k for k in range(m.n_x) if k not in skip_idx]
        if not keep:
            raise ValueError("skip leaves no state for features and labels")
        T, shift = self._signal['T'], int(shift)
        if not 0 <= shift < T:
            raise ValueError(f"shift = {shift} leaves no row: the run has {T} sampling intervals and a row needs shift + 1 of them")
        if self.seed is None:
            self._fresh_seed(None)
        noise = self._noise(add_noise, keep)

        h = m._plant_handle(None)
        dev = h._dev
        host = not isinstance(self._x0, torch.Tensor)
        xt = to_dev(self._x0, dev).reshape(-1, m.n_x)
        parts = [torch.zeros(1, m.n_u, dtype=torch.float64, device=dev)]
        if h._n_p:
            if self._p0 is None:
                raise RuntimeError("No parameter values found. Please supply parameter values or set values for the "
                                   "parameters of the model before generating data!")
            parts.append(to_dev(self._p0, dev).reshape(-1, h._n_p))
        B = max(xt.shape[0], parts[-1].shape[0])
        if xt.shape[0] not in (1, B) or parts[-1].shape[0] not in (1, B):
            raise ValueError(f"x0 holds {xt.shape[0]} rows, p0 {parts[-1].shape[0]}: give one row per instance, or one row for all")
        xt = xt.expand(B, -1).contiguous()
        Bp = parts[-1].shape[0]
        up = torch.cat([t.expand(Bp, -1) for t in parts], dim=1).contiguous()
        up_stride = up.shape[1] if Bp == B else 0

        opts = _lib.DatagenOpts()
        opts.seed, opts.instance_offset = self.seed, self._instance_offset
        opts.kind, opts.hold = self._signal['kind'], self._signal['hold']
        opts.shift, opts.difference = shift, int(output == 'difference')
        opts.skip_mask = sum(1 << k for k in skip_idx)
        for i in range(m.n_u):
            opts.a[i], opts.b[i] = self._signal['a'][i], self._signal['b'][i]
        for k, (kind, seed, a, b) in noise.items():
            opts.noise_kind[k], opts.noise_seed[k], opts.na[k], opts.nb[k] = kind, seed, a, b
        table = None if self._signal['table'] is None else to_dev(self._signal['table'], dev)
        sim = _lib.SimOpts()
        sim.t0 = float(t0)
        if m._solver is not None:
            o = m._solver_options
            sim.method, sim.max_steps = SOLVERS[m._solver], o['max_num_steps']
            sim.rtol, sim.atol, sim.h0 = o['reltol'], o['abstol'], o['first_step']
        N, nk = T - shift, len(keep)
        F = torch.empty(N, B, (shift + 1) * nk + m.n_u, dtype=torch.float64, device=dev)
        L = torch.empty(N, B, nk, dtype=torch.float64, device=dev)
        X = torch.empty(T + 1, B, m.n_x, dtype=torch.float64, device=dev)
        U = torch.empty(T, B, m.n_u, dtype=torch.float64, device=dev)
        stats = torch.empty(B, 4, dtype=torch.int32, device=dev)
        _lib.check(_lib.lib().hilo_datagen_run(h._handle, C.byref(sim), C.byref(opts), ptr(table), B, T, ptr(xt), ptr(up), up_stride,
                                               ptr(F), ptr(L), ptr(X), ptr(U), ptr(stats), stream_ptr(dev)))
        self._buffers = (F, L)                      # the kernel's buffers: raw_data of a device run are views of them
        st = stats.cpu().numpy()
        failed = int(np.count_nonzero(st[:, 0]))
        if failed:
            warnings.warn(f"{failed} of {B} instances did not reach the end of the run (integrator status in DataSet.status); their "
                          f"rows hold NaN from the first state they did not reach - DataSet.finite_rows() indexes the others")
        out = (lambda t: t.cpu().numpy()) if host else (lambda t: t)
        features, labels = feature_label_names(names, m.input_names, keep, output, shift)
        time = float(t0) + (np.arange(N) + shift + 1) * m.dt
        stats_o = out(stats)
        self._data_set = DataSet(features, labels, out(F), out(L), time if host else torch.as_tensor(time, device=dev),
                                 stats_o[:, 0], out(X), out(U), m.dt,
                                 stats={'status': stats_o[:, 0], 'n_accepted': stats_o[:, 1], 'n_rejected': stats_o[:, 2],
                                        'n_rhs': stats_o[:, 3]})
        return self._data_set


__all__ = ['DataGenerator', 'DataSet']
