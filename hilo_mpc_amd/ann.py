"""Feed-forward neural network: the inference half of the reference's `ArtificialNeuralNetwork`
(hilo_mpc/modules/machine_learning/nn/nn.py, layer.py) on the device.

    ann = ANN(['S', 'I'], ['mu', 'Rfp', 'Rab'])
    ann.add_layers(Layer.dense(10, activation='sigmoid'))
    ann.load_torch(trained_sequential)              # or set_weights(weights, bias)
    ann.setup()
    y = ann.predict(X)                              # X [n_features, m] -> [n_labels, m], one fused kernel (csrc/hilo_ann.hip)
    model.substitute_from(ann)                      # the network as expressions inside a model (Model.substitute_from)

The network is input scaling `(x - mean) / scale`, the dense layers `h <- act(W h + b)`, a linear output layer ("the output layer
is assumed to be linear", util/machine_learning.py:521-578 `net_to_casadi_graph`) and output scaling `y * scale + mean`.
Training stays with torch: `load_torch` reads the `Linear` layers of a trained `nn.Sequential`.
"""
import ctypes as C

import numpy as np

from . import _lib
from . import expr as ex
from .expr import Expr

ACTIVATIONS = {'linear': 0, 'sigmoid': 1, 'tanh': 2, 'relu': 3, 'softplus': 4}      # include/hilo_hip.h HILO_ANN_ACT_*
_REFUSED = ('softmax', 'scale')
MAX_FEATURES, MAX_LABELS, MAX_WIDTH, MAX_HIDDEN = 32, 16, 64, 8                   # include/hilo_hip.h HILO_ANN_MAX_*


def _is_list_like(v):
    return isinstance(v, (list, tuple, set, np.ndarray))


def _activation(name):
    name = 'sigmoid' if name is None else str(name).lower().replace(' ', '_')
    if name in _REFUSED:
        raise NotImplementedError(f"Activation function '{name}' is not built (available: {sorted(ACTIVATIONS)})")
    if name not in ACTIVATIONS:
        raise ValueError(f"Activation function '{name}' not recognized (available: {sorted(ACTIVATIONS)})")
    return name


class Layer:
    """layer.py `Layer`: base layer; `Layer.dense(...)` / `Layer.dropout(...)` build the layers."""
    type = None

    def __init__(self, nodes, activation=None, initializer=None, parent=None, **kwargs):
        self._nodes = int(nodes)
        self._activation = _activation(activation)
        self._initializer = initializer          # kept for the record: weights come from set_weights / load_torch
        self.parent = parent

    def __len__(self):
        return self._nodes

    nodes = property(lambda s: s._nodes)
    activation = property(lambda s: s._activation)
    initializer = property(lambda s: s._initializer)

    @staticmethod
    def dense(nodes, activation='linear', initializer=None, parent=None, **kwargs):
        """One Dense layer for an integer `nodes`, a list of them for a list; activation (and initializer) are then one value for
        all layers or a list with one entry per layer.  Dropout layers are added on their own with `Layer.dropout`."""
        n = len(nodes) if _is_list_like(nodes) else None
        what = "nodes" if n is None else f"nodes list of length {n}"

        def per_layer(value, label):
            if not _is_list_like(value):
                return (n or 1) * [value]
            if len(value) != (n if n is not None else -1):
                raise ValueError(f"Dimension mismatch between supplied {what} and supplied {label} list of length {len(value)}")
            return list(value)
        acts, inits = per_layer(activation, "activation function"), per_layer(initializer, "initializer")
        layers = [Dense(k, activation=a, initializer=i, parent=parent, **kwargs)
                  for k, a, i in zip(nodes if n is not None else [nodes], acts, inits)]
        return layers if n is not None else layers[0]

    @staticmethod
    def dropout(rate, parent=None):
        return Dropout(rate, parent=parent)


class Dense(Layer):
    """layer.py:298-316."""
    type = 'Dense'

    def __init__(self, nodes, activation='linear', initializer=None, parent=None, **kwargs):
        super().__init__(nodes, activation=activation, initializer=initializer, parent=parent, **kwargs)
        if self._nodes < 1:
            raise ValueError(f"A dense layer needs at least one node, got {nodes}")


class Dropout(Layer):
    """layer.py:319-340: only acts during training; accepted and ignored by inference and by the expression graph."""
    type = 'Dropout'

    def __init__(self, rate, parent=None):
        super().__init__(0, activation='linear', parent=parent)
        self.rate = float(rate)


# ---- activations as expressions ------------------------------------------------------------------------------------------
# Forms whose values AND derivatives stay finite for any pre-activation the exponent range allows (+-800 and beyond):
#   sigmoid(v)  = 1 / (1 + exp(-max(v, -700)))           one exponential.  Without the clamp the value at v = -800 is the right 0 but
#                 the derivative (1/inf)^2 * inf = NaN; with it exp stays finite, the derivative below -700 is 0 (the clamp's) and the
#                 value there is 1e-304 instead of something smaller still
#   tanh(v)     = 2 sigmoid(2 v) - 1                      (expr.tanh is inf / inf for large v)
#   softplus(v) = max(v, 0) + log(1 + exp(-|v|))
# max in the |.| form of expr.fmax (derivative 1/2 at the tie).
_CLAMP = 700.0


def _sigmoid(v):
    w = v + _CLAMP
    c = v + 0.5 * (ex.fabs(w) - w)                # max(v, -700), and exactly v above the clamp: |w| - w is an exact 0 there
    return 1.0 / (1.0 + ex.exp(-c))


def _softplus(v):
    a = ex.fabs(v)
    return 0.5 * (v + a) + ex.log(1.0 + ex.exp(-a))


_ACT_EXPR = {
    'linear': lambda v: v,
    'sigmoid': _sigmoid,
    'tanh': lambda v: 2.0 * _sigmoid(2.0 * v) - 1.0,
    'relu': lambda v: ex.fmax(0.0, v),
    'softplus': _softplus,
}


class ArtificialNeuralNetwork:
    """nn.py `ArtificialNeuralNetwork(features, labels, id=None, name=None, **kwargs)`; inference and neural terms in models."""

    def __init__(self, features, labels, id=None, name=None, **kwargs):
        self._features = [features] if isinstance(features, str) else list(features)
        self._labels = [labels] if isinstance(labels, str) else list(labels)
        if not self._features or not self._labels:
            raise ValueError("an ANN needs at least one feature and one label")
        self.id, self.name = id, name
        self.seed = kwargs.get('seed')
        self.learning_rate = kwargs.get('learning_rate', .001)
        self.loss, self.optimizer, self.metric = kwargs.get('loss', 'mse'), kwargs.get('optimizer', 'adam'), kwargs.get('metric')
        self._layers = []
        self._weights = self._bias = None
        self._x_scaling = self._y_scaling = None
        self._handle, self._dev = None, None

    features = property(lambda s: list(s._features))
    labels = property(lambda s: list(s._labels))
    n_features = property(lambda s: len(s._features))
    n_labels = property(lambda s: len(s._labels))
    layers = property(lambda s: list(s._layers))

    def _dense(self):
        return [l for l in self._layers if l.type != 'Dropout']

    @property
    def depth(self):
        """nn.py:238-243: number of layers that are not dropout layers."""
        return len(self._dense())

    @property
    def shape(self):
        """nn.py:246-252: (n_features, nodes of the hidden layers ..., n_labels)."""
        return (self.n_features,) + tuple(l.nodes for l in self._dense()) + (self.n_labels,)

    def add_layers(self, layers):
        """nn.py:266-277: a layer or a (nested) list of layers."""
        if _is_list_like(layers):
            for layer in layers:
                self.add_layers(layer)
            return
        if not isinstance(layers, Layer):
            raise TypeError(f"expected a Layer, got {type(layers).__name__}")
        self._layers.append(layers)
        layers.parent = self
        self._weights = self._bias = None        # the weights belonged to the old shape
        self._destroy()

    # ---- weights ------------------------------------------------------------------------------------------------------
    def _map_shapes(self):
        s = self.shape
        return [(s[k + 1], s[k]) for k in range(len(s) - 1)]

    def _map_name(self, k):
        return f"dense layer {k}" if k < self.depth else "the output layer"

    def set_weights(self, weights, bias):
        """One `W_k [n_out, n_in]` and one `b_k [n_out]` per dense layer plus the (linear) output layer: the `nn.Linear` convention,
        what the reference's `get_weights_and_bias` returns."""
        shapes = self._map_shapes()
        weights, bias = list(weights), list(bias)
        if len(weights) != len(shapes) or len(bias) != len(shapes):
            raise ValueError(f"the network has {self.depth} dense layers and an output layer: expected {len(shapes)} weight matrices "
                             f"and bias vectors, got {len(weights)} and {len(bias)}")
        W, b = [], []
        for k, (shp, w, v) in enumerate(zip(shapes, weights, bias)):
            w = np.array(w.detach().cpu().numpy() if hasattr(w, 'detach') else w, dtype=np.float64)
            v = np.array(v.detach().cpu().numpy() if hasattr(v, 'detach') else v, dtype=np.float64).reshape(-1)
            if w.shape != shp:
                raise ValueError(f"Dimension mismatch. The weights of {self._map_name(k)} have the shape {tuple(w.shape)}, but the "
                                 f"required shape is {shp}.")
            if v.shape != (shp[0],):
                raise ValueError(f"Dimension mismatch. The bias of {self._map_name(k)} has {v.size} entries, but {shp[0]} are "
                                 f"required.")
            if not (np.isfinite(w).all() and np.isfinite(v).all()):
                raise ValueError(f"non-finite weights or bias in {self._map_name(k)}")
            W.append(w)
            b.append(v)
        self._weights, self._bias = W, b
        self._destroy()

    def load_torch(self, module_or_state_dict):
        """Weights from a trained torch network: the `Linear` layers of an `nn.Sequential` (or any module) in order, or the
        `<k>.weight` / `<k>.bias` pairs of its state dict in order."""
        import torch
        if isinstance(module_or_state_dict, torch.nn.Module):
            lin = [m for m in module_or_state_dict.modules() if isinstance(m, torch.nn.Linear)]
            if any(m.bias is None for m in lin):
                raise ValueError("a Linear layer without bias cannot be loaded")
            W, b = [m.weight for m in lin], [m.bias for m in lin]
        else:
            sd = module_or_state_dict
            W = [v for k, v in sd.items() if k.endswith('weight') and getattr(v, 'ndim', 0) == 2]
            b = [v for k, v in sd.items() if k.endswith('bias')]
        self.set_weights(W, b)
        return self

    def is_trained(self):
        return self._weights is not None

    def train(self, *args, **kwargs):
        raise NotImplementedError("training is not offloaded: train the network with torch and hand it over with "
                                  "ANN.load_torch(module) (or ANN.set_weights(weights, bias))")

    # ---- scaling ---------------------------------------------------------------------------------------------------------
    @staticmethod
    def _scaling(mean, scale, n, what):
        if mean is None and scale is None:
            return None
        if hasattr(mean, 'mean_') and scale is None:          # a fitted StandardScaler
            mean, scale = mean.mean_, mean.scale_
        mean = np.zeros(n) if mean is None else np.array(mean, dtype=np.float64).reshape(-1)
        scale = np.ones(n) if scale is None else np.array(scale, dtype=np.float64).reshape(-1)
        if mean.size != n or scale.size != n:
            raise ValueError(f"Dimension mismatch. The {what} scaling has {mean.size} means and {scale.size} scales, but required "
                             f"dimension is {n}.")
        if not (np.isfinite(mean).all() and np.isfinite(scale).all()) or (scale == 0).any():
            raise ValueError(f"the {what} scaling needs finite means and finite non-zero scales")
        return mean, scale

    def set_input_scaling(self, mean=None, scale=None):
        """`StandardScaler` semantics: the network sees (x - mean) / scale."""
        self._x_scaling = self._scaling(mean, scale, self.n_features, 'input')
        self._destroy()

    def set_output_scaling(self, mean=None, scale=None):
        """`StandardScaler` semantics: the labels are y * scale + mean."""
        self._y_scaling = self._scaling(mean, scale, self.n_labels, 'output')
        self._destroy()

    def set_scaling(self, input_mean=None, input_scale=None, output_mean=None, output_scale=None):
        self.set_input_scaling(input_mean, input_scale)
        self.set_output_scaling(output_mean, output_scale)

    # ---- device ----------------------------------------------------------------------------------------------------------
    def _pack(self):
        """The arguments of `hilo_ann_create` (include/hilo_hip.h): every map zero padded, W row-major [n_out_pad][n_in_pad] with
        n_out_pad = nodes rounded up to 16 and n_in_pad = n_features rounded up to 4 (first map) or the n_out_pad before."""
        if not self.is_trained():
            raise RuntimeError("The ANN has not been trained yet. Hand the weights over with load_torch() or set_weights().")
        hidden = self._dense()
        widths = np.array([l.nodes for l in hidden], dtype=np.int32)
        acts = np.array([ACTIVATIONS[l.activation] for l in hidden], dtype=np.int32)
        n_in = -(-self.n_features // 4) * 4
        Wp, bp, w_off, b_off = [], [], [], []
        wo = bo = 0
        for w, v in zip(self._weights, self._bias):
            n_out = -(-w.shape[0] // 16) * 16
            blk = np.zeros((n_out, n_in))
            blk[:w.shape[0], :w.shape[1]] = w
            vec = np.zeros(n_out)
            vec[:v.size] = v
            Wp.append(blk.ravel())
            bp.append(vec)
            w_off.append(wo)
            b_off.append(bo)
            wo += blk.size
            bo += n_out
            n_in = n_out
        return dict(widths=widths, acts=acts, W=np.ascontiguousarray(np.concatenate(Wp)), b=np.ascontiguousarray(np.concatenate(bp)),
                    w_offsets=w_off, b_offsets=b_off,
                    x_mean=None if self._x_scaling is None else np.ascontiguousarray(self._x_scaling[0]),
                    x_scale=None if self._x_scaling is None else np.ascontiguousarray(self._x_scaling[1]),
                    y_mean=None if self._y_scaling is None else np.ascontiguousarray(self._y_scaling[0]),
                    y_scale=None if self._y_scaling is None else np.ascontiguousarray(self._y_scaling[1]))

    def setup(self, device_index=None, **kwargs):
        """Packs the network and uploads it (nn.py:405 `setup` builds the torch module; here the device copy)."""
        from ._device import device
        pk = self._pack()
        self._dev = device(device_index)

        def p(a):
            return None if a is None else a.ctypes.data
        h = C.c_void_p()
        _lib.check(_lib.lib().hilo_ann_create(self._dev.index, self.n_features, self.n_labels, len(pk['widths']), p(pk['widths']),
                                              p(pk['acts']), p(pk['W']), p(pk['b']), p(pk['x_mean']), p(pk['x_scale']), p(pk['y_mean']),
                                              p(pk['y_scale']), C.byref(h)))
        self._destroy()
        self._handle = h
        return self

    def is_setup(self):
        """nn.py:470 `is_setup`."""
        return self._handle is not None

    def _destroy(self):
        if getattr(self, '_handle', None) is not None:
            _lib.lib().hilo_ann_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self._destroy()
        except Exception:
            pass

    def predict(self, X_query, out=None):
        """nn.py:536-544: X_query [n_features, m] -> [n_labels, m]; numpy in -> numpy out, a device tensor in -> a device tensor
        out without a host copy.  Device arrays with unit stride along the queries are read (and, `out`, written) in place whatever
        their row pitch: a column block of a larger array needs no copy."""
        import torch
        from ._device import ptr, stream_ptr, to_dev
        if self._handle is None:
            raise RuntimeError("The ANN has not been set up yet. Please run the setup() method before predicting.")

        def view_ok(t):
            return (isinstance(t, torch.Tensor) and t.ndim == 2 and t.dtype is torch.float64 and t.device == self._dev and
                    t.stride(1) == 1 and (t.shape[0] == 1 or t.stride(0) >= t.shape[1]))
        host = not isinstance(X_query, torch.Tensor)
        if host:
            Xa = np.asarray(X_query, dtype=np.float64)
            Xq = to_dev(Xa.reshape(-1, 1) if Xa.ndim == 1 else Xa, self._dev)      # a vector is one query
        else:
            Xq = X_query if view_ok(X_query) else to_dev(X_query, self._dev)
        if Xq.ndim == 1:
            Xq = Xq.reshape(-1, 1)
        if Xq.shape[0] != self.n_features:
            raise ValueError(f"Dimension mismatch. Supplied dimension for the features is {Xq.shape[0]}, but required "
                             f"dimension is {self.n_features}.")
        m = Xq.shape[1]
        if out is None:
            Y = torch.empty(self.n_labels, m, dtype=torch.float64, device=self._dev)
        else:
            if host or not view_ok(out) or tuple(out.shape) != (self.n_labels, m):
                raise ValueError(f"out must be a float64 device array [{self.n_labels}, {m}] with unit stride along the queries "
                                 f"(and the queries a device array)")
            Y = out
        ldx = Xq.stride(0) if Xq.shape[0] > 1 else max(m, 1)
        ldy = Y.stride(0) if Y.shape[0] > 1 else max(m, 1)
        _lib.check(_lib.lib().hilo_ann_predict(self._handle, m, ptr(Xq), max(ldx, m, 1), ptr(Y), max(ldy, m, 1), stream_ptr(self._dev)))
        return Y.cpu().numpy() if host else Y

    # ---- the network as expressions ------------------------------------------------------------------------------------------
    def n_nodes(self):
        """Neurons of the expression graph (hidden nodes + labels): what the size thresholds of `Model.substitute_from` count."""
        return sum(l.nodes for l in self._dense()) + self.n_labels

    def expressions(self, feature_exprs):
        """The graph `net_to_casadi_graph` writes (util/machine_learning.py:521-578) over the given feature expressions: a list
        of n_labels `Expr`, the weights as numbers.  The hidden activations are shared objects, so code emitted for several
        labels evaluates the network once."""
        if not self.is_trained():
            raise RuntimeError("The ANN has not been trained yet. Hand the weights over with load_torch() or set_weights().")
        f = [Expr.wrap(e) for e in feature_exprs]
        if len(f) != self.n_features:
            raise ValueError(f"Dimension mismatch. Supplied dimension for the features is {len(f)}, but required "
                             f"dimension is {self.n_features}.")
        if self._x_scaling is not None:
            f = [(e - float(mu)) / float(sc) for e, mu, sc in zip(f, *self._x_scaling)]
        acts = [_ACT_EXPR[l.activation] for l in self._dense()] + [_ACT_EXPR['linear']]
        # Creation order is emission order (codegen.Emitter), and every value of the emitted code carries its derivative
        # directions, so the order decides how many of them are alive at once.  A hidden neuron is created on demand, as the row
        # sum over its inputs followed by its activation; the output layer goes column by column - neuron j of the last hidden
        # layer is created and at once added to the running sums of the labels.  With one hidden layer a hidden value then lives
        # for one column; deeper networks keep one layer of activations, not two.  Each sum runs over its inputs in order, then
        # the bias.
        hidden = list(zip(self._weights[:-1], self._bias[:-1], acts[:-1]))
        memo = {}

        def value(l, j):                          # activation j of hidden layer l (l = 0: the features)
            if l == 0:
                return f[j]
            if (l, j) not in memo:
                W, b, act = hidden[l - 1]
                sm = None
                for k in range(W.shape[1]):
                    if W[j, k] != 0.0:
                        t = float(W[j, k]) * value(l - 1, k)
                        sm = t if sm is None else sm + t
                memo[(l, j)] = act(Expr.wrap(float(b[j])) if sm is None else sm + float(b[j]))
            return memo[(l, j)]
        W, b = self._weights[-1], self._bias[-1]
        sums = [None] * W.shape[0]
        for j in range(W.shape[1]):
            for i in range(W.shape[0]):
                if W[i, j] != 0.0:
                    t = float(W[i, j]) * value(len(hidden), j)
                    sums[i] = t if sums[i] is None else sums[i] + t
        f = [Expr.wrap(float(b[i])) if sums[i] is None else sums[i] + float(b[i]) for i in range(W.shape[0])]
        if self._y_scaling is not None:
            f = [e * float(sc) + float(mu) for e, mu, sc in zip(f, *self._y_scaling)]
        return f


ANN = ArtificialNeuralNetwork
