"""Numpy oracle of the feed-forward network the product evaluates (hilo_mpc_amd/ann.py, csrc/hilo_ann.hip): a restatement of the
algorithm of the reference's `net_to_casadi_graph` (util/machine_learning.py:521-578) - input scaling (x - mean) / scale, the
chain h <- act(W h + b), a linear output layer, output scaling y * scale + mean - in float64 and, for the error bars of the tests,
in numpy's extended precision.  Also the shared fixtures of the ANN tests: random networks and the reference test's bioreactor
(tests/test_hybrid_models_func.py:18-49) with a network for (mu, Rs, Rfp)."""
import numpy as np


def _sigmoid(v):
    e = np.exp(-np.abs(v))                     # overflow-free on both sides
    return np.where(v >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


ACT = {
    'linear': lambda v: v,
    'sigmoid': _sigmoid,
    'tanh': np.tanh,
    'relu': lambda v: np.maximum(v, 0),
    'softplus': lambda v: np.maximum(v, 0) + np.log1p(np.exp(-np.abs(v))),
}


def forward(X, weights, bias, activations, x_scaling=None, y_scaling=None, dtype=np.float64):
    """X [nf, m] -> [nl, m].  weights[k] [n_out, n_in], bias[k] [n_out]; activations: one name per hidden layer (the last map
    is linear).  dtype=np.longdouble evaluates everything in extended precision (64-bit mantissa on x86)."""
    h = np.asarray(X, dtype=dtype)
    if x_scaling is not None:
        h = (h - np.asarray(x_scaling[0], dtype=dtype)[:, None]) / np.asarray(x_scaling[1], dtype=dtype)[:, None]
    acts = list(activations) + ['linear']
    for W, b, a in zip(weights, bias, acts):
        h = ACT[a](np.asarray(W, dtype=dtype) @ h + np.asarray(b, dtype=dtype)[:, None])
    if y_scaling is not None:
        h = h * np.asarray(y_scaling[1], dtype=dtype)[:, None] + np.asarray(y_scaling[0], dtype=dtype)[:, None]
    return h


def tolerance(X, weights, bias, activations, x_scaling=None, y_scaling=None):
    """(y64, atol): 32 x the largest difference between the float64 and the extended-precision evaluation on this data, floor
    4 ulp of max|y| (the device sums in k-blocks of 4 and its exp / log are good to 1-2 ulp)."""
    y = forward(X, weights, bias, activations, x_scaling, y_scaling)
    yl = forward(X, weights, bias, activations, x_scaling, y_scaling, dtype=np.longdouble)
    fin = np.isfinite(y)
    err = float(np.max(np.abs(y[fin] - yl[fin]))) if fin.any() else 0.0
    ymax = float(np.max(np.abs(y[fin]))) if fin.any() else 1.0
    return y, max(32.0 * err, 4.0 * np.spacing(ymax))


def random_net(nf, widths, nl, seed=0, scale=1.0):
    """Weights of the order 1 / sqrt(n_in) (pre-activations of order one), biases of order one."""
    rng = np.random.default_rng(seed)
    dims = [nf] + list(widths) + [nl]
    W = [scale * rng.normal(size=(dims[k + 1], dims[k])) / np.sqrt(dims[k]) for k in range(len(dims) - 1)]
    b = [rng.normal(size=dims[k + 1]) for k in range(len(dims) - 1)]
    return W, b


def make_ann(features, labels, widths, activations, W, b, x_scaling=None, y_scaling=None):
    from hilo_mpc_amd import ANN, Layer
    ann = ANN(features, labels)
    if widths:
        ann.add_layers(Layer.dense(list(widths), activation=list(activations)))
    ann.set_weights(W, b)
    if x_scaling is not None:
        ann.set_input_scaling(*x_scaling)
    if y_scaling is not None:
        ann.set_output_scaling(*y_scaling)
    return ann


def torch_sequential(W, b, activations):
    import torch
    mods = []
    acts = {'linear': None, 'sigmoid': torch.nn.Sigmoid, 'tanh': torch.nn.Tanh, 'relu': torch.nn.ReLU, 'softplus': torch.nn.Softplus}
    for k, (w, v) in enumerate(zip(W, b)):
        lin = torch.nn.Linear(w.shape[1], w.shape[0]).double()
        with torch.no_grad():
            lin.weight.copy_(torch.as_tensor(w))
            lin.bias.copy_(torch.as_tensor(v))
        mods.append(lin)
        if k < len(activations) and acts[activations[k]] is not None:
            mods.append(acts[activations[k]]())
    return torch.nn.Sequential(*mods)


# ---- the reference test's bioreactor (tests/test_hybrid_models_func.py:18-49) ------------------------------------------------------
FEATURES, LABELS = ['S', 'I'], ['mu', 'Rs', 'Rfp']
X0 = np.array([0.1, 40., 0., 0.])
P_REST = np.array([100., 4.])                  # Sf, If: what is left of the parameter vector


def bioreactor(dt=0.5, rates=None):
    """The model with (mu, Rs, Rfp) as parameters, or - `rates`: a function (S, I) -> three expressions - with the rates written
    into the equations by hand (parameters Sf, If only)."""
    from hilo_mpc_amd import Model
    m = Model(name='mpc_model')
    x = m.set_dynamical_states(['X', 'S', 'P', 'I'])
    u = m.set_inputs(['DS', 'DI'])
    if rates is None:
        p = m.set_parameters(['Sf', 'If', 'mu', 'Rs', 'Rfp'])
        Sf, If, mu, Rs, Rfp = p[0], p[1], p[2], p[3], p[4]
    else:
        p = m.set_parameters(['Sf', 'If'])
        Sf, If = p[0], p[1]
        mu, Rs, Rfp = rates(x[1], x[3])
    X, S, P, I = x[0], x[1], x[2], x[3]
    DS, DI = u[0], u[1]
    D_tot = DS + DI
    m.set_dynamical_equations([mu * X - D_tot * X, -Rs * X - D_tot * S + DS * Sf, Rfp * X - D_tot * P, -D_tot * I + DI * If])
    m.set_measurement_equations([X, S, P])
    m._bio_dt = dt
    return m


def bio_net(widths=(10,), activations=('sigmoid',), seed=3):
    """A network for the bioreactor's rates with inputs scaled to the operating range (S ~ 40, I ~ 2) and small outputs."""
    W, b = random_net(2, widths, 3, seed=seed)
    xs = (np.array([20., 2.]), np.array([15., 2.]))
    ys = (np.array([0.3, 0.5, 0.1]), np.array([0.05, 0.1, 0.02]))
    return W, b, list(activations), xs, ys


def bio_rhs(x, u, W, b, acts, xs, ys, p=P_REST):
    """dx/dt of the hybrid bioreactor for a batch: x [B, 4], u [B, 2] -> [B, 4] (numpy, the oracle network)."""
    r = forward(np.stack([x[:, 1], x[:, 3]]), W, b, acts, xs, ys)
    mu, Rs, Rfp = r[0], r[1], r[2]
    D = u[:, 0] + u[:, 1]
    return np.stack([mu * x[:, 0] - D * x[:, 0], -Rs * x[:, 0] - D * x[:, 1] + u[:, 0] * p[0], Rfp * x[:, 0] - D * x[:, 2],
                     -D * x[:, 3] + u[:, 1] * p[1]], axis=1)


def hand_rates(W, b, acts, xs, ys):
    """The same network written by hand with the product's expression functions (for the twin model): plain textbook forms."""
    from hilo_mpc_amd import expr as ex

    def act(a, v):
        if a == 'sigmoid':
            return 1.0 / (1.0 + ex.exp(-v))
        if a == 'tanh':
            return ex.tanh(v)
        if a == 'relu':
            return ex.fmax(0.0, v)
        if a == 'softplus':
            return ex.log(1.0 + ex.exp(v))
        return v

    def rates(S, I):
        h = [(S - float(xs[0][0])) / float(xs[1][0]), (I - float(xs[0][1])) / float(xs[1][1])]
        for k, (w, v) in enumerate(zip(W, b)):
            a = acts[k] if k < len(acts) else 'linear'
            nxt = []
            for i in range(w.shape[0]):
                s = float(v[i])
                for j in range(w.shape[1]):
                    s = s + float(w[i, j]) * h[j]
                nxt.append(act(a, s))
            h = nxt
        return [h[i] * float(ys[1][i]) + float(ys[0][i]) for i in range(3)]
    return rates
