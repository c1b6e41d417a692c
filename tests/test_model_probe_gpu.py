"""GPU: run-time compiled models evaluated on their own (hilo_jit_probe) in every scalar type and through their generated derivative
code, against sympy -> mpmath at 50 digits (tests/model_probe_reference.py: models, points, tolerance - the host test's bounds
times the measured device-over-host factor 2.4).

Per model and per way of compiling sine / cosine (HILO_TRIG_CALLS off and on): one launch at 64 points x (1 + n_z (n_z + 1) / 2)
directions - a random one, then e_i, and e_i + e_j for the polarisation."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import model_probe_reference as mr

pytestmark = pytest.mark.gpu


def _close(got, ref, bound, what):
    err = np.abs(got - ref)
    assert np.all(err <= bound), f"{what}: error {err.max():.3e} at {np.unravel_index(np.argmax(err - bound), err.shape)}, allowed " \
                                 f"{bound.ravel()[np.argmax(err - bound)]:.3e}"


@pytest.mark.parametrize('trig_calls', [0, 1])
@pytest.mark.parametrize('name', sorted(mr.MODELS))
def test_model_in_every_scalar_type_against_sympy(name, trig_calls):
    from hilo_mpc_amd import _lib
    m = mr.MODELS[name][0]()
    nx, nu, npar, ny = m.n_x, m.n_u, m.n_p, m.n_y
    nz, nh, nhx = nx + nu, (nx + nu) * (nx + nu + 1) // 2, nx * (nx + 1) // 2
    X, U, p = mr.points(name)
    R = mr.reference(name, X, U, p)
    n0 = len(X)
    rng = np.random.default_rng(11)
    dirs = [None]                                            # a random direction per point, then the polarisation set
    pairs = []
    for i in range(nz):
        dirs.append(np.eye(nz)[i])
    for i in range(nz):
        for j in range(i):
            pairs.append((i, j, len(dirs)))
            dirs.append(np.eye(nz)[i] + np.eye(nz)[j])
    D0 = rng.normal(size=(n0, nz))
    kb, kby = rng.normal(size=(n0, nx)), rng.normal(size=(n0, ny))
    rows = []
    for d in dirs:
        D = D0 if d is None else np.tile(d, (n0, 1))
        rows.append(np.concatenate([X, U, np.tile(p, (n0, 1)), D, kb, kby], axis=1))
    IN = np.ascontiguousarray(np.concatenate(rows))
    width = 5 * (nx + ny) + (nx + ny) * nz + nx * nx + nx * nz + nh + ny + ny * nx + nhx
    assert IN.shape[1] == 3 * nx + 2 * nu + npar + ny
    dev = torch.as_tensor(IN, device='cuda')
    out = torch.full((len(IN), width), np.nan, dtype=torch.float64, device='cuda')
    flags = torch.zeros(2, dtype=torch.int32, device='cuda')
    _lib.check(_lib.lib().hilo_jit_probe(m.user_source().encode(), trig_calls, nx, nu, npar, ny, len(IN), dev.data_ptr(), out.data_ptr(),
                                         flags.data_ptr(), None))
    O = out.cpu().numpy().reshape(len(dirs), n0, width)
    assert flags.cpu().tolist() == [1, 1 if ny else 0]
    o = np.cumsum([0, nx, ny, nx, ny, nx * nz, ny * nz, 3 * nx, 3 * ny, nx * nx, nx * nz, nh, ny, ny * nx, nhx])
    part = lambda k, q=0: O[q][:, o[k]:o[k + 1]]
    ref_v = np.concatenate([R['f'], R['y']], axis=1)
    ref_J = np.concatenate([R['Jf'], R['Jy']], axis=1)                      # [n][nx + ny][nz]
    ref_H = np.concatenate([R['Hf'], R['Hy']], axis=1)                      # [n][nx + ny][nz][nz]
    EJ = mr.J_RTOL * np.abs(ref_J) + mr.J_ATOL                              # per-entry bounds
    EH = mr.H_RTOL * np.abs(ref_H) + mr.H_ATOL
    # values: double, FastD (its quotients go through rcp_fast: 2 ulp instead of 0.5, far inside the bound), Jet2's and mjh's
    for what, got in (('double', np.concatenate([part(0), part(1)], axis=1)), ('FastD', np.concatenate([part(2), part(3)], axis=1)),
                      ('Jet2.v', np.concatenate([part(6)[:, :nx], part(7)[:, :ny]], axis=1))):
        assert np.isfinite(got).all(), what
        _close(got, ref_v, mr.V_RTOL * np.abs(ref_v), f"{name} {what} values")
    # Jacobians: Dual seeded with the identity, jx, jh's J, mjh's Jy - against the reference and (same bound) each other
    Jd = np.concatenate([part(4).reshape(n0, nx, nz), part(5).reshape(n0, ny, nz)], axis=1)
    _close(Jd, ref_J, EJ, f"{name} Dual Jacobian")
    _close(part(8).reshape(n0, nx, nx), ref_J[:, :nx, :nx], EJ[:, :nx, :nx], f"{name} jx")
    _close(part(9).reshape(n0, nx, nz), ref_J[:, :nx], EJ[:, :nx], f"{name} jh J")
    _close(part(9).reshape(n0, nx, nz), Jd[:, :nx], 2 * EJ[:, :nx], f"{name} jh J against Dual")
    if ny:
        _close(part(11), R['y'], mr.V_RTOL * np.abs(R['y']), f"{name} mjh y")
        _close(part(12).reshape(n0, ny, nx), R['Jy'][:, :, :nx], EJ[:, nx:, :nx], f"{name} mjh Jy")
    # Jet2 along the random direction: .a = J d, .b = d'H d
    ja = np.concatenate([part(6)[:, nx:2 * nx], part(7)[:, ny:2 * ny]], axis=1)
    jb = np.concatenate([part(6)[:, 2 * nx:], part(7)[:, 2 * ny:]], axis=1)
    _close(ja, np.einsum('nmj,nj->nm', ref_J, D0), np.einsum('nmj,nj->nm', EJ, np.abs(D0)), f"{name} Jet2.a = J d")
    _close(jb, np.einsum('nmij,ni,nj->nm', ref_H, D0, D0), np.einsum('nmij,ni,nj->nm', EH, np.abs(D0), np.abs(D0)), f"{name} Jet2.b = d'H d")
    # jh's packed H = sum_m kb_m Hess f_m, and the same from polarising Jet2 over e_i, e_j, e_i + e_j
    Hc = np.einsum('nm,nmij->nij', kb, R['Hf'])
    Ec = np.einsum('nm,nmij->nij', np.abs(kb), EH[:, :nx])
    tri = [(i, j) for i in range(nz) for j in range(i + 1)]
    Hp = part(10)
    _close(Hp, np.stack([Hc[:, i, j] for i, j in tri], axis=1), np.stack([Ec[:, i, j] for i, j in tri], axis=1), f"{name} jh H")
    qb = lambda q: O[q][:, o[6] + 2 * nx:o[6] + 3 * nx]                    # Jet2.b of ode along direction q: d'H_m d per row m
    pol = np.zeros((n0, nz, nz))
    for i in range(nz):
        pol[:, i, i] = np.einsum('nm,nm->n', kb, qb(1 + i))
    for i, j, q in pairs:
        pol[:, i, j] = pol[:, j, i] = np.einsum('nm,nm->n', kb, (qb(q) - qb(1 + i) - qb(1 + j)) / 2)
    bound = Ec.copy()
    for i, j, q in pairs:                                    # (q(e_i + e_j) - q(e_i) - q(e_j)) / 2: the entries each direction sees
        bound[:, i, j] = bound[:, j, i] = (Ec[:, i, i] + Ec[:, j, j] + 2 * Ec[:, i, j] + Ec[:, i, i] + Ec[:, j, j]) / 2
    _close(pol, Hc, bound, f"{name} polarised Jet2 against the exact Hessian")
    _close(np.stack([pol[:, i, j] for i, j in tri], axis=1), Hp, np.stack([bound[:, i, j] + Ec[:, i, j] for i, j in tri], axis=1),
           f"{name} polarised Jet2 against jh's packed H")
    if ny:
        Hyc = np.einsum('nm,nmij->nij', kby, R['Hy'])[:, :nx, :nx]
        Eyc = np.einsum('nm,nmij->nij', np.abs(kby), EH[:, nx:])[:, :nx, :nx]
        trx = [(i, j) for i in range(nx) for j in range(i + 1)]
        _close(part(13), np.stack([Hyc[:, i, j] for i, j in trx], axis=1), np.stack([Eyc[:, i, j] for i, j in trx], axis=1), f"{name} mjh Hy")
    if name == 'edges':
        far = np.abs(1000. * X[:, 0]) > 354.9                # beyond the overflow of exp(2 k a): the composed tanh was NaN here
        assert far.sum() > 20 and np.isfinite(O[0][far]).all()
        ka, kbc = np.abs(1000. * X[:, 0]), np.abs(1000. * X[:, 1] * U[:, 0])
        assert ((ka > .05) & (ka < 25.)).sum() >= 3 and ((kbc > .05) & (kbc < 25.)).sum() >= 2       # and tanh's transition region
