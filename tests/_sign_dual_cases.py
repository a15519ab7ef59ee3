"""The non-symmetric pencils of the dual-solve tests (tests/test_sign_dual_host.py, tests/test_gpu_sign_dual.py) with their CPU references,
computed once per process.

On SteelProfile without convection E and A are symmetric, the dual equation equals the primal one and a wrong transposition passes.  Here E is
non-symmetric as well as F:
  steel(n)   steel_profile(n, convection=3e-3) with E <- E (I + 0.1 N), N strictly upper triangular (fixed seed) of spectral norm 1, and
             F = A - E / (2 tau), tau = 20 (the operator of a Ros1 step);
  small(n)   a fixed-seed random pencil: E = U diag(s) V' with cond(E) = 10^2.5 <= 1e3, F = E M with the spectrum of M around -1.
`stable()` checks c-stability on the CPU (generalized eigenvalues).  The right-hand side is G S G' with an indefinite S of width 11.
"""
import functools

import numpy as np
import scipy.linalg as sla

import dre_amd as D
import dre_oracle as o
import _sign_model as sm
import _sign_dual_model as dm

TAU = 20.0


def stable(F, E):
    """largest real part of the generalized eigenvalues of (F, E): negative for a c-stable pencil"""
    return float(sla.eigvals(F, E).real.max())


def _rhs(n, B, rng):
    m = B.shape[1]
    G = np.hstack([B, rng.standard_normal((n, 11 - m)) * (np.linalg.norm(B) / np.sqrt(n * m))])
    S = np.diag([1.0] * m + [-0.3] * (11 - m))
    return G, S


@functools.lru_cache(maxsize=None)
def pencil(n):
    """(E, F, G, S): steel(n) for n >= 371, small(n) below"""
    if n >= 371:
        d = D.steel_profile(n, convection=3e-3)
        rng = np.random.default_rng(109)
        N = np.triu(rng.standard_normal((n, n)), 1)
        N /= np.linalg.norm(N, 2)
        E = d.E.toarray() @ (np.eye(n) + 0.1 * N)
        F = d.A.toarray() - E / (2.0 * TAU)
        G, S = _rhs(n, np.asarray(d.B, float), rng)
    else:
        rng = np.random.default_rng(1000 + n)
        U, V = np.linalg.qr(rng.standard_normal((n, n)))[0], np.linalg.qr(rng.standard_normal((n, n)))[0]
        E = (U * np.logspace(0.0, -2.5, n)) @ V.T
        F = E @ (-np.eye(n) + 0.4 * rng.standard_normal((n, n)) / np.sqrt(n))
        G, S = _rhs(n, rng.standard_normal((n, 7)), rng)
    for M in (E, F, G, S):
        M.setflags(write=False)
    return E, F, G, S


@functools.lru_cache(maxsize=None)
def model(n, tol=None):
    E, F, _, _ = pencil(n)
    return sm.SignModel(F, E, tol=tol)


@functools.lru_cache(maxsize=None)
def model_of_transposed_pencil(n):
    E, F, _, _ = pencil(n)
    return sm.SignModel(F.T, E.T)


def rhs(n, cols=None):
    """(G, S, R = G S G') of the full right-hand side, or of the columns `cols` of G"""
    _, _, G, S = pencil(n)
    if cols is not None:
        G, S = G[:, cols], S[np.ix_(cols, cols)]
    return G, S, G @ S @ G.T


@functools.lru_cache(maxsize=None)
def oracle(n, cols=None, dual=True):
    """lyap_dense on (F', E') for the dual equation, on (F, E) for the primal one"""
    E, F, _, _ = pencil(n)
    R = rhs(n, None if cols is None else list(cols))[2]
    Y = o.lyap_dense(F.T, E.T, R) if dual else o.lyap_dense(F, E, R)
    Y.setflags(write=False)
    return Y


@functools.lru_cache(maxsize=None)
def model_dual(n, tol=None, max_refine=2):
    """(Y, steps, res0, res) of the dense dual model for the full right-hand side"""
    return dm.solve_t(model(n, tol), rhs(n)[2], max_refine)
