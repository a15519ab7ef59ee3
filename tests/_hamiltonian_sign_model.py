"""Host NumPy model of the device's dense GARE solver (csrc/dense_are.hip): the Hamiltonian sign iteration with the same scaling, structure
averaging, stopping rule and stagnation test, the Householder QR extraction and the Newton-Kleinman refinement, step for step.

Solves Q + A'XE + E'XA - E'XGXE = 0 for the stabilizing X (G = G' >= 0, Q = Q'):

    H = [[A, -G], [-Q, -A']],  K = diag(E, E')                     (2n x 2n; the stable deflating subspace is range [I; XE])
    Z0 = H,  Z_{k+1} = struct((Z_k / c_k + c_k K Z_k^-1 K) / 2)
    c_k = (|det Z_k| / |det K|)^(1/2n) while ||Z_{k+1} - Z_k||_F >= SCALE_OFF ||Z_{k+1}||_F, else 1
    struct: Z12, Z21 symmetrised, Z11 := (Z11 - Z22')/2, Z22 := -Z11'     (JZ symmetric, Byers 1987)
    stop when ||Z_{k+1} - Z_k||_F <= tol ||Z_{k+1}||_F
    (Z_inf + K)[I; Y] = 0:  M = [Z12; Z22 + E'] = QR (Householder),  Y = R^-1 (Q' (-[Z11 + E; Z21]))[0:n],  X = sym(Y E^-1)
    Newton-Kleinman: (A - GXE)' D E + E' D (A - GXE) = -R(X),  X <- X + D   while the scaled residual decreases and exceeds REFINE_TARGET
"""
import numpy as np

import _sign_model as sm

EPS = np.finfo(float).eps
SCALE_OFF = 1e-2          # determinantal scaling is switched off once the relative step is below this
STAG_WINDOW = 3           # unscaled phase: NOT_STABLE when the relative step has not reached a new minimum for this many iterations


class NotStable(Exception):
    pass


class Singular(Exception):
    pass


def default_tol(n):
    """Stopping tolerance on the relative step of the 2n x 2n iteration: 10 (2n) eps, as the issue proposes; the model's figures (tests/
    test_dense_gare_host.py) reach it on every stabilizable and detectable problem tried."""
    return 10.0 * (2 * n) * EPS


def refine_target(n):
    return 100.0 * n * EPS


def _sym(M):
    return 0.5 * (M + M.T)


def hamiltonian(E, A, G, Q):
    return np.block([[A, -G], [-Q, -A.T]]), np.block([[E, np.zeros_like(E)], [np.zeros_like(E), E.T]])


def structure(Z, n):
    """The structured average of the update kernel: JZ symmetric."""
    Z11, Z12, Z21, Z22 = Z[:n, :n], Z[:n, n:], Z[n:, :n], Z[n:, n:]
    S11 = 0.5 * (Z11 - Z22.T)
    return np.block([[S11, _sym(Z12)], [_sym(Z21), -S11.T]])


def residual(E, A, G, Q, X):
    """R(X) and the scaled residual ||R||_F / (||Q||_F + 2 ||A'XE||_F + ||E'XGXE||_F)."""
    XE = X @ E
    AXE = A.T @ XE
    XGX = XE.T @ (G @ XE)
    R = _sym(Q + AXE + AXE.T - XGX)
    den = np.linalg.norm(Q) + 2.0 * np.linalg.norm(AXE) + np.linalg.norm(XGX)
    return R, np.linalg.norm(R) / den if den > 0 else np.linalg.norm(R)


def sign_iteration(E, A, G, Q, maxiters=50, tol=None):
    """Z_inf and the number of iterations; NotStable / Singular as the device."""
    n = E.shape[0]
    tol = default_tol(n) if tol is None else tol
    H, K = hamiltonian(E, A, G, Q)
    ldK = 2.0 * np.linalg.slogdet(E)[1]
    Z = structure(H, n)
    scale, best, since = True, np.inf, 0
    steps = []
    for k in range(maxiters):
        sgn, ldZ = np.linalg.slogdet(Z)
        if sgn == 0 or not np.isfinite(ldZ):
            raise Singular(f"singular Z_{k}")
        c = float(np.exp((ldZ - ldK) / (2 * n))) if scale else 1.0
        W = np.linalg.inv(Z)
        Zn = structure((Z / c + c * (K @ W @ K)) / 2.0, n)
        d = np.linalg.norm(Zn - Z) / np.linalg.norm(Zn)
        steps.append(d)
        Z = Zn
        if not np.isfinite(d):
            raise NotStable("non-finite values in the sign iteration")
        if d <= tol:
            return Z, k + 1, steps
        if d < best:
            best, since = d, 0
        elif not scale:           # (the scaled phase is not monotone: its first steps often grow)
            since += 1
            if since >= STAG_WINDOW:
                raise NotStable(f"sign iteration stagnated at a relative step {d:.3e} (Hamiltonian eigenvalues on or near the imaginary axis)")
        if d < SCALE_OFF:
            scale = False
    raise NotStable(f"no convergence in {maxiters} sign iterations (relative step {d:.3e})")


def extract(Z, E):
    n = E.shape[0]
    Z11, Z12, Z21, Z22 = Z[:n, :n], Z[:n, n:], Z[n:, :n], Z[n:, n:]
    M = np.vstack([Z12, Z22 + E.T])
    rhs = -np.vstack([Z11 + E, Z21])
    Qf, R = np.linalg.qr(M)                                   # the device's blocked Householder QR of the 2n x n operand
    Y = np.linalg.inv(R) @ (Qf.T @ rhs)                       # R^-1 by the same Gauss-Jordan inversion as every other inverse
    return _sym(Y @ np.linalg.inv(E))


def gare_sign(E, A, G, Q, maxiters=50, tol=None, max_refine=2):
    """(X, info) with info = dict(iters, refinements, res0, res)."""
    E, A, G, Q = (np.asarray(M, dtype=float) for M in (E, A, G, Q))
    n = E.shape[0]
    Z, iters, steps = sign_iteration(E, A, G, Q, maxiters, tol)
    X = extract(Z, E)
    R, r = residual(E, A, G, Q, X)
    r0, refinements = r, 0
    while r > refine_target(n) and refinements < max_refine:
        F = A - G @ X @ E
        try:
            D, _ = sm.sign_lyap(F, E, R, maxiters=maxiters)
        except sm.NotStable as e:
            raise NotStable(f"refinement: the closed loop is not c-stable ({e})")
        Xn = X + D
        Rn, rn = residual(E, A, G, Q, Xn)
        refinements += 1
        if not rn < r:            # stopped decreasing: keep the better iterate
            break
        X, R, r = Xn, Rn, rn
    return X, dict(iters=iters, refinements=refinements, res0=r0, res=r, steps=steps)
