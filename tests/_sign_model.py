"""Host NumPy model of the device's generalized matrix-sign-function Lyapunov solver (csrc/dense_sign.hip):
the same scaling, stopping rule, stagnation test and replay refinement, step for step.

Solves F'XE + E'XF = -R (R symmetric) for a c-stable pencil (F, E)  (Benner & Quintana-Orti, Numer. Algorithms 20, 1999):

    Z0 = F, W0 = R
    P_k = Z_k^-1 E,  c_k = (|det Z_k| / |det E|)^(1/n) while ||Z_k + E|| / ||E|| >= 1e-2, else 1
    Z_{k+1} = Z_k / (2 c_k) + (c_k / 2) E P_k
    W_{k+1} = sym(W_k / (2 c_k) + (c_k / 2) P_k' W_k P_k)
    stop when ||Z_{k+1} + E||_F <= tol ||E||_F;   X = E^-T (W_inf / 2) E^-1
"""
import numpy as np

EPS = np.finfo(float).eps
SCALE_OFF = 1e-2          # determinantal scaling is switched off below this relative distance of Z to -E
STAG_STEP = 1e-8          # ||Z_{k+1} - Z_k||_F <= STAG_STEP ||Z_{k+1}||_F ...
STAG_DIST = 1e-4          # ... while ||Z_{k+1} + E||_F > STAG_DIST ||E||_F: a sign of E^-1 F other than -I, the pencil is not c-stable


class NotStable(Exception):
    pass


def default_tol(n):
    return 10.0 * n * EPS


def _sym(M):
    return 0.5 * (M + M.T)


class SignModel:
    """One pencil: the sign iteration and its kept (P_k, c_k) sequence."""

    def __init__(self, F, E, maxiters=50, tol=None):
        F, E = np.asarray(F, dtype=float), np.asarray(E, dtype=float)
        n = F.shape[0]
        self.n, self.F, self.E = n, F, E
        tol = default_tol(n) if tol is None else tol
        self.Einv = np.linalg.inv(E)
        ldE = np.linalg.slogdet(E)[1]
        nE = np.linalg.norm(E)
        Z = F.copy()
        self.seq = []
        self.dist = []
        scale = True
        for _ in range(maxiters):
            ldZ = np.linalg.slogdet(Z)[1]
            P = np.linalg.inv(Z) @ E
            c = float(np.exp((ldZ - ldE) / n)) if scale else 1.0
            Zn = Z / (2.0 * c) + (c / 2.0) * (E @ P)
            self.seq.append((P, c))
            e = np.linalg.norm(Zn + E) / nE
            d = np.linalg.norm(Zn - Z) / np.linalg.norm(Zn)
            self.dist.append(e)
            Z = Zn
            if e <= tol:
                break
            if d <= STAG_STEP and e > STAG_DIST:
                raise NotStable(f"sign iteration stagnated at ||Z + E|| / ||E|| = {e:.3e}")
            if e < SCALE_OFF:
                scale = False
        else:
            raise NotStable(f"no convergence in {maxiters} sign iterations (||Z + E|| / ||E|| = {e:.3e})")
        self.iters = len(self.seq)

    def replay(self, R):
        W = np.asarray(R, dtype=float).copy()
        for P, c in self.seq:
            W = _sym(W / (2.0 * c) + (c / 2.0) * (P.T @ (W @ P)))
        return _sym(self.Einv.T @ (0.5 * W) @ self.Einv)

    def residual(self, X, R):
        T = self.F.T @ (X @ self.E)
        return _sym(R + T + T.T)

    def solve(self, R, max_refine=2):
        """X, refinement steps taken, relative residual before and after refinement."""
        R = np.asarray(R, dtype=float)
        nR = np.linalg.norm(R)
        X = self.replay(R)
        Res = self.residual(X, R)
        r0 = r = np.linalg.norm(Res) / nR
        steps = 0
        while r > 100.0 * self.n * EPS and steps < max_refine:
            X = X + self.replay(Res)
            Res = self.residual(X, R)
            r = np.linalg.norm(Res) / nR
            steps += 1
        return X, steps, r0, r


def sign_lyap(F, E, R, maxiters=50, tol=None, max_refine=2):
    """F'XE + E'XF = -R: (X, info) with info = dict(iters, refinements, res0, res)."""
    m = SignModel(F, E, maxiters, tol)
    X, steps, r0, r = m.solve(R, max_refine)
    return X, dict(iters=m.iters, refinements=steps, res0=r0, res=r)
