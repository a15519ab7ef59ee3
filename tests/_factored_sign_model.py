"""Host NumPy model of the device's factored sign-function Lyapunov solver (csrc/dense_sign_lr.hip, SignLyap::solve_lr) on top of
`_sign_model.SignModel`: the same width cap, truncation rule and refinement rule, step for step.

Solves F'XE + E'XF = -G S G' (S symmetric, indefinite allowed) with the kept (P_k, c_k) applied to the factor
(Benner & Quintana-Orti 1999, section 4):

    L_{k+1} = [L_k, P_k' L_k],   D_{k+1} = blkdiag(D_k / (2 c_k), (c_k / 2) D_k),   X = (E^-T L) (D / 2) (E^-T L)'

compressed (QR, eigenvalues of R D R', |lambda| > rtol max|lambda| kept) whenever the width exceeds max_width and once at the end.
"""
import numpy as np

from _sign_model import EPS


def default_rtol(n):
    return n * EPS


def small_form(L, Dm):
    """(Q, S) with L D L' = Q S Q': the QR's basis, or the identity when L has at least as many columns as rows"""
    n, w = L.shape
    if w >= n:
        S = (L @ Dm) @ L.T
        Q = None
    else:
        Q, R = np.linalg.qr(L)
        S = (R @ Dm) @ R.T
    return Q, 0.5 * (S + S.T)


def truncate(Q, S, rtol):
    lam, V = np.linalg.eigh(S)
    wmax = np.abs(lam).max() if lam.size else 0.0
    keep = np.abs(lam) > rtol * wmax
    B = V[:, keep]
    return (B if Q is None else Q @ B), lam[keep]


def compress(L, Dm, rtol):
    """L D L' -> (L_new with orthonormal columns, kept eigenvalues ascending)"""
    Q, S = small_form(L, Dm)
    return truncate(Q, S, rtol)


class FactoredReplay:
    def __init__(self, model, rtol=None, max_width=256, max_refine=1):
        self.m = model
        self.n = model.n
        self.rtol = default_rtol(self.n) if rtol is None else rtol
        self.max_width, self.max_refine = max_width, max_refine
        if not 0.0 < self.rtol < 1.0:
            raise ValueError("rtol must lie in (0, 1)")

    def _replay(self, L, Dm, st):
        lam = None
        for P, c in self.m.seq:
            if L.shape[1] == 0:
                break
            L = np.hstack([L, P.T @ L])
            r = Dm.shape[0]
            Dn = np.zeros((2 * r, 2 * r))
            Dn[:r, :r] = Dm / (2.0 * c)
            Dn[r:, r:] = (0.5 * c) * Dm
            Dm, lam = Dn, None
            st["peak_width"] = max(st["peak_width"], L.shape[1])
            if L.shape[1] > self.max_width:
                L, lam = compress(L, Dm, self.rtol)
                Dm = np.diag(lam)
                st["compressions"] += 1
        if lam is None and L.shape[1] > 0:
            L, lam = compress(L, Dm, self.rtol)
            st["compressions"] += 1
        if lam is None:
            lam = np.zeros(0)
        return self.m.Einv.T @ L, np.diag(0.5 * lam)

    def _residual_factor(self, G, S, LX, DX):
        r, p = G.shape[1], LX.shape[1]
        Rf = np.hstack([G, self.m.F.T @ LX, self.m.E.T @ LX])
        T = np.zeros((r + 2 * p,) * 2)
        T[:r, :r] = S
        T[r:r + p, r + p:] = DX
        T[r + p:, r:r + p] = DX
        return Rf, T

    def solve(self, G, S):
        """(L, D, info): X = L D L' with D diagonal; info as the device reports it"""
        G, S = np.asarray(G, float).reshape(self.n, -1), np.asarray(S, float)
        r = G.shape[1]
        if self.max_width < max(r, 1):
            raise ValueError("max_width must be at least the width of G (and 1)")
        st = dict(iters=self.m.iters, rank=0, peak_width=r, compressions=0, refinements=0, res0=0.0, res=0.0)
        if r == 0:
            st["peak_width"] = 0
            return np.zeros((self.n, 0)), np.zeros((0, 0)), st
        normR = np.linalg.norm(small_form(G, S)[1])
        LX, DX = self._replay(G, S, st)

        def residual():
            Rf, T = self._residual_factor(G, S, LX, DX)
            Q, Sm = small_form(Rf, T)
            nr = np.linalg.norm(Sm)
            return Q, Sm, (nr / normR if normR > 0 else nr)

        Q, Sm, res = residual()
        st["res0"] = st["res"] = res
        target = 100.0 * self.n * EPS + 10.0 * self.rtol
        while st["res"] > target and st["refinements"] < self.max_refine:
            Lr, lam = truncate(Q, Sm, self.rtol)
            st["compressions"] += 1
            if lam.size == 0:
                break
            LdX, DdX = self._replay(Lr, np.diag(lam), st)
            if LdX.shape[1] == 0:
                break
            cat = np.hstack([LX, LdX])
            p, pd = LX.shape[1], LdX.shape[1]
            Dc = np.zeros((p + pd,) * 2)
            Dc[:p, :p] = DX
            Dc[p:, p:] = DdX
            st["peak_width"] = max(st["peak_width"], p + pd)
            LX, lam = compress(cat, Dc, self.rtol)
            DX = np.diag(lam)
            st["compressions"] += 1
            st["refinements"] += 1
            Q, Sm, st["res"] = residual()
        st["rank"] = LX.shape[1]
        return LX, DX, st


def factored_sign_lyap(model, G, S, rtol=None, max_width=256, max_refine=1):
    return FactoredReplay(model, rtol, max_width, max_refine).solve(G, S)
