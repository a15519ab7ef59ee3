"""Host NumPy model of the dual replays on a kept sign factorisation (csrc/dense_sign.hip: SignLyap::solve_t; csrc/dense_sign_lr.hip:
SignLyap::solve_lr_t), on top of `_sign_model.SignModel` and `_factored_sign_model`: the same order of operations as the device, step for step.

The kept sequence (P_k, c_k) of the pencil (F, E) belongs to  F'XE + E'XF = -R.  The sign iteration of (F', E') has the iterates Z_k' and the
same c_k, and with V = E^-1 W E^-T its W recursion needs only what is kept.  For  F Y E' + E Y F' = -R :

    V_0 = sym(E^-1 R E^-T),   V_{k+1} = sym(V_k / (2 c_k) + (c_k / 2) P_k V_k P_k'),   Y = V_inf / 2

and in factored form, R = G S G':

    L_0 = E^-1 G,   L_{k+1} = [L_k, P_k L_k],   D_{k+1} = blkdiag(D_k / (2 c_k), (c_k / 2) D_k),   Y = L_inf (D_inf / 2) L_inf'
"""
import numpy as np

from _sign_model import EPS, _sym
from _factored_sign_model import FactoredReplay, compress


def replay_t(m, R):
    V = _sym((m.Einv @ np.asarray(R, dtype=float)) @ m.Einv.T)
    for P, c in m.seq:
        V = _sym(V / (2.0 * c) + (c / 2.0) * ((P @ V) @ P.T))
    return 0.5 * V


def residual_t(m, Y, R):
    T = m.F @ (Y @ m.E.T)
    return _sym(R + T + T.T)


def solve_t(m, R, max_refine=2):
    """Y, refinement steps taken, relative residual before and after refinement (the rule of SignModel.solve)"""
    R = np.asarray(R, dtype=float)
    nR = np.linalg.norm(R)
    Y = replay_t(m, R)
    Res = residual_t(m, Y, R)
    r0 = r = np.linalg.norm(Res) / nR
    steps = 0
    while r > 100.0 * m.n * EPS and steps < max_refine:
        Y = Y + replay_t(m, Res)
        Res = residual_t(m, Y, R)
        r = np.linalg.norm(Res) / nR
        steps += 1
    return Y, steps, r0, r


class FactoredReplayT(FactoredReplay):
    """FactoredReplay with the two places where the dual differs: the recursion (entry transform, no transposition, no exit transform) and the
    residual factor [G, F L, E L]; cap, truncation, refinement and statistics are inherited"""

    def _replay(self, L, Dm, st):
        lam = None
        L = self.m.Einv @ L
        for P, c in self.m.seq:
            if L.shape[1] == 0:
                break
            L = np.hstack([L, P @ L])
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
        return L, np.diag(0.5 * lam)

    def _residual_factor(self, G, S, LY, DY):
        r, p = G.shape[1], LY.shape[1]
        Rf = np.hstack([G, self.m.F @ LY, self.m.E @ LY])
        T = np.zeros((r + 2 * p,) * 2)
        T[:r, :r] = S
        T[r:r + p, r + p:] = DY
        T[r + p:, r:r + p] = DY
        return Rf, T


def factored_sign_lyap_t(model, G, S, rtol=None, max_width=256, max_refine=1):
    """(L, D, info) with Y = L D L' for F Y E' + E Y F' = -G S G'"""
    return FactoredReplayT(model, rtol, max_width, max_refine).solve(G, S)
