"""Plain NumPy model of the dense-inverse ADI chain (csrc/dense.hip: adi_fast_build, adi_fast_iter, adi_group_pack, adi_group_iter) and the
error bounds the device tests hold it to.  Products of at most LD_MAX multiply-adds run in np.longdouble, larger ones in float64 (the caller then
doubles its bound: the reference's own rounding is of the size of the kernel's).  Nothing here is derived from a device result."""
import numpy as np

EPS = float(np.finfo(np.float64).eps)
LD_MAX = 2.0e7
RING = 512


def _mm(A, B):
    """(A B, exact): longdouble product rounded to float64 when it is small enough, else float64; exact tells which"""
    madds = A.shape[0] * A.shape[1] * B.shape[1]
    if madds <= LD_MAX:
        return (A.astype(np.longdouble) @ B.astype(np.longdouble)), True
    return A @ B, False


# ---- the effective stack ---------------------------------------------------------------------------------------------------------------
def seff(stack, wks, n):
    """Seff = [N; E'N] - WKS (U'N) from the (2n + m) x n stack [N; E'N; U'N] and WKS (2n x m, or None).  Returns (Seff float64, |.|-bound operand):
    the second entry is |[N; E'N]| + |WKS| |U'N|, the componentwise size every rounding error of the build is relative to."""
    top = stack[:2 * n]
    if wks is None or stack.shape[0] == 2 * n:
        return top.copy(), np.abs(top)
    corr, _ = _mm(wks, stack[2 * n:])
    S = (top.astype(np.longdouble) - corr).astype(np.float64)
    return S, np.abs(top) + np.abs(wks) @ np.abs(stack[2 * n:])


# ---- the two packed layouts ---------------------------------------------------------------------------------------------------------------
def nstrip(n):
    return (n + 15) // 16


def kst(n):
    return (n + 3) // 4


def pack_a(M, n):
    """A-operand order of nblk = M.shape[0] / n row blocks of n x n (dense.hpp, k_pack_blocks): entry (row 16 s + (lane & 15), column 4 t + (lane >> 4)) of
    block b at ((b nstrip + s) kst + t) 64 + lane, zero padded"""
    nblk = M.shape[0] // n
    assert M.shape == (nblk * n, n)
    ns, ks = nstrip(n), kst(n)
    P = np.zeros((nblk, ns * 16, ks * 4))
    P[:, :n, :n] = M.reshape(nblk, n, n)
    # [b, s, r16, t, c4] -> [b, s, t, c4, r16]  (lane = 16 c4 + r16)
    return np.ascontiguousarray(P.reshape(nblk, ns, 16, ks, 4).transpose(0, 1, 3, 4, 2)).ravel()


def unpack_a(flat, n, nblk):
    """(M, padding): the nblk n x n blocks stacked, and every entry of the packed array that lies in the padding"""
    ns, ks = nstrip(n), kst(n)
    P = flat.reshape(nblk, ns, ks, 4, 16).transpose(0, 1, 4, 2, 3).reshape(nblk, ns * 16, ks * 4)
    mask = np.ones_like(P, dtype=bool)
    mask[:, :n, :n] = False
    return P[:, :n, :n].reshape(nblk * n, n).copy(), P[mask]


def rpack_doubles(n, k):
    return 4 * nstrip(n) * ((k + 15) // 16) * 64


def pack_r(R):
    """B-operand order of the n x k residual (dense.hpp, AdiFastArgs::Rpc; k_adi_pack_r): element (row 4 t + (lane >> 4), column 16 c + (lane & 15)) at
    (t ct + c) 64 + lane, zero padded to 4 nstrip K-steps and ct = ceil(k / 16) column tiles"""
    n, k = R.shape
    nt_, ct = 4 * nstrip(n), (k + 15) // 16
    P = np.zeros((nt_ * 4, ct * 16))
    P[:n, :k] = R
    # [t, r4, c, c16] -> [t, c, r4, c16]   (lane = 16 r4 + c16)
    return np.ascontiguousarray(P.reshape(nt_, 4, ct, 16).transpose(0, 2, 1, 3)).ravel()


def unpack_r(flat, n, k):
    nt_, ct = 4 * nstrip(n), (k + 15) // 16
    P = flat.reshape(nt_, ct, 4, 16).transpose(0, 2, 1, 3).reshape(nt_ * 4, ct * 16)
    mask = np.ones_like(P, dtype=bool)
    mask[:n, :k] = False
    return P[:n, :k].copy(), P[mask]


# ---- one iteration, its norm, the decision ---------------------------------------------------------------------------------------------
def step(S, R, mu):
    """V = Seff_top R,  R+ = R - 2 mu Seff_bot R  (adi.jl:149-179 with the solve written as a product).  Returns a dict with V, Rn (float64), the
    componentwise bound operands aV = |Seff_top| |R|, aR = |R| + 2 |mu| |Seff_bot| |R|, and f = 1 (longdouble reference) or 2 (float64 reference)."""
    n = R.shape[0]
    W, exact = _mm(S, R)
    V = W[:n]
    Rn = R.astype(W.dtype) - (2.0 * mu) * W[n:]
    aW = np.abs(S) @ np.abs(R)
    return dict(V=np.asarray(V, dtype=np.float64), Rn=np.asarray(Rn, dtype=np.float64), aV=aW[:n], aR=np.abs(R) + 2.0 * abs(mu) * aW[n:], f=1.0 if exact else 2.0)


def gram(R):
    G, exact = _mm(np.ascontiguousarray(R.T), R)
    return np.asarray(G, dtype=np.float64), np.abs(R).T @ np.abs(R), 1.0 if exact else 2.0


def norm2(R, T, alpha):
    """(nrm^2, bound operand, f):  nrm = |alpha| sqrt(tr((T R'R)^2))  (LDLt.jl:77-89 in Gram form);  the operand is
    alpha^2 sum_ij (|T| |R|'|R|)_ij (|R|'|R| |T|)_ij"""
    Rl, Tl = R.astype(np.longdouble), T.astype(np.longdouble)
    n, k = R.shape
    exact = n * k * k <= LD_MAX and 2 * k ** 3 <= LD_MAX
    if exact:
        G = Rl.T @ Rl
        M = Tl @ G
        s = float(np.sum(M * (G @ Tl.T)))           # tr(M M) = sum_ij M_ij M_ji, and (G T')_ij = M_ji for symmetric G
    else:
        G = R.T @ R
        M = T @ G
        s = float(np.sum(M * (G @ T.T)))
    aG = np.abs(R).T @ np.abs(R)
    aT = np.abs(T)
    op = float(np.sum((aT @ aG) * (aG @ aT.T))) * alpha * alpha
    return alpha * alpha * s, op, 1.0 if exact else 2.0


def norm(R, T, alpha):
    return float(np.sqrt(max(norm2(R, T, alpha)[0], 0.0)))


def decide(norms, base_it, abstol, maxiters):
    """adi.jl:115-123 applied in iteration order to norms[j - 1] = norm after iteration base_it + j: (iters, done, accepted) — the first iteration
    at or below abstol or at maxiters ends the solve; without one every iteration counts and done stays 0"""
    for j, v in enumerate(norms, start=1):
        if v <= abstol or base_it + j >= maxiters:
            return base_it + j, 1, j
    return base_it + len(norms), 0, len(norms)


# ---- the group operators ---------------------------------------------------------------------------------------------------------------
def group_ops(Ss, mus):
    """[Om_0 .. Om_(g-1); Pi_1 .. Pi_g] for the g effective stacks Ss (2n x n each) and shifts mus:  P_s = I - 2 mu_s Seff_bot_s,  Pi_i = P_(i-1) ... P_0,
    Om_i = Seff_top_i Pi_i, so that V_i = Om_i R_0 and R_i = Pi_i R_0 (longdouble products, rounded once)"""
    g, n = len(Ss), Ss[0].shape[1]
    Pi = [np.eye(n, dtype=np.longdouble)]
    Om = []
    for S, mu in zip(Ss, mus):
        Sl = S.astype(np.longdouble)
        Om.append(Sl[:n] @ Pi[-1])
        Pi.append(Pi[-1] - (2.0 * mu) * (Sl[n:] @ Pi[-1]))
    return np.vstack(Om + Pi[1:]).astype(np.float64)


# ---- bounds (componentwise, from the issue's derivation: K sequential fused multiply-adds, K = n, plus the fixed-order sums) -------------------
def bound_step(n, operand, f=1.0):
    return f * 2.0 * (n + 8) * EPS * operand


def bound_norm2(n, k, operand, f=1.0):
    return f * 2.0 * (n + 2 * k + 8) * EPS * operand
