"""Plain NumPy model of the stages of the warm-started compression (csrc/warm.hip), stage by stage as dre_warm_probe exposes them.  float64
throughout, np.longdouble where a bound is held against the result (products, sums of squares).  The model is pinned to independent facts by
tests/test_warm_host.py; the GPU tests hold each kernel against the model applied to the device's own inputs of that stage."""
import numpy as np

EPS = 2.0 ** -52
PIVOT_FLOOR = 1e-10          # k_warm_project: a pivot at or below this times the largest diagonal entry of Z_1'Z_1 is dead
LD = np.longdouble


def mm(A, B):
    """A B accumulated in long double, rounded once"""
    return np.asarray(np.asarray(A, dtype=LD) @ np.asarray(B, dtype=LD), dtype=np.float64)


def amm(A, B):
    """|A| |B|: what the componentwise bounds of the products are multiples of"""
    return np.abs(A) @ np.abs(B)


def project_rows(n):
    strips = (n + 15) // 16
    return 16 if strips <= 256 else 16 * ((strips + 255) // 256)


def project_slabs(n):
    r = project_rows(n)
    return (n + r - 1) // r


# ---- PROJECT ------------------------------------------------------------------------------------------------------------------------------
def slab_shares(Z1):
    """(shares (nslab, 16, 16), bounds): workgroup b's share of Z_1'Z_1 and (rows + 2) eps |Z_1b|'|Z_1b|"""
    n = Z1.shape[0]
    rows = project_rows(n)
    sh, bd = [], []
    for r0 in range(0, n, rows):
        Zb = Z1[r0:r0 + rows]
        sh.append(mm(Zb.T, Zb))
        bd.append((rows + 2) * EPS * amm(Zb.T, Zb))
    return np.array(sh), np.array(bd)


def sum_slabs(slab):
    """the last workgroup's sum: sequential, in slab order (float64 additions in exactly the device's order)"""
    G = np.zeros((16, 16))
    for b in range(slab.shape[0]):
        G = G + slab[b]
    return G


def chol_c(G):
    """thresholded right-looking Cholesky of the 16 x 16 Gram matrix; (C = L^-T with zero rows and columns at dead pivots, live flags, L)"""
    k = G.shape[0]
    A = np.array(G, dtype=np.float64)
    floor = PIVOT_FLOOR * max(float(np.max(np.diag(A))), 0.0)
    L = np.zeros((k, k))
    live = np.zeros(k, dtype=bool)
    for j in range(k):
        piv = A[j, j]
        live[j] = bool(piv > floor and piv > 0.0)
        if not live[j]:
            continue
        col = A[:, j] / np.sqrt(piv)
        L[j:, j] = col[j:]
        A[j + 1:, j + 1:] -= np.outer(col[j + 1:], col[j + 1:])
    C = np.zeros((k, k))
    idx = np.flatnonzero(live)
    if idx.size:
        C[np.ix_(idx, idx)] = np.linalg.inv(L[np.ix_(idx, idx)]).T
    return C, live, L


def project(Q, Yf, Pf, slab=None):
    """Z_1 = Y_f - Q P_f, its bound (q + 2) eps (|Y_f| + |Q| |P_f|), G (from the device's shares when given), C, live"""
    Z1 = np.asarray(np.asarray(Yf, dtype=LD) - np.asarray(Q, dtype=LD) @ np.asarray(Pf, dtype=LD), dtype=np.float64)
    bound = (Q.shape[1] + 2) * EPS * (np.abs(Yf) + amm(Q, Pf))
    G = sum_slabs(slab) if slab is not None else sum_slabs(slab_shares(Z1)[0])
    C, live, _ = chol_c(G)
    return Z1, bound, G, C, live


def zapply(Z1, Cw):
    """Z = Z_1 C and (16 + 2) eps |Z_1| |C|"""
    return mm(Z1, Cw), 18 * EPS * amm(Z1, Cw)


def mfma_bound(A, B):
    """2 (K + 8) eps |A| |B| for a K-term product on the matrix cores"""
    return 2.0 * (A.shape[1] + 8) * EPS * amm(A, B)


# ---- SMALL --------------------------------------------------------------------------------------------------------------------------------
def tolerances(parts, reltol, abstol, frac, budget_frac):
    s = float(np.sum(np.asarray(parts, dtype=LD))) if parts is not None and len(parts) else 0.0
    nc = np.sqrt(s)
    at = abstol if abstol >= 0.0 else reltol * nc
    tolc = frac * at
    return at, tolc, nc, budget_frac * tolc * tolc


def split_cc(Cc, q, m):
    """(P, H symmetrised, G12 (q x 16), G22 symmetrised (16 x 16)) out of [P_p | . | B'W | B'Z | B'W_2]"""
    nf = m - q
    P = Cc[:m, :16]
    Hraw = np.hstack([Cc[:m, 32:32 + q], Cc[:m, 48 + q:48 + q + nf]])
    H = 0.5 * (Hraw + Hraw.T)
    if nf == 0:
        return P, H, np.zeros((q, 0)), np.zeros((0, 0))
    Gz = Cc[:m, 32 + q:48 + q]
    return P, H, Gz[:q], 0.5 * (Gz[q:] + Gz[q:].T)


def whiten(G12, G22, q):
    """(L^-T = [I, X'; 0, N], S, dead flags): S = G22 - G12'G12 with a unit pivot for a dead direction, N = S^(-1/2), X = -N G12'"""
    nf = G22.shape[0]
    if nf == 0:
        return np.eye(q), np.zeros((0, 0)), np.zeros(0, dtype=bool)
    dead = ~(np.diag(G22) > 1e-30)
    S = G22 - G12.T @ G12
    S = 0.5 * (S + S.T)
    for d in np.flatnonzero(dead):
        S[d, :] = 0.0; S[:, d] = 0.0; S[d, d] = 1.0
    w, V = np.linalg.eigh(S)
    N = (V / np.sqrt(w)) @ V.T
    N = 0.5 * (N + N.T)
    X = -N @ G12.T
    LT = np.zeros((q + nf, q + nf))
    LT[:q, :q] = np.eye(q); LT[:q, q:] = X.T; LT[q:, q:] = N
    return LT, S, dead


def gram(G12, G22, q, dead):
    """G = B'B as the whitening sees it: identity block, G12, and the unit pivot of a dead direction"""
    nf = G22.shape[0]
    G = np.eye(q + nf)
    G[:q, q:] = G12; G[q:, :q] = G12.T; G[q:, q:] = G22
    for d in np.flatnonzero(dead):
        G[q + d, :] = 0.0; G[:, q + d] = 0.0; G[q + d, q + d] = 1.0
    return G


def optimal_J(lam, budget, defl2=0.0):
    """fewest kept eigenvalues (largest |lam| first) whose dropped squares, with defl2, stay within the budget"""
    a = np.sort(np.abs(lam))[::-1]
    J = len(a)
    d2 = defl2
    for c in range(len(a) - 1, -1, -1):
        if d2 + a[c] ** 2 <= budget:
            d2 += a[c] ** 2; J = c
        else:
            break
    return J, d2


def deflate(Mm, budget):
    """(deflated coordinates, the kernel's figure for them): the rows of smallest norm while twice their squared norms stay within a quarter of the
    budget.  The figure 2 sum ||row||^2 counts the block M[D, D] twice (a dropped row takes its column along, and among themselves the dropped rows
    and columns meet twice): it is the mass that leaves, ||M||_F^2 - ||M[K, K]||_F^2 with K the complement, PLUS ||M[D, D]||_F^2 — an upper bound."""
    rho = np.sum(Mm * Mm, axis=1)
    order = np.argsort(rho, kind="stable")
    cum, D = 0.0, []
    for i in order:
        if 2.0 * (cum + rho[i]) <= 0.25 * budget:
            cum += rho[i]; D.append(int(i))
        else:
            break
    return np.array(D, dtype=int), 2.0 * cum


def small(Cc, q, m, parts, reltol, abstol, frac, budget_frac):
    """dict: at, tolc, nc, budget, H, G, LT, M, lam (eigenvalues of M, decreasing |.|), J, Cp"""
    at, tolc, nc, budget = tolerances(parts, reltol, abstol, frac, budget_frac)
    P, H, G12, G22 = split_cc(Cc, q, m)
    LT, S, dead = whiten(G12, G22, q)
    G = gram(G12, G22, q, dead)
    M = LT.T @ H @ LT
    M = 0.5 * (M + M.T)
    lam = np.linalg.eigvalsh(M)
    lam = lam[np.argsort(-np.abs(lam), kind="stable")]
    J, d2 = optimal_J(lam, budget)
    return dict(at=at, tolc=tolc, nc=nc, budget=budget, P=P, H=H, G=G, S=S, LT=LT, M=M, lam=lam, J=J, d2=d2, Cp=LT @ (LT.T @ P), dead=dead)


# ---- EIG ----------------------------------------------------------------------------------------------------------------------------------
def jacobi_sweeps(S, rel=1e-10, max_sweeps=12):
    """sweeps of a cyclic Jacobi iteration (round-robin pairing over the rows that are not exactly zero) until off(A) <= rel ||S||_F"""
    A = 0.5 * (np.array(S, dtype=np.float64) + np.array(S, dtype=np.float64).T)
    act = np.flatnonzero(np.sum(A * A, axis=1) > 0.0)
    A = A[np.ix_(act, act)]
    k = A.shape[0]
    fro = np.linalg.norm(A)
    ke = k + (k & 1)
    if ke > k:
        A = np.pad(A, ((0, 1), (0, 1)))
    for sweep in range(max_sweeps + 1):
        off = np.linalg.norm(A - np.diag(np.diag(A)))
        if off <= rel * fro:
            return sweep
        if sweep == max_sweeps:
            break
        for r in range(ke - 1):
            for b in range(ke // 2):
                if b == 0:
                    p, qq = ke - 1, r
                else:
                    p, qq = (r + b) % (ke - 1), (r - b) % (ke - 1)
                if p > qq:
                    p, qq = qq, p
                if qq >= k or A[p, qq] == 0.0:
                    continue
                tau = (A[qq, qq] - A[p, p]) / (2.0 * A[p, qq])
                t = np.sign(tau) / (abs(tau) + np.hypot(1.0, tau)) if tau != 0.0 else 1.0
                c = 1.0 / np.hypot(1.0, t); s = t * c
                rp, rq = A[p].copy(), A[qq].copy()
                A[p], A[qq] = c * rp - s * rq, s * rp + c * rq
                cp, cq = A[:, p].copy(), A[:, qq].copy()
                A[:, p], A[:, qq] = c * cp - s * cq, s * cp + c * cq
    return max_sweeps + 1


# ---- FINISH -------------------------------------------------------------------------------------------------------------------------------
def finish(B, Wk, Yp, Pp, tolc, rej_in, d2):
    """(R, est2, reject): R = B Wk, est^2 = ||Y_p - B P_p||_F^2 / 16, rejected iff already so or not 2 est^2 + d2 <= tolc^2"""
    R = mm(B, Wk)
    D = np.asarray(Yp, dtype=LD) - np.asarray(B, dtype=LD) @ np.asarray(Pp, dtype=LD)
    est2 = float(np.sum(D * D) / 16)
    rej = bool(rej_in == 1.0) or not (2.0 * est2 + d2 <= tolc * tolc)
    return R, est2, rej
