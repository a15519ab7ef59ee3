"""NumPy restatement of the device's complex Gauss-Jordan inversion (csrc/dense_cgj.hip, csrc/dense_cgj_body.hpp) and of the transfer function
built on it (csrc/transfer_eval.hip): the same steps in the same order, with the host's BLAS where the device has the strided MFMA GEMM.

Inversion: blocked Gauss-Jordan with row pivoting on planar storage.  Per panel of nb = panel_nb(n) columns: per column the pivot by
|re| + |im| over the rows below (ties go to the smaller row index), the interchange, the pivot's reciprocal by Smith's formula, the scaled pivot
row, the elimination; then the interchanges of the columns outside the panel, whose panel rows move into W and leave zeros behind, and the
rank-kb update written as ONE real product
    [Cr | Ci] += [Pr | Pi] [[Wr, Wi], [-Wi, Wr]]          (n x 2kb) (2kb x 2n)
with P the panel's columns of the transform and the panel's own columns of W zero; at the end the column interchanges in reverse."""
import numpy as np
from scipy.linalg.blas import dgemm


def panel_nb(n):
    """cgj_batch_nb / fr_panel_nb_c: R = ceil(n / 512) rows per thread, 32 columns at R = 1, 16 up to 3, 8 up to 5, 4 above"""
    R = -(-n // 512)
    return 32 if R <= 1 else (16 if R <= 3 else (8 if R <= 5 else 4))


def reciprocal(pr, pi):
    """1 / (pr + i pi) by Smith's formula -> (re, im): no pr^2 + pi^2"""
    pr, pi = float(pr), float(pi)
    if abs(pr) >= abs(pi):
        r = pi / pr
        den = pr + pi * r
        return 1.0 / den, -r / den
    r = pr / pi
    den = pi + pr * r
    return r / den, -1.0 / den


def block_form(Wr, Wi):
    """[[Wr, Wi], [-Wi, Wr]]"""
    return np.block([[Wr, Wi], [-Wi, Wr]])


def block_update(Cr, Ci, Pr, Pi, Wr, Wi):
    """(Cr + i Ci) + (Pr + i Pi)(Wr + i Wi) as one real product -> (Cr, Ci)"""
    n = Cr.shape[1]
    T = np.hstack([Cr, Ci]) + np.hstack([Pr, Pi]) @ block_form(Wr, Wi)
    return T[:, :n], T[:, n:]


class Singular(Exception):
    pass


def invert(A, nb=None):
    """-> (inv(A) complex, piv (row j was swapped with row piv[j] >= j), log|det A|); Singular on an exactly zero or non-finite pivot column"""
    A = np.asarray(A, dtype=complex)
    n = A.shape[0]
    nb = nb or panel_nb(n)
    Z = np.empty((n, 2 * n), order="F")          # the planar member [Zr | Zi], at the same time an n x 2n real matrix
    Zr, Zi = Z[:, :n], Z[:, n:]
    Zr[...], Zi[...] = A.real, A.imag
    piv = np.zeros(n, dtype=np.int32)
    logdet = 0.0
    for k in range(0, n, nb):
        kb = min(nb, n - k)
        ar, ai = Zr[:, k:k + kb].copy(), Zi[:, k:k + kb].copy()
        for jj in range(kb):
            j = k + jj
            v = np.abs(ar[j:, jj]) + np.abs(ai[j:, jj])
            v = np.where(np.isnan(v), -1.0, v)                  # a NaN never wins
            p = j + int(np.argmax(v))                           # the first of equals
            best = v[p - j]
            if not best > 0.0 or not np.isfinite(best):
                raise Singular(j)
            piv[j] = p
            pr, pi = ar[p].copy(), ai[p].copy()
            if p != j:
                ar[p], ai[p] = ar[j], ai[j]
            dr, di = reciprocal(pr[jj], pi[jj])
            logdet += np.log(np.hypot(pr[jj], pi[jj]))
            sr, si = pr * dr - pi * di, pr * di + pi * dr       # the scaled pivot row; the pivot's own column holds its reciprocal
            sr[jj], si[jj] = dr, di
            fr, fi = ar[:, jj].copy(), ai[:, jj].copy()
            ar[:, jj] = 0.0
            ai[:, jj] = 0.0
            ar -= np.outer(fr, sr) - np.outer(fi, si)
            ai -= np.outer(fr, si) + np.outer(fi, sr)
            ar[j], ai[j] = sr, si
        # the interchanges on the columns outside the panel, W = rows k .. k+kb of them (the panel's own columns zero)
        for jj in range(kb):
            j, p = k + jj, piv[k + jj]
            if p != j:
                Z[[j, p]] = Z[[p, j]]
        Wr, Wi = Zr[k:k + kb].copy(), Zi[k:k + kb].copy()
        Wr[:, k:k + kb] = 0.0
        Wi[:, k:k + kb] = 0.0
        Z[k:k + kb] = 0.0                                        # the update writes M W into the panel's rows
        Zr[:, k:k + kb], Zi[:, k:k + kb] = ar, ai               # (the panel's columns carry their interchanges already)
        Pt = np.hstack([ar, ai])
        Z = dgemm(1.0, Pt, block_form(Wr, Wi), beta=1.0, c=Z, overwrite_c=True)          # Z += Pt Wt in place (Z is column-major)
        Zr, Zi = Z[:, :n], Z[:, n:]
    for j in range(n - 1, -1, -1):
        p = piv[j]
        if p != j:
            Zr[:, [j, p]] = Zr[:, [p, j]]
            Zi[:, [j, p]] = Zi[:, [p, j]]
    return Zr + 1j * Zi, piv, float(logdet)


def unblocked_pivots(A):
    """the interchanges of a plain complex Gauss-Jordan elimination with the same pivot rule, one column at a time"""
    Z = np.array(A, dtype=complex)
    n = Z.shape[0]
    piv = np.zeros(n, dtype=np.int32)
    for j in range(n):
        v = np.abs(Z[j:, j].real) + np.abs(Z[j:, j].imag)
        p = j + int(np.argmax(v))
        piv[j] = p
        if p != j:
            Z[[j, p]] = Z[[p, j]]
        row = Z[j] / Z[j, j]
        f = Z[:, j].copy()
        f[j] = 0.0
        Z -= np.outer(f, row)
        Z[j] = row
    return piv


def transfer(E, A, B, C, s, refine=True):
    """H(s_k) = C (s_k E - A)^-1 B at every point of s: complex (K, q, m).  Per point: the planes of s E - A, the inversion above, Y = X B, one
    refinement step with the residual from E and A, Y += X R through the block form, C Y."""
    H = np.empty((len(s), C.shape[0], B.shape[1]), dtype=complex)
    m = B.shape[1]
    for k, sk in enumerate(s):
        sg, w = float(np.real(sk)), float(np.imag(sk))
        X = invert((sg * E - A) + 1j * (w * E))[0]
        Xr, Xi = X.real, X.imag
        Yr, Yi = Xr @ B, Xi @ B
        if refine:
            Rr = B + A @ Yr - sg * (E @ Yr) + w * (E @ Yi)
            Ri = A @ Yi - sg * (E @ Yi) - w * (E @ Yr)
            T = np.hstack([Yr, Yi]) + np.hstack([Xr, Xi]) @ block_form(Rr, Ri)
            Yr, Yi = T[:, :m], T[:, m:]
        H[k] = C @ Yr + 1j * (C @ Yi)
    return H


def lapack(E, A, B, C, s):
    """the complex LU solve per point"""
    return np.array([C @ np.linalg.solve(sk * E - A, B.astype(complex)) for sk in s])


def rel_dist(H, Href):
    """per point ||H - Href||_F / ||Href||_F"""
    return np.array([np.linalg.norm(h - r) / np.linalg.norm(r) for h, r in zip(np.asarray(H), np.asarray(Href))])


# ---- the matrices of the inversion tests ---------------------------------------------------------------------------------------------------
def test_matrix(n, b=0):
    """randn + i randn + 4 sqrt(n) e^{i theta} I, seeded by (n, b): cond of order 10"""
    rng = np.random.default_rng(1000 * n + b)
    theta = rng.uniform(0.0, 2.0 * np.pi)
    return rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)) + 4.0 * np.sqrt(n) * np.exp(1j * theta) * np.eye(n)


test_matrix.__test__ = False


def probes(n):
    """four seeded complex probe vectors (n x 4)"""
    rng = np.random.default_rng(77 + n)
    return rng.standard_normal((n, 4)) + 1j * rng.standard_normal((n, 4))


def probe_residual(A, X):
    """max over the four probes of ||A (X v) - v|| / ||v||"""
    V = probes(A.shape[0])
    R = A @ (X @ V) - V
    return float((np.linalg.norm(R, axis=0) / np.linalg.norm(V, axis=0)).max())


def full_residual(A, X):
    """||A X - I||_F / ||I||_F"""
    n = A.shape[0]
    return float(np.linalg.norm(A @ X - np.eye(n)) / np.sqrt(n))
