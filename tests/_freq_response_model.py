"""NumPy restatement of the device's frequency response (csrc/freq_response.hip): per frequency the real form of i w E - A, its inverse, the
product with B, one refinement step with the residual formed from E and A, and the two products with C.  The device replaces numpy.linalg.inv
by the register-panel Gauss-Jordan inversion and the products by the strided MFMA GEMM; the steps and their order are the same."""
import numpy as np


def embedding(E, A, w):
    """M = [[-A, -w E], [w E, -A]]:  (i w E - A)(x + i y) = b  <=>  M [x; y] = [b; 0]"""
    return np.block([[-A, -w * E], [w * E, -A]])


def freq_response(E, A, B, C, omega):
    """H(i w) = C (i w E - A)^-1 B at every frequency of omega: complex (K, q, m)"""
    n = E.shape[0]
    H = np.empty((len(omega), C.shape[0], B.shape[1]), dtype=complex)
    for k, w in enumerate(omega):
        Minv = np.linalg.inv(embedding(E, A, float(w)))
        Y = Minv[:, :n] @ B
        # R = [B; 0] - M Y from E and A (M is not kept), Y <- Y + M^-1 R
        R = np.vstack([B + A @ Y[:n] + w * (E @ Y[n:]), A @ Y[n:] - w * (E @ Y[:n])])
        Y = Y + Minv @ R
        H[k] = C @ Y[:n] + 1j * (C @ Y[n:])
    return H


def lapack(E, A, B, C, omega):
    """the complex LU solve per frequency (what tests/_balance_cases.py: transfer does)"""
    return np.array([C @ np.linalg.solve(1j * w * E - A, B.astype(complex)) for w in omega])


def rel_dist(H, Href):
    """per frequency ||H - Href||_F / ||Href||_F"""
    H, Href = np.asarray(H), np.asarray(Href)
    return np.array([np.linalg.norm(h - r) / np.linalg.norm(r) for h, r in zip(H, Href)])
