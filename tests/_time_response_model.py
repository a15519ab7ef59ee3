"""NumPy restatement of the device's time response (csrc/time_response.hip): P = E - theta A and numpy.linalg.inv of it, M and N, the stack
O = [G_0; ...; G_K] of G_j = C M^j by doubling up to the block length L and block marching beyond it, the thin product h = O N, and the
output stage: the chunked exclusive prefix sum (step), O E^-1 B (impulse), the causal convolution in ascending j (simulate).  The device
replaces numpy.linalg.inv by the Gauss-Jordan inversion and the products by the MFMA GEMM; the steps and their order are the same.
`sequential` is the plain float64 recurrence x_{k+1} = M x_k + N w_k with a LAPACK solve ("LAPACK" in the record)."""
import numpy as np

METHODS = ("tustin", "backward_euler")
SCAN_T = 64        # TR_SCAN_T of the device


def theta_beta(method, dt):
    """(theta of P = E - theta A, beta of the step response)"""
    if method == "tustin":
        return 0.5 * dt, 2.0
    if method == "backward_euler":
        return dt, 1.0
    raise ValueError(method)


def one_step(E, A, B, dt, method):
    """(M, N) of x_{k+1} = M x_k + N w_k"""
    th, _ = theta_beta(method, dt)
    Pinv = np.linalg.inv(E - th * A)
    n = E.shape[0]
    M = 2.0 * (Pinv @ E) - np.eye(n) if method == "tustin" else Pinv @ E
    return M, th * (Pinv @ B)


def inputs_w(u, method):
    """w_k, k = 0 .. K-1, from u (K+1, m)"""
    return u[:-1] + u[1:] if method == "tustin" else u[1:].copy()


def default_block(q, K, n):
    """tr_default_block of the device: L fills 256 compute units with the 64 x 64 tiles of one marching GEMM, is at most the power of two
    >= K + 1, and is halved while the stack of whole blocks would hold over 5/4 (K + 1) sample rows"""
    coltiles, K1 = -(-n // 64), K + 1
    L = 1
    while -(-L * q // 64) * coltiles < 256:
        L *= 2
    L = min(L, _pow2_at_least(K1))
    while L > 1 and -(-K1 // L) * L * 4 > K1 * 5:
        L //= 2
    return L


def _pow2_at_least(v):
    p = 1
    while p < v:
        p *= 2
    return p


def block_in_force(q, K, n, block=None):
    return min(block, _pow2_at_least(K + 1)) if block else default_block(q, K, n)


def markov_stack(C, M, K, L):
    """O (nblocks L, q, n): doubling to L rows of G, then block_{b+1} = block_b M^L; info = (blocks, squarings)"""
    q, n = C.shape
    nblocks = -(-(K + 1) // L)
    O = np.empty((nblocks * L * q, n))
    O[:q] = C
    Mp, J, squarings = M, 1, 0
    while J < L:
        O[J * q:2 * J * q] = O[:J * q] @ Mp
        if 2 * J < L or nblocks > 1:
            Mp = Mp @ Mp
            squarings += 1
        J *= 2
    for b in range(nblocks - 1):
        O[(b + 1) * L * q:(b + 2) * L * q] = O[b * L * q:(b + 1) * L * q] @ Mp
    return O, nblocks, squarings


def _scan(h, beta):
    """exclusive prefix sum over k of h (K+1, q, m) in chunks of SCAN_T: chunk sums, their scan, add (the device's three phases)"""
    K1 = h.shape[0]
    nch = -(-K1 // SCAN_T)
    sums = np.zeros((nch,) + h.shape[1:])
    for t in range(nch):
        for k in range(t * SCAN_T, min((t + 1) * SCAN_T, K1)):
            sums[t] = sums[t] + h[k]
    off = np.zeros_like(sums)
    for t in range(1, nch):
        off[t] = off[t - 1] + sums[t - 1]
    Y = np.empty_like(h)
    for t in range(nch):
        run = off[t].copy()
        for k in range(t * SCAN_T, min((t + 1) * SCAN_T, K1)):
            Y[k] = beta * run
            run = run + h[k]
    return Y


def _stack(E, A, B, C, dt, K, method, block):
    M, N = one_step(E, A, B, dt, method)
    L = block_in_force(C.shape[0], K, C.shape[1], block)
    O, nblocks, sq = markov_stack(C, M, K, L)
    return M, N, O, dict(block=L, blocks=nblocks, squarings=sq)


def step_response(E, A, B, C, dt, K, method="tustin", block=None, return_info=False):
    """(K+1, q, m): y_k = beta sum_{j<k} h_j"""
    q, m = C.shape[0], B.shape[1]
    _, N, O, info = _stack(E, A, B, C, dt, K, method, block)
    h = (O @ N)[:(K + 1) * q].reshape(K + 1, q, m)
    Y = _scan(h, theta_beta(method, dt)[1])
    return (Y, info) if return_info else Y


def impulse_response(E, A, B, C, dt, K, method="tustin", block=None):
    """(K+1, q, m): y_k = G_k E^-1 B"""
    q, m = C.shape[0], B.shape[1]
    _, _, O, _ = _stack(E, A, B, C, dt, K, method, block)
    return (O @ (np.linalg.inv(E) @ B))[:(K + 1) * q].reshape(K + 1, q, m)


def simulate(E, A, B, C, u, dt, x0=None, method="tustin", block=None):
    """u (K+1, m) -> (K+1, q): y_k = G_k x_0 + sum_{j<k} h_j w_{k-1-j}, j ascending (D is the caller's)"""
    u = np.asarray(u, dtype=float)
    K, q, m = u.shape[0] - 1, C.shape[0], B.shape[1]
    _, N, O, _ = _stack(E, A, B, C, dt, K, method, block)
    h = (O @ N)[:(K + 1) * q].reshape(K + 1, q, m)
    w = inputs_w(u, method)
    Y = np.zeros((K + 1, q))
    for j in range(K):              # every output accumulates in ascending j, the input channel innermost (vectorised over k > j)
        for c in range(m):
            Y[j + 1:] += np.outer(w[:K - j, c], h[j][:, c])
    if x0 is not None:
        Y = Y + (O @ np.asarray(x0, dtype=float))[:(K + 1) * q].reshape(K + 1, q)
    return Y


# ---- the plain recurrence in float64 ("LAPACK") --------------------------------------------------------------------------------------------
def sequential(E, A, B, C, dt, K, method, kind, u=None, x0=None):
    """kind "step" / "impulse": (K+1, q, m); "simulate": (K+1, q).  x_{k+1} = M x_k + N w_k step by step, P by numpy.linalg.solve"""
    th, _ = theta_beta(method, dt)
    n, m = B.shape
    P = E - th * A
    PE, N = np.linalg.solve(P, E), th * np.linalg.solve(P, B)
    M = 2.0 * PE - np.eye(n) if method == "tustin" else PE
    if kind == "step":
        X, W = np.zeros((n, m)), (2.0 if method == "tustin" else 1.0) * np.eye(m)
    elif kind == "impulse":
        X, W = np.linalg.solve(E, B), None
    else:
        u = np.asarray(u, dtype=float)
        X = np.zeros(n) if x0 is None else np.array(x0, dtype=float)
        w = inputs_w(u, method)
    out = []
    for k in range(K + 1):
        out.append(C @ X)
        if k == K:
            break
        if kind == "step":
            X = M @ X + N @ W
        elif kind == "impulse":
            X = M @ X
        else:
            X = M @ X + N @ w[k]
    return np.array(out)


def rel_dist(Y, Yref):
    """max_k ||Y_k - Yref_k||_F / max_k ||Yref_k||_F"""
    Y, Yref = np.asarray(Y), np.asarray(Yref)
    K1 = Y.shape[0]
    d = (Y - Yref).reshape(K1, -1)
    return float(np.linalg.norm(d, axis=1).max() / np.linalg.norm(Yref.reshape(K1, -1), axis=1).max())
