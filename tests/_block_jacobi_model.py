"""NumPy model of the device's block Jacobi eigensolver (csrc/sym_jacobi.hip): the same blocking (b = 16, zero padding to a multiple of 16 and
to at least two blocks), the same round-robin ordering of the block pairs and of the 32 indices inside a pivot block, the same rotation
threshold and the same stopping rule.  It fixes the expected sweep counts and is where the bounds of tests/test_gpu_sym_jacobi.py come from.

    threshold   a rotation (r, c) of a pivot block is done when |a_rc| > (tol / Q) ||A||_F  (Q the padded order): once every pivot block
                skips all its rotations, every off-diagonal entry is at most that, so off(A) <= tol ||A||_F
    pivot       cyclic Jacobi on the 32 x 32 block, at most INNER_MAX sweeps, ended by the first sweep without a rotation
    stop        off(A) <= tol ||A||_F with tol = q eps by default, both norms measured after every sweep; more than MAX_SWEEPS is an error
"""
import numpy as np

B = 16
INNER_MAX = 10
MAX_SWEEPS = 30
EPS = np.finfo(float).eps


class NotConverged(RuntimeError):
    pass


def padded_order(q):
    return max(2, -(-q // B)) * B


def rr_pair(players, step, k):
    """pair k (0 <= k < players / 2) of round `step` (0 <= step < players - 1) of the round-robin tournament of an even number of players"""
    m = players - 1
    if k == 0:
        return m, step
    return (step + k) % m, (step - k + m) % m


def schedule(p):
    """the rounds of p blocks: (list of disjoint block pairs (i < j), block that sits out or -1); an odd p plays against a dummy"""
    players = p + (p & 1)
    rounds = []
    for step in range(players - 1):
        pairs, sit = [], -1
        for k in range(players // 2):
            a, b = rr_pair(players, step, k)
            if a >= p:
                sit = b
            elif b >= p:
                sit = a
            else:
                pairs.append((min(a, b), max(a, b)))
        rounds.append((pairs, sit))
    return rounds


_INNER = []
for _s in range(2 * B - 1):
    _pq = [rr_pair(2 * B, _s, k) for k in range(B)]
    _INNER.append((np.array([min(a, b) for a, b in _pq]), np.array([max(a, b) for a, b in _pq])))


def pivot_jacobi(G, thr):
    """cyclic Jacobi on a batch of 32 x 32 blocks G (m, 32, 32), in place: (J (m, 32, 32), rotated (m,) bool)"""
    m = G.shape[0]
    J = np.broadcast_to(np.eye(2 * B), G.shape).copy()
    rotated = np.zeros(m, dtype=bool)
    live = np.ones(m, dtype=bool)
    for _ in range(INNER_MAX):
        any_rot = np.zeros(m, dtype=bool)
        for p, q in _INNER:
            app, aqq, apq = G[:, p, p], G[:, q, q], G[:, p, q]
            rot = (np.abs(apq) > thr) & live[:, None]
            with np.errstate(all="ignore"):
                tau = (aqq - app) / (2.0 * np.where(rot, apq, 1.0))
                t = np.where(tau >= 0, 1.0, -1.0) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
                c = 1.0 / np.sqrt(1.0 + t * t)
            c = np.where(rot, c, 1.0)
            s = np.where(rot, t * c, 0.0)
            for M in (G, J):
                x, y = M[:, :, p], M[:, :, q]
                M[:, :, p], M[:, :, q] = c[:, None, :] * x - s[:, None, :] * y, s[:, None, :] * x + c[:, None, :] * y
            x, y = G[:, p, :], G[:, q, :]
            G[:, p, :], G[:, q, :] = c[:, :, None] * x - s[:, :, None] * y, s[:, :, None] * x + c[:, :, None] * y
            bi, ki = np.nonzero(rot)
            G[bi, p[ki], q[ki]] = 0.0
            G[bi, q[ki], p[ki]] = 0.0
            any_rot |= rot.any(axis=1)
        rotated |= any_rot
        live &= any_rot                     # a block whose sweep made no rotation is finished
        if not live.any():
            break
    return J, rotated


def _measure(A):
    d = np.diag(A)
    off2 = float(np.sum((A - np.diag(d)) ** 2))
    return np.sqrt(off2), np.sqrt(off2 + float(np.sum(d * d)))


def solve(S, tol=None):
    """(w (q,), V (q, q), sweeps, rounds): unsorted eigenvalues, column i of V belongs to w[i]"""
    S = np.asarray(S, dtype=float)
    q = S.shape[0]
    assert S.shape == (q, q) and q >= 1
    tol = q * EPS if tol is None or not tol > 0 else float(tol)
    Q = padded_order(q)
    p = Q // B
    A = np.zeros((Q, Q))
    A[:q, :q] = S
    V = np.eye(Q)
    off, norm = _measure(A)
    if not np.isfinite(norm):
        raise ValueError("non-finite input")
    rounds = schedule(p)
    sweeps = nrounds = 0
    while not off <= tol * norm:
        if sweeps >= MAX_SWEEPS:
            raise NotConverged(f"{sweeps} sweeps")
        thr = tol / Q * norm
        for pairs, _sit in rounds:
            idx = np.array([np.r_[i * B:(i + 1) * B, j * B:(j + 1) * B] for i, j in pairs])
            G = A[idx[:, :, None], idx[:, None, :]].copy()
            J, rotated = pivot_jacobi(G, thr)
            nrounds += 1
            if not rotated.any():
                continue
            Jf = np.eye(Q)
            for k in range(len(pairs)):
                Jf[np.ix_(idx[k], idx[k])] = J[k]
            A = Jf.T @ A @ Jf
            V = V @ Jf
        sweeps += 1
        off, norm = _measure(A)
        if not np.isfinite(norm):
            raise ValueError("non-finite values")
    return np.diag(A)[:q].copy(), V[:q, :q].copy(), sweeps, nrounds


def errors(S, w, V):
    """the three error measures of a computed decomposition against numpy.linalg.eigh: (max |lambda - lambda_ref| / ||S||_2,
    ||S V - V diag(w)||_F / ||S||_F, ||V'V - I||_F)"""
    S = np.asarray(S, dtype=float)
    ref = np.linalg.eigvalsh(S)
    n2 = max(np.abs(ref).max(), np.finfo(float).tiny)
    nf = max(np.linalg.norm(S), np.finfo(float).tiny)
    return (float(np.abs(np.sort(w) - ref).max() / n2), float(np.linalg.norm(S @ V - V * w) / nf),
            float(np.linalg.norm(V.T @ V - np.eye(len(w)))))


# ---- the matrices of the tests (fixed seeds) ---------------------------------------------------------------------------------------
def _orth(n, rng):
    return np.linalg.qr(rng.standard_normal((n, n)))[0]


def from_spectrum(lam, seed):
    lam = np.asarray(lam, dtype=float)
    U = _orth(len(lam), np.random.default_rng(seed))
    A = (U * lam) @ U.T
    return 0.5 * (A + A.T)


def random_indefinite(n, seed=0):
    M = np.random.default_rng(1000 + n + seed).standard_normal((n, n))
    return 0.5 * (M + M.T)


def diagonal(n=64):
    return np.diag(np.random.default_rng(7).standard_normal(n))


def plus_minus_pairs(n=64):
    lam = np.random.default_rng(8).uniform(0.1, 2.0, n // 2)
    return from_spectrum(np.r_[lam, -lam], 9)


def rank3(n=96):
    G = np.random.default_rng(10).standard_normal((n, 3))
    return (G * np.array([2.0, -1.0, 0.5])) @ G.T


def cluster20(n=64):
    lam = np.random.default_rng(11).uniform(-1.0, 1.0, n)
    lam[10:30] = 0.75
    return from_spectrum(lam, 12)


def graded(n=64):
    return from_spectrum(np.logspace(0, -12, n), 13)


RANDOM_ORDERS = (1, 2, 15, 16, 17, 33, 48, 64, 130, 352)
SPECIAL = {"diagonal": diagonal, "plus_minus_pairs": plus_minus_pairs, "rank3": rank3, "cluster20": cluster20, "graded": graded}


def cases():
    """name -> matrix, every input of the host and the device tests"""
    out = {f"random{n}": random_indefinite(n) for n in RANDOM_ORDERS}
    out.update({k: f() for k, f in SPECIAL.items()})
    return out


_RUNS = {}


def run(name):
    """the model's run of a named case, computed once per process: dict(S, w, V, sweeps, rounds, err)"""
    if name not in _RUNS:
        S = cases()[name]
        w, V, sweeps, rounds = solve(S)
        _RUNS[name] = dict(S=S, w=w, V=V, sweeps=sweeps, rounds=rounds, err=errors(S, w, V))
    return _RUNS[name]


# ---- the recorded run ------------------------------------------------------------------------------------------------------------------
# The model's figures for every case, as JSON: the device tests read their bounds from this record (the order-352 case takes the model ten
# seconds, too long to repeat in every session); tests/test_sym_jacobi_host.py repeats the cheaper cases live and compares.
# Regenerate with:  python tests/_block_jacobi_model.py
def record_path():
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "block_jacobi_model.json")


def recorded():
    import json
    with open(record_path()) as f:
        return json.load(f)


if __name__ == "__main__":
    import json
    out = {}
    for name in cases():
        r = run(name)
        out[name] = dict(order=int(r["S"].shape[0]), sweeps=int(r["sweeps"]), rounds=int(r["rounds"]), eig_err=r["err"][0], residual=r["err"][1],
                         orth=r["err"][2])
        print(name, out[name])
    with open(record_path(), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
