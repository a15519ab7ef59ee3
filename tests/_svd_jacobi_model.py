"""NumPy model of the device's one-sided block Jacobi SVD (csrc/svd_jacobi.hip) and of square-root balanced truncation on top of it
(csrc/balance.hip): the same padding, tournament, rotation test, inner-sweep cap, floor and exit.  It fixes the expected sweep counts and is
where the bounds of tests/test_gpu_svd_jacobi.py and tests/test_gpu_balance.py come from.

    layout      A (m x w, m >= w; a wide input is transposed at the entry and U, V are swapped at the exit) is padded with zero columns to
                W = 16 p, p >= 2: G (m x W), V = I (W x W).  The rounds are those of tests/_block_jacobi_model.py (schedule).
    block pair  H = [G_i G_j]'[G_i G_j] (32 x 32) is diagonalised by cyclic Jacobi (at most INNER_MAX sweeps, ended by the first sweep without
                a rotation), J accumulated; [G_i G_j] <- [G_i G_j] J, [V_i V_j] <- [V_i V_j] J when anything was rotated.
    rotation    (r, c) is rotated when h_rc != 0, h_rr h_cc > 0, |h_rc| > tol sqrt(h_rr h_cc) and sqrt(h_rr h_cc) > (tol ||A||_F)^2.  The last
                condition leaves pairs of noise columns alone; h_rr h_cc > 0 also covers a diagonal entry that the inner sweeps drove to zero
                or slightly below.
    stop        a whole sweep without a rotation (that sweep is counted); more than MAX_SWEEPS sweeps is an error.  tol = sqrt(m) eps.
    exit        sigma = column norms of G, sorted descending (stable); U = G / sigma for sigma > tol ||A||_F, zero columns otherwise (their
                number defines the numerical rank); V = the first w rows of the permuted V.
"""
import functools
import json
import os

import numpy as np

from _block_jacobi_model import B, INNER_MAX, _INNER, schedule

MAX_SWEEPS = 60
EPS = np.finfo(float).eps


class NotConverged(RuntimeError):
    pass


def padded_width(w):
    return max(2, -(-w // B)) * B


def gram_jacobi(H, tol, floor):
    """cyclic Jacobi with the SVD's rotation test on a batch of Gram blocks H (k, 32, 32), in place: (J, rotated (k,) bool)"""
    k = H.shape[0]
    J = np.broadcast_to(np.eye(2 * B), H.shape).copy()
    rotated = np.zeros(k, dtype=bool)
    live = np.ones(k, dtype=bool)
    for _ in range(INNER_MAX):
        any_rot = np.zeros(k, dtype=bool)
        for p, q in _INNER:
            app, aqq, apq = H[:, p, p], H[:, q, q], H[:, p, q]
            prod = app * aqq
            with np.errstate(all="ignore"):
                g = np.sqrt(np.where(prod > 0.0, prod, 0.0))
                rot = (apq != 0.0) & (prod > 0.0) & (np.abs(apq) > tol * g) & (g > floor) & live[:, None]
                tau = (aqq - app) / (2.0 * np.where(rot, apq, 1.0))
                t = np.where(tau >= 0, 1.0, -1.0) / (np.abs(tau) + np.sqrt(1.0 + tau * tau))
                c = 1.0 / np.sqrt(1.0 + t * t)
            c = np.where(rot, c, 1.0)
            s = np.where(rot, t * c, 0.0)
            for M in (H, J):
                x, y = M[:, :, p], M[:, :, q]
                M[:, :, p], M[:, :, q] = c[:, None, :] * x - s[:, None, :] * y, s[:, None, :] * x + c[:, None, :] * y
            x, y = H[:, p, :], H[:, q, :]
            H[:, p, :], H[:, q, :] = c[:, :, None] * x - s[:, :, None] * y, s[:, :, None] * x + c[:, :, None] * y
            bi, ki = np.nonzero(rot)
            H[bi, p[ki], q[ki]] = 0.0
            H[bi, q[ki], p[ki]] = 0.0
            any_rot |= rot.any(axis=1)
        rotated |= any_rot
        live &= any_rot
        if not live.any():
            break
    return J, rotated


def default_tol(m, w):
    return np.sqrt(max(m, w)) * EPS


def svd(A, tol=None):
    """(U (m x k), s (k,), V (w x k), stats) with k = min(m, w), A ~ U diag(s) V'; stats = dict(sweeps, rounds, rank)"""
    A = np.asarray(A, dtype=float)
    if A.shape[0] < A.shape[1]:
        V, s, U, st = svd(A.T, tol)
        return U, s, V, st
    m, w = A.shape
    if w == 0:
        return np.zeros((m, 0)), np.zeros(0), np.zeros((0, 0)), dict(sweeps=0, rounds=0, rank=0)
    tol = default_tol(m, w) if tol is None or not tol > 0 else float(tol)
    normA = float(np.linalg.norm(A))
    if not np.isfinite(normA):
        raise ValueError("non-finite input")
    floor = (tol * normA) ** 2
    W = padded_width(w)
    G = np.zeros((m, W))
    G[:, :w] = A
    V = np.eye(W)
    rounds = schedule(W // B)
    sweeps = nrounds = 0
    while True:
        if sweeps >= MAX_SWEEPS:
            raise NotConverged(f"{sweeps} sweeps")
        any_rot = False
        for pairs, _sit in rounds:
            idx = np.array([np.r_[i * B:(i + 1) * B, j * B:(j + 1) * B] for i, j in pairs])
            X = G[:, idx]                                        # (m, pairs, 32)
            H = np.einsum("mka,mkb->kab", X, X)
            H = 0.5 * (H + H.transpose(0, 2, 1))
            J, rotated = gram_jacobi(H, tol, floor)
            nrounds += 1
            for k in np.nonzero(rotated)[0]:
                G[:, idx[k]] = G[:, idx[k]] @ J[k]
                V[:, idx[k]] = V[:, idx[k]] @ J[k]
            any_rot |= bool(rotated.any())
        sweeps += 1
        if not any_rot:
            break
    sig = np.sqrt(np.sum(G[:, :w] ** 2, axis=0))
    perm = np.argsort(-sig, kind="stable")
    sig = sig[perm]
    keep = sig > tol * normA
    U = np.zeros((m, w))
    U[:, keep] = G[:, perm[keep]] / sig[keep]
    return U, sig, V[:w, perm], dict(sweeps=sweeps, rounds=nrounds, rank=int(keep.sum()))


def errors(A, U, s, V):
    """the four error measures: max |sigma - sigma_ref| / sigma_1 against numpy.linalg.svd, ||V'V - I||_F, ||A - U S V'||_F / ||A||_F and
    ||U'U - I||_F over the columns with sigma > 1e-8 sigma_1"""
    A = np.asarray(A, dtype=float)
    ref = np.linalg.svd(A, compute_uv=False)
    s1 = max(ref[0], np.finfo(float).tiny) if len(ref) else 1.0
    nf = max(np.linalg.norm(A), np.finfo(float).tiny)
    big = s > 1e-8 * s1
    Ub = U[:, big]
    return (float(np.abs(s - ref).max() / s1) if len(ref) else 0.0, float(np.linalg.norm(V.T @ V - np.eye(V.shape[1]))),
            float(np.linalg.norm(A - (U * s) @ V.T) / nf), float(np.linalg.norm(Ub.T @ Ub - np.eye(Ub.shape[1]))))


MEASURES = ("sigma", "orth_v", "residual", "orth_u")


# ---- the matrices of the tests (fixed seeds) ---------------------------------------------------------------------------------------
def _graded(m, w, lo, seed):
    rng = np.random.default_rng(seed)
    U = np.linalg.qr(rng.standard_normal((m, w)))[0]
    V = np.linalg.qr(rng.standard_normal((w, w)))[0]
    return (U * np.logspace(0.0, lo, w)) @ V.T


def _random(m, w):
    return np.random.default_rng(3000 + 100 * m + w).standard_normal((m, w))


def _rank5():
    rng = np.random.default_rng(31)
    return rng.standard_normal((50, 5)) @ rng.standard_normal((5, 40))


def hankel371():
    """Z_o'E Z_c of the n = 371 pencil of tests/_sign_dual_cases.py (118 x 106), as tests/test_svd_balance_host.py's reference chain forms it;
    recorded in tests/golden/svd_jacobi_hankel371.npy (regenerated by running this file)"""
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svd_jacobi_hankel371.npy"))


CASES = {
    "random40x33": lambda: _random(40, 33),
    "random70x17": lambda: _random(70, 17),
    "graded64x48": lambda: _graded(64, 48, -20.0, 21),
    "graded100x80": lambda: _graded(100, 80, -30.0, 22),
    "rank5_50x40": _rank5,
    "one_column": lambda: _random(23, 1),
    "zero": lambda: np.zeros((20, 12)),
    "hankel371": hankel371,
    # the shapes at which the device code takes another path: the K tail of the MFMA loop, several row slabs, the transposed entry
    "random33x32": lambda: _random(33, 32),
    "random35x32": lambda: _random(35, 32),
    "random300x32": lambda: _random(300, 32),
    "wide33x40": lambda: _random(33, 40),
}


@functools.lru_cache(maxsize=None)
def case(name):
    A = CASES[name]()
    A.setflags(write=False)
    return A


@functools.lru_cache(maxsize=None)
def run(name):
    """the model's run of a named case, computed once per process: dict(U, s, V, sweeps, rounds, rank, err)"""
    A = case(name)
    U, s, V, st = svd(A)
    return dict(U=U, s=s, V=V, err=errors(A, U, s, V), **st)


# ---- balanced truncation (the steps of csrc/balance.hip) -------------------------------------------------------------------------------
def sqrt_factor(L, d):
    """Z = L sqrt(d) over the columns with d > 0: (Z, dropped, largest |d| among the dropped)"""
    d = np.diag(d) if np.ndim(d) == 2 and min(np.shape(d)) > 1 else np.ravel(d)
    pos = d > 0
    neg = np.abs(d[~pos])
    return L[:, pos] * np.sqrt(d[pos]), int((~pos).sum()), float(neg.max()) if neg.size else 0.0


def choose_order(s, rank, tol):
    """the smallest r with 2 sum_{i > r} sigma_i <= tol sigma_1 (tail summed from the smallest sigma upward), at most the numerical rank"""
    r, tail = len(s), 0.0
    while r > 0 and 2.0 * (tail + s[r - 1]) <= tol * s[0]:
        tail += s[r - 1]
        r -= 1
    return min(r, rank)


def balance(E, A, Bm, Cm, Lc, dc, Lo, do, order=0, tol=1e-8, svd_fn=None):
    """square-root balanced truncation from the Gramians P = Lc diag(dc) Lc', Q = Lo diag(do) Lo': dict(hsv, T, W, Ar, Br, Cr, order, rank,
    r_c, r_o, dropped, sweeps, eye_err, bound, neg_max)"""
    Zc, drop_c, neg_c = sqrt_factor(Lc, dc)
    Zo, drop_o, neg_o = sqrt_factor(Lo, do)
    M = Zo.T @ (E @ Zc)
    U, s, V, st = (svd_fn or svd)(M)
    rank = st["rank"]
    if order > 0:
        if order > rank:
            raise ValueError(f"order {order} above the numerical rank {rank}")
        r = order
    else:
        r = choose_order(s, rank, tol)
    sc = 1.0 / np.sqrt(s[:r])
    Wm, T = (Zo @ U[:, :r]) * sc, (Zc @ V[:, :r]) * sc
    return dict(hsv=s, T=T, W=Wm, Ar=Wm.T @ (A @ T), Br=Wm.T @ Bm, Cr=Cm @ T, order=r, rank=rank, r_c=Zc.shape[1], r_o=Zo.shape[1],
                dropped=drop_c + drop_o, sweeps=st["sweeps"], eye_err=float(np.linalg.norm(Wm.T @ (E @ T) - np.eye(r))),
                bound=2.0 * float(np.sum(s[r:][::-1])), neg_max=max(neg_c, neg_o), M=M)


# ---- the recorded run ------------------------------------------------------------------------------------------------------------------
# Regenerate with:  python tests/_svd_jacobi_model.py   (tests/ and oracle/ on the path; writes the Hankel matrix first, then the record)
def record_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "svd_jacobi_model.json")


@functools.lru_cache(maxsize=None)
def recorded():
    with open(record_path()) as f:
        return json.load(f)


if __name__ == "__main__":
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), os.path.join(os.path.dirname(here), "oracle")]
    import _balance_cases as bc
    np.save(os.path.join(here, "golden", "svd_jacobi_hankel371.npy"), bc.reference(371)["M"])
    out = {}
    for name in CASES:
        r = run(name)
        out[name] = dict(shape=list(case(name).shape), sweeps=int(r["sweeps"]), rounds=int(r["rounds"]), rank=int(r["rank"]),
                         **{k: v for k, v in zip(MEASURES, r["err"])})
        print(name, out[name])
    out["balance"] = bc.record()
    print(out["balance"])
    np.savez(bc.golden_path(), **bc.golden_arrays())
    with open(record_path(), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
