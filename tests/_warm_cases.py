"""The input families of tests/test_gpu_warm.py, with the condition each one is built to meet.  tests/test_warm_host.py asserts the conditions on the
CPU for exactly these inputs (same functions, same seeds), so that no GPU test can hide a failure behind a borderline input:
  * dead / live pivots of PROJECT sit a factor >= 1e4 away from the 1e-10 floor;
  * every spectrum used for a J assertion has a gap: kept eigenvalues >= 100 sqrt(budget) in magnitude, squared sum of the others <= budget / 100;
  * accepted / rejected cases sit a factor >= 4 on either side of their thresholds;
  * the EIG inputs held to the off-diagonal bound need at most 6 sweeps of the model's Jacobi iteration (at most one case in six may be exempt)."""
import functools

import numpy as np

import _warm_model as M

# ---- PROJECT ----------------------------------------------------------------------------------------------------------------------------
PROJECT_N = (96, 97, 111, 371, 1024, 4112)
PROJECT_Q = (1, 16, 17, 63, 64)
PROJECT_DEAD = (("dup", 97, 17), ("zero", 111, 16), ("allzero", 97, 16), ("dup", 4112, 64), ("zero", 371, 63), ("near", 97, 17), ("near", 371, 16))


def _orth(rng, n, k):
    return np.linalg.qr(rng.standard_normal((n, k)))[0]


@functools.lru_cache(maxsize=None)
def project_inputs(kind, n, q):
    """(Q, Yf, Pf, expected live flags).  plain: 16 independent columns of different scales;  dup: column 9 repeats column 2 exactly;  near: column 9 is column 2 plus 8e-8 of noise (a POSITIVE pivot a
    factor 1e4 below the floor: without the floor it would be live);  zero: column 5
    is zero;  allzero: Y_f = 0."""
    rng = np.random.default_rng(100000 + 97 * n + q)
    Q = _orth(rng, n, q)
    Yf = rng.standard_normal((n, 16)) * np.linspace(1.0, 0.3, 16)
    live = np.ones(16, dtype=bool)
    if kind == "dup":
        Yf[:, 9] = Yf[:, 2]; live[9] = False
    elif kind == "near":
        Yf[:, 9] = Yf[:, 2] + 8e-8 * rng.standard_normal(n); live[9] = False
    elif kind == "zero":
        Yf[:, 5] = 0.0; live[5] = False
    elif kind == "allzero":
        Yf[:] = 0.0; live[:] = False
    else:
        assert kind == "plain"
    Pf = Q.T @ Yf
    return Q, Yf, Pf, live


def project_pivots(kind, n, q):
    """the model's pivots relative to the floor 1e-10 max diag (the condition: none within a factor 1e4 of 1)"""
    Q, Yf, Pf, live = project_inputs(kind, n, q)
    Z1, _, G, _, _ = M.project(Q, Yf, Pf)
    A = G.copy()
    mx = float(np.max(np.diag(A)))
    ratios = []
    for j in range(16):
        piv = A[j, j]
        ratios.append(piv / (M.PIVOT_FLOOR * mx) if mx > 0.0 else 0.0)
        if piv > M.PIVOT_FLOOR * mx and piv > 0.0:
            col = A[:, j] / np.sqrt(piv)
            A[j + 1:, j + 1:] -= np.outer(col[j + 1:], col[j + 1:])
    return np.array(ratios), live


# ---- Z / ZAPPLY -----------------------------------------------------------------------------------------------------------------------
Z_N = (33, 96, 97, 371, 385, 1024)
ZAPPLY_N = (97, 256, 257, 4112)


@functools.lru_cache(maxsize=None)
def z_inputs(n, with_res=True):
    rng = np.random.default_rng(200000 + n)
    Z1 = rng.standard_normal((n, 16)) * np.logspace(0, -3, 16)
    Cw = np.triu(rng.standard_normal((16, 16)))
    Cw[7, :] = 0.0; Cw[:, 7] = 0.0                      # a dead pivot
    Res = None
    if with_res:
        Res = rng.standard_normal((n, n)) / np.sqrt(n)
        Res = 0.5 * (Res + Res.T)
    return Z1, Cw, Res


# ---- SMALL --------------------------------------------------------------------------------------------------------------------------------
SMALL_QM = ((16, 32), (17, 33), (32, 48), (33, 49), (48, 64), (49, 65), (64, 80), (16, 16), (64, 64))
AT, FRAC, BF = 1e-4, 0.5, 0.4          # tolc = 5e-5, budget = 1e-9


def small_tols(branch, nparts=64):
    """keyword arguments for the two branches of the tolerance: an absolute one, or reltol ||rhs||_F from the partial sums (both give at = AT)"""
    if branch == "abs":
        return dict(parts=None, abstol=AT, reltol=0.0, frac=FRAC, budget_frac=BF)
    rng = np.random.default_rng(7)
    parts = rng.random(nparts) + 0.5
    return dict(parts=parts, abstol=-1.0, reltol=AT / float(np.sqrt(np.sum(parts))), frac=FRAC, budget_frac=BF)


@functools.lru_cache(maxsize=None)
def small_inputs(q, m, family="full", nkeep=11, na0=0, dead=-1, kappa_s=2.5, decouple=-1):
    """(Cc, info).  G = [I, G12; G12', G22] with ||G12||_2 = 0.2 and S = G22 - G12'G12 of condition kappa_s;  M = U diag(lam) U' with nkeep eigenvalues
    between 1 and 0.01 (alternating signs) and the others of one magnitude, their squares adding up to budget / 120;  H = L M L'.
    family full: U a random orthogonal matrix (every coordinate active);  block: U mixes na0 coordinates only (the others are deflated: na = na0).
    dead = d: fresh direction d is a zero column of Z;  decouple = d: the same problem with that direction live, of unit norm and coupled to nothing."""
    rng = np.random.default_rng(300000 + 101 * q + m + 7 * nkeep + na0)
    nf = m - q
    budget = BF * (FRAC * AT) ** 2
    lam = np.empty(m)
    lam[:nkeep] = np.logspace(0, -2, nkeep) * np.where(np.arange(nkeep) % 2, -1.0, 1.0)
    lam[nkeep:] = np.sqrt(budget / (120.0 * (m - nkeep))) * np.where(np.arange(m - nkeep) % 2, -1.0, 1.0)
    d = dead if dead >= 0 else decouple
    if family == "full":
        U = _orth(rng, m, m)
        perm = np.arange(m)
    else:
        assert nkeep <= na0 <= m
        U = np.eye(m)
        U[:na0, :na0] = _orth(rng, na0, na0)
        perm = rng.permutation(m)
    if d >= 0:
        # the direction is decoupled: coordinate q + d carries one of the small eigenvalues... of value exactly zero (its row of H is zero)
        keep = np.array([i for i in range(m) if i != q + d])
        Ur = _orth(rng, m - 1, m - 1) if family == "full" else np.eye(m - 1)
        Mm = np.zeros((m, m))
        Mm[np.ix_(keep, keep)] = (Ur * lam[:m - 1]) @ Ur.T
        lam = np.append(lam[:m - 1], 0.0)
    else:
        Up = np.zeros((m, m)); Up[perm] = U
        Mm = (Up * lam) @ Up.T
    Mm = 0.5 * (Mm + Mm.T)
    if nf:
        G12 = rng.standard_normal((q, nf))
        G12 *= 0.2 / np.linalg.norm(G12, 2)
        V = _orth(rng, nf, nf)
        S = (V * np.geomspace(1.5 / kappa_s, 1.5, nf)) @ V.T if kappa_s < 100 else (V * np.geomspace(1.0 / kappa_s, 1.0, nf)) @ V.T
        S = 0.5 * (S + S.T)
        if d >= 0:
            G12[:, d] = 0.0
            S[d, :] = 0.0; S[:, d] = 0.0; S[d, d] = 1.0
        G22 = S + G12.T @ G12
        G22 = 0.5 * (G22 + G22.T)
        LT, S2, _ = M.whiten(G12, G22, q)
    else:
        G12, G22, LT = np.zeros((q, 0)), np.zeros((0, 0)), np.eye(q)
    Linv_T = np.linalg.inv(LT)            # H = L M L' with L' = LT^-1
    H = Linv_T.T @ Mm @ Linv_T
    H = 0.5 * (H + H.T)
    K = rng.standard_normal((m, m)) * 1e-3
    Hraw = H + (K - K.T)                  # the kernel symmetrises: the antisymmetric part must not show
    P = rng.standard_normal((m, 16))
    Cc = np.full((m, 64 + q), np.nan)     # (columns 16 .. 32, B'Y_f, are never read: NaN there must not show either)
    Cc[:, :16] = P
    Cc[:, 32:32 + q] = Hraw[:, :q]
    if nf:                                # (m = q: the blocks of Z and W_2 are never read either)
        Cc[:, 32 + q:48 + q] = np.vstack([G12, G22])
        Cc[:, 48 + q:64 + q] = Hraw[:, q:]
    if d >= 0:
        Cc[q + d, :16] = 0.0
        Hz = Hraw.copy(); Hz[q + d, :] = 0.0; Hz[:, q + d] = 0.0
        Cc[:, 32:32 + q] = Hz[:, :q]; Cc[:, 48 + q:64 + q] = Hz[:, q:]
        if dead >= 0:
            Cc[q + d, 32 + q:48 + q] = 0.0; Cc[:, 32 + q + d] = 0.0      # a zero column of Z: its row and column of B'Z vanish
    return Cc, dict(lam=lam, nkeep=nkeep, budget=budget, na0=na0 if family == "block" else m)


def small_gap(q, m, **kw):
    """(smallest kept |lambda| / sqrt(budget), squared sum of the others / budget) of the model's M for the inputs: the condition is >= 100 and <= 0.01"""
    Cc, info = small_inputs(q, m, **kw)
    r = M.small(Cc, q, m, None, 0.0, AT, FRAC, BF)
    a = np.abs(r["lam"])
    k = info["nkeep"]
    return a[k - 1] / np.sqrt(r["budget"]), float(np.sum(a[k:] ** 2)) / r["budget"], r


# ---- EIG ----------------------------------------------------------------------------------------------------------------------------------
EIG_CASES = tuple((m, z, "near") for m in (16, 17, 63, 64, 65, 80) for z in (0, 3)) + ((64, 0, "dense"), (80, 3, "dense"))
# cases whose model Jacobi iteration needs more than 6 sweeps: exempt from the off-diagonal bound only (at most one case in six)
EIG_SLOW = ((64, 0, "dense"), (80, 3, "dense"))


@functools.lru_cache(maxsize=None)
def eig_input(m, nzero, kind="near"):
    """a symmetric matrix with a geometric spectrum 1 .. 1e-6 of alternating signs, the eigenvalues in RANDOM order along the coordinates (the kernel's
    ordering by decreasing |eigenvalue| has work to do);  near: in a basis close to the coordinates (the Q factor of I + 0.001 N: the model's iteration
    converges within six sweeps),  dense: in a random orthogonal basis (more sweeps than the off-diagonal assertion allows for);  nzero rows and columns
    are exactly zero"""
    rng = np.random.default_rng(400000 + 10 * m + nzero + (0 if kind == "near" else 5))
    k = m - nzero
    U = np.linalg.qr(np.eye(k) + 0.001 * rng.standard_normal((k, k)))[0] if kind == "near" else _orth(rng, k, k)
    lam = (np.logspace(0, -6, k) * np.where(np.arange(k) % 2, -1.0, 1.0))[rng.permutation(k)]
    A = (U * lam) @ U.T
    A = 0.5 * (A + A.T)
    S = np.zeros((m, m))
    idx = np.sort(rng.permutation(m)[:k])
    S[np.ix_(idx, idx)] = A
    return S


# ---- FINISH -------------------------------------------------------------------------------------------------------------------------------
FINISH_CASES = ((96, 32, 16), (97, 33, 20), (97, 33, 27), (97, 33, 16), (97, 33, 64), (371, 80, 64), (371, 32, 27), (4112, 80, 64), (4112, 33, 20), (96, 80, 64),
                (97, 80, 64))
FINISH_TOLC = 1e-5


@functools.lru_cache(maxsize=None)
def finish_inputs(n, q, kl, side="accept"):
    """(B, Wk, Yp, Pp, tols_in).  Y_p = B P_p + noise with 2 est^2 + d2 a factor 4 below (accept) or above (reject) tolc^2; d2 is a quarter of the total."""
    rng = np.random.default_rng(500000 + 31 * n + 7 * q + kl)
    B = rng.standard_normal((n, q)) / np.sqrt(n)
    Wk = rng.standard_normal((q, kl))
    Pp = rng.standard_normal((q, 16))
    total = FINISH_TOLC ** 2 * (0.25 if side == "accept" else 4.0)
    d2 = 0.25 * total
    est2 = 0.5 * (total - d2)
    E = rng.standard_normal((n, 16))
    E *= np.sqrt(16.0 * est2) / np.linalg.norm(E)
    Yp = B @ Pp + E
    tols = np.full(12, np.nan)
    tols[1], tols[5], tols[7] = FINISH_TOLC, 0.0, d2
    return B, Wk, Yp, Pp, tols


# ---- CHAIN --------------------------------------------------------------------------------------------------------------------------------
CHAIN_CASES = tuple((n, qb) for n in (96, 371) for qb in (16, 32, 64))
CHAIN_AT = 1e-5


@functools.lru_cache(maxsize=None)
def chain_inputs(n, qb, r):
    """(Res, basis (n x (32 + qb)), kl, qn, info).  Res = V diag(lam) V' + 1e-14 noise with kd dominant eigenvalues (1 .. 0.05, alternating signs) and a tail
    of 1e-9 and below;  Q = the eigenvectors of all but r of the dominant directions (the r missing ones are spread over the dominant range) and of the
    leading tail directions.  r = 3: the 16 fresh directions catch what is missing;  r = 24: they cannot."""
    rng = np.random.default_rng(600000 + 10 * n + qb + r)
    kd = min(qb, 12) if r == 3 else 30
    V = _orth(rng, n, n)
    lam = np.empty(n)
    lam[:kd] = np.geomspace(1.0, 0.05, kd) * np.where(np.arange(kd) % 2, -1.0, 1.0)
    lam[kd:] = 1e-9 * np.geomspace(1.0, 1e-3, n - kd) * np.where(np.arange(n - kd) % 2, -1.0, 1.0)
    Res = (V * lam) @ V.T
    N = rng.standard_normal((n, n)) * 1e-14
    Res = 0.5 * (Res + Res.T) + 0.5 * (N + N.T)
    missing = np.round(np.linspace(0, kd - 1, r)).astype(int)
    have = [i for i in range(kd) if i not in set(missing)][:qb]
    cols = have + list(range(kd, kd + qb - len(have)))
    Q = V[:, cols]
    Om = rng.standard_normal((n, 32))
    kl = min(qb, 16)
    qn = min(qb + 16, 64, kl + 16)
    return Res, np.hstack([Om, Q]), kl, qn, dict(lam=lam, kd=kd, have=len(have), missing=missing)
