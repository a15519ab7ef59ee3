"""NumPy model of the device's Householder + QL eigensolver (csrc/qr_band.hip: k_tridiag, k_tql / host_tql_log + k_tql_replay, k_backtransform),
stage by stage and in the same order of operations, plus the inputs and the error measures of tests/test_gpu_sym_ql.py.

    tridiag        Householder tridiagonalisation of the full symmetric matrix, one column at a time, that stops at the first j with
                   ||S22||_F^2 + 2 e_(j-1)^2 <= tol^2 (S22 the trailing block not yet reduced).  tol = tolfac eps ||S||_F; abs_tol > 0 replaces
                   it (floor_mode 0) or is its lower limit (floor_mode 1).  A column that is already reduced gets tau = 0 and no update.
    ql             implicit QL with Wilkinson shift on T_j: an off-diagonal entry counts as zero at eps (|d_m| + |d_m+1|) or at
                   deflate eps ||S||_F; at most 80 iterations per eigenvalue; a sweep ends early where f^2 + g^2 == 0.
                   ASYMMETRY mirrored from the device: for j <= 128 (k_tql<true>) the second constant is 1e-3 whatever `deflate` says.
    backtransform  B = H_0 ... H_(nref-1) [Z(:, ids); 0], reflector by reflector, tau == 0 skipped.

The model is the yardstick of the device tests: each of their error measures is bounded by MARGIN times the model's own value for the same
input (tests/golden/sym_ql_model.json, written by tests/golden/make_fixtures_sym_ql.py; tests/test_sym_ql_host.py repeats the cheap cases)."""
import json
import math
import os

import numpy as np

import _block_jacobi_model as bm

EPS = np.finfo(float).eps
MARGIN = 10.0
LDS_QL_MAX = 128          # k_tql<true>: Z in LDS
REPLAY_MAX = 2048         # host generator + k_tql_replay up to here, k_tql<false> above
LONGDOUBLE_MAX = 600      # the orthogonal factor is formed in np.longdouble up to this order


class NotConverged(RuntimeError):
    pass


def slab_rows(j):
    """row slab of k_tql_replay: the largest of 64, 32, 16, 8 (4) whose rows x j doubles fit 150 KiB of LDS"""
    rows = 64
    while rows > 4 and rows * j * 8 > 150 * 1024:
        rows >>= 1
    return rows


def stop_tol(snorm, tolfac=4.0, abs_tol=-1.0, floor_mode=0):
    if floor_mode:
        return max(tolfac * EPS * snorm, abs_tol)
    return abs_tol if abs_tol > 0.0 else tolfac * EPS * snorm


def tridiag(S, tolfac=4.0, abs_tol=-1.0, floor_mode=0, want_v=True, trace=None, max_steps=None):
    """dict(jdim, nref, snorm, tol, d (jdim), e (jdim - 1), e_full, tau (q), V (q x q) or None); trace (a list) receives the two terms
    (||S22||_F^2, e_(j-1)) of the stop rule at every j; max_steps ends the loop early (for the trace alone)"""
    S = np.array(S, dtype=float, order="F")
    q = S.shape[0]
    d, e, tau = np.zeros(q), np.zeros(q), np.zeros(q)
    V = np.zeros((q, q), order="F") if want_v else None
    rem2 = float(np.sum(S * S))
    snorm = np.sqrt(rem2)
    tol = stop_tol(snorm, tolfac, abs_tol, floor_mode)
    tol2 = tol * tol
    jdim, nref, eprev = q, 0, 0.0
    for j in range(q):
        if trace is not None:
            trace.append((rem2, eprev))
        if rem2 + 2.0 * eprev * eprev <= tol2 or (max_steps is not None and j >= max_steps):
            jdim = j
            break
        if j == q - 1:
            d[j] = S[j, j]
            break
        x = S[j + 1:, j]
        xs = float(np.sum(x[1:] * x[1:]))
        alpha = float(x[0])
        t, beta, scale = 0.0, alpha, 0.0
        if xs > 0.0:
            nrm = np.sqrt(alpha * alpha + xs)
            beta = -nrm if alpha >= 0.0 else nrm
            t = (beta - alpha) / beta
            scale = 1.0 / (alpha - beta)
        d[j], e[j], tau[j] = S[j, j], beta, t
        v = x * scale
        v[0] = 1.0
        if want_v:
            V[j + 1:, j] = v
        nref, eprev = j + 1, beta
        S22 = S[j + 1:, j + 1:]
        if t != 0.0:
            w = t * (S22 @ v)
            w += (-0.5 * t * float(w @ v)) * v
            S22 -= np.outer(v, w)
            S22 -= np.outer(w, v)
        rem2 = float(np.sum(S22 * S22))
    return dict(jdim=jdim, nref=nref, snorm=snorm, tol=tol, d=d[:jdim].copy(), e=e[:max(jdim - 1, 0)].copy(), e_full=e, tau=tau, V=V)


def ql(d, e, anorm, deflate=1e-3, want_z=True):
    """(w unsorted, Z or None, sweeps [(m, ilo)]) of tridiag(d, e); e has len(d) - 1 entries.  Mirrors host_tql_log / k_tql."""
    n = len(d)
    d = [float(x) for x in d]
    e = [float(x) for x in e[:max(n - 1, 0)]] + [0.0]
    if n <= LDS_QL_MAX:
        deflate = 1e-3          # (k_tql<true> has the constant built in)
    abstiny = deflate * EPS * anorm
    Zt = np.eye(n) if want_z else None          # Zt[i] = column i of Z
    sweeps = []
    sqrt = math.sqrt
    l = it = 0
    while l < n:
        m = l
        while m < n - 1:
            em = abs(e[m])
            if em <= EPS * (abs(d[m]) + abs(d[m + 1])) or em <= abstiny:
                break
            m += 1
        if m == l:
            l += 1
            it = 0
            continue
        if it >= 80:
            raise NotConverged(f"eigenvalue {l}")
        it += 1
        dl, el = d[l], e[l]
        g = (d[l + 1] - dl) / (2.0 * el)
        r = sqrt(g * g + 1.0)
        g = d[m] - dl + el / (g + (r if g >= 0.0 else -r))
        s = c = 1.0
        p = 0.0
        rots = []
        broke = False
        i = m - 1
        while i >= l:
            f, b = s * e[i], c * e[i]
            h = f * f + g * g
            if h == 0.0:
                e[i + 1] = 0.0
                d[i + 1] -= p
                e[m] = 0.0
                broke = True
                break
            rr = sqrt(h)
            e[i + 1] = rr
            s, c = f / rr, g / rr
            g = d[i + 1] - p
            r = (d[i] - g) * s + 2.0 * c * b
            p = s * r
            d[i + 1] = g + p
            g = c * r - b
            rots.append((c, s))
            i -= 1
        ilo = l
        if broke:
            ilo = i + 1
        else:
            d[l] -= p
            e[l] = g
            e[m] = 0.0
        if m - 1 >= ilo:
            sweeps.append((m, ilo))
            if want_z:
                zi1 = Zt[m].copy()
                for k, (c, s) in enumerate(rots):
                    i = m - 1 - k
                    zi = Zt[i]
                    Zt[i + 1] = s * zi + c * zi1
                    zi1 = c * zi - s * zi1
                Zt[ilo] = zi1
    return np.array(d), (np.ascontiguousarray(Zt.T) if want_z else None), sweeps


def sweep_stats(sweeps):
    """what the read-ahead of k_tql_replay depends on: sweep lengths (rotations per sweep) by residue mod 16"""
    lens = [m - ilo for m, ilo in sweeps]
    return dict(nsweeps=len(lens), nrot=int(sum(lens)), residues=sorted({x % 16 for x in lens}), below8=int(sum(1 for x in lens if x < 8)),
                from9to15=int(sum(1 for x in lens if 9 <= x <= 15)), longest=int(max(lens, default=0)))


def form_q(V, tau, nref, j, dtype=float):
    """Q_j = H_0 ... H_(nref-1) [I_j; 0]  (q x j), reflector by reflector in `dtype`"""
    q = V.shape[0]
    B = np.zeros((q, j), dtype=dtype)
    B[:j, :j] = np.eye(j, dtype=dtype)
    for i in range(min(nref, j - 1) - 1, -1, -1):          # (a reflector i >= j - 1 leaves the first j unit vectors alone)
        if tau[i] == 0.0:
            continue
        v = V[i + 1:, i].astype(dtype)
        sub = B[i + 1:, i + 1:]          # (the columns before i + 1 are still unit vectors with zeros from row i + 1 on)
        sub -= np.outer(dtype(tau[i]) * v, v @ sub)
    return B


def form_q_lapack(V, tau, nref, j):
    """the same in float64 through LAPACK's blocked dorgqr (orders above LONGDOUBLE_MAX)"""
    from scipy.linalg import lapack
    q = V.shape[0]
    Q = np.zeros((q, j))
    if j == 0:
        return Q
    Q[0, 0] = 1.0
    n = max(min(nref, q - 1), j - 1)
    if n > 0:
        a = np.asfortranarray(V[1:, :n])
        qq, _, info = lapack.dorgqr(a, np.ascontiguousarray(tau[:n]), lwork=64 * n)
        assert info == 0
        Q[1:, 1:j] = qq[:, :j - 1]
    return Q


def orthogonal_factor(V, tau, nref, j):
    q = V.shape[0]
    return form_q(V, tau, nref, j, np.longdouble) if q <= LONGDOUBLE_MAX else form_q_lapack(V, tau, nref, j)


def tri_dense(d, e, dtype=float):
    T = np.diag(np.asarray(d, dtype=dtype))
    k = len(d) - 1
    if k > 0:
        idx = np.arange(k)
        T[idx + 1, idx] = T[idx, idx + 1] = np.asarray(e[:k], dtype=dtype)
    return T


def stage_a(S, Q, d, e):
    """(a1, a2, a3) = (||Q'SQ - T||_F / ||S||_F, ||Q'Q - I||_F, ||S - Q T Q'||_F / ||S||_F) in the precision of Q"""
    j = Q.shape[1]
    nf = max(float(np.linalg.norm(S)), np.finfo(float).tiny)
    if j == 0:
        return 0.0, 0.0, float(np.linalg.norm(S)) / nf
    dt = Q.dtype.type
    Sx = np.asarray(S).astype(dt)
    T = tri_dense(d, e, dt)
    SQ = Sx @ Q
    a1 = float(np.linalg.norm((Q.T @ SQ - T).astype(float))) / nf
    a2 = float(np.linalg.norm((Q.T @ Q - np.eye(j, dtype=dt)).astype(float)))
    a3 = float(np.linalg.norm((Sx - (Q @ T) @ Q.T).astype(float))) / nf
    return a1, a2, a3


def stage_b(d, e, w, Z):
    """(b1, b2, b3) = (max |w - w_ref| / ||T||_2, ||T Z - Z diag(w)||_F / ||T||_F, ||Z'Z - I||_F), w_ref from scipy's eigh_tridiagonal"""
    from scipy.linalg import eigh_tridiagonal
    n = len(d)
    ref = eigh_tridiagonal(np.asarray(d, float), np.asarray(e[:n - 1], float), eigvals_only=True) if n > 1 else np.asarray(d, float)
    n2 = max(float(np.abs(ref).max()), np.finfo(float).tiny)
    ee = np.asarray(e[:n - 1], float)
    TZ = Z * np.asarray(d, float)[:, None]
    if n > 1:
        TZ[:-1] += ee[:, None] * Z[1:]
        TZ[1:] += ee[:, None] * Z[:-1]
    nf = max(float(np.sqrt(np.sum(np.square(d)) + 2.0 * np.sum(ee * ee))), np.finfo(float).tiny)
    return (float(np.abs(np.sort(w) - ref).max() / n2), float(np.linalg.norm(TZ - Z * w)) / nf, float(np.linalg.norm(Z.T @ Z - np.eye(n))))


def backtransform(V, tau, nref, Zsel):
    """B = H_0 ... H_(nref-1) [Zsel; 0] in float64, reflector by reflector (the order of k_backtransform)"""
    q = V.shape[0]
    B = np.zeros((q, Zsel.shape[1]))
    B[:Zsel.shape[0]] = Zsel
    for i in range(nref - 1, -1, -1):
        if tau[i] == 0.0:
            continue
        v = V[i + 1:, i]
        B[i + 1:] -= np.outer(tau[i] * v, v @ B[i + 1:])
    return B


def stage_c(B, Q, Zsel):
    """||B - Q_j Zsel||_F against the product in the precision of Q"""
    return float(np.linalg.norm((B.astype(Q.dtype) - Q @ Zsel.astype(Q.dtype)).astype(float)))


def end_to_end(S, w, U):
    """j = q: the three measures of _block_jacobi_model.errors; j < q: (||U diag(w) U' - S||_F / ||S||_F, residual, orthogonality)"""
    q, j = S.shape[0], len(w)
    if j == q:
        return bm.errors(S, w, U)
    nf = max(float(np.linalg.norm(S)), np.finfo(float).tiny)
    return (float(np.linalg.norm((U * w) @ U.T - S)) / nf, float(np.linalg.norm(S @ U - U * w)) / nf, float(np.linalg.norm(U.T @ U - np.eye(j))))


def solve(S, tolfac=4.0, abs_tol=-1.0, floor_mode=0, deflate=1e-3):
    """the whole chain: dict of tridiag's entries plus w, Z (unsorted), sweeps"""
    t = tridiag(S, tolfac, abs_tol, floor_mode)
    if t["jdim"] > 0:
        t["w"], t["Z"], t["sweeps"] = ql(t["d"], t["e"], t["snorm"], deflate)
    else:
        t["w"], t["Z"], t["sweeps"] = np.zeros(0), np.zeros((0, 0)), []
    return t


def measure(S, r):
    """every figure of the record for a run r = solve(S, ...)"""
    q, j = S.shape[0], r["jdim"]
    Q = orthogonal_factor(r["V"], r["tau"], r["nref"], j)
    a1, a2, a3 = stage_a(S, Q, r["d"], r["e"])
    out = dict(order=q, jdim=j, nref=r["nref"], tau0=int(np.sum(r["tau"][:r["nref"]] == 0.0)), a1=a1, a2=a2, a3=a3)
    out.update(sweep_stats(r["sweeps"]))
    if j > 0:
        b1, b2, b3 = stage_b(r["d"], r["e"], r["w"], r["Z"])
        B = backtransform(r["V"], r["tau"], r["nref"], r["Z"])
        order = np.argsort(r["w"], kind="stable")
        e1, e2, e3 = end_to_end(S, r["w"][order], B[:, order])
        out.update(b1=b1, b2=b2, b3=b3, c=stage_c(B, Q, r["Z"]), eig_err=e1, residual=e2, orth=e3)
    else:
        out.update(b1=0.0, b2=0.0, b3=0.0, c=0.0, eig_err=0.0, residual=0.0, orth=0.0)
    return out


# ---- the matrices of the tests (fixed seeds) ---------------------------------------------------------------------------------------
QL_ORDERS = (1, 2, 3, 63, 65, 127, 128, 129, 300, 301, 600, 601, 1200, 1201, 2048)
HARD_ORDERS = (64, 160)


def dense(q, seed=0):
    A = np.random.default_rng(4000 + q + seed).standard_normal((q, q))
    return A + A.T


def spectrum(q):
    """from_spectrum with eigenvalues of both signs, none near zero: the reduction never stops early"""
    rng = np.random.default_rng(5000 + q)
    lam = rng.uniform(0.2, 1.0, q) * np.where(rng.uniform(size=q) < 0.5, -1.0, 1.0)
    return bm.from_spectrum(lam, 6000 + q)


def block_tridiagonal(q, straddle):
    """random tridiagonal blocks of order 1 to 40, non-zero diagonal; one block lies across the indices straddle - 1 / straddle, one at each end"""
    rng = np.random.default_rng(7000 + q)
    sizes, pos = [], 0
    while pos < q:
        b = int(rng.integers(1, 41))
        if pos + b == straddle:          # no block boundary there: one block holds both straddle - 1 and straddle
            b = b + 1 if b < 40 else b - 1
        b = min(b, q - pos)
        sizes.append(b)
        pos += b
    d = rng.uniform(0.5, 1.5, q) * np.where(rng.uniform(size=q) < 0.5, -1.0, 1.0)
    e = rng.standard_normal(q - 1)
    ends = np.cumsum(sizes)[:-1]
    e[ends - 1] = 0.0
    assert not (ends == straddle).any() and sizes[0] >= 1 and sizes[-1] >= 1
    return tri_dense(d, e), sizes


def low_rank_spectrum(r):
    return 0.5 ** np.arange(r) * np.where(np.arange(r) % 3 == 1, -1.0, 1.0)


LOW_RANK_SEED = {3841: 2}          # (chosen so that the model's jdim window is at most 10 wide: tests/test_sym_ql_host.py)


def low_rank(q, r, seed=None):
    """B Lambda B' with orthonormal B (q x r), |lambda_k| = 0.5^k, mixed signs: (S, lambda)"""
    rng = np.random.default_rng(8000 + q + r + (LOW_RANK_SEED.get(q, 0) if seed is None else seed))
    Bq = np.linalg.qr(rng.standard_normal((q, r)))[0]
    lam = low_rank_spectrum(r)
    S = (Bq * lam) @ Bq.T
    return 0.5 * (S + S.T), lam


def repeated4(q):
    return bm.from_spectrum(np.repeat([-2.0, -0.5, 1.0, 3.0], q // 4), 21 + q)


def cluster(q):
    return bm.from_spectrum(1.0 + 1e-13 * np.arange(q), 22 + q)


def graded_alt(q):
    return bm.from_spectrum(10.0 ** (-np.arange(q) / 10.0) * np.where(np.arange(q) % 2 == 0, 1.0, -1.0), 23 + q)


def wilkinson(q):
    m = (q - 1) / 2.0
    return tri_dense(np.abs(np.arange(q) - m), np.ones(q - 1))


def diagonal(q):
    return np.diag(np.random.default_rng(24 + q).standard_normal(q))


def rank3(q):
    G = np.random.default_rng(10).standard_normal((q, 3))
    return (G * np.array([2.0, -1.0, 0.5])) @ G.T


def padded(q=9, k=5):
    S = np.zeros((q, q))
    S[:k, :k] = dense(k)
    return S


HARD = dict(repeated4=repeated4, cluster=cluster, graded_alt=graded_alt, wilkinson=wilkinson, diagonal=diagonal,
            plus_minus_pairs=lambda q: bm.plus_minus_pairs(q), rank3=rank3)
BLOCKTRI = {2049: 2048, 2600: 2048}          # order -> the index its straddling block crosses (the QL switch lies at 2048)
LOW_RANK = ((3840, 12), (3841, 12), (8192, 12), (1000, 20))


def stop_edge_tol(S, j=10):
    tr = []
    tridiag(S, want_v=False, trace=tr, max_steps=j)
    rem2, eprev = tr[j]
    return math.sqrt(rem2 + 1.5 * eprev * eprev)


def cases():
    """name -> (builder of S, keyword arguments of the solver; abs_tol_rel is relative to ||S||_F).  Built on demand: some inputs are large."""
    out = {}
    for q in QL_ORDERS:
        out[f"dense{q}"] = (lambda q=q: dense(q), {})
        out[f"spectrum{q}"] = (lambda q=q: spectrum(q), {})
    for q, at in BLOCKTRI.items():
        out[f"blocktri{q}"] = (lambda q=q, at=at: block_tridiagonal(q, at)[0], {})
    for q, r in LOW_RANK:
        out[f"lowrank{q}_r{r}"] = (lambda q=q, r=r: low_rank(q, r)[0], {})
    lr = lambda: low_rank(1000, 20)[0]
    out["abs_tol"] = (lr, dict(abs_tol_rel=1e-6, floor_mode=0))
    out["floor_wins"] = (lr, dict(abs_tol_rel=1e-6, floor_mode=1))
    out["floor_loses"] = (lr, dict(abs_tol_rel=1e-18, floor_mode=1))
    # (1e-6 ||S|| lies next to |lambda_20| = 1.9e-6: it moves jdim by a column at most.  1e-3 ||S|| cuts ten columns off: a run that took the
    # wrong one of the three forms cannot pass for the right one)
    out["abs_tol_coarse"] = (lr, dict(abs_tol_rel=1e-3, floor_mode=0))
    out["floor_coarse"] = (lr, dict(abs_tol_rel=1e-3, floor_mode=1))
    # the factor 2 of the stop rule: tol^2 between ||S22||^2 + e^2 and ||S22||^2 + 2 e^2 at j = 10 (the model's own two terms there; half
    # of e^2 to either side, 5 % of tol^2 and far above any rounding), and the same by hand at order 2: 2 * 0.8^2 > 1 > 0.8^2
    out["stop_edge"] = (lr, dict(abs_tol_fn=stop_edge_tol))
    out["stop_edge2"] = (lambda: np.array([[1.0, 0.8], [0.8, 0.0]]), dict(abs_tol=1.0))
    out["zero1"] = (lambda: np.zeros((1, 1)), {})
    out["zero6"] = (lambda: np.zeros((6, 6)), {})
    out["padded9"] = (padded, {})
    for q in HARD_ORDERS:
        for name, f in HARD.items():
            out[f"{name}{q}"] = (lambda q=q, f=f: f(q), {})
    for q in (100, 160):
        out[f"dense{q}_deflate1"] = (lambda q=q: dense(q), dict(deflate=1.0))
        out[f"dense{q}_deflate1e-3"] = (lambda q=q: dense(q), dict(deflate=1e-3))
    return out


def cases_order(name):
    """the order of a named case's matrix (from the name; the stop-rule cases share the order-1000 input)"""
    import re
    m = re.search(r"[0-9]+", name)
    return int(m.group()) if m else 1000


def solver_args(S, kw):
    kw = dict(kw)
    rel, fn = kw.pop("abs_tol_rel", None), kw.pop("abs_tol_fn", None)
    if rel is not None:
        kw["abs_tol"] = rel * float(np.linalg.norm(S))
    if fn is not None:
        kw["abs_tol"] = fn(S)
    return kw


def run_case(name):
    """the model's figures for a named case (what the record holds)"""
    build, kw = cases()[name]
    S = build()
    args = solver_args(S, kw)
    out = measure(S, solve(S, **args))
    if name.startswith(("lowrank", "abs_tol", "floor_", "stop_edge")):
        tf = args.get("tolfac", 4.0)
        rest = {k: v for k, v in args.items() if k != "tolfac"}
        out["jdim_loose"] = tridiag(S, 4.0 * tf, want_v=False, **rest)["jdim"]
        out["jdim_tight"] = tridiag(S, tf / 4.0, want_v=False, **rest)["jdim"]
    return out


def window_width_max(name):
    """widest allowed jdim window [jdim at 4 tolfac, jdim at tolfac / 4]: 10 columns; the graded spectrum 10^(-k/10) loses one decade per ten
    columns, so the factor 16 between the two tolerances is 10 log10(16) = 12.04 columns by construction: 13"""
    return 13 if name.startswith("graded_alt") else 10


HOST_MAX_ORDER = 301          # tests/test_sym_ql_host.py repeats the cases up to this order live


def record_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sym_ql_model.json")


def recorded():
    with open(record_path()) as f:
        return json.load(f)
