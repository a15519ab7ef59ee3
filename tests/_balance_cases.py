"""The systems of the balanced-truncation tests (tests/test_svd_balance_host.py, tests/test_gpu_balance.py) with their CPU references, computed
once per process.  E x' = A x + B u, y = C x on the pencils of tests/_sign_dual_cases.py (A is that file's F):
    n = 33, 70   B = G[:, :7], C = default_rng(2000 + n).standard_normal((5, n))
    n = 371      B and C of steel_profile(371, convection=3e-3)
reference(n)   oracle.lyap_dense Gramians, eigh factors (eigenvalues above n eps times the largest kept), numpy.linalg.svd; the matrix
               products in extended precision
chain(n)       the NumPy restatement of the device's path: factored sign models of tests/_sign_dual_model.py, the SVD model and the steps of
               csrc/balance.hip (tests/_svd_jacobi_model.py: balance)
"""
import functools

import numpy as np

import dre_amd as D
import dre_oracle as o
import _sign_dual_cases as cs
import _sign_dual_model as dm
import _factored_sign_model as fm
import _svd_jacobi_model as sv

SIZES = (33, 70, 371)
ORDERS = (4, 8, 12)
OMEGA = np.logspace(-5.0, 3.0, 60)
EPS = np.finfo(float).eps


def rank_rtol(n):
    """eigenvalues of a reference Gramian at or below this times the largest are rounding noise of lyap_dense (n eps, the rule of compress!)"""
    return n * EPS


@functools.lru_cache(maxsize=None)
def system(n):
    """(E, A, B, C)"""
    E, F, G, _ = cs.pencil(n)
    if n >= 371:
        d = D.steel_profile(n, convection=3e-3)
        Bm, Cm = np.array(d.B, dtype=float), np.array(d.C, dtype=float)
    else:
        Bm, Cm = np.array(G[:, :7]), np.random.default_rng(2000 + n).standard_normal((5, n))
    for M in (Bm, Cm):
        M.setflags(write=False)
    return E, F, Bm, Cm


def _eigh_factor(X, rtol):
    lam, V = np.linalg.eigh(X)
    keep = lam > rtol * lam.max()
    return V[:, keep], lam[keep]


def _numpy_svd(M):
    U, s, Vt = np.linalg.svd(M, full_matrices=False)
    return U, s, Vt.T, dict(sweeps=0, rounds=0, rank=int((s > sv.default_tol(*M.shape) * np.linalg.norm(M)).sum()))


@functools.lru_cache(maxsize=None)
def gramians(n):
    """reference factors (Lc, dc, Lo, do): P = Lc diag(dc) Lc' from A P E' + E P A' = -B B', Q = Lo diag(do) Lo' from A'Q E + E'Q A = -C'C"""
    E, A, Bm, Cm = system(n)
    P, Q = o.lyap_dense(A.T, E.T, Bm @ Bm.T), o.lyap_dense(A, E, Cm.T @ Cm)
    return _eigh_factor(P, rank_rtol(n)) + _eigh_factor(Q, rank_rtol(n))


LD = np.longdouble      # the reference's products are accumulated in extended precision (64-bit mantissa where the platform has one)


def _reference_balance(E, A, Bm, Cm, Lc, dc, Lo, do, order, tol):
    """the steps of sv.balance with every matrix product carried in extended precision and rounded to double once, the SVD by LAPACK in
    double: what is left in ||W'ET - I||_F is the SVD's backward error scaled by sigma_1 / sigma_r, not the rounding of the products (in
    double those alone put 7.7e-14 into it at n = 70, r = 12).  W'ET - I is measured on the rounded W and T, in extended precision."""
    Zc, drop_c, neg_c = sv.sqrt_factor(Lc, dc)
    Zo, drop_o, neg_o = sv.sqrt_factor(Lo, do)
    El, Al, Zcl, Zol = (X.astype(LD) for X in (E, A, Zc, Zo))
    M = (Zol.T @ (El @ Zcl)).astype(float)
    U, s, V, st = _numpy_svd(M)
    rank = st["rank"]
    if order > 0:
        if order > rank:
            raise ValueError(f"order {order} above the numerical rank {rank}")
        r = order
    else:
        r = sv.choose_order(s, rank, tol)
    sc = 1.0 / np.sqrt(s[:r].astype(LD))
    Wm, T = ((Zol @ U[:, :r].astype(LD)) * sc).astype(float), ((Zcl @ V[:, :r].astype(LD)) * sc).astype(float)
    Wl, Tl = Wm.astype(LD), T.astype(LD)
    eye = (Wl.T @ (El @ Tl) - np.eye(r)).astype(float)
    return dict(hsv=s, T=T, W=Wm, Ar=(Wl.T @ (Al @ Tl)).astype(float), Br=(Wl.T @ Bm.astype(LD)).astype(float), Cr=(Cm.astype(LD) @ Tl).astype(float),
                order=r, rank=rank, r_c=Zc.shape[1], r_o=Zo.shape[1], dropped=drop_c + drop_o, sweeps=0, eye_err=float(np.linalg.norm(eye)),
                bound=2.0 * float(np.sum(s[r:][::-1])), neg_max=max(neg_c, neg_o), M=M)


@functools.lru_cache(maxsize=None)
def reference(n, order=0, tol=1e-8):
    E, A, Bm, Cm = system(n)
    return _reference_balance(E, A, Bm, Cm, *gramians(n), order, tol)


@functools.lru_cache(maxsize=None)
def model_gramians(n):
    """the factored sign models' (Lc, dc, Lo, do): one kept sequence, the primal replay with C'C and the dual one with B B'"""
    _, _, Bm, Cm = system(n)
    m = cs.model(n)
    Lo, Do, _ = fm.factored_sign_lyap(m, Cm.T, np.eye(Cm.shape[0]))
    Lc, Dc, _ = dm.factored_sign_lyap_t(m, Bm, np.eye(Bm.shape[1]))
    return Lc, np.diag(Dc).copy(), Lo, np.diag(Do).copy()


@functools.lru_cache(maxsize=None)
def chain(n, order=0, tol=1e-8):
    E, A, Bm, Cm = system(n)
    return sv.balance(E, A, Bm, Cm, *model_gramians(n), order=order, tol=tol)


def transfer(E, A, Bm, Cm, omega=OMEGA):
    """H(i omega) = C (i omega E - A)^-1 B at every frequency: (len(omega), outputs, inputs)"""
    return np.array([Cm @ np.linalg.solve(1j * w * E - A, Bm.astype(complex)) for w in omega])


@functools.lru_cache(maxsize=None)
def full_transfer(n):
    H = transfer(*system(n))
    H.setflags(write=False)
    return H


def reduced_transfer(red):
    return transfer(np.eye(red["order"]), red["Ar"], red["Br"], red["Cr"])


def max_norm2(H):
    return float(max(np.linalg.norm(h, 2) for h in H))


def h0_norm(n):
    E, A, Bm, Cm = system(n)
    return float(np.linalg.norm(Cm @ np.linalg.solve(-A, Bm), 2))


def chain_errors(n, order):
    """the NumPy chain against the reference at one order: (max |sigma - sigma_ref| / sigma_1, ||W'ET - I||_F, max_w ||H_r - H_r^ref||_2 / ||H(0)||_2)"""
    ref, ch = reference(n, order), chain(n, order)
    k = min(len(ref["hsv"]), len(ch["hsv"]))
    sig = float(np.abs(ch["hsv"][:k] - ref["hsv"][:k]).max() / ref["hsv"][0])
    return sig, ch["eye_err"], max_norm2(reduced_transfer(ch) - reduced_transfer(ref)) / h0_norm(n)


def tail_ratio(s, r, tol):
    """2 sum_{i > r} sigma_i / (tol sigma_1): the order rule picks the smallest r at which this is <= 1"""
    return 2.0 * float(np.sum(s[r:][::-1])) / (tol * s[0])


TOL_ORDER = 10


def clear_tol(s, r=TOL_ORDER):
    """a tolerance at which the order rule gives r by a clear margin: the geometric mean of the two values of 2 sum tail / sigma_1 around r"""
    return float(np.sqrt(tail_ratio(s, r, 1.0) * tail_ratio(s, r - 1, 1.0)))


def record():
    """the chain's figures for tests/golden/svd_jacobi_model.json: per n the ranks, the SVD's sweeps and chain_errors at order 8 and at the
    order chosen by clear_tol"""
    out = {}
    for n in SIZES:
        ref, ch = reference(n, 8), chain(n, 8)
        tol = clear_tol(ref["hsv"])
        rt = reference(n, 0, tol)["order"]
        assert chain(n, 0, tol)["order"] == rt == TOL_ORDER
        out[str(n)] = dict(ref_r_o=ref["r_o"], ref_r_c=ref["r_c"], r_o=ch["r_o"], r_c=ch["r_c"], rank=ch["rank"], sweeps=ch["sweeps"], tol=tol,
                           tol_order=rt, **{f"{k}_{lab}": v for lab, r in (("order8", 8), ("tol", rt))
                                            for k, v in zip(("sigma", "eye", "transfer"), chain_errors(n, r))})
    return out


# ---- the recorded reference (tests/golden/balance_reference.npz): what the device tests need of reference(n), which takes the CPU half a minute
# at n = 371.  tests/test_svd_balance_host.py compares the record with the live reference.  Regenerate with:  python tests/_svd_jacobi_model.py
def golden_path():
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "balance_reference.npz")


def golden_arrays():
    out = {}
    for n in SIZES:
        ref = reference(n, 8)
        out[f"hsv_{n}"] = ref["hsv"]
        out[f"H_{n}"] = np.array(full_transfer(n))
        out[f"h0_{n}"] = np.array(h0_norm(n))
        for lab, r in (("order8", 8), ("tol", TOL_ORDER)):
            out[f"Hr_{lab}_{n}"] = reduced_transfer(reference(n, r))
    return out


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(golden_path()) as z:
        return {k: z[k] for k in z.files}
