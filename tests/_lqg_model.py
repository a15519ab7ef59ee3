"""Host NumPy model of LQG balanced truncation as the device runs it (csrc/dense_are.hip: dense_gare_solve_pair; csrc/balance.hip: lqg_balance),
on top of tests/_hamiltonian_sign_model.py and tests/_svd_jacobi_model.py, which it imports and leaves as they are.

    regulator   A'XE + E'XA - E'XGXE + Q = 0         G = B B', Q = C'C
    filter      A Y E' + E Y A' - E Y Q Y E' + G = 0

ONE sign iteration of the regulator's Hamiltonian pencil (H, K) gives Z_inf.  The filter's pencil is (H', K'); inversion, the determinantal
scaling and the structured average commute with transposition, so its Z_inf is Z_inf':

    regulator   [Z12; Z22 + E'] Yr = -[Z11 + E; Z21],        X = sym(Yr E^-1)            (hm.extract)
    filter      [Z21'; Z22' + E] Yr = -[Z11' + E'; Z12'],    Y = sym(Yr E^-T)            (extract_t)
    refinement  regulator: hm.gare_sign's loop;  filter: F_f = A - E Y Q,  F_f D E' + E D F_f' = -R_f(Y),  Y <- Y + D  (the dual replay of
                tests/_sign_dual_model.py on the sign model of (F_f, E))

lqg_balance: X = Lo diag(do) Lo', Y = Lc diag(dc) Lc' by eigh, entries that are not positive left out, and the steps of sv.balance with the
order rule  2 sum_{i > r} nu_i <= tol,  nu_i = mu_i / sqrt(1 + mu_i^2);  Kr = Br' Sigma_r, Lr = Sigma_r Cr', Ac = Ar - Br Kr - Lr Cr.

The systems of the tests, their SciPy reference chain and the recorded figures (tests/golden/lqg_model.json, tests/golden/lqg_reference.npz) are
here too.  Regenerate both with:  python tests/_lqg_model.py   (a few minutes: the n = 371 chain runs the NumPy model of the block Jacobi SVD).
"""
import functools
import json
import os

import numpy as np
import scipy.linalg as sla

import _hamiltonian_sign_model as hm
import _sign_dual_model as dm
import _sign_model as sm
import _svd_jacobi_model as sv

EPS = np.finfo(float).eps
GENERATED = {1: (1, 1, 11), 12: (2, 3, 12), 33: (3, 2, 33), 70: (4, 3, 70)}      # n: (m, q, seed)
SIZES = (1, 12, 33, 70, 371)
ORDERS = {1: 1, 12: 6, 33: 8, 70: 12, 371: 16}
OMEGA = np.logspace(-3.0, 3.0, 200)
OMEGA_371 = np.logspace(-3.0, 3.0, 60)          # the recorded reduced transfer function of the n = 371 reference (the record stays small)


# ---- the systems ----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def system(n):
    """(E, A, B, C).  n in GENERATED: nonsymmetric E and A with two unstable poles (one for n = 1), m != q; n = 371: SteelProfile with its five
    rightmost poles moved into the right half plane (test_dense_gare_host.unstable_variant)"""
    if n == 371:
        from test_dense_gare_host import steel_dense, unstable_variant
        E, A, B, C = steel_dense(371)
        out = (E, unstable_variant(E, A), B, C)
    else:
        m, q, seed = GENERATED[n]
        rng = np.random.default_rng(seed)
        E = np.eye(n) + 0.1 * rng.standard_normal((n, n)) / np.sqrt(n)
        A0 = -np.diag(np.linspace(0.5, 20.0, n)) + 0.3 * rng.standard_normal((n, n)) / np.sqrt(n)
        for k in range(min(2, n)):
            A0[k, k] = 0.7 - 0.4 * k
        out = (E, E @ A0, rng.standard_normal((n, m)), rng.standard_normal((q, n)))
    for M in out:
        M.setflags(write=False)
    return out


# ---- the pair solve -------------------------------------------------------------------------------------------------------------------------
def residual_f(E, A, G, Q, Y):
    """R_f(Y) and its scaled norm ||R_f||_F / (||G||_F + 2 ||A Y E'||_F + ||E Y Q Y E'||_F): hm.residual with the transposition flags flipped"""
    YE = Y @ E.T
    AYE = A @ YE
    YQY = YE.T @ (Q @ YE)
    R = hm._sym(G + AYE + AYE.T - YQY)
    den = np.linalg.norm(G) + 2.0 * np.linalg.norm(AYE) + np.linalg.norm(YQY)
    return R, np.linalg.norm(R) / den if den > 0 else np.linalg.norm(R)


def extract_t(Z, E):
    """the filter's solution from the transposed blocks of the regulator's Z_inf"""
    n = E.shape[0]
    Z11, Z12, Z21, Z22 = Z[:n, :n], Z[:n, n:], Z[n:, :n], Z[n:, n:]
    M = np.vstack([Z21.T, Z22.T + E])
    rhs = -np.vstack([Z11.T + E.T, Z12.T])
    Qf, R = np.linalg.qr(M)
    Yr = np.linalg.inv(R) @ (Qf.T @ rhs)
    return hm._sym(Yr @ np.linalg.inv(E).T)


def _refine(n, X, res_fn, step_fn, max_refine):
    R, r = res_fn(X)
    r0, steps = r, 0
    while r > hm.refine_target(n) and steps < max_refine:
        Xn = X + step_fn(X, R)
        Rn, rn = res_fn(Xn)
        steps += 1
        if not rn < r:
            break
        X, R, r = Xn, Rn, rn
    return X, dict(refinements=steps, res0=r0, res=r)


def gare_pair(E, A, B, C, maxiters=50, tol=None, max_refine=2):
    """(X, Y, info): info = dict(iters, regulator = dict(refinements, res0, res), filter = the same)"""
    E, A, B, C = (np.asarray(M, dtype=float) for M in (E, A, B, C))
    n = E.shape[0]
    G, Q = B @ B.T, C.T @ C
    Z, iters, _ = hm.sign_iteration(E, A, G, Q, maxiters, tol)

    def step_x(X, R):
        try:
            return sm.sign_lyap(A - G @ X @ E, E, R, maxiters=maxiters)[0]
        except sm.NotStable as e:
            raise hm.NotStable(f"regulator refinement: the closed loop is not c-stable ({e})")

    def step_y(Y, R):
        try:
            return dm.solve_t(sm.SignModel(A - E @ Y @ Q, E, maxiters), R)[0]
        except sm.NotStable as e:
            raise hm.NotStable(f"filter refinement: the closed loop is not c-stable ({e})")

    Y, iy = _refine(n, extract_t(Z, E), lambda Y_: residual_f(E, A, G, Q, Y_), step_y, max_refine)
    X, ix = _refine(n, hm.extract(Z, E), lambda X_: hm.residual(E, A, G, Q, X_), step_x, max_refine)
    return X, Y, dict(iters=iters, regulator=ix, filter=iy)


# ---- balancing ------------------------------------------------------------------------------------------------------------------------------
def nu(mu):
    mu = np.asarray(mu, dtype=float)
    return mu / np.sqrt(1.0 + mu * mu)


def bound(mu, r):
    """2 sum_{i > r} nu_i, summed from the smallest upward"""
    return 2.0 * float(np.sum(nu(mu)[r:][::-1]))


def choose_order(mu, rank, tol):
    """the smallest r with 2 sum_{i > r} nu_i <= tol (absolute), at most the numerical rank"""
    v = nu(mu)
    r, tail = len(v), 0.0
    while r > 0 and 2.0 * (tail + v[r - 1]) <= tol:
        tail += v[r - 1]
        r -= 1
    return min(r, rank)


def clear_tol(mu, r):
    """a tolerance at which the order rule gives r by a clear margin: the geometric mean of the two bound values around r"""
    return float(np.sqrt(bound(mu, r) * bound(mu, r - 1)))


def eig_factor(S, rtol=None):
    """S = L diag(d) L' by eigh, d ascending; rtol: keep d > rtol max(d) (the reference); None: everything (the device's sqrt_factor drops d <= 0)"""
    d, L = np.linalg.eigh(hm._sym(S))
    if rtol is not None:
        keep = d > rtol * d.max()
        d, L = d[keep], L[:, keep]
    return L, d


def _numpy_svd(M):
    U, s, Vt = np.linalg.svd(M, full_matrices=False)
    return U, s, Vt.T, dict(sweeps=0, rounds=0, rank=int((s > sv.default_tol(*M.shape) * np.linalg.norm(M)).sum()))


def lqg_balance(E, A, B, C, X, Y, order=0, tol=1e-8, svd_fn=None, rtol=None):
    """dict(mu, T, W, Ar, Br, Cr, Kr, Lr, Ac, order, rank, r_c, r_o, dropped, sweeps, eye_err, bound, neg_max)"""
    Lo, do = eig_factor(X, rtol)
    Lc, dc = eig_factor(Y, rtol)
    Zc, drop_c, neg_c = sv.sqrt_factor(Lc, dc)
    Zo, drop_o, neg_o = sv.sqrt_factor(Lo, do)
    M = Zo.T @ (E @ Zc)
    U, s, V, st = (svd_fn or sv.svd)(M)
    rank = st["rank"]
    if order > 0:
        if order > rank:
            raise ValueError(f"order {order} above the numerical rank {rank}")
        r = order
    else:
        r = choose_order(s, rank, tol)
    sc = 1.0 / np.sqrt(s[:r])
    W, T = (Zo @ U[:, :r]) * sc, (Zc @ V[:, :r]) * sc
    Ar, Br, Cr = W.T @ (A @ T), W.T @ B, C @ T
    Sig = np.diag(s[:r])
    Kr, Lr = Br.T @ Sig, Sig @ Cr.T
    return dict(mu=s, T=T, W=W, Ar=Ar, Br=Br, Cr=Cr, Kr=Kr, Lr=Lr, Ac=Ar - Br @ Kr - Lr @ Cr, order=r, rank=rank, r_c=Zc.shape[1], r_o=Zo.shape[1],
                dropped=drop_c + drop_o, sweeps=st["sweeps"], eye_err=float(np.linalg.norm(W.T @ (E @ T) - np.eye(r))), bound=bound(s, r),
                neg_max=max(neg_c, neg_o))


# ---- measures -------------------------------------------------------------------------------------------------------------------------------
def transfer(E, A, B, C, omega):
    return np.array([C @ np.linalg.solve(1j * w * E - A, B.astype(complex)) for w in omega])


def max_norm2(H):
    return float(max(np.linalg.norm(h, 2) for h in H))


def reduced_transfer(red, omega):
    return transfer(np.eye(red["order"]), red["Ar"], red["Br"], red["Cr"], omega)


def riccati_residuals(red):
    """the relative residuals of the two reduced Riccati equations with X_r = Y_r = Sigma_r"""
    r = red["order"]
    S, Ar, Br, Cr = np.diag(red["mu"][:r]), red["Ar"], red["Br"], red["Cr"]
    T1, T2 = Ar.T @ S, Ar @ S
    R1 = T1 + T1.T - S @ Br @ Br.T @ S + Cr.T @ Cr
    R2 = T2 + T2.T - S @ Cr.T @ Cr @ S + Br @ Br.T
    return (float(np.linalg.norm(R1) / (np.linalg.norm(Cr.T @ Cr) + 2 * np.linalg.norm(T1) + np.linalg.norm(S @ Br @ Br.T @ S))),
            float(np.linalg.norm(R2) / (np.linalg.norm(Br @ Br.T) + 2 * np.linalg.norm(T2) + np.linalg.norm(S @ Cr.T @ Cr @ S))))


def coprime_systems(E, A, B, C, X, red):
    """the right normalised coprime factors [N; M] of the plant and of the reduced model, without their common D = [0; I]: two (E, A, B, C)"""
    K, Kr, r = B.T @ X @ E, red["Kr"], red["order"]
    return (E, A - B @ K, B, np.vstack([C, -K])), (np.eye(r), red["Ar"] - red["Br"] @ Kr, red["Br"], np.vstack([red["Cr"], -Kr]))


def coprime_error(E, A, B, C, X, red, omega=OMEGA):
    full, small = coprime_systems(E, A, B, C, X, red)
    return max_norm2(transfer(*full, omega) - transfer(*small, omega))


def closed_loop_abscissa(E, A, B, C, red):
    """the largest real part of the plant in the loop with the reduced controller: Ecl = diag(E, I), Acl = [[A, -B Kr], [Lr C, Ac]]"""
    n, r = E.shape[0], red["order"]
    Ecl = np.block([[E, np.zeros((n, r))], [np.zeros((r, n)), np.eye(r)]])
    Acl = np.block([[A, -B @ red["Kr"]], [red["Lr"] @ C, red["Ac"]]])
    return float(sla.eigvals(Acl, Ecl).real.max())


# ---- the SciPy reference chain and the model's run, once per process ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference_xy(n):
    """(X, Y) by scipy.linalg.solve_continuous_are on the standard form (E^-1 A, E^-1 B): X = E^-T Xs E^-1, Y = Ys"""
    E, A, B, C = system(n)
    Ei = np.linalg.inv(E)
    a, b = Ei @ A, Ei @ B
    Xs = sla.solve_continuous_are(a, b, C.T @ C, np.eye(B.shape[1]))
    Y = sla.solve_continuous_are(a.T, C.T, b @ b.T, np.eye(C.shape[0]))
    return hm._sym(Ei.T @ Xs @ Ei), hm._sym(Y)


@functools.lru_cache(maxsize=None)
def reference(n, order=0, tol=1e-8):
    """the reference chain: SciPy's X and Y, eigh factors above n eps times the largest eigenvalue, numpy.linalg.svd"""
    return lqg_balance(*system(n), *reference_xy(n), order=order, tol=tol, svd_fn=_numpy_svd, rtol=n * EPS)


@functools.lru_cache(maxsize=None)
def model_xy(n):
    return gare_pair(*system(n))


@functools.lru_cache(maxsize=None)
def chain(n, order=0, tol=1e-8):
    X, Y, _ = model_xy(n)
    return lqg_balance(*system(n), X, Y, order=order, tol=tol)


def rel(X, Xr):
    return float(np.linalg.norm(X - Xr) / np.linalg.norm(Xr))


def omega_of(n):
    return OMEGA_371 if n == 371 else OMEGA


def case_errors(n, red, ref, Hr_ref=None):
    """a reduced model against the reference at the same order: (max |mu - mu_ref| / mu_1, ||W'ET - I||_F, max_w ||H_r - H_r^ref||_2 / max_w ||H_r^ref||_2)"""
    k = min(len(red["mu"]), len(ref["mu"]))
    Hr_ref = reduced_transfer(ref, omega_of(n)) if Hr_ref is None else Hr_ref
    return (float(np.abs(red["mu"][:k] - ref["mu"][:k]).max() / ref["mu"][0]), float(red["eye_err"]),
            max_norm2(reduced_transfer(red, omega_of(n)) - Hr_ref) / max_norm2(Hr_ref))


def record_case(n):
    """the model's figures for one system: iterations, residuals, distances from the reference"""
    E, A, B, C = system(n)
    r = ORDERS[n]
    X, Y, info = model_xy(n)
    Xr, Yr = reference_xy(n)
    ch, ref = chain(n, r), reference(n, r)
    e_mu, e_eye, e_tr = case_errors(n, ch, ref)
    mu_direct = np.sort(np.sqrt(np.abs(sla.eigvals(Yr @ E.T @ Xr @ E).real)))[::-1]
    out = dict(m=B.shape[1], q=C.shape[0], order=r, iters=info["iters"], refinements_x=info["regulator"]["refinements"],
               refinements_y=info["filter"]["refinements"], res_x=info["regulator"]["res"], res_y=info["filter"]["res"], x_err=rel(X, Xr),
               y_err=rel(Y, Yr), mu=e_mu, eye=e_eye, transfer=e_tr, mu_direct=float(np.abs(ref["mu"][:r] - mu_direct[:r]).max() / mu_direct[0]),
               riccati=max(riccati_residuals(ch)), bound=ch["bound"], err=coprime_error(E, A, B, C, X, ch), rank=ch["rank"], r_o=ch["r_o"],
               r_c=ch["r_c"], abscissa_ref=closed_loop_abscissa(E, A, B, C, ref), abscissa=closed_loop_abscissa(E, A, B, C, ch),
               open_loop=float(sla.eigvals(A, E).real.max()))
    if n > 2:
        rt = ORDERS[n] - 1
        tol = clear_tol(ref["mu"], rt)
        assert chain(n, 0, tol)["order"] == reference(n, 0, tol)["order"] == rt
        out.update(tol=tol, tol_order=rt)
    return out


def record_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lqg_model.json")


def golden_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lqg_reference.npz")


@functools.lru_cache(maxsize=None)
def recorded():
    with open(record_path()) as f:
        return json.load(f)


@functools.lru_cache(maxsize=None)
def golden():
    """what the device tests need of the n = 371 reference, whose SciPy solves and transfer functions take the CPU a while: mu, the reduced
    transfer function on OMEGA_371 at order 16"""
    with np.load(golden_path()) as z:
        return {k: z[k] for k in z.files}


if __name__ == "__main__":
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), os.path.join(os.path.dirname(here), "oracle")]
    out = {}
    for n_ in SIZES:
        out[str(n_)] = record_case(n_)
        print(n_, out[str(n_)], flush=True)
    ref371 = reference(371, ORDERS[371])
    np.savez(golden_path(), mu_371=ref371["mu"], Hr_371=reduced_transfer(ref371, OMEGA_371))
    with open(record_path(), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
