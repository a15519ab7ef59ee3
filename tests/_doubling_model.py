"""Host NumPy model of the discrete-time dense solvers as the device runs them (csrc/dense_doubling.hip): the same order of operations, the
same decision rule (csrc/doubling_decide.hpp, repeated line by line in `decide`) and the same refinement rule.

    Stein       A'XA - E'XE = -Q            M_0 = E^-1 A, H_0 = sym(Q), H_{k+1} = H_k + sym(M_k' H_k M_k), M_{k+1} = M_k^2, X = sym(E^-T H E^-1)
    dual        A Y A' - E Y E' = -Q        M_0 = A E^-1, H_{k+1} = H_k + sym(M_k H_k M_k'), Y = sym(E^-1 H E^-T)
    DARE        Q + A'X(I + GX)^-1 A - E'XE = 0, G = B Rinv B', Q = C'SC, by the SDA on A_0 = E^-1 A, G_0 = sym(E^-1 G E^-T), H_0 = sym(Q):
                W = I + G_k H_k, V = W^-1 and one Newton-Schulz step V + V (I - W V);  [T1 T2] = V [A_k G_k];  A_{k+1} = A_k T1;  G_{k+1} = G_k + sym(A_k T2 A_k');  H_{k+1} = H_k + sym(A_k' H_k T1)
                X = sym(E^-T H_inf E^-1),  Y = G_inf  (the filter's  G + A Y (I + QY)^-1 A' - E Y E' = 0)
    refinement  A_c' D A_c - E'DE = -R(X), X <- X + D on A_c = (I + GX)^-1 A while the scaled residual exceeds 100 n eps and decreases;
                the filter's Y by the dual Stein solve on A_c = A (I + YQ)^-1

The systems of the tests, their SciPy reference chain and the recorded figures (tests/golden/doubling_model.json) are here too.  Regenerate
the record with:  python tests/_doubling_model.py   (under a minute; the n = 371 Tustin case runs two SciPy solves).
"""
import functools
import json
import os

import numpy as np
import scipy.linalg as sla

EPS = np.finfo(float).eps
RUNNING, CONVERGED, NON_FINITE, SINGULAR, OUT_OF_ITERS = 0, 1, 3, 4, 5      # doubling_decide.hpp
DARE_SIZES = {1: (1, 1, 11), 12: (2, 3, 12), 33: (3, 2, 33), 70: (4, 3, 70), 130: (3, 2, 130)}      # n: (m, q, seed)
TUSTIN_SIZES = (12, 40, 70, 371)
TUSTIN_THETA = 0.25          # of the generated continuous pencils; steel 371: tustin_theta
LOOSE_N, LOOSE_TOL = 33, 1e-3


class NotStable(Exception):
    """the device's DRE_ERR_NOT_STABLE; .done is NON_FINITE or OUT_OF_ITERS, .iters the iteration it was decided at (1-based)"""
    def __init__(self, msg, done, iters):
        super().__init__(msg)
        self.done, self.iters = done, iters


class Singular(Exception):
    """the device's DRE_ERR_SINGULAR"""


def sym(M):
    return 0.5 * (M + M.T)


def rel(X, Xr):
    return float(np.linalg.norm(X - Xr) / np.linalg.norm(Xr))


# ---- the decision rule (csrc/doubling_decide.hpp) -------------------------------------------------------------------------------------------
def default_tol(n, tol):
    return tol if tol is not None and tol > 0 else 10.0 * n * EPS


def refine_target(n):
    return 100.0 * n * EPS


def _rel_step(d2, x2):
    return 0.0 if d2 == 0.0 else float(np.sqrt(d2 / x2))


def decide(dh2, h2, a2, dg2, g2, tol):
    """(done, step, normA) from the sums of squares ||dH||^2, ||H_{k+1}||^2, ||A_{k+1}||^2, ||dG||^2, ||G_{k+1}||^2"""
    with np.errstate(all="ignore"):
        normA = float(np.sqrt(a2))
        if not all(np.isfinite(v) for v in (dh2, h2, a2, dg2, g2)):
            return NON_FINITE, float("inf"), normA
        step = max(_rel_step(dh2, h2), _rel_step(dg2, g2))
        if not np.isfinite(step):
            return NON_FINITE, step, normA
        return (CONVERGED if step <= tol and normA < 1.0 else RUNNING), step, normA


def _sq(M):
    with np.errstate(all="ignore"):
        return float(np.sum(M * M))


def _inv(M, what):
    try:
        with np.errstate(all="ignore"):
            Mi = np.linalg.inv(M)
    except np.linalg.LinAlgError:
        raise Singular(f"{what} is singular") from None
    if not np.isfinite(Mi).all():
        raise Singular(f"{what} is singular")
    return Mi


def _inv_left(M, what):
    """an inverse Z of M with the small residual on the LEFT (Z M - I), as the device's Gauss-Jordan inversion with row pivoting leaves it; the
    LU-based np.linalg.inv leaves the small one on the right, so this is the transpose of the inverse of the transpose"""
    return _inv(M.T, what).T


# ---- Stein ----------------------------------------------------------------------------------------------------------------------------------
def _stein_run(Einv, A, Q, dual, maxiters, tol):
    n = A.shape[0]
    tol1 = default_tol(n, tol)
    M = A @ Einv if dual else Einv @ A
    H = sym(Q)
    step = 0.0
    with np.errstate(all="ignore"):
        for k in range(maxiters):
            D = (M @ H) @ M.T if dual else (M.T @ H) @ M
            Mn = M @ M
            d = sym(D)
            H = H + d
            done, step, _ = decide(_sq(d), _sq(H), _sq(Mn), 0.0, 0.0, tol1)
            M = Mn
            if done == CONVERGED:
                X = sym((Einv @ H) @ Einv.T) if dual else sym((Einv.T @ H) @ Einv)
                return X, dict(iters=k + 1, step=step)
            if done:
                raise NotStable(f"non-finite values at iteration {k} (E^-1 A has eigenvalues on or outside the unit circle)", done, k + 1)
    raise NotStable(f"no convergence in {maxiters} iterations (relative step {step}; E^-1 A has eigenvalues on or outside the unit circle)",
                    OUT_OF_ITERS, maxiters)


def stein(E, A, Q, dual=False, maxiters=50, tol=None):
    """(X, dict(iters, step)) of A'XA - E'XE = -Q (dual: A X A' - E X E' = -Q)"""
    E, A, Q = (np.asarray(M, dtype=float) for M in (E, A, Q))
    return _stein_run(_inv(E, "E"), A, Q, dual, maxiters, tol)


def stein_residual(E, A, Q, X, dual=False, dtype=float):
    """(R, scaled): R = sym(Q + A'XA - E'XE), scaled = ||R||_F / (||Q||_F + ||A'XA||_F + ||E'XE||_F); dtype np.longdouble for the tests' check"""
    E, A, Q, X = (np.asarray(M).astype(dtype) for M in (E, A, Q, X))
    if dual:
        E, A = E.T, A.T
    AXA, EXE = A.T @ (X @ A), E.T @ (X @ E)
    R = sym(Q) + sym(AXA) - sym(EXE)
    den = np.linalg.norm(Q) + np.linalg.norm(AXA) + np.linalg.norm(EXE)
    return R, float(np.linalg.norm(R) / den) if den > 0 else float(np.linalg.norm(R))


# ---- DARE -----------------------------------------------------------------------------------------------------------------------------------
def grams(B, C, Rinv=None, S=None):
    B, C = np.asarray(B, dtype=float), np.asarray(C, dtype=float)
    G = B @ B.T if Rinv is None else (B @ np.asarray(Rinv, dtype=float)) @ B.T
    Q = C.T @ C if S is None else (C.T @ np.asarray(S, dtype=float)) @ C
    return G, Q


def dare_residual(E, A, G, Q, X, dual=False, dtype=float):
    """(R, scaled, A_c).  Regulator: R = sym(Q + A'X A_c - E'XE), A_c = (I + GX)^-1 A.  dual (the caller passes the filter's roles, G := Q and
    Q := G): R = sym(Q + A_c Y A' - E Y E'), A_c = A (I + YG)^-1.  scaled = ||R||_F / (||Q||_F + ||A'X A_c||_F + ||E'XE||_F)."""
    E, A, G, Q, X = (np.asarray(M).astype(dtype) for M in (E, A, G, Q, X))
    n = E.shape[0]
    eye = np.eye(n, dtype=dtype)
    if dtype is float:
        # (the device inverts I + Y Q, resp. (I + G X)' = I + X G', and applies the latter transposed: the small residual on the side that matters)
        Wi = _inv_left(eye + X @ G, "I + Y Q") if dual else _inv_left(eye + X @ G.T, "I + G X").T
    else:       # (numpy has no extended-precision inverse: one step of Newton-Schulz in extended precision on the double inverse)
        W = eye + (X @ G if dual else G @ X)
        W0 = np.linalg.inv(W.astype(float)).astype(dtype)
        Wi = W0 + W0 @ (eye - W @ W0)
        Wi = Wi + Wi @ (eye - W @ Wi)
    if dual:
        Ac = A @ Wi
        AXA, EXE = (Ac @ X) @ A.T, E @ (X @ E.T)
    else:
        Ac = Wi @ A
        AXA, EXE = A.T @ (X @ Ac), E.T @ (X @ E)
    R = sym(Q) + sym(AXA) - sym(EXE)
    den = np.linalg.norm(Q) + np.linalg.norm(AXA) + np.linalg.norm(EXE)
    return R, (float(np.linalg.norm(R) / den) if den > 0 else float(np.linalg.norm(R))), Ac


def sda(Einv, A, G, Q, maxiters=50, tol=None):
    """the doubling itself on A_0 = E^-1 A, G_0 = sym(E^-1 G E^-T), H_0 = sym(Q) -> (H_inf, G_inf, iters)"""
    n = A.shape[0]
    tol1 = default_tol(n, tol)
    Ak, Gk, H = Einv @ A, sym((Einv @ G) @ Einv.T), sym(Q)
    step = 0.0
    with np.errstate(all="ignore"):
        for k in range(maxiters):
            W = Gk @ H + np.eye(n)
            if not np.isfinite(W).all():
                raise Singular(f"W_{k} = I + G_k H_k is not finite")
            V = _inv_left(W, f"W_{k} = I + G_k H_k")
            Wi = V + V @ (np.eye(n) - W @ V)          # one Newton-Schulz step: small residuals on both sides (dense_doubling.hip, the sides of the inversion)
            T1, T2 = Wi @ Ak, Wi @ Gk
            An = Ak @ T1
            dG = sym((Ak @ T2) @ Ak.T)
            dH = sym((Ak.T @ H) @ T1)
            Gn, H = Gk + dG, H + dH
            done, step, _ = decide(_sq(dH), _sq(H), _sq(An), _sq(dG), _sq(Gn), tol1)
            Ak, Gk = An, Gn
            if done == CONVERGED:
                return H, Gk, k + 1
            if done:
                raise NotStable(f"non-finite values at iteration {k} (symplectic pencil has eigenvalues on or near the unit circle / not "
                                "d-stabilizable)", done, k + 1)
    raise NotStable(f"no convergence in {maxiters} iterations (relative step {step}; symplectic pencil has eigenvalues on or near the unit circle / "
                    "not d-stabilizable)", OUT_OF_ITERS, maxiters)


def _refine(Einv, E, A, Gq, C0, X, dual, maxiters, tol, max_refine):
    n = E.shape[0]
    R, r, Ac = dare_residual(E, A, Gq, C0, X, dual)
    r0, steps = r, 0
    while r > refine_target(n) and steps < max_refine:
        D, _ = _stein_run(Einv, Ac, R, dual, maxiters, tol)
        Xn = X + D
        Rn, rn, Acn = dare_residual(E, A, Gq, C0, Xn, dual)
        steps += 1
        if not rn < r:
            break
        X, R, r, Ac = Xn, Rn, rn, Acn
    return X, dict(refinements=steps, res0=r0, res=r)


def dare_pair(E, A, B, C, Rinv=None, S=None, maxiters=50, tol=None, max_refine=2):
    """(X, Y, info): info = dict(iters, regulator = dict(refinements, res0, res), filter = the same)"""
    E, A = np.asarray(E, dtype=float), np.asarray(A, dtype=float)
    G, Q = grams(B, C, Rinv, S)
    Einv = _inv(E, "E")
    H, Ginf, iters = sda(Einv, A, G, Q, maxiters, tol)
    X, ix = _refine(Einv, E, A, G, Q, sym((Einv.T @ H) @ Einv), False, maxiters, tol, max_refine)
    Y, iy = _refine(Einv, E, A, Q, G, Ginf, True, maxiters, tol, max_refine)
    return X, Y, dict(iters=iters, regulator=ix, filter=iy)


def feedback(E, A, B, X, Rinv=None):
    RB = B.T if Rinv is None else Rinv @ B.T
    return RB @ X @ np.linalg.solve(np.eye(E.shape[0]) + B @ (RB @ X), A)


def closed_loop_radius(E, A, G, X):
    """the spectral radius of E^-1 (I + GX)^-1 A"""
    return float(np.abs(sla.eigvals(np.linalg.solve(np.eye(E.shape[0]) + G @ X, A), E)).max())


# ---- the systems ----------------------------------------------------------------------------------------------------------------------------
def _frozen(*Ms):
    for M in Ms:
        M.setflags(write=False)
    return Ms


def _pencil(n, seed, outside):
    rng = np.random.default_rng(seed)
    E = np.eye(n) + 0.1 * rng.standard_normal((n, n)) / np.sqrt(n)
    A0 = np.diag(np.linspace(-0.7, 0.7, n)) + 0.3 * rng.standard_normal((n, n)) / np.sqrt(n)
    for k, v in enumerate(outside[:n]):
        A0[k, k] = v
    return rng, E, E @ A0


@functools.lru_cache(maxsize=None)
def dare_system(n):
    """(E, A, B, C): nonsymmetric pencil with two poles outside the unit circle (one for n = 1), m != q"""
    m, q, seed = DARE_SIZES[n]
    rng, E, A = _pencil(n, seed, (1.3, 1.7))
    return _frozen(E, A, rng.standard_normal((n, m)), rng.standard_normal((q, n)))


@functools.lru_cache(maxsize=None)
def stein_system(n):
    """(E, A, Q): the stable variant of the same generator (nothing moved outside), Q = W W' / n"""
    m, q, seed = DARE_SIZES[n]
    rng, E, A = _pencil(n, seed, ())
    rng.standard_normal((n, m)), rng.standard_normal((q, n))
    W = rng.standard_normal((n, n))
    return _frozen(E, A, W @ W.T / n)


@functools.lru_cache(maxsize=None)
def continuous_system(n):
    """(E, A, Q, theta) of a c-stable continuous pencil for the Tustin identity: the stable generator of tests/_lqg_model.py (no pole moved
    into the right half plane), or SteelProfile(371) with Q = C'C"""
    if n == 371:
        from test_dense_gare_host import steel_dense
        E, A, B, C = steel_dense(371)
        return _frozen(E, A, C.T @ C) + (tustin_theta(E, A),)
    rng = np.random.default_rng(1000 + n)
    E = np.eye(n) + 0.1 * rng.standard_normal((n, n)) / np.sqrt(n)
    A0 = -np.diag(np.linspace(0.5, 20.0, n)) + 0.3 * rng.standard_normal((n, n)) / np.sqrt(n)
    W = rng.standard_normal((n, n))
    return _frozen(E, E @ A0, W @ W.T / n) + (TUSTIN_THETA,)


def tustin_theta(E, A):
    """1 / sqrt(|lambda|_min |lambda|_max) of the pencil, rounded to two digits: the Cayley transform then maps both ends of the spectrum
    equally far inside the unit circle"""
    lam = np.abs(sla.eigvals(A, E))
    return float(f"{1.0 / np.sqrt(lam.min() * lam.max()):.2g}")


def tustin(E, A, Q, theta):
    """(E_d, A_d, Q_d) = (E - theta A, E + theta A, 2 theta Q):  A_d'XA_d - E_d'XE_d = 2 theta (A'XE + E'XA)"""
    return E - theta * A, E + theta * A, 2.0 * theta * Q


# the failure cases of the tests: name -> (kind, operands, maxiters, expected done, expected iteration or None)
def failure_cases():
    I4 = np.eye(4)
    return {
        "stein_unit_circle": ("stein", (I4, np.diag([1.0, 0.5, 0.3, -0.2]), I4), 50, OUT_OF_ITERS, 50),
        "stein_unstable": ("stein", (I4, np.diag([1.3, 0.5, 0.3, -0.2]), I4), 50, NON_FINITE, 10),
        "dare_unit_circle": ("dare", (np.eye(2), np.diag([1.0, 0.5]), np.array([[0.0], [1.0]]), np.array([[1.0, 0.0]])), 50, OUT_OF_ITERS, 50),
        "dare_uncontrollable": ("dare", (np.eye(2), np.diag([1.5, 0.5]), np.array([[0.0], [1.0]]), np.array([[1.0, 0.0]])), 50, NON_FINITE, None),
    }


def run_failure(name):
    """-> (done, iters) of the model on a failure case"""
    kind, ops, maxiters, _, _ = failure_cases()[name]
    try:
        stein(*ops, maxiters=maxiters) if kind == "stein" else dare_pair(*ops, maxiters=maxiters)
    except NotStable as e:
        return e.done, e.iters
    return CONVERGED, 0


# ---- the SciPy reference chain --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def stein_reference(n):
    """(X, Y) of the Stein system, primal and dual: solve_discrete_lyapunov on E^-1 A (dual: A E^-1), mapped back with E^-T . E^-1 (E^-1 . E^-T)"""
    E, A, Q = stein_system(n)
    Ei = np.linalg.inv(E)
    Hx = sla.solve_discrete_lyapunov((Ei @ A).T, sym(Q))          # M'HM - H = -Q
    Hy = sla.solve_discrete_lyapunov(A @ Ei, sym(Q))              # N H N' - H = -Q
    return sym(Ei.T @ Hx @ Ei), sym(Ei @ Hy @ Ei.T)


@functools.lru_cache(maxsize=None)
def dare_reference(n):
    """(X, Y): solve_discrete_are in standard form on (E^-1 A, E^-1 B) for X = E^-T Xs E^-1 and on the transposed data for Y"""
    E, A, B, C = dare_system(n)
    Ei = np.linalg.inv(E)
    a, b = Ei @ A, Ei @ B
    Xs = sla.solve_discrete_are(a, b, C.T @ C, np.eye(B.shape[1]))
    Y = sla.solve_discrete_are(a.T, C.T, b @ b.T, np.eye(C.shape[0]))
    return sym(Ei.T @ Xs @ Ei), sym(Y)


@functools.lru_cache(maxsize=None)
def lyapc_reference(n):
    """X of A'XE + E'XA = -Q by solve_continuous_lyapunov on E^-1 A, mapped back with E^-T . E^-1"""
    E, A, Q, _ = continuous_system(n)
    Ei = np.linalg.inv(E)
    Xs = sla.solve_continuous_lyapunov((Ei @ A).T, -sym(Q))
    return sym(Ei.T @ Xs @ Ei)


@functools.lru_cache(maxsize=None)
def model_pair(n):
    return dare_pair(*dare_system(n))


# ---- the record -----------------------------------------------------------------------------------------------------------------------------
def record_dare(n):
    E, A, B, C = dare_system(n)
    G, Q = grams(B, C)
    X, Y, info = model_pair(n)
    Xr, Yr = dare_reference(n)
    return dict(m=B.shape[1], q=C.shape[0], iters=info["iters"], refinements_x=info["regulator"]["refinements"],
                refinements_y=info["filter"]["refinements"], res_x=info["regulator"]["res"], res_y=info["filter"]["res"],
                res_x_ext=dare_residual(E, A, G, Q, X, False, np.longdouble)[1], res_y_ext=dare_residual(E, A, Q, G, Y, True, np.longdouble)[1],
                x_err=rel(X, Xr), y_err=rel(Y, Yr), open_loop=float(np.abs(sla.eigvals(A, E)).max()), closed_loop=closed_loop_radius(E, A, G, X))


def record_stein(n):
    E, A, Q = stein_system(n)
    X, ix = stein(E, A, Q)
    Y, iy = stein(E, A, Q, dual=True)
    Xr, Yr = stein_reference(n)
    return dict(rho=float(np.abs(sla.eigvals(A, E)).max()), iters=ix["iters"], iters_dual=iy["iters"],
                res=stein_residual(E, A, Q, X, False, np.longdouble)[1], res_dual=stein_residual(E, A, Q, Y, True, np.longdouble)[1],
                x_err=rel(X, Xr), y_err=rel(Y, Yr))


def record_tustin(n):
    E, A, Q, theta = continuous_system(n)
    Ed, Ad, Qd = tustin(E, A, Q, theta)
    X, info = stein(Ed, Ad, Qd)
    return dict(theta=theta, iters=info["iters"], rho=float(np.abs(sla.eigvals(Ad, Ed)).max()), x_err=rel(X, lyapc_reference(n)))


def record_loose():
    n = LOOSE_N
    E, A, B, C = dare_system(n)
    Xr, Yr = dare_reference(n)
    X0, Y0, i0 = dare_pair(E, A, B, C, tol=LOOSE_TOL, max_refine=0)
    X, Y, info = dare_pair(E, A, B, C, tol=LOOSE_TOL)
    return dict(n=n, tol=LOOSE_TOL, iters=info["iters"], res0_x=i0["regulator"]["res"], res0_y=i0["filter"]["res"], res_x=info["regulator"]["res"],
                res_y=info["filter"]["res"], refinements_x=info["regulator"]["refinements"], refinements_y=info["filter"]["refinements"],
                x_err0=rel(X0, Xr), x_err=rel(X, Xr), y_err0=rel(Y0, Yr), y_err=rel(Y, Yr))


def record(part, key=None):
    return {"dare": record_dare, "stein": record_stein, "tustin": record_tustin}[part](key) if key is not None else record_loose()


def record_all():
    out = dict(dare={str(n): record_dare(n) for n in DARE_SIZES}, stein={str(n): record_stein(n) for n in DARE_SIZES},
               tustin={str(n): record_tustin(n) for n in TUSTIN_SIZES}, loose=record_loose(),
               failures={k: list(run_failure(k)) for k in failure_cases()})
    return out


def record_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "doubling_model.json")


@functools.lru_cache(maxsize=None)
def recorded():
    with open(record_path()) as f:
        return json.load(f)


if __name__ == "__main__":
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path[:0] = [os.path.dirname(here), os.path.join(os.path.dirname(here), "oracle")]
    out_ = record_all()
    for part_, v_ in out_.items():
        print(part_, json.dumps(v_, indent=1), flush=True)
    with open(record_path(), "w") as f:
        json.dump(out_, f, indent=1)
        f.write("\n")
