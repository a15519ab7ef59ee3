"""NumPy model of the dense generalized Sylvester solver (csrc/dense_sylvester.hip): the coupled sign iteration of Benner,
Quintana-Orti and Quintana-Orti for

    A X F + E X B = -C        (A, E n x n;  B, F m x m;  C, X n x m;  both pencils c-stable)

line by line as the device runs it: the joint determinant scaling with its switch, the decision rule of csrc/sylvester_decide.hpp (decide),
the kept sequence (L_k, R_k, c_k), the replay of a right-hand side in both directions and the refinement by replaying the residual.  The H2
formulas of api.py (h2_norm, h2_inner, h2_error) are repeated on it.

The systems of the tests, their SciPy references and the recorded figures (tests/golden/sylvester_model.json) are here too.  Regenerate the
record with:  python tests/_sylvester_model.py   (well under a minute).
"""
import functools
import json
import os

import numpy as np
import scipy.linalg as sla

EPS = float(np.finfo(float).eps)
SCALE_OFF, STAG_STEP, STAG_DIST = 1e-2, 1e-8, 1e-4          # csrc/dense_sign_body.hpp
RUNNING, CONVERGED, STAGNATED, NON_FINITE, SINGULAR, OUT_OF_ITERS = 0, 1, 2, 3, 4, 5
SIDE_NONE, SIDE_LEFT, SIDE_RIGHT, SIDE_RHS = 0, 1, 2, 3      # the pencil at fault: (A, E), (B, F); 3: the right-hand side C
SIDE_NAMES = {SIDE_LEFT: "left pencil (A, E)", SIDE_RIGHT: "right pencil (B, F)", SIDE_RHS: "right-hand side C"}
SIZES = ((1, 1), (12, 5), (33, 1), (7, 130), (70, 70), (130, 7), (257, 40))
ALPHA_LEFT, ALPHA_RIGHT = 0.5, 2.0                           # the spectral abscissae -alpha of the two generated pencils differ
H2_SIZES = dict(n=60, r=6, m=2, q=3)
H2_GPU_N, STEEL_N, STEEL_ORDER = 70, 371, 10


class NotStable(Exception):
    """the device's DRE_ERR_NOT_STABLE; .done is STAGNATED, NON_FINITE or OUT_OF_ITERS, .side the pencil at fault"""
    def __init__(self, msg, done, side, iters):
        super().__init__(msg)
        self.done, self.side, self.iters = done, side, iters


class Singular(Exception):
    """the device's DRE_ERR_SINGULAR"""


class NonFiniteRhs(Exception):
    """the device's DRE_ERR_INVALID for a right-hand side with non-finite entries"""


def rel(X, Xr):
    return float(np.linalg.norm(X - Xr) / np.linalg.norm(Xr))


def key(n, m):
    return f"{n}x{m}"


# ---- the decision rule (csrc/sylvester_decide.hpp) ------------------------------------------------------------------------------------------
def default_tol(n, m, tol):
    return tol if tol is not None and tol > 0 else 10.0 * max(n, m) * EPS


def refine_target(n, m):
    return 100.0 * max(n, m) * EPS


def rel_step(d2, x2):
    return 0.0 if d2 == 0.0 else float(np.sqrt(d2 / x2))


def decide(eA, eB, dA, dB, dC, sing_left, sing_right, tol):
    """(done, side) from the distances e = ||Z + E|| / ||E||, the steps d = ||dZ|| / ||Z|| of both sides, the step of C and the inversions'
    singular flags"""
    if sing_left or sing_right:
        return SINGULAR, (SIDE_LEFT if sing_left else SIDE_RIGHT)
    if not (np.isfinite(eA) and np.isfinite(dA)):
        return NON_FINITE, SIDE_LEFT
    if not (np.isfinite(eB) and np.isfinite(dB)):
        return NON_FINITE, SIDE_RIGHT
    if not np.isfinite(dC):
        return NON_FINITE, SIDE_RHS
    if eA <= tol and eB <= tol:
        return CONVERGED, SIDE_NONE
    if dA <= STAG_STEP and eA > STAG_DIST:
        return STAGNATED, SIDE_LEFT
    if dB <= STAG_STEP and eB > STAG_DIST:
        return STAGNATED, SIDE_RIGHT
    return RUNNING, SIDE_NONE


# ---- the iteration ------------------------------------------------------------------------------------------------------------------------------
def _inv_logdet(M, what):
    if not np.isfinite(M).all():
        return np.full_like(M, np.nan), np.nan, False
    sign, logdet = np.linalg.slogdet(M)
    if sign == 0:
        return None, -np.inf, True
    return np.linalg.inv(M), float(logdet), False


def _fro2(M):
    return float(np.sum(M * M))


class SignSylvester:
    """the device's class of the same name: E and F fixed, factor(A, B) keeps (L_k, R_k, c_k), solve / solve_t replay and refine"""

    def __init__(self, E, F, maxiters=50, tol=None, max_refine=2):
        self.E, self.F = np.array(E, dtype=float), np.array(F, dtype=float)
        self.n, self.m = self.E.shape[0], self.F.shape[0]
        self.maxiters, self.max_refine = maxiters, max_refine
        self.tol = default_tol(self.n, self.m, tol)
        self.Einv, self.logdetE, sing = _inv_logdet(self.E, "E")
        if sing:
            raise Singular("E is singular")
        self.Finv, self.logdetF, sing = _inv_logdet(self.F, "F")
        if sing:
            raise Singular("F is singular")
        self.seq = []

    def factor(self, A, B, C=None):
        """the coupled sign iteration; C (optional) rides along and is returned as C_inf"""
        E, F, n, m = self.E, self.F, self.n, self.m
        self.A, self.B = np.array(A, dtype=float), np.array(B, dtype=float)
        Ak, Bk = self.A.copy(), self.B.copy()
        W = None if C is None else np.array(C, dtype=float)
        nE2, nF2 = _fro2(E), _fro2(F)
        self.seq, self.step_c = [], 0.0
        scale = True
        eA = eB = np.inf
        with np.errstate(all="ignore"):
            for k in range(self.maxiters):
                Ai, ldA, singA = _inv_logdet(Ak, "A")
                Bi, ldB, singB = _inv_logdet(Bk, "B")
                if singA or singB:
                    done, side = decide(0.0, 0.0, 0.0, 0.0, 0.0, singA, singB, self.tol)
                    raise Singular(f"singular {'A' if singA else 'B'}_{k} in the sign iteration ({SIDE_NAMES[side]})")
                c = float(np.exp((ldA + ldB - self.logdetE - self.logdetF) / (n + m))) if scale else 1.0
                L, R = E @ Ai, Bi @ F
                dC = 0.0
                if W is not None:
                    W, dC = self._c_step(W, L, R, c, False)
                An = Ak / (2.0 * c) + (0.5 * c) * (L @ E)
                Bn = Bk / (2.0 * c) + (0.5 * c) * (F @ R)
                eA, dA = np.sqrt(_fro2(An + E) / nE2), np.sqrt(_fro2(An - Ak) / _fro2(An))
                eB, dB = np.sqrt(_fro2(Bn + F) / nF2), np.sqrt(_fro2(Bn - Bk) / _fro2(Bn))
                Ak, Bk = An, Bn
                self.seq.append((L, R, c))
                self.step_c = dC
                done, side = decide(eA, eB, dA, dB, dC, False, False, self.tol)
                if done == CONVERGED:
                    return W
                if done == NON_FINITE and side == SIDE_RHS:
                    raise NonFiniteRhs("the right-hand side C has non-finite entries")
                if done:
                    raise NotStable(f"the {SIDE_NAMES[side]} is not c-stable (done {done})", done, side, k + 1)
                if eA < SCALE_OFF and eB < SCALE_OFF:
                    scale = False
        side = SIDE_LEFT if eA > self.tol else SIDE_RIGHT
        raise NotStable(f"no convergence in {self.maxiters} iterations: the {SIDE_NAMES[side]} is not c-stable", OUT_OF_ITERS, side, self.maxiters)

    @property
    def iters(self):
        return len(self.seq)

    @staticmethod
    def _c_step(W, L, R, c, transposed):
        U = (L.T @ W) @ R.T if transposed else (L @ W) @ R
        Wn = W / (2.0 * c) + (0.5 * c) * U
        return Wn, rel_step(_fro2(Wn - W), _fro2(Wn))

    def replay(self, C, transposed=False):
        W = (self.Einv.T @ C) @ self.Finv.T if transposed else np.array(C, dtype=float)
        for L, R, c in self.seq:
            W, self.step_c = self._c_step(W, L, R, c, transposed)
        return 0.5 * W if transposed else 0.5 * ((self.Einv @ W) @ self.Finv)

    def exit_transform(self, W):
        return 0.5 * ((self.Einv @ W) @ self.Finv)

    def residual(self, C, X, transposed=False, dtype=float):
        return residual(self.E, self.A, self.F, self.B, C, X, transposed, dtype)

    def solve(self, C, transposed=False, X0=None):
        """(X, dict(iters, refinements, res0, res, step)): the replay (X0: the ride-along's result instead), refined by replaying the residual while
        the relative residual ||Res|| / ||C|| exceeds 100 max(n, m) eps, at most max_refine times (the rule of SignLyap::solve_impl)"""
        C = np.array(C, dtype=float)
        with np.errstate(all="ignore"):
            X = self.replay(C, transposed) if X0 is None else X0
            step = self.step_c
            nC = np.linalg.norm(C)

            def relres(X):
                Res = self.residual(C, X, transposed)[0]
                r = np.linalg.norm(Res)
                return Res, float(r / nC if nC > 0 else r)
            Res, res = relres(X)
            res0, refinements = res, 0
            while res > refine_target(self.n, self.m) and refinements < self.max_refine:
                X = X + self.replay(Res, transposed)
                Res, res = relres(X)
                refinements += 1
        if not np.isfinite(res):
            raise NonFiniteRhs("the right-hand side C has non-finite entries")
        return X, dict(iters=self.iters, refinements=refinements, res0=res0, res=res, step=step)


def residual(E, A, F, B, C, X, transposed=False, dtype=float):
    """(Res, scaled) with Res = C + A X F + E X B (transposed: C + A'X F' + E'X B') and scaled = ||Res|| / (||C|| + ||AXF|| + ||EXB||), in dtype"""
    E, A, F, B, C, X = (np.asarray(M, dtype=dtype) for M in (E, A, F, B, C, X))
    if transposed:
        E, A, F, B = E.T, A.T, F.T, B.T
    G1, G2 = A @ (X @ F), E @ (X @ B)
    Res = C + G1 + G2
    den = np.linalg.norm(C) + np.linalg.norm(G1) + np.linalg.norm(G2)
    r = np.linalg.norm(Res)
    return Res, float(r / den if den > 0 else r)


def solve(E, A, F, B, C, transposed=False, maxiters=50, tol=None, max_refine=2):
    """the one-shot solve of the device (dre_dense_sylvester_solve): C rides along in the iteration (the transposed direction replays)"""
    n, m = np.shape(C)
    s = SignSylvester(np.eye(n) if E is None else E, np.eye(m) if F is None else F, maxiters, tol, max_refine)
    if transposed:
        s.factor(A, B)
        return s.solve(C, True)
    W = s.factor(A, B, C)
    return s.solve(C, False, X0=s.exit_transform(W))


# ---- the systems of the tests ----------------------------------------------------------------------------------------------------------------
def _frozen(*mats):
    for M in mats:
        M.setflags(write=False)
    return mats


def _pencil(rng, n, alpha):
    """nonsymmetric E != I and A = E M with the symmetric part of M below -alpha I: (A, E) is c-stable with spectral abscissa <= -alpha"""
    E = np.eye(n) + 0.25 * rng.standard_normal((n, n)) / np.sqrt(n)
    G, S = rng.standard_normal((n, n)), rng.standard_normal((n, n))
    M = -alpha * np.eye(n) - G @ G.T / n + 0.5 * (S - S.T) / np.sqrt(n)
    return E, E @ M


@functools.lru_cache(maxsize=None)
def system(n, m):
    """(E, A, F, B, C, C2): two generated pencils with different spectral abscissae and two right-hand sides"""
    rng = np.random.default_rng(7000 + 13 * n + m)
    E, A = _pencil(rng, n, ALPHA_LEFT)
    F, Bt = _pencil(rng, m, ALPHA_RIGHT)
    return _frozen(E, A, np.ascontiguousarray(F.T), np.ascontiguousarray(Bt.T), rng.standard_normal((n, m)), rng.standard_normal((n, m)))


@functools.lru_cache(maxsize=None)
def reference(n, m, transposed=False, second=False):
    """SciPy's solve_sylvester on the standard form (E^-1 A) X + X (B F^-1) = -E^-1 C F^-1"""
    E, A, F, B, C, C2 = system(n, m)
    return _frozen(scipy_reference(E, A, F, B, C2 if second else C, transposed))[0]


def scipy_reference(E, A, F, B, C, transposed=False):
    if transposed:
        E, A, F, B = E.T, A.T, F.T, B.T
    Ei, Fi = np.linalg.inv(E), np.linalg.inv(F)
    return sla.solve_sylvester(Ei @ A, B @ Fi, -Ei @ C @ Fi)


@functools.lru_cache(maxsize=None)
def lyapunov_system(n):
    """(E, A, R) for the tie to the Lyapunov solver: GSYLEProblem(E, A, E', A', R) is A X E' + E X A' = -R"""
    if n == STEEL_N:
        E, A, Bs, Cs = steel()
        return _frozen(E, A, Bs @ Bs.T)
    rng = np.random.default_rng(7100 + n)
    E, A = _pencil(rng, n, ALPHA_LEFT)
    W = rng.standard_normal((n, n))
    return _frozen(E, A, W @ W.T / n)


@functools.lru_cache(maxsize=None)
def steel():
    from test_dense_gare_host import steel_dense
    return _frozen(*steel_dense(STEEL_N))


def failure_cases():
    """name -> ((E, A, F, B, C), expected): the cases the device must refuse, and C = 0"""
    E, A, F, B, C, _ = (M.copy() for M in system(12, 5))
    Fs = F.copy()
    Fs[:, 2] = 0.0
    Cn = C.copy()
    Cn[3, 1] = np.inf
    return {
        "unstable_left": ((E, A + 3.0 * E, F, B, C), (NotStable, SIDE_LEFT)),
        "unstable_right": ((E, A, F, B + 6.0 * F, C), (NotStable, SIDE_RIGHT)),
        "singular_F": ((E, A, Fs, B, C), (Singular, None)),
        "non_finite_C": ((E, A, F, B, Cn), (NonFiniteRhs, None)),
    }


# ---- H2 norm, inner product and error -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def h2_system(n, m, q, seed=0):
    rng = np.random.default_rng(7200 + n + seed)
    E, A = _pencil(rng, n, ALPHA_LEFT)
    return _frozen(E, A, rng.standard_normal((n, m)), rng.standard_normal((q, n)))


def host_bt(E, A, B, C, r):
    """square-root balanced truncation on the host (SciPy Gramians): (I, Ar, Br, Cr)"""
    Ei = np.linalg.inv(E)
    As, Bs = Ei @ A, Ei @ B
    P = sla.solve_continuous_lyapunov(As, -Bs @ Bs.T)
    Q = sla.solve_continuous_lyapunov(As.T, -C.T @ C)
    wp, Vp = np.linalg.eigh(0.5 * (P + P.T))
    wq, Vq = np.linalg.eigh(0.5 * (Q + Q.T))
    Zc, Zo = Vp * np.sqrt(np.maximum(wp, 0)), Vq * np.sqrt(np.maximum(wq, 0))
    U, s, Vt = np.linalg.svd(Zo.T @ Zc)
    T = Zc @ Vt[:r].T / np.sqrt(s[:r])
    W = Zo @ U[:, :r] / np.sqrt(s[:r])
    return np.eye(r), W.T @ As @ T, W.T @ Bs, C @ T


def _refined_trace(E, A, F, B, R, Cl, Cr):
    """tr(Cl X Cr') for A X F + E X B = -R with the first-order correction of api.py (_h2_trace): the residual of X is replayed once through the
    kept sequence and its trace added; the formulas cancel, and the solver's own rule stops refining at a relative residual of 100 n eps"""
    s = SignSylvester(E, F)
    W = s.factor(A, B, R)
    X, _ = s.solve(R, False, X0=s.exit_transform(W))
    dX = s.replay(s.residual(R, X)[0])
    return float(np.trace(Cl @ X @ Cr.T) + np.trace(Cl @ dX @ Cr.T))


def h2_norm2(E, A, B, C):
    """||H||_H2^2 = tr(C P C') with A P E' + E P A' = -B B', the Sylvester model on the Lyapunov-shaped problem"""
    return _refined_trace(E, A, E.T, A.T, B @ B.T, C, C)


def h2_inner(sys1, sys2):
    """<H1, H2> = tr(C1 X C2') with A1 X E2' + E1 X A2' = -B1 B2'"""
    (E1, A1, B1, C1), (E2, A2, B2, C2) = sys1, sys2
    return _refined_trace(E1, A1, E2.T, A2.T, B1 @ B2.T, C1, C2)


def h2_error(full, rom):
    """dict(err, err2, norm2, norm2_r, inner, floor) of the formula err^2 = ||H||^2 - 2 <H, H_r> + ||H_r||^2; floor = eps (||H||^2 + ||H_r||^2)"""
    n2, n2r, inner = h2_norm2(*full), h2_norm2(*rom), h2_inner(full, rom)
    err2 = n2 - 2.0 * inner + n2r
    return dict(err=float(np.sqrt(max(err2, 0.0))), err2=err2, norm2=n2, norm2_r=n2r, inner=inner, floor=EPS * (n2 + n2r))


def h2_reference(full, rom=None):
    """||H||^2, or ||H - H_r||^2 from the controllability Gramian of the block-diagonal error system, by SciPy in standard form"""
    E, A, B, C = full
    Ei = np.linalg.inv(E)
    As, Bs, Cs = Ei @ A, Ei @ B, C
    if rom is not None:
        Er, Ar, Br, Cr = rom
        Eri = np.linalg.inv(Er)
        As, Bs, Cs = sla.block_diag(As, Eri @ Ar), np.vstack([Bs, Eri @ Br]), np.hstack([C, -Cr])
    P = sla.solve_continuous_lyapunov(As, -Bs @ Bs.T)
    return float(np.trace(Cs @ P @ Cs.T))


@functools.lru_cache(maxsize=None)
def h2_case(name):
    """(full, rom) of the H2 tests: 'model' (n = 60, r = 6, m = 2, q = 3), 'gpu' (n = 70) and 'steel' (SteelProfile(371), order 10)"""
    if name == "steel":
        full = steel()
        return full, _frozen(*host_bt(*full, STEEL_ORDER))
    n = H2_SIZES["n"] if name == "model" else H2_GPU_N
    full = h2_system(n, H2_SIZES["m"], H2_SIZES["q"])
    return full, _frozen(*host_bt(*full, H2_SIZES["r"]))


# ---- the record ---------------------------------------------------------------------------------------------------------------------------------
def record_size(n, m):
    E, A, F, B, C, C2 = system(n, m)
    out = dict(n=n, m=m)
    LD = np.longdouble
    X, info = solve(E, A, F, B, C)
    Y, info_t = solve(E, A, F, B, C, transposed=True)
    out.update(iters=info["iters"], refinements=info["refinements"], refinements_t=info_t["refinements"],
               res=residual(E, A, F, B, C, X)[1], res_ext=residual(E, A, F, B, C, X, False, LD)[1],
               res_t=residual(E, A, F, B, C, Y, True)[1], res_t_ext=residual(E, A, F, B, C, Y, True, LD)[1],
               x_err=rel(X, reference(n, m)), y_err=rel(Y, reference(n, m, True)))
    # the kept sequence: the replay is the ride-along, a second right-hand side, the transposed problem from scratch
    s = SignSylvester(E, F)
    s.factor(A, B)
    Xk, _ = s.solve(C)
    X2, _ = s.solve(C2)
    Yt, _ = solve(E.T, A.T, F.T, B.T, C)
    out.update(replay_equal=bool(np.array_equal(Xk, X)), res2_ext=residual(E, A, F, B, C2, X2, False, LD)[1], x2_err=rel(X2, reference(n, m, False, True)),
               t_err=rel(Y, Yt))
    return out


def record_lyapunov(n):
    E, A, R = lyapunov_system(n)
    X, info = solve(E, A, E.T, A.T, R)
    Ei = np.linalg.inv(E)
    Xr = sla.solve_continuous_lyapunov(Ei @ A, -Ei @ R @ Ei.T)
    return dict(n=n, iters=info["iters"], x_err=rel(X, Xr), asym=float(np.linalg.norm(X - X.T) / np.linalg.norm(X)))


def record_h2(name):
    full, rom = h2_case(name)
    live, ref2, refn2 = h2_error(full, rom), h2_reference(full, rom), h2_reference(full)
    own = h2_error(full, full)
    return dict(norm2=live["norm2"], norm_err=abs(np.sqrt(live["norm2"]) - np.sqrt(refn2)) / np.sqrt(refn2), err2=live["err2"], err2_ref=ref2,
                err2_diff=abs(live["err2"] - ref2), err2_rel=abs(live["err2"] - ref2) / ref2, floor=live["floor"],
                own_err2_over_norm2=abs(own["err2"]) / own["norm2"], own_floor=own["floor"])


def run_failure(name):
    (E, A, F, B, C), (exc, side) = failure_cases()[name]
    try:
        solve(E, A, F, B, C)
    except (NotStable, Singular, NonFiniteRhs) as e:
        return [type(e).__name__, getattr(e, "done", None), getattr(e, "side", None)]
    return ["none", None, None]


def record_all():
    return dict(sizes={key(n, m): record_size(n, m) for n, m in SIZES},
                lyapunov={str(n): record_lyapunov(n) for n in (H2_GPU_N, STEEL_N)},
                h2={name: record_h2(name) for name in ("model", "gpu", "steel")},
                failures={name: run_failure(name) for name in failure_cases()})


def record_path():
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sylvester_model.json")


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
