"""Discrete-time dense solvers on the device (solve(GDALEProblem / GDAREProblem, Doubling()), solve_gdare_pair, gdale_residual_dense,
gdare_residual_dense; csrc/dense_doubling.hip) on the systems of tests/_doubling_model.py: generated nonsymmetric pencils (n = 1, 12, 33, 70,
130; the DARE's with two poles outside the unit circle, m != q; n = 130 crosses a 128-wide GEMM tile) and the Tustin pencil of SteelProfile(371).

Bounds.  Every scaled residual, formed in np.longdouble, is at most the solver's own target 100 n eps.  Every distance from the SciPy reference
(solve_discrete_lyapunov, solve_discrete_are in standard form, solve_continuous_lyapunov) is at most MARGIN = 10 x the NumPy model's recorded
distance, with the floor n eps of tests/test_gpu_lqg.py (tests/golden/doubling_model.json).  Symmetry and the pair's X are bit for bit."""
import numpy as np
import pytest
import scipy.linalg as sla

import dre_amd as D
import _doubling_model as dm

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
MARGIN = 10.0
REC = dm.recorded()
LD = np.longdouble
SIZES = list(dm.DARE_SIZES)


def _bound(n, recorded):
    return max(MARGIN * recorded, n * EPS)


def _gdare(E, A, B, C):
    return D.GDAREProblem(E, A, D.lowrank(B), D.lowrank(np.ascontiguousarray(C.T)))


@pytest.mark.parametrize("n", SIZES)
def test_stein_primal_and_dual_against_scipy(ctx, n):
    E, A, Q = dm.stein_system(n)
    rec, target = REC["stein"][str(n)], 100 * n * EPS
    prob = D.GDALEProblem(E, A, Q)
    for dual, ref, err_key, it_key in ((False, dm.stein_reference(n)[0], "x_err", "iters"), (True, dm.stein_reference(n)[1], "y_err", "iters_dual")):
        X, info = D.solve(prob, D.Doubling(), dual=dual, ctx=ctx, return_info=True)
        res = dm.stein_residual(E, A, Q, X, dual, LD)[1]
        Rd, rinfo = D.gdale_residual_dense(prob, X, dual=dual, ctx=ctx, return_info=True)
        print(f"n={n} dual={dual}: iters {info['iters']} (model {rec[it_key]}) step {info['step']:.2e} residual {res:.2e} (device {rinfo['scaled']:.2e}; "
              f"target {target:.2e}) |X - X_ref| {dm.rel(X, ref):.2e} (model {rec[err_key]:.2e}) rho {rec['rho']:.3f}")
        assert np.array_equal(X, X.T)
        assert res <= target
        assert dm.rel(X, ref) <= _bound(n, rec[err_key])
        assert abs(info["iters"] - rec[it_key]) <= 1
        assert np.array_equal(D.solve(prob, D.Doubling(), dual=dual, ctx=ctx), X)
        # the device's residual is the model's: R within rounding of the terms' scale, the scaled norm at the target's level
        Rm = dm.stein_residual(E, A, Q, X, dual, LD)[0]
        scale = np.linalg.norm(Q) + 2 * np.linalg.norm(E.T @ X @ E)
        assert np.array_equal(Rd, Rd.T) and np.linalg.norm(Rd - Rm.astype(float)) <= 8 * n * EPS * scale and rinfo["scaled"] <= target
        assert rinfo["norm"] == pytest.approx(np.linalg.norm(Rd), rel=1e-12)


@pytest.mark.parametrize("n", dm.TUSTIN_SIZES)
def test_tustin_identity_ties_the_stein_solver_to_the_sign_solver(ctx, n):
    """A_d'XA_d - E_d'XE_d = 2 theta (A'XE + E'XA) with (E_d, A_d) = (E - theta A, E + theta A) is exact algebra: the Stein solve of the Tustin
    pencil is the continuous Lyapunov solve of the sign path"""
    E, A, Q, theta = dm.continuous_system(n)
    rec = REC["tustin"][str(n)]
    assert theta == rec["theta"]
    Xd, info = D.solve(D.GDALEProblem(*dm.tustin(E, A, Q, theta)), D.Doubling(), ctx=ctx, return_info=True)
    Xc = D.solve(D.GALEProblem(E, A, Q), D.MatrixSign(), ctx=ctx)
    print(f"n={n} theta={theta}: iters {info['iters']} (model {rec['iters']}) rho {rec['rho']:.4f} |X_stein - X_sign| {dm.rel(Xd, Xc):.2e} (model against "
          f"solve_continuous_lyapunov {rec['x_err']:.2e})")
    assert dm.rel(Xd, Xc) <= _bound(n, rec["x_err"])
    assert abs(info["iters"] - rec["iters"]) <= 1 and np.array_equal(Xd, Xd.T)


@pytest.mark.parametrize("n", SIZES)
def test_dare_against_scipy(ctx, n):
    E, A, B, C = dm.dare_system(n)
    G, Q = dm.grams(B, C)
    rec, target = REC["dare"][str(n)], 100 * n * EPS
    X, info = D.solve(_gdare(E, A, B, C), D.Doubling(), ctx=ctx, return_info=True)
    res = dm.dare_residual(E, A, G, Q, X, False, LD)[1]
    Xr = dm.dare_reference(n)[0]
    rho = dm.closed_loop_radius(E, A, G, X)
    Rd, rinfo = D.gdare_residual_dense(_gdare(E, A, B, C), X, ctx=ctx, return_info=True)
    print(f"n={n}: iters {info['iters']} (model {rec['iters']}) refinements {info['refinements']} res0 {info['res0']:.2e} res {info['res']:.2e} extended "
          f"{res:.2e} (model {rec['res_x_ext']:.2e}; target {target:.2e}) |X - X_ref| {dm.rel(X, Xr):.2e} (model {rec['x_err']:.2e}) closed loop {rho:.4f} "
          f"(open {rec['open_loop']:.3f})")
    assert np.array_equal(X, X.T)
    assert res <= target
    assert dm.rel(X, Xr) <= _bound(n, rec["x_err"])
    assert abs(info["iters"] - rec["iters"]) <= 1
    assert rho < 1.0 < rec["open_loop"]
    assert info["res"] <= info["res0"]
    K = dm.feedback(E, A, B, X)
    assert info["K"].shape == (B.shape[1], n)
    assert np.linalg.norm(info["K"] - K) <= 8 * n * EPS * np.linalg.norm(B) * np.linalg.norm(X) * np.linalg.norm(A)
    assert rinfo["scaled"] == info["res"] and np.array_equal(Rd, Rd.T) and rinfo["norm"] == pytest.approx(np.linalg.norm(Rd), rel=1e-12)


@pytest.mark.parametrize("n", SIZES)
def test_pair_x_is_the_single_solve_bit_for_bit_and_y_solves_the_filter_equation(ctx, n):
    E, A, B, C = dm.dare_system(n)
    G, Q = dm.grams(B, C)
    rec, target = REC["dare"][str(n)], 100 * n * EPS
    (X, Y), info = D.solve_gdare_pair(E, A, B, C, ctx=ctx, return_info=True)
    Xs, single = D.solve(_gdare(E, A, B, C), D.Doubling(), ctx=ctx, return_info=True)
    assert np.array_equal(X, Xs)
    assert info["iters"] == info["regulator"]["iters"] == info["filter"]["iters"] == single["iters"]
    assert (info["regulator"]["refinements"], info["regulator"]["res0"], info["regulator"]["res"]) == (single["refinements"], single["res0"], single["res"])
    assert np.array_equal(info["K"], single["K"])
    # the filter's Y against its equation, against SciPy and against the single solve on the transposed data
    res = dm.dare_residual(E, A, Q, G, Y, True, LD)[1]
    Yr = dm.dare_reference(n)[1]
    Yt = D.solve(_gdare(np.ascontiguousarray(E.T), np.ascontiguousarray(A.T), np.ascontiguousarray(C.T), np.ascontiguousarray(B.T)), D.Doubling(), ctx=ctx)
    print(f"n={n}: iters {info['iters']} refinements X {info['regulator']['refinements']} Y {info['filter']['refinements']} residual of Y {res:.2e} "
          f"(reported {info['filter']['res']:.2e}; model {rec['res_y_ext']:.2e}; target {target:.2e}) |Y - Y_ref| {dm.rel(Y, Yr):.2e} (model "
          f"{rec['y_err']:.2e}) |Y - Y_transposed| {dm.rel(Y, Yt):.2e}")
    assert res <= target
    assert info["filter"]["res"] <= info["filter"]["res0"]
    assert dm.rel(Y, Yr) <= _bound(n, rec["y_err"])
    assert np.array_equal(Y, Y.T) and np.linalg.eigvalsh(Y).min() >= -n * EPS * np.linalg.norm(Y, 2)
    assert dm.rel(Y, Yt) <= _bound(n, rec["y_err"])
    # the Kalman gain L = A Y (I + QY)^-1 C'
    L = A @ Y @ np.linalg.solve(np.eye(n) + Q @ Y, C.T)
    assert info["L"].shape == (n, C.shape[0])
    assert np.linalg.norm(info["L"] - L) <= 8 * n * EPS * np.linalg.norm(A) * np.linalg.norm(Y) * np.linalg.norm(C)


def test_scaled_inner_matrices(ctx):
    """G = beta B Rinv B', Q = gamma C' S C through the problem type, and Rinv, S through the pair call: the same X"""
    n = 33
    E, A, B, C = dm.dare_system(n)
    rng = np.random.default_rng(5)
    Rinv, S = (M @ M.T + k * np.eye(k) for k, M in ((B.shape[1], rng.standard_normal((B.shape[1],) * 2)), (C.shape[0], rng.standard_normal((C.shape[0],) * 2))))
    beta, gamma = 2.5, 0.7
    prob = D.GDAREProblem(E, A, beta * D.lowrank(B, Rinv), gamma * D.lowrank(np.ascontiguousarray(C.T), S))
    X, info = D.solve(prob, D.Doubling(), ctx=ctx, return_info=True)
    G, Q = dm.grams(B, C, beta * Rinv, gamma * S)
    res = dm.dare_residual(E, A, G, Q, X, False, LD)[1]
    Xm, Ym, _ = dm.dare_pair(E, A, B, C, beta * Rinv, gamma * S)
    Ei = np.linalg.inv(E)
    Xr = dm.sym(Ei.T @ sla.solve_discrete_are(Ei @ A, Ei @ B, Q, np.linalg.inv(beta * Rinv)) @ Ei)
    print(f"scaled inner matrices: res {info['res']:.2e} extended {res:.2e} |X - X_ref| {dm.rel(X, Xr):.2e} (model {dm.rel(Xm, Xr):.2e})")
    assert res <= 100 * n * EPS and dm.rel(X, Xr) <= _bound(n, dm.rel(Xm, Xr))
    (Xp, Yp) = D.solve_gdare_pair(E, A, B, C, Rinv=beta * Rinv, S=gamma * S, ctx=ctx)
    assert np.array_equal(Xp, X) and dm.dare_residual(E, A, Q, G, Yp, True, LD)[1] <= 100 * n * EPS
    assert np.linalg.norm(info["K"] - dm.feedback(E, A, B, X, beta * Rinv)) <= 8 * n * EPS * np.linalg.norm(beta * Rinv) * np.linalg.norm(B) * np.linalg.norm(X) * np.linalg.norm(A)


def test_a_loose_tolerance_is_repaired_by_the_refinement(ctx):
    """tol = 1e-3 ends the doubling early (model: res0 7.8e-11 for X and 1.3e-10 for Y at n = 33, above the target 7.3e-13): max_refine = 0 returns
    that, the default makes one or two Newton steps on the Stein solver, reaches the target and beats the unrefined distance"""
    n, rec = dm.LOOSE_N, REC["loose"]
    E, A, B, C = dm.dare_system(n)
    G, Q = dm.grams(B, C)
    target = 100 * n * EPS
    Xr, Yr = dm.dare_reference(n)
    assert rec["res0_x"] > target and rec["res0_y"] > target
    (X0, Y0), i0 = D.solve_gdare_pair(E, A, B, C, D.Doubling(tol=dm.LOOSE_TOL, max_refine=0), ctx=ctx, return_info=True)
    (X, Y), info = D.solve_gdare_pair(E, A, B, C, D.Doubling(tol=dm.LOOSE_TOL), ctx=ctx, return_info=True)
    Xs, single = D.solve(_gdare(E, A, B, C), D.Doubling(tol=dm.LOOSE_TOL), ctx=ctx, return_info=True)
    print(f"n={n}: iters {info['iters']} (model {rec['iters']}) X: res0 {info['regulator']['res0']:.2e} res {info['regulator']['res']:.2e} (model "
          f"{rec['res0_x']:.2e}, {rec['res_x']:.2e}) refinements {info['regulator']['refinements']} |X - X_ref| {dm.rel(X0, Xr):.2e} -> {dm.rel(X, Xr):.2e} "
          f"(model {rec['x_err0']:.2e} -> {rec['x_err']:.2e});  Y: res0 {info['filter']['res0']:.2e} res {info['filter']['res']:.2e} refinements "
          f"{info['filter']['refinements']} |Y - Y_ref| {dm.rel(Y0, Yr):.2e} -> {dm.rel(Y, Yr):.2e} (model {rec['y_err0']:.2e} -> {rec['y_err']:.2e})")
    assert np.array_equal(X, Xs) and info["iters"] == single["iters"] == i0["iters"] and abs(info["iters"] - rec["iters"]) <= 1
    for side in ("regulator", "filter"):
        assert i0[side]["refinements"] == 0 and i0[side]["res"] == i0[side]["res0"] == info[side]["res0"] > target
        assert 1 <= info[side]["refinements"] <= 2 and info[side]["res"] <= target
    assert dm.dare_residual(E, A, G, Q, X, False, LD)[1] <= target and dm.dare_residual(E, A, Q, G, Y, True, LD)[1] <= target
    assert dm.rel(X, Xr) <= _bound(n, rec["x_err"]) < dm.rel(X0, Xr)
    assert dm.rel(Y, Yr) <= _bound(n, rec["y_err"]) < dm.rel(Y0, Yr)


def test_failures_leave_the_context_usable(ctx):
    def alive():
        E, A, B, C = dm.dare_system(12)
        X = D.solve(_gdare(E, A, B, C), D.Doubling(), ctx=ctx)
        assert dm.rel(X, dm.dare_reference(12)[0]) <= _bound(12, REC["dare"]["12"]["x_err"])
        Es, As, Qs = dm.stein_system(12)
        Xs = D.solve(D.GDALEProblem(Es, As, Qs), D.Doubling(), ctx=ctx)
        assert dm.rel(Xs, dm.stein_reference(12)[0]) <= _bound(12, REC["stein"]["12"]["x_err"])

    for name, (kind, ops, maxiters, done, _) in dm.failure_cases().items():
        with pytest.raises(D.DREError) as e:
            if kind == "stein":
                D.solve(D.GDALEProblem(*ops), D.Doubling(maxiters=maxiters), ctx=ctx)
            else:
                D.solve(_gdare(*ops), D.Doubling(maxiters=maxiters), ctx=ctx)
        print(name, "->", e.value)
        assert e.value.code == -7, name
        assert ("non-finite" in str(e.value)) == (done == dm.NON_FINITE), name
        assert "unit circle" in str(e.value), name
        alive()
    # the pair call fails the same way
    with pytest.raises(D.DREError) as e:
        D.solve_gdare_pair(*dm.failure_cases()["dare_unit_circle"][1], ctx=ctx)
    assert e.value.code == -7
    alive()
    # Q = 0 on an unstable pencil: dH = 0 from the first iteration on, and the iteration must not "converge" to X = 0
    with pytest.raises(D.DREError) as e:
        D.solve(D.GDALEProblem(np.eye(3), 1.5 * np.eye(3), np.zeros((3, 3))), D.Doubling(), ctx=ctx)
    assert e.value.code == -7
    alive()
    # ... while on a stable one X = 0 is the answer
    assert np.array_equal(D.solve(D.GDALEProblem(np.eye(3), 0.5 * np.eye(3), np.zeros((3, 3))), D.Doubling(), ctx=ctx), np.zeros((3, 3)))
    # a singular E
    E, A, B, C = (M.copy() for M in dm.dare_system(12))
    E[3, :] = 0.0
    for call in (lambda: D.solve(_gdare(E, A, B, C), D.Doubling(), ctx=ctx), lambda: D.solve_gdare_pair(E, A, B, C, ctx=ctx),
                 lambda: D.solve(D.GDALEProblem(E, A, np.eye(12)), D.Doubling(), ctx=ctx)):
        with pytest.raises(D.DREError) as e:
            call()
        assert e.value.code == -4 and "singular" in str(e.value)
        alive()
