"""Dense generalized Sylvester solver on the device (solve(GSYLEProblem, MatrixSign()), gsyle_residual_dense, SylvesterFactorization, h2_norm,
h2_inner, h2_error; csrc/dense_sylvester.hip) on the systems of tests/_sylvester_model.py: generated nonsymmetric pencils with E, F != I and
different spectral abscissae on the two sides, (n, m) in {(1,1), (12,5), (33,1), (7,130), (70,70), (130,7), (257,40)} (130 and 257 cross the
128- and 256-wide GEMM tiles, (7,130) has the wide side on the right, (33,1) is a single column), and SteelProfile(371).

Bounds.  Every scaled residual, formed in np.longdouble, is at most the solver's own target 100 max(n, m) eps.  Every distance from the SciPy
reference (solve_sylvester in standard form, solve_continuous_lyapunov) is at most MARGIN = 10 x the NumPy model's recorded distance, with the
floor max(n, m) eps (tests/golden/sylvester_model.json; the convention of tests/test_gpu_doubling.py).  The device's residual matrix agrees
with the extended-precision one to 8 max(n, m) eps of the terms' scale."""
import numpy as np
import pytest
import scipy.linalg as sla

import dre_amd as D
import _sylvester_model as sm

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
MARGIN = 10.0
REC = sm.recorded()
LD = np.longdouble
T = np.ascontiguousarray


def _bound(k, recorded):
    return max(MARGIN * recorded, k * EPS)


def _terms_scale(E, A, F, B, C, X, transposed):
    if transposed:
        E, A, F, B = E.T, A.T, F.T, B.T
    return np.linalg.norm(C) + np.linalg.norm(A @ X @ F) + np.linalg.norm(E @ X @ B)


@pytest.mark.parametrize("n,m", sm.SIZES)
def test_both_directions_against_scipy(ctx, n, m):
    E, A, F, B, C, _ = sm.system(n, m)
    rec, k = REC["sizes"][sm.key(n, m)], max(n, m)
    target = 100 * k * EPS
    prob = D.GSYLEProblem(E, A, F, B, C)
    for transposed, err_key in ((False, "x_err"), (True, "y_err")):
        X, info = D.solve(prob, D.MatrixSign(), transposed=transposed, ctx=ctx, return_info=True)
        Rm, res = sm.residual(E, A, F, B, C, X, transposed, LD)
        Rd, rinfo = D.gsyle_residual_dense(prob, X, transposed=transposed, ctx=ctx, return_info=True)
        ref = sm.reference(n, m, transposed)
        print(f"({n},{m}) transposed={transposed}: iters {info['iters']} (model {rec['iters']}) refinements {info['refinements']} res0 {info['res0']:.2e} "
              f"res {info['res']:.2e} step {info['step']:.2e} scaled residual {res:.2e} (device {rinfo['scaled']:.2e}; target {target:.2e}) "
              f"|X - X_ref| {sm.rel(X, ref):.2e} (model {rec[err_key]:.2e})")
        assert X.shape == (n, m)
        assert res <= target
        assert sm.rel(X, ref) <= _bound(k, rec[err_key])
        assert abs(info["iters"] - rec["iters"]) <= 1
        assert np.array_equal(D.solve(prob, D.MatrixSign(), transposed=transposed, ctx=ctx), X)
        scale = _terms_scale(E, A, F, B, C, X, transposed)
        dR = np.linalg.norm(Rd - Rm.astype(float))
        print(f"    |Res_device - Res_extended| {dR:.2e} (bound {8 * k * EPS * scale:.2e})")
        assert dR <= 8 * k * EPS * scale
        assert rinfo["norm"] == pytest.approx(np.linalg.norm(Rd), rel=1e-12) and rinfo["scaled"] <= target


@pytest.mark.parametrize("n,m", ((12, 5), (7, 130), (130, 7)))
def test_kept_factorisation(ctx, n, m):
    E, A, F, B, C, C2 = sm.system(n, m)
    rec, k = REC["sizes"][sm.key(n, m)], max(n, m)
    X, info = D.solve(D.GSYLEProblem(E, A, F, B, C), D.MatrixSign(), ctx=ctx, return_info=True)
    with D.SylvesterFactorization(E, A, F, B, ctx=ctx) as fac:
        assert (fac.n, fac.m, fac.iters) == (n, m, info["iters"])
        Xk, ik = fac.solve(C)
        assert np.array_equal(Xk, X) and (ik["iters"], ik["refinements"], ik["res0"], ik["res"], ik["step"]) == tuple(
            info[key] for key in ("iters", "refinements", "res0", "res", "step"))
        X2, _ = fac.solve(C2)
        res2 = sm.residual(E, A, F, B, C2, X2, False, LD)[1]
        Y, _ = fac.solve(C, transposed=True)
        Xd, _ = fac.solve(C, download=False)
        assert isinstance(Xd, D.DenseMatrix) and np.array_equal(Xd.numpy(), X)
    Yt = D.solve(D.GSYLEProblem(T(E.T), T(A.T), T(F.T), T(B.T), C), D.MatrixSign(), ctx=ctx)
    print(f"({n},{m}): second right-hand side: scaled residual {res2:.2e} |X2 - ref| {sm.rel(X2, sm.reference(n, m, False, True)):.2e} (model "
          f"{rec['x2_err']:.2e});  transposed replay against the transposed problem {sm.rel(Y, Yt):.2e} (model {rec['t_err']:.2e}, y_err {rec['y_err']:.2e})")
    assert res2 <= 100 * k * EPS
    assert sm.rel(X2, sm.reference(n, m, False, True)) <= _bound(k, rec["x2_err"])
    assert sm.rel(Y, Yt) <= _bound(k, rec["y_err"])


@pytest.mark.parametrize("n", (sm.H2_GPU_N, sm.STEEL_N))
def test_tie_to_the_lyapunov_solver(ctx, n):
    """GSYLEProblem(E, A, E', A', R) is A X E' + E X A' = -R, the dual equation of the sign solver's pencil"""
    E, A, R = sm.lyapunov_system(n)
    rec = REC["lyapunov"][str(n)]
    X, info = D.solve(D.GSYLEProblem(E, A, T(E.T), T(A.T), R), D.MatrixSign(), ctx=ctx, return_info=True)
    sign = D.SignFactorization(E, A, ctx=ctx)
    try:
        Xl, _ = sign.solve_dense(R, transposed=True)
    finally:
        sign.close()
    asym = np.linalg.norm(X - X.T) / np.linalg.norm(X)
    print(f"n={n}: iters {info['iters']} (model {rec['iters']}; the Lyapunov solver {sign.iters}) |X_sylvester - X_lyapunov| {sm.rel(X, Xl):.2e} (model against "
          f"SciPy {rec['x_err']:.2e}) asymmetry {asym:.2e} (model {rec['asym']:.2e})")
    assert sm.rel(X, Xl) <= _bound(n, rec["x_err"])
    assert asym <= _bound(n, rec["x_err"])
    assert abs(info["iters"] - rec["iters"]) <= 1


def test_identity_E_and_F_is_the_standard_equation(ctx):
    n, m = 33, 12
    rng = np.random.default_rng(77)
    A, B = (np.linalg.solve(*sm._pencil(rng, k, alpha)) for k, alpha in ((n, 0.5), (m, 1.5)))       # E^-1 A of a generated pencil: c-stable
    C = rng.standard_normal((n, m))
    Xr = sla.solve_sylvester(A, B, -C)
    cond_floor = sm.rel(sm.solve(None, A, None, B, C)[0], Xr)
    for transposed, ref in ((False, Xr), (True, sla.solve_sylvester(A.T, B.T, -C))):
        X, info = D.solve(D.GSYLEProblem(None, A, None, B, C), D.MatrixSign(), transposed=transposed, ctx=ctx, return_info=True)
        res = sm.residual(np.eye(n), A, np.eye(m), B, C, X, transposed, LD)[1]
        Rd, rinfo = D.gsyle_residual_dense(D.GSYLEProblem(None, A, None, B, C), X, transposed=transposed, ctx=ctx, return_info=True)
        print(f"standard equation transposed={transposed}: iters {info['iters']} residual {res:.2e} (device {rinfo['scaled']:.2e}) |X - X_scipy| "
              f"{sm.rel(X, ref):.2e} (model {cond_floor:.2e})")
        assert res <= 100 * n * EPS and rinfo["scaled"] <= 100 * n * EPS
        assert sm.rel(X, ref) <= _bound(n, cond_floor)
    with D.SylvesterFactorization(None, A, None, B, ctx=ctx) as fac:
        assert np.array_equal(fac.solve(C)[0], D.solve(D.GSYLEProblem(None, A, None, B, C), D.MatrixSign(), ctx=ctx))


def test_failures_leave_the_context_usable(ctx):
    E, A, F, B, C, _ = sm.system(12, 5)

    def alive():
        X = D.solve(D.GSYLEProblem(E, A, F, B, C), D.MatrixSign(), ctx=ctx)
        assert sm.rel(X, sm.reference(12, 5)) <= _bound(12, REC["sizes"]["12x5"]["x_err"])

    cases = sm.failure_cases()
    for name, code, words in (("unstable_right", -7, ("right pencil (B, F)",)), ("unstable_left", -7, ("left pencil (A, E)",)),
                              ("singular_F", -4, ("F is singular",)), ("non_finite_C", -1, ("non-finite",))):
        ops = cases[name][0]
        for call in (lambda: D.solve(D.GSYLEProblem(*ops), D.MatrixSign(), ctx=ctx),
                     lambda: D.SylvesterFactorization(*ops[:4], ctx=ctx).solve(ops[4])):
            with pytest.raises(D.DREError) as e:
                call()
            print(name, "->", e.value)
            assert e.value.code == code, name
            assert all(w in str(e.value) for w in words), name
            alive()
    # the transposed direction refuses a non-finite right-hand side too
    with pytest.raises(D.DREError) as e:
        D.solve(D.GSYLEProblem(*cases["non_finite_C"][0]), D.MatrixSign(), transposed=True, ctx=ctx)
    assert e.value.code == -1
    alive()
    # a singular A
    As = A.copy()
    As[:, 4] = 0.0
    with pytest.raises(D.DREError) as e:
        D.solve(D.GSYLEProblem(E, As, F, B, C), D.MatrixSign(), ctx=ctx)
    print("singular A ->", e.value)
    assert e.value.code == -4 and "A_0" in str(e.value)
    alive()
    # C = 0: exact zeros, both directions and on the kept factorisation
    Z = np.zeros((12, 5))
    for transposed in (False, True):
        X0, info = D.solve(D.GSYLEProblem(E, A, F, B, Z), D.MatrixSign(), transposed=transposed, ctx=ctx, return_info=True)
        assert np.array_equal(X0, Z) and info["res"] == 0.0 and info["refinements"] == 0
    with D.SylvesterFactorization(E, A, F, B, ctx=ctx) as fac:
        assert np.array_equal(fac.solve(Z)[0], Z)
    alive()


def _h2_rom(ctx, name):
    full, host_rom = sm.h2_case(name)
    if name == "steel":
        return full, D.balanced_truncation(*full, alg=D.MatrixSign(), order=sm.STEEL_ORDER, ctx=ctx)
    return full, D.ReducedModel(*host_rom, hsv=np.zeros(0), T=np.zeros((0, 0)), W=np.zeros((0, 0)))


@pytest.mark.parametrize("name", ("gpu", "steel"))
def test_h2_norm_inner_and_error(ctx, name):
    full, rom = _h2_rom(ctx, name)
    rec = REC["h2"][name]
    n = full[0].shape[0]
    rsys = (rom.Er, rom.Ar, rom.Br, rom.Cr)
    nrm = D.h2_norm(*full, ctx=ctx)
    ref_n = np.sqrt(sm.h2_reference(full))
    err, info = D.h2_error(*full, rom, return_info=True, ctx=ctx)
    ref2 = sm.h2_reference(full, rsys)
    print(f"{name} (n = {n}, r = {rom.order}): h2_norm {nrm:.12e} |rel diff| {abs(nrm - ref_n) / ref_n:.2e} (model {rec['norm_err']:.2e});  err2 {info['err2']:.6e} "
          f"reference {ref2:.6e} |diff| {abs(info['err2'] - ref2):.2e} (model {rec['err2_diff']:.2e}, floor {info['floor']:.2e})")
    assert abs(nrm - ref_n) / ref_n <= _bound(n, rec["norm_err"])
    assert info["norm2"] == pytest.approx(nrm * nrm, rel=1e-14) and info["floor"] == EPS * (info["norm2"] + info["norm2_r"])
    assert abs(info["err2"] - ref2) <= MARGIN * max(rec["err2_diff"], info["floor"])
    assert err == np.sqrt(max(info["err2"], 0.0))
    assert info["inner"] == D.h2_inner(full, rsys, ctx=ctx)
    assert rom.h2_error(*full, ctx=ctx) == err


@pytest.mark.parametrize("name", ("gpu", "steel"))
def test_h2_error_of_a_system_against_itself_is_at_the_floor(ctx, name):
    """With the full system as its own reduced model h2_error is at most sqrt(10 floor), floor = eps (||H||^2 + ||H_r||^2).  The two norms come
    from the Lyapunov path and the inner product from the Sylvester path; without the first-order correction of the traces (api.py, _h2_trace) the
    steel case stood at err2 = 26 eps ||H||^2 against the 20 allowed: the Gramian's residual of 2e-12 is below the solver's own refinement target."""
    full, _ = sm.h2_case(name)
    own, info = D.h2_error(*full, full, return_info=True, ctx=ctx)
    print(f"{name}: err {own:.3e} err2 {info['err2']:.3e} = {info['err2'] / info['norm2'] / EPS:.1f} eps ||H||^2; floor {info['floor']:.3e}, bound on err "
          f"{np.sqrt(MARGIN * info['floor']):.3e}")
    assert own <= np.sqrt(MARGIN * info["floor"])


def test_h2_error_refuses_a_reduced_model_that_is_not_c_stable(ctx):
    full, host_rom = sm.h2_case("gpu")
    Er, Ar, Br, Cr = host_rom
    bad = D.ReducedModel(Er, Ar + 3.0 * np.eye(Ar.shape[0]), Br, Cr, hsv=np.zeros(0), T=np.zeros((0, 0)), W=np.zeros((0, 0)))
    with pytest.raises(D.DREError) as e:
        D.h2_error(*full, bad, ctx=ctx)
    print(e.value)
    assert e.value.code == -7 and "reduced model" in str(e.value)
    with pytest.raises(D.DREError) as e:
        D.h2_inner(full, (Er, Ar + 3.0 * np.eye(Ar.shape[0]), Br, Cr), ctx=ctx)
    assert e.value.code == -7 and "right pencil (B, F)" in str(e.value)
    # the context still solves
    E, A, F, B, C, _ = sm.system(12, 5)
    assert sm.rel(D.solve(D.GSYLEProblem(E, A, F, B, C), D.MatrixSign(), ctx=ctx), sm.reference(12, 5)) <= _bound(12, REC["sizes"]["12x5"]["x_err"])
