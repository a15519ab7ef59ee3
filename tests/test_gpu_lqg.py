"""LQG balanced truncation on the device (solve_gare_pair, lqg_balanced_truncation, lqg_error; csrc/dense_are.hip: dense_gare_solve_pair,
csrc/balance.hip: lqg_balance) on the systems of tests/_lqg_model.py: four generated nonsymmetric plants with two unstable poles (n = 1, 12,
33, 70; m != q) and the unstable SteelProfile(371).

Bounds.  X of the pair call: bit for bit the X of the single solver.  Y: its scaled residual, formed in extended precision, at most the
solver's own target 100 n eps (or 10 x what the single solver reaches on the transposed problem, if that is above the target), and its
distance from SciPy's Y at most MARGIN = 10 x the NumPy model's recorded distance, with the floor n eps of tests/test_gpu_svd_jacobi.py.  The
reduced model: mu, ||W'ET - I||_F and the reduced transfer function each within MARGIN x the model's recorded distance from the reference
chain (SciPy's Riccati solutions, eigh factors, numpy.linalg.svd; tests/golden/lqg_model.json).  err <= bound is a theorem; the measured err
is a difference of two frequency responses of norm 1, each accurate to a small multiple of eps, so RESPONSE_ROUNDING = 1e3 eps is added to the
bound (it matters only at (1, 1), where nothing is truncated and the bound is 0)."""
import numpy as np
import pytest

import dre_amd as D
import _lqg_model as lm
from test_dense_gare_host import oscillator_pencil

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
MARGIN = 10.0
RESPONSE_ROUNDING = 1e3 * EPS
REC = lm.recorded()
LD = np.longdouble
CASES = [(12, 6), (33, 8), (70, 12), (1, 1), (371, 16)]
_runs = {}


def _lqgbt(ctx, n, r):
    """one lqg_balanced_truncation per (n, r) and session: (rom, info)"""
    if (n, r) not in _runs:
        _runs[n, r] = D.lqg_balanced_truncation(*lm.system(n), order=r, ctx=ctx, return_info=True)
    return _runs[n, r]


def _as_dict(rom):
    return dict(order=rom.order, mu=rom.mu, Ar=rom.Ar, Br=rom.Br, Cr=rom.Cr, Kr=rom.Kr, Lr=rom.Lr, Ac=rom.Ac)


def _residual_f_extended(E, A, B, C, Y):
    El, Al, Bl, Cl, Yl = (M.astype(LD) for M in (E, A, B, C, Y))
    G, Q = Bl @ Bl.T, Cl.T @ Cl
    YE = Yl @ El.T
    AYE = Al @ YE
    YQY = YE.T @ (Q @ YE)
    R = G + AYE + AYE.T - YQY
    return float(np.linalg.norm(R) / (np.linalg.norm(G) + 2 * np.linalg.norm(AYE) + np.linalg.norm(YQY)))


@pytest.mark.parametrize("n", [12, 33, 70])
def test_pair_x_is_the_single_solve_bit_for_bit_and_y_solves_the_filter_equation(ctx, n):
    E, A, B, C = lm.system(n)
    (X, Y), info = D.solve_gare_pair(E, A, B, C, ctx=ctx, return_info=True)
    Xs, single = D.solve(D.GAREProblem(E, A, D.lowrank(B), D.lowrank(np.ascontiguousarray(C.T))), D.MatrixSign(), ctx=ctx, return_info=True)
    assert np.array_equal(X, Xs)
    assert info["iters"] == info["regulator"]["iters"] == info["filter"]["iters"] == single["iters"] and info["factorizations"] == 1
    assert (info["regulator"]["refinements"], info["regulator"]["res0"], info["regulator"]["res"]) == (single["refinements"], single["res0"], single["res"])
    # the filter's Y: the single solver needs a full sign iteration of its own on the transposed problem
    Yt, it = D.solve(D.GAREProblem(np.ascontiguousarray(E.T), np.ascontiguousarray(A.T), D.lowrank(np.ascontiguousarray(C.T)), D.lowrank(B)),
                     D.MatrixSign(), ctx=ctx, return_info=True)
    assert it["iters"] >= 1
    target = 100 * n * EPS
    res, res_t = _residual_f_extended(E, A, B, C, Y), _residual_f_extended(E, A, B, C, Yt)
    _, Yr = lm.reference_xy(n)
    rec = REC[str(n)]
    print(f"n={n}: iters {info['iters']} (transposed single solve {it['iters']}) refinements X {info['regulator']['refinements']} Y "
          f"{info['filter']['refinements']} residual of Y {res:.2e} (reported {info['filter']['res']:.2e}; transposed single solve {res_t:.2e}; target "
          f"{target:.2e}) |Y - Y_ref| {lm.rel(Y, Yr):.2e} (model {rec['y_err']:.2e}; transposed single solve {lm.rel(Yt, Yr):.2e})")
    assert res <= (target if res_t <= target else MARGIN * res_t)
    assert info["filter"]["res"] <= target and info["filter"]["res"] <= info["filter"]["res0"]
    assert lm.rel(Y, Yr) <= max(MARGIN * rec["y_err"], n * EPS)
    assert np.array_equal(Y, Y.T) and np.linalg.eigvalsh(Y).min() > -n * EPS * np.linalg.norm(Y, 2)


@pytest.mark.parametrize("n", [12, 70])
def test_a_loose_sign_tolerance_is_repaired_by_both_refinements(ctx, n):
    """tol = 1e-3 ends the sign iteration early (model: Y at 4.9e-9 and 2.8e-6 after extraction at n = 12 and 70): the filter's Newton-Kleinman
    steps on the dual closed loop A - E Y Q bring it to the target like the regulator's (model: 1 and 2 steps); max_refine = 0 returns the
    extracted pair as it is.  X stays the single solver's bit for bit."""
    E, A, B, C = lm.system(n)
    target = 100 * n * EPS
    loose = D.MatrixSign(tol=1e-3)
    (X0, Y0), i0 = D.solve_gare_pair(E, A, B, C, D.MatrixSign(tol=1e-3, max_refine=0), ctx=ctx, return_info=True)
    (X, Y), info = D.solve_gare_pair(E, A, B, C, loose, ctx=ctx, return_info=True)
    Xs, single = D.solve(D.GAREProblem(E, A, D.lowrank(B), D.lowrank(np.ascontiguousarray(C.T))), loose, ctx=ctx, return_info=True)
    Xm, Ym, model = lm.gare_pair(E, A, B, C, tol=1e-3)
    _, Yr = lm.reference_xy(n)
    fil, res = info["filter"], _residual_f_extended(E, A, B, C, Y)
    print(f"n={n}: iters {info['iters']} (model {model['iters']}) refinements X {info['regulator']['refinements']} Y {fil['refinements']} (model "
          f"{model['regulator']['refinements']}, {model['filter']['refinements']}) Y: res0 {fil['res0']:.2e} res {fil['res']:.2e} extended {res:.2e} (model "
          f"{model['filter']['res0']:.2e}, {model['filter']['res']:.2e}; target {target:.2e}) |Y - Y_ref| {lm.rel(Y, Yr):.2e} (model {lm.rel(Ym, Yr):.2e})")
    assert np.array_equal(X, Xs) and info["regulator"]["refinements"] == single["refinements"] and info["iters"] == single["iters"] == i0["iters"]
    for side in ("regulator", "filter"):
        assert i0[side]["refinements"] == 0 and i0[side]["res"] == i0[side]["res0"] == info[side]["res0"] > target
        assert 1 <= info[side]["refinements"] <= 2 and info[side]["res"] <= target
    assert res <= target
    assert lm.rel(Y, Yr) <= max(MARGIN * lm.rel(Ym, Yr), n * EPS) < lm.rel(Y0, Yr)


@pytest.mark.parametrize("n,r", CASES)
def test_lqgbt_against_the_reference_chain(ctx, n, r):
    E, A, B, C = lm.system(n)
    rec = REC[str(n)]
    assert rec["order"] == r
    rom, info = _lqgbt(ctx, n, r)
    if n == 371:
        mu_ref, Hr_ref = lm.golden()["mu_371"], lm.golden()["Hr_371"]
    else:
        ref = lm.reference(n, r)
        mu_ref, Hr_ref = ref["mu"], lm.reduced_transfer(ref, lm.omega_of(n))
    assert info["order"] == rom.order == r and info["factorizations"] == 1 and info["iters"] == rec["iters"]
    m, q = B.shape[1], C.shape[0]
    assert rom.Ar.shape == rom.Ac.shape == (r, r) and rom.Br.shape == (r, m) and rom.Cr.shape == (q, r) and rom.T.shape == rom.W.shape == (n, r)
    assert rom.Kr.shape == (m, r) and rom.Lr.shape == (r, q) and np.array_equal(rom.Er, np.eye(r))
    k = min(len(mu_ref), len(rom.mu))
    e_mu = float(np.abs(rom.mu[:k] - mu_ref[:k]).max() / mu_ref[0])
    e_eye = float(np.linalg.norm(rom.W.T @ E @ rom.T - np.eye(r)))
    e_tr = lm.max_norm2(lm.reduced_transfer(_as_dict(rom), lm.omega_of(n)) - Hr_ref) / lm.max_norm2(Hr_ref)
    print(f"n={n} r={r}: iters {info['iters']} refinements {info['regulator']['refinements']}/{info['filter']['refinements']} rank {info['rank']} r_c "
          f"{info['r_c']} r_o {info['r_o']} dropped {info['dropped']} sweeps {info['svd_sweeps']} mu {e_mu:.2e} (model {rec['mu']:.2e}) eye {e_eye:.2e} "
          f"(model {rec['eye']:.2e}; reported {info['eye_err']:.2e}) transfer {e_tr:.2e} (model {rec['transfer']:.2e})")
    assert e_mu <= MARGIN * rec["mu"]
    assert e_eye <= MARGIN * rec["eye"] and info["eye_err"] <= MARGIN * rec["eye"]
    assert e_tr <= MARGIN * rec["transfer"]
    assert (np.diff(rom.mu) <= 0).all() and (rom.mu >= 0).all()
    # the controller is made of the reduced matrices and mu
    Sig = np.diag(rom.mu[:r])
    Ac, Lr, Kr = rom.controller()
    for got, want in ((Kr, rom.Br.T @ Sig), (Lr, Sig @ rom.Cr.T), (Ac, rom.Ar - rom.Br @ Kr - Lr @ rom.Cr)):
        scale = np.linalg.norm(rom.Ar) + np.linalg.norm(rom.Br @ Kr) + np.linalg.norm(Lr @ rom.Cr) if got is Ac else np.linalg.norm(want)
        assert np.linalg.norm(got - want) <= 8 * r * EPS * scale
    assert max(lm.riccati_residuals(_as_dict(rom))) <= MARGIN * max(rec["riccati"], n * EPS)


@pytest.mark.parametrize("n,r", CASES)
def test_the_coprime_factor_bound(ctx, n, r):
    E, A, B, C = lm.system(n)
    rom, info = _lqgbt(ctx, n, r)
    err, bound = D.lqg_error(E, A, B, C, rom, lm.omega_of(n), ctx=ctx)
    print(f"n={n} r={r}: err {err:.4e} bound {bound:.4e} (model err {REC[str(n)]['err']:.4e} bound {REC[str(n)]['bound']:.4e})")
    assert bound == pytest.approx(lm.bound(rom.mu, r), rel=1e-13, abs=0.0) and info["bound"] == pytest.approx(bound, rel=1e-13, abs=0.0)
    assert err <= bound + RESPONSE_ROUNDING


@pytest.mark.parametrize("n,r", [(12, 6), (33, 8), (70, 12), (371, 16)])
def test_the_reduced_controller_stabilises_the_plant(ctx, n, r):
    E, A, B, C = lm.system(n)
    rec = REC[str(n)]
    rom, info = _lqgbt(ctx, n, r)
    absc = lm.closed_loop_abscissa(E, A, B, C, _as_dict(rom))
    print(f"n={n} r={r}: closed-loop abscissa {absc:.6e} (reference {rec['abscissa_ref']:.6e}, model {rec['abscissa']:.6e}; open loop "
          f"{rec['open_loop']:.3f}) bound {info['bound']:.3e} against 1/sqrt(1 + mu_1^2) = {1.0 / np.sqrt(1.0 + rom.mu[0] ** 2):.3e}")
    if n == 371:          # the reference's own abscissa is -2.9e-3: the device's is compared with it, its sign alone says little
        assert abs(absc - rec["abscissa_ref"]) <= MARGIN * abs(rec["abscissa"] - rec["abscissa_ref"])
    else:
        assert absc < 0.0 < rec["open_loop"]


def test_an_unstable_plant_is_reduced_where_balanced_truncation_refuses(ctx):
    E, A, B, C = lm.system(33)
    with pytest.raises(D.DREError) as e:
        D.balanced_truncation(E, A, B, C, order=8, ctx=ctx)
    assert e.value.code == -7
    rom, _ = _lqgbt(ctx, 33, 8)
    assert rom.order == 8 and np.isfinite(rom.Ar).all()


@pytest.mark.parametrize("n", [12, 33, 70])
def test_order_rule(ctx, n):
    rec = REC[str(n)]
    tol, r = rec["tol"], rec["tol_order"]
    mu_ref = lm.reference(n, r)["mu"]
    assert tol == pytest.approx(lm.clear_tol(mu_ref, r), rel=1e-6) and lm.bound(mu_ref, r) <= tol / 1.1 and lm.bound(mu_ref, r - 1) >= 1.1 * tol
    rom, info = D.lqg_balanced_truncation(*lm.system(n), tol=tol, ctx=ctx, return_info=True)
    assert info["order"] == rom.order == r and info["bound"] <= tol
    mu = D.lqg_characteristic_values(*lm.system(n), ctx=ctx)
    assert np.array_equal(mu, rom.mu)


def test_failures_leave_the_context_usable(ctx):
    def alive():
        E, A, B, C = lm.system(12)
        X, Y = D.solve_gare_pair(E, A, B, C, ctx=ctx)
        assert lm.rel(Y, lm.reference_xy(12)[1]) <= max(MARGIN * REC["12"]["y_err"], 12 * EPS)
    # Hamiltonian eigenvalues on the imaginary axis: the shared iteration fails the call
    Eo, Ao, Bo, Co = oscillator_pencil()
    with pytest.raises(D.DREError) as e:
        D.solve_gare_pair(Eo, Ao, Bo, Co, D.MatrixSign(maxiters=25), ctx=ctx)
    assert e.value.code == -7
    alive()
    with pytest.raises(D.DREError) as e:
        D.lqg_balanced_truncation(Eo, Ao, Bo, Co, D.MatrixSign(maxiters=25), ctx=ctx)
    assert e.value.code == -7
    alive()
    # a singular E
    E, A, B, C = (M.copy() for M in lm.system(12))
    E[3, :] = 0.0
    with pytest.raises(D.DREError) as e:
        D.solve_gare_pair(E, A, B, C, ctx=ctx)
    assert e.value.code == -4 and "singular" in str(e.value)
    alive()
    # the memory check comes before any kernel: (1000 + 37) n^2 doubles at n = 8000 are 530 GB
    n = 8000
    with pytest.raises(D.DREError) as e:
        D.solve_gare_pair(np.eye(n), -np.eye(n), np.ones((n, 1)), np.ones((1, n)), D.MatrixSign(maxiters=1000), ctx=ctx)
    assert e.value.code == -3
    alive()
    # an order above the numerical rank
    with pytest.raises(D.DREError) as e:
        D.lqg_balanced_truncation(*lm.system(12), order=13, ctx=ctx)
    assert e.value.code == -1 and "lqg_balance" in str(e.value) and "numerical rank" in str(e.value)
    alive()
