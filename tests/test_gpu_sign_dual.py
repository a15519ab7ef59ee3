"""Dual solves on a kept sign factorisation on the device (SignFactorization.solve_dense / solve_lr with transposed=True, solve_gale_pair):
F Y E' + E Y F' = -R from the factorisation of (F, E), against oracle.lyap_dense(F', E', R), against a fresh factorisation of (F', E'), and
against the NumPy model (tests/_sign_dual_model.py).  The pencils are non-symmetric in E and F (tests/_sign_dual_cases.py): on a symmetric
pencil the dual equals the primal and a wrong transposition would pass.

No bound here is a fixed number: each is MARGIN = 10 times the model's distance to the same reference for the same input (DESIGN.md §9.2's
rule), computed on the CPU; a distance between two device results is bounded by the sum of their two bounds to the common reference.
Measured device values: DESIGN.md §9.7."""
import numpy as np
import pytest

import dre_amd as D
import dre_oracle as o
import _sign_dual_cases as cs
import _sign_dual_model as dm
import _factored_sign_model as fm

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
MARGIN = 10.0


def _dense_dual_checks(ctx, n, what):
    """one dense dual solve on a fresh handle of pencil(n) against the oracle; returns the handle's pieces for further checks"""
    E, F, _, _ = cs.pencil(n)
    R = cs.rhs(n)[2]
    m = cs.model(n)
    Ym, _, _, res_m = cs.model_dual(n)
    Yo = cs.oracle(n)
    bound = MARGIN * o.delta(Ym, Yo)
    sign = D.SignFactorization(E, F, ctx=ctx)
    Y, info = sign.solve_dense(R, transposed=True)
    dist = D.delta(Y, Yo)
    target = 100 * n * EPS
    print(f"{what} n={n}: iters {info['iters']} (model {m.iters}) refinements {info['refinements']} res0 {info['res0']:.2e} res {info['res']:.2e} "
          f"(model {res_m:.2e}) d_oracle {dist:.2e} (model {bound / MARGIN:.2e}, bound {bound:.2e})")
    assert info["iters"] == m.iters
    assert dist < bound
    assert info["res"] <= MARGIN * max(res_m, target)
    assert np.array_equal(Y, Y.T)
    return sign, R, Y, Yo, bound


@pytest.mark.parametrize("n", [33, 70, 371])
def test_dense_dual_against_oracle_and_a_factorisation_of_the_transposed_pencil(ctx, n):
    E, F, _, _ = cs.pencil(n)
    sign, R, Y, Yo, bound = _dense_dual_checks(ctx, n, "dense dual")
    X, _ = sign.solve_dense(R)
    sign.close()
    # today's only way: a second factorisation, of (F', E'), and its primal replay
    signT = D.SignFactorization(E.T.copy(), F.T.copy(), ctx=ctx)
    Yt, _ = signT.solve_dense(R)
    signT.close()
    bound_t = MARGIN * o.delta(cs.model_of_transposed_pencil(n).solve(R)[0], Yo)
    d_t, d_primal = D.delta(Y, Yt), D.delta(X, Yo)
    print(f"n={n}: d(dual, primal of the transposed pencil) {d_t:.2e} (bound {bound + bound_t:.2e}); the primal replay against the dual oracle {d_primal:.2e}")
    assert d_t < bound + bound_t
    assert d_primal > 1e3 * bound                     # the primal solution is not the dual one on this pencil


def test_primal_dual_primal_leaves_the_kept_state_alone(ctx):
    n = 70
    E, F, _, _ = cs.pencil(n)
    R = cs.rhs(n)[2]
    sign = D.SignFactorization(E, F, ctx=ctx)
    X1, _ = sign.solve_dense(R)
    Y1, _ = sign.solve_dense(R, transposed=True)
    X2, _ = sign.solve_dense(R)
    Y2, _ = sign.solve_dense(R, transposed=True)
    G, S, _ = cs.rhs(n, [0, 8])
    L1, D1, _ = sign.solve_lr(G, S)
    sign.solve_lr(G, S, transposed=True)
    L2, D2, _ = sign.solve_lr(G, S)
    sign.close()
    assert np.array_equal(X1.view(np.uint64), X2.view(np.uint64)) and np.array_equal(Y1.view(np.uint64), Y2.view(np.uint64))
    assert np.array_equal(L1.view(np.uint64), L2.view(np.uint64)) and np.array_equal(D1.view(np.uint64), D2.view(np.uint64))


def test_dense_dual_refines_once_after_a_loose_sign_iteration(ctx):
    n = 70
    E, F, _, _ = cs.pencil(n)
    R = cs.rhs(n)[2]
    m = cs.model(n, 1e-3)
    Ym, steps, r0m, r1m = cs.model_dual(n, 1e-3, 1)
    Yo = cs.oracle(n)
    bound = MARGIN * o.delta(Ym, Yo)
    sign = D.SignFactorization(E, F, tol=1e-3, ctx=ctx)
    Y0, info0 = sign.solve_dense(R, max_refine=0, transposed=True)
    Y, info = sign.solve_dense(R, max_refine=1, transposed=True)
    sign.close()
    dist = D.delta(Y, Yo)
    print(f"loose tol: iters {info['iters']} (model {m.iters}) res0 {info['res0']:.2e} -> res {info['res']:.2e} (model {r0m:.2e} -> {r1m:.2e}) "
          f"d_oracle {D.delta(Y0, Yo):.2e} -> {dist:.2e} (model {bound / MARGIN:.2e}, bound {bound:.2e})")
    assert steps == 1 and info["iters"] == m.iters
    assert info0["refinements"] == 0 and info["refinements"] == 1
    assert info["res0"] == info0["res0"] > 100 * n * EPS
    assert info["res"] <= MARGIN * r1m
    assert dist < bound


def test_dense_dual_on_the_tournament_panel_factorisation(ctx):
    before = ctx.get_option("dense_gj_panel")
    ctx.set_option("dense_gj_panel", 2)
    try:
        sign = _dense_dual_checks(ctx, 70, "dense_gj_panel = 2")[0]
        sign.close()
    finally:
        ctx.set_option("dense_gj_panel", before)


LR_CASES = [((0,), 256, 1), ((0, 8), 2, 1), ((0, 8), 4096, 0), ((0, 8), 4096, 1), (None, 256, 0), (None, 256, 1)]


@pytest.mark.parametrize("cols,cap,max_refine", LR_CASES, ids=["r1", "r2-cap2", "r2-cap-never-reached-norefine", "r2-cap-never-reached", "r11-norefine", "r11"])
def test_factored_dual_against_the_dense_dual_replay_the_oracle_and_the_model(ctx, cols, cap, max_refine):
    n = 371
    E, F, _, _ = cs.pencil(n)
    G, S, R = cs.rhs(n, None if cols is None else list(cols))
    r = G.shape[1]
    m = cs.model(n)
    rtol = fm.default_rtol(n)
    Lm, Dm, st = dm.factored_sign_lyap_t(m, G, S, rtol, cap, max_refine)
    Ym = Lm @ Dm @ Lm.T
    Yo = cs.oracle(n, cols)
    bound_dense, bound_or = MARGIN * o.delta(Ym, dm.replay_t(m, R)), MARGIN * o.delta(Ym, Yo)
    sign = D.SignFactorization(E, F, ctx=ctx)
    L, Dd, info = sign.solve_lr(G, S, rtol, cap, max_refine, transposed=True)
    Yd, _ = sign.solve_dense(R, max_refine=0, transposed=True)          # the dense dual replay on the same handle
    sign.close()
    Y = L @ Dd @ L.T
    d_dense, d_or = D.delta(Y, Yd), D.delta(Y, Yo)
    res = np.linalg.norm(dm.residual_t(m, Y, R)) / np.linalg.norm(R)
    print(f"r={r} cap {cap} max_refine {max_refine}: rank {info['rank']} (model {st['rank']}) peak {info['peak_width']} (model {st['peak_width']}) "
          f"compressions {info['compressions']} (model {st['compressions']}) refinements {info['refinements']} (model {st['refinements']}) "
          f"res0 {info['res0']:.2e} res {info['res']:.2e} (model {st['res0']:.2e} / {st['res']:.2e}) independent res {res:.2e} "
          f"d_dense {d_dense:.2e} (bound {bound_dense:.2e}) d_oracle {d_or:.2e} (bound {bound_or:.2e})")
    assert L.shape == (n, info["rank"]) and np.count_nonzero(Dd - np.diag(np.diag(Dd))) == 0
    if r > 1:
        assert (np.diag(S) < 0).any() and (np.diag(Dd) < 0).any() and (np.diag(Dd) > 0).any()          # indefinite in, indefinite out
    assert d_dense < bound_dense and d_or < bound_or
    assert info["iters"] == m.iters and abs(info["rank"] - st["rank"]) <= 2
    assert info["refinements"] <= max_refine
    target = 100 * n * EPS + 10 * rtol
    assert res <= MARGIN * max(st["res"], target) and info["res"] <= MARGIN * max(st["res"], target)
    if cap == 2:
        assert info["compressions"] >= m.iters                            # one compression per iteration
    if cap == 4096:
        assert r * 2 ** m.iters <= cap and info["peak_width"] >= r * 2 ** m.iters >= n       # never reached; the one compression is QR-free


def test_factored_dual_failure_paths_leave_the_context_usable(ctx):
    n = 33
    E, F, G, S = cs.pencil(n)
    sign = D.SignFactorization(E, F, ctx=ctx)
    for kw in (dict(max_width=3), dict(max_width=0), dict(rtol=0.0), dict(rtol=1.0), dict(max_refine=-1), dict(max_width=5000)):
        with pytest.raises(D.DREError) as e:
            sign.solve_lr(G, S, transposed=True, **kw)
        assert e.value.code == -1, kw
    with pytest.raises(D.DREError) as e:
        sign.solve_dense(np.eye(n + 1), transposed=True)
    assert e.value.code == -1
    L0, D0, info = sign.solve_lr(np.zeros((n, 0)), np.zeros((0, 0)), transposed=True)
    assert L0.shape == (n, 0) and info["rank"] == 0 and info["compressions"] == 0
    L, Dd, _ = sign.solve_lr(G, S, transposed=True)                         # the handle and the context still work
    sign.close()
    Lm, Dm, _ = dm.factored_sign_lyap_t(cs.model(n), G, S)
    assert D.delta(L @ Dd @ L.T, cs.oracle(n)) < MARGIN * o.delta(Lm @ Dm @ Lm.T, cs.oracle(n))


def test_solve_gale_pair_matrix_sign(ctx):
    n = 70
    E, F, _, _ = cs.pencil(n)
    R_obs, R_ctr = cs.rhs(n)[2], cs.rhs(n, [0, 8])[2]
    m, mt = cs.model(n), cs.model_of_transposed_pencil(n)
    Xo, Yo = cs.oracle(n, None, False), cs.oracle(n, (0, 8))
    bX, bY = MARGIN * o.delta(m.solve(R_obs)[0], Xo), MARGIN * o.delta(dm.solve_t(m, R_ctr)[0], Yo)
    bYs = MARGIN * o.delta(mt.solve(R_ctr)[0], Yo)
    (X, Y), info = D.solve_gale_pair(E, F, R_obs, D.lowrank(*cs.rhs(n, [0, 8])[:2]), D.MatrixSign(), return_info=True)
    Xs = D.solve_gale_dense(D.GALEProblem(E, F, R_obs), D.MatrixSign())
    Ys = D.solve_gale_dense(D.GALEProblem(E.T.copy(), F.T.copy(), R_ctr), D.MatrixSign())
    print(f"pair MatrixSign: X d_oracle {D.delta(X, Xo):.2e} (bound {bX:.2e}) d_single {D.delta(X, Xs):.2e}; "
          f"Y d_oracle {D.delta(Y, Yo):.2e} (bound {bY:.2e}) d_single {D.delta(Y, Ys):.2e} (bound {bY + bYs:.2e}); {info}")
    assert info["factorizations"] == 1 and info["primal"]["iters"] == info["dual"]["iters"] == m.iters
    assert D.delta(X, Xo) < bX and D.delta(Y, Yo) < bY
    assert D.delta(X, Xs) < 2 * bX and D.delta(Y, Ys) < bY + bYs


def test_solve_gale_pair_factored_sign(ctx):
    n = 371
    E, F, _, _ = cs.pencil(n)
    (G1, S1, R1), (G2, S2, R2) = cs.rhs(n), cs.rhs(n, [0, 8])
    m, mt = cs.model(n), cs.model_of_transposed_pencil(n)
    Xo, Yo = cs.oracle(n, None, False), cs.oracle(n, (0, 8))
    alg = D.FactoredSign()
    rtol = fm.default_rtol(n)
    dense = lambda t: t[0] @ t[1] @ t[0].T
    bX = MARGIN * o.delta(dense(fm.factored_sign_lyap(m, G1, S1, rtol, alg.max_width, alg.max_refine)), Xo)
    bY = MARGIN * o.delta(dense(dm.factored_sign_lyap_t(m, G2, S2, rtol, alg.max_width, alg.max_refine)), Yo)
    bYs = MARGIN * o.delta(dense(fm.factored_sign_lyap(mt, G2, S2, rtol, alg.max_width, alg.max_refine)), Yo)
    (X, Y), info = D.solve_gale_pair(E, F, D.lowrank(G1, S1), D.lowrank(G2, S2), alg, return_info=True)
    Xs = D.solve(D.GALEProblem(E, F, D.lowrank(G1, S1)), alg)
    Ys = D.solve(D.GALEProblem(E.T.copy(), F.T.copy(), D.lowrank(G2, S2)), alg)
    assert all(isinstance(Z, D.LDLt) for Z in (X, Y, Xs, Ys))
    Xd, Yd = X.dense(), Y.dense()
    print(f"pair FactoredSign: X rank {X.rank()} d_oracle {D.delta(Xd, Xo):.2e} (bound {bX:.2e}) d_single {D.delta(Xd, Xs.dense()):.2e}; "
          f"Y rank {Y.rank()} d_oracle {D.delta(Yd, Yo):.2e} (bound {bY:.2e}) d_single {D.delta(Yd, Ys.dense()):.2e} (bound {bY + bYs:.2e}); {info}")
    assert info["factorizations"] == 1 and info["primal"]["rank"] == X.rank() and info["dual"]["rank"] == Y.rank()
    assert D.delta(Xd, Xo) < bX and D.delta(Yd, Yo) < bY
    assert D.delta(Xd, Xs.dense()) < 2 * bX and D.delta(Yd, Ys.dense()) < bY + bYs
