"""Dense path beyond n = 4096: the tournament-pivoting Gauss-Jordan panel (csrc/dense_gj.hip, k_gj_tslu) through dre_dense_invert, the
matrix-sign GALE solver and dense Ros1 at SteelProfile(5177) against the committed low-rank fixture (the reference's dense == low-rank
criterion, test/rail.jl:52-70), the forced tournament panel against the dense fixtures of the register panel, and the option dense_gj_panel."""
import os
from contextlib import contextmanager

import numpy as np
import pytest

import dre_amd as D
import _tslu_model as tm
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
MS = D.MatrixSign(maxiters=40)


@contextmanager
def _panel(ctx, v):
    before = ctx.get_option("dense_gj_panel")
    ctx.set_option("dense_gj_panel", v)
    try:
        yield
    finally:
        ctx.set_option("dense_gj_panel", before)


def _check_inverse(A, X, ld):
    n = A.shape[0]
    r = np.linalg.norm(A @ X - np.eye(n)) / (np.linalg.norm(A) * np.linalg.norm(X))
    assert r <= 100 * n * EPS, r
    s, ldn = np.linalg.slogdet(A)
    assert s != 0 and abs(ld - ldn) <= 1e-12 * abs(ldn)


def _random(n, seed):
    return np.random.default_rng(seed).standard_normal((n, n)) + 2.0 * np.eye(n)


@pytest.mark.parametrize("n", [4097, 5177])
def test_dense_invert_above_the_register_limit(ctx, n):
    with _panel(ctx, 0):
        A = _random(n, n)
        X, piv, ld = D.dense_invert(A)
        _check_inverse(A, X, ld)
        assert all(piv >= np.arange(n))


@pytest.mark.parametrize("n", [371, 1357])
def test_dense_invert_forced_tournament(ctx, n):
    with _panel(ctx, 2):
        A = _random(n, n)
        X, piv, ld = D.dense_invert(A)
    _check_inverse(A, X, ld)


@pytest.mark.parametrize("n,panel", [(1357, 2), (4097, 0)])
def test_dense_invert_pivot_sequence_is_the_models(ctx, n, panel):
    A = tm.pivot_forcing(n)
    with _panel(ctx, panel):
        X, piv, ld = D.dense_invert(A)
    Xm, pm, ldm, sing = tm.tslu_invert(A)
    assert not sing and np.array_equal(piv, pm)
    assert np.array_equal(X, Xm) and ld == 0.0 == ldm


def test_singular_at_4500_and_recovery(ctx):
    n = 4500
    with _panel(ctx, 0):
        A = _random(n, 1)
        Az = A.copy(); Az[:, 3001] = 0.0                  # a zero column
        with pytest.raises(D.DREError) as e:
            D.dense_invert(Az)
        assert e.value.code == -4
        Ae = A.copy(); Ae[:, 11] = Ae[:, 10]              # two equal columns
        with pytest.raises(D.DREError) as e:
            D.dense_invert(Ae)
        assert e.value.code == -4
        B = _random(300, 2)                               # the context still works
        X, _, ld = D.dense_invert(B)
        _check_inverse(B, X, ld)


def test_option_handling(ctx, steel5177):
    before = ctx.get_option("dense_gj_panel")
    assert before == 0.0
    for bad in (-1, 3, 0.5):
        with pytest.raises(D.DREError) as e:
            ctx.set_option("dense_gj_panel", bad)
        assert e.value.code == -1
    assert ctx.get_option("dense_gj_panel") == before
    with _panel(ctx, 1):
        assert ctx.get_option("dense_gj_panel") == 1.0
        with pytest.raises(D.DREError) as e:
            D.dense_invert(_random(5177, 3))
        assert e.value.code == -1
        d = steel5177[0]
        E, A, R = d.E.toarray(), d.A.toarray(), d.C.T @ d.C
        with pytest.raises(D.DREError) as e:
            D.solve_gale_dense(D.GALEProblem(E, A - E / 200.0, R), MS)
        assert e.value.code == -1
    assert ctx.get_option("dense_gj_panel") == before


@pytest.fixture(scope="module")
def steel5177():
    d = D.steel_profile(5177)
    L, Dm = D.initial_value(d)
    return d, L, Dm


def test_gale_dense_5177(ctx, steel5177):
    d, _, _ = steel5177
    n = 5177
    E, A, R = d.E.toarray(), d.A.toarray(), d.C.T @ d.C
    F = A - E / 200.0
    with _panel(ctx, 0):
        X, info = D.solve_gale_dense(D.GALEProblem(E, F, R), MS, return_info=True)
    assert info["res"] <= 100 * n * EPS
    T = F.T @ (X @ E)
    assert np.linalg.norm(R + T + T.T) / np.linalg.norm(R) <= 100 * n * EPS
    assert np.isfinite(X).all()


def test_ros1_dense_5177_matches_the_lowrank_fixture(ctx, steel5177):
    """dense Ros1(MatrixSign()) at SteelProfile(5177) against the low-rank oracle fixture of test_gpu_r02_configs: sampled columns of K,
    ||K||_F and a seeded functional, each within 1e-7"""
    d, L, Dm = steel5177
    g = np.load(os.path.join(GOLDEN, "ros1_5177.npz"))
    X0 = D.lowrank(L, Dm).dense()
    with _panel(ctx, 0):
        sol = D.solve(D.GDREProblem(d.E, d.A, d.B, d.C, X0, (4500.0, 4200.0)), D.Ros1(MS), dt=-100.0, save_state=True)
    assert len(sol.K) == 4 and np.allclose(sol.t, g["t"])
    n = sol.K[0].shape[1]
    w = np.random.default_rng(1).standard_normal(n)
    for i, K in enumerate(sol.K):
        assert np.linalg.norm(K[:, ::16] - g["K_cols"][i]) < 1e-7 * g["K_norm"][i]
        assert abs(np.linalg.norm(K) - g["K_norm"][i]) <= 1e-7 * g["K_norm"][i]
        assert np.linalg.norm(K @ w - g["K_w"][i]) <= 1e-7 * max(np.linalg.norm(g["K_w"][i]), 1e-300)
    Es = d.E.tocsr()
    for X, K in zip(sol.X, sol.K):
        KX = (Es.T @ (X @ d.B)).T                         # K = B'XE
        assert np.linalg.norm(K - KX) <= 1e-12 * np.linalg.norm(K)


@pytest.fixture(scope="module")
def rail371():
    d = D.steel_profile(371)
    L, Dm = D.initial_value(d)
    return d, L, Dm, D.lowrank(L, Dm).dense()


@pytest.mark.parametrize("name,Ros,order", [("ros1_371_full", D.Ros1, 1), ("ros2_371_full", D.Ros2, 2)])
def test_forced_tournament_reproduces_the_dense_fixtures(ctx, rail371, name, Ros, order):
    d, L, Dm, X0 = rail371
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    prob = D.GDREProblem(d.E, d.A, d.B, d.C, X0, (4500.0, 0.0))
    with _panel(ctx, 0):
        _, st0 = D.solve(prob, Ros(D.MatrixSign()), dt=-100.0, return_stats=True)
    with _panel(ctx, 2):
        sol, st = D.solve(prob, Ros(D.MatrixSign()), dt=-100.0, return_stats=True)
    assert len(sol.K) == 46
    for i in range(46):
        assert D.delta(sol.K[i], g["K_dense"][i]) < 1e-10, i
    it0 = np.array([s["iters"] for s in st0["solves"]])
    it = np.array([s["iters"] for s in st["solves"]])
    assert np.abs(it - it0).max() <= 1


def test_forced_tournament_agrees_with_the_register_panel_at_1357(ctx):
    d = D.steel_profile(1357)
    E, A, R = d.E.toarray(), d.A.toarray(), d.C.T @ d.C
    F = A - E / 200.0
    with _panel(ctx, 0):
        X0, i0 = D.solve_gale_dense(D.GALEProblem(E, F, R), D.MatrixSign(), return_info=True)
    with _panel(ctx, 2):
        X2, i2 = D.solve_gale_dense(D.GALEProblem(E, F, R), D.MatrixSign(), return_info=True)
    assert D.delta(X2, X0) < 1e-12
    assert abs(i2["iters"] - i0["iters"]) <= 1
