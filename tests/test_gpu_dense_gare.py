"""Dense GARE solver on the device: solve(GAREProblem, MatrixSign()) (csrc/dense_are.hip) against SciPy's generalized
solve_continuous_are, the Kleinman-Newton fixture, the low-rank Newton-ADI path and the NumPy model (tests/_hamiltonian_sign_model.py).
Tolerances follow the model's measured figures (tests/test_dense_gare_host.py) with the slack stated at each assertion."""
import os
import warnings

import numpy as np
import pytest
import scipy.linalg as sla

import dre_amd as D
import _hamiltonian_sign_model as hm
from conftest import GOLDEN
from test_dense_gare_host import closed_loop_max_real, oscillator_pencil, spd, steel_dense, unstable_variant

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps


def _are(E, A, B, C, beta=1.0, Rinv=None, gamma=1.0, S=None):
    Rinv = np.eye(B.shape[1]) if Rinv is None else Rinv
    S = np.eye(C.shape[0]) if S is None else S
    return D.GAREProblem(E, A, beta * D.lowrank(B, Rinv), gamma * D.lowrank(np.ascontiguousarray(C.T), S))


def _dense_gq(are):
    (b, B, R), (g, Ct, S) = are.G, are.Q
    return b * B @ R @ B.T, g * Ct @ S @ Ct.T


def _scaled_residual(E, A, G, Q, X):
    return hm.residual(E, A, G, Q, X)[1]


@pytest.fixture(scope="module")
def steel():
    return steel_dense(371)


def test_steel_profile_371(ctx, steel):
    E, A, B, C = steel
    are = _are(E, A, B, C)
    X, info = D.solve(are, D.MatrixSign(), return_info=True)
    G, Q = _dense_gq(are)
    assert 10 <= info["iters"] <= 20 and info["res"] <= 100 * 371 * EPS
    Xr = sla.solve_continuous_are(A, B, Q, np.eye(B.shape[1]), e=E)
    assert D.delta(X, Xr) < 1e-10                      # model: 1.4e-12
    g = np.load(os.path.join(GOLDEN, "gare_371.npz"))
    assert D.delta(info["K"], g["K_dense"]) < 1e-7
    # the device residual agrees with a NumPy evaluation of the same formula
    R = D.residual(are, X)
    XE = X @ E
    Rn = Q + A.T @ XE + XE.T @ A - XE.T @ G @ XE
    scale = np.linalg.norm(Q) + 2 * np.linalg.norm(A.T @ XE) + np.linalg.norm(XE.T @ G @ XE)
    assert np.linalg.norm(R - Rn) <= 1e-13 * scale
    assert np.array_equal(R, R.T)
    # an LDLᵀ X still takes the low-rank residual
    assert isinstance(D.residual(are, D.lowrank(np.zeros((371, 0)), np.zeros((0, 0)))), D.LDLt)


def test_unstable_plant(ctx, steel):
    E, A, B, C = steel
    Au = unstable_variant(E, A)
    are = _are(E, Au, B, C)
    X, info = D.solve(are, D.MatrixSign(), return_info=True)
    G, Q = _dense_gq(are)
    assert info["res"] <= 100 * 371 * EPS and _scaled_residual(E, Au, G, Q, X) <= 100 * 371 * EPS
    assert closed_loop_max_real(E, Au, G, X) < 0
    Xr = sla.solve_continuous_are(Au, B, Q, np.eye(B.shape[1]), e=E)
    assert D.delta(X, Xr) < 1e-10                      # model: 1e-13


def test_scaled_inner_matrices(ctx, steel):
    E, A, B, C = steel
    beta, gamma = 2.5, 0.7
    Rinv, S = spd(B.shape[1], 1), spd(C.shape[0], 2)
    are = _are(E, A, B, C, beta, Rinv, gamma, S)
    X, info = D.solve(are, D.MatrixSign(), return_info=True)
    G, Q = _dense_gq(are)
    Xr = sla.solve_continuous_are(A, B, Q, np.linalg.inv(beta * Rinv), e=E)
    assert D.delta(X, Xr) < 1e-10
    assert np.allclose(info["K"], beta * Rinv @ B.T @ X @ E, rtol=1e-12, atol=0)
    # the model reaches the same X
    Xm, _ = hm.gare_sign(E, A, G, Q)
    assert D.delta(X, Xm) < 1e-10


def test_tiny_system_and_imaginary_axis(ctx):
    rng = np.random.default_rng(11)
    n = 10                                              # the size of the reference's test/cuda.jl
    E = np.eye(n) + 0.1 * rng.standard_normal((n, n))
    A = rng.standard_normal((n, n)) @ E                 # generic: some unstable modes
    B, C = rng.standard_normal((n, 2)), rng.standard_normal((3, n))
    are = _are(E, A, B, C)
    X, info = D.solve(are, D.MatrixSign(), return_info=True)
    G, Q = _dense_gq(are)
    assert sla.eigvals(A, E).real.max() > 0
    assert _scaled_residual(E, A, G, Q, X) <= 100 * n * EPS
    assert closed_loop_max_real(E, A, G, X) < 0
    Xm, _ = hm.gare_sign(E, A, G, Q)
    assert D.delta(X, Xm) < 1e-10
    # uncontrollable and unobservable oscillator: the Hamiltonian has eigenvalues +-i, the iteration does not converge
    Eo, Ao, Bo, Co = oscillator_pencil()
    with pytest.raises(D.DREError) as e:
        D.solve(_are(Eo, Ao, Bo, Co), D.MatrixSign(maxiters=25))
    assert e.value.code == -7


def test_newton_kleinman_refinement(ctx, steel):
    """A loose sign tolerance leaves X at a scaled residual of about 2e-9 (model: 1.8e-9 after 12 iterations); one Newton-Kleinman step
    brings it below 100 n eps (model: 3e-15).  max_refine = 0 returns the extracted X as it is."""
    E, A, B, C = steel
    Au = unstable_variant(E, A)
    are = _are(E, Au, B, C)
    G, Q = _dense_gq(are)
    X0, i0 = D.solve(are, D.MatrixSign(tol=1e-3, max_refine=0), return_info=True)
    assert i0["refinements"] == 0 and i0["res"] == i0["res0"] > 100 * 371 * EPS
    X, info = D.solve(are, D.MatrixSign(tol=1e-3), return_info=True)
    assert info["iters"] == i0["iters"] and info["res0"] == i0["res0"]
    assert 1 <= info["refinements"] <= 2 and info["res"] <= 100 * 371 * EPS
    assert _scaled_residual(E, Au, G, Q, X) <= 100 * 371 * EPS
    Xr = sla.solve_continuous_are(Au, B, Q, np.eye(B.shape[1]), e=E)
    assert D.delta(X, Xr) < 1e-10 < D.delta(X0, Xr)


def test_tournament_panel_1357(ctx):
    E, A, B, C = steel_dense(1357)
    before = ctx.get_option("dense_gj_panel")
    ctx.set_option("dense_gj_panel", 2)                 # the 2714-order inversions take the tournament panel
    try:
        are = _are(E, A, B, C)
        X, info = D.solve(are, D.MatrixSign(), return_info=True)
    finally:
        ctx.set_option("dense_gj_panel", before)
    G, Q = _dense_gq(are)
    assert info["res"] <= 100 * 1357 * EPS and _scaled_residual(E, A, G, Q, X) <= 100 * 1357 * EPS
    assert closed_loop_max_real(E, A, G, X) < 0


def test_5177_against_lowrank_newton(ctx):
    d = D.steel_profile(5177)
    are = D.GAREProblem(d.E, d.A, D.lowrank(d.B), D.lowrank(np.ascontiguousarray(d.C.T)))
    X, info = D.solve(are, D.MatrixSign(), return_info=True)
    assert info["res"] <= 100 * 5177 * EPS
    S = D.Shifts
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        XL, linfo = D.solve(are, D.Newton(D.ADI(maxiters=200, ignore_initial_guess=True, shifts=S.Cyclic(S.Heuristic(20, 30, 30))), maxiters=20,
                                          reltol=1e-10), return_info=True)
    assert linfo["converged"]
    KL = D.api.gare_feedback(are, XL)
    # two independent algorithms; the low-rank Newton stops at a relative residual of 1e-10, which bounds K's difference at about 1e-8
    # (measured on one MI355X: 9.8e-13, 18 sign iterations, scaled residual 2.4e-12 without refinement)
    assert D.delta(info["K"], KL) < 1e-8


def test_memory_check_before_any_kernel(ctx):
    n = 8000
    E, A = np.eye(n), -np.eye(n)
    are = _are(E, A, np.ones((n, 1)), np.ones((1, n)))
    # the refinement's SignLyap keeps maxiters n x n matrices: (1000 + 36) n^2 doubles = 530 GB, far above the device's memory
    with pytest.raises(D.DREError) as e:
        D.solve(are, D.MatrixSign(maxiters=1000))
    assert e.value.code == -3
