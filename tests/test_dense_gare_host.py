"""Dense GARE solver, host side: the NumPy model of the device's Hamiltonian sign iteration, extraction and Newton-Kleinman refinement
(tests/_hamiltonian_sign_model.py) against SciPy's generalized solve_continuous_are, plus the dispatch rules of solve() that need no device."""
import numpy as np
import pytest
import scipy.linalg as sla

import dre_amd as D
import _hamiltonian_sign_model as hm

EPS = np.finfo(float).eps


def steel_dense(n=371):
    d = D.steel_profile(n)
    return d.E.toarray(), d.A.toarray(), np.asarray(d.B, dtype=float), np.asarray(d.C, dtype=float)


def unstable_variant(E, A):
    """A - 1.001 lambda_5 E: the five rightmost eigenvalues of (A, E) (all real for SteelProfile) move into the right half plane."""
    lam = np.sort(sla.eigvals(A, E).real)[::-1]
    return A - 1.001 * lam[4] * E


def oscillator_pencil(n=10, seed=7):
    """A pencil with an uncontrollable and unobservable oscillator (eigenvalues +-i of (A, E)), hidden by a random similarity: the
    Hamiltonian has eigenvalues on the imaginary axis."""
    rng = np.random.default_rng(seed)
    A0 = np.zeros((n, n))
    A0[0, 1], A0[1, 0] = 1.0, -1.0
    A0[2:, 2:] = np.diag(-rng.uniform(0.5, 3.0, n - 2)) + np.triu(rng.standard_normal((n - 2, n - 2)), 1)
    B0 = np.zeros((n, 2))
    B0[2:] = rng.standard_normal((n - 2, 2))
    C0 = np.zeros((2, n))
    C0[:, 2:] = rng.standard_normal((2, n - 2))
    T = np.eye(n) + 0.3 * rng.standard_normal((n, n))
    E = np.eye(n) + 0.1 * rng.standard_normal((n, n))
    return E, E @ T @ A0 @ np.linalg.inv(T), E @ T @ B0, C0 @ np.linalg.inv(T)


def spd(k, seed):
    M = np.random.default_rng(seed).standard_normal((k, k))
    return M @ M.T + k * np.eye(k)


def closed_loop_max_real(E, A, G, X):
    return sla.eigvals(A - G @ X @ E, E).real.max()


@pytest.fixture(scope="module")
def steel():
    return steel_dense()


def test_steel_profile_against_scipy(steel):
    E, A, B, C = steel
    G, Q = B @ B.T, C.T @ C
    X, info = hm.gare_sign(E, A, G, Q)
    # measured: 14 sign iterations, scaled residual 7e-14 after extraction (no refinement needed), 1.4e-12 from SciPy
    assert 10 <= info["iters"] <= 20
    assert info["res"] <= hm.refine_target(371)
    Xr = sla.solve_continuous_are(A, B, Q, np.eye(B.shape[1]), e=E)
    assert np.linalg.norm(X - Xr) / np.linalg.norm(Xr) < 1e-10
    assert closed_loop_max_real(E, A, G, X) < 0


def test_unstable_plant_against_scipy(steel):
    E, A, B, C = steel
    Au = unstable_variant(E, A)
    lam = sla.eigvals(Au, E)
    unstable = lam[lam.real > 0]
    assert len(unstable) == 5
    for mu in unstable:                     # Hautus: rank [A - mu E, B] = n on every unstable mode, i.e. (A, B, E) is stabilizable
        s = np.linalg.svd(np.hstack([Au - mu * E, B]), compute_uv=False)
        assert s[-1] > 1e-8 * s[0]
    G, Q = B @ B.T, C.T @ C
    X, info = hm.gare_sign(E, Au, G, Q)
    # measured: 14 iterations, scaled residual 3e-13 after extraction, 1e-13 from SciPy
    assert info["res"] <= hm.refine_target(371)
    Xr = sla.solve_continuous_are(Au, B, Q, np.eye(B.shape[1]), e=E)
    assert np.linalg.norm(X - Xr) / np.linalg.norm(Xr) < 1e-10
    assert closed_loop_max_real(E, Au, G, X) < 0


def test_scaled_inner_matrices_against_scipy(steel):
    E, A, B, C = steel
    beta, gamma = 2.5, 0.7
    Rinv, S = spd(B.shape[1], 1), spd(C.shape[0], 2)
    G, Q = beta * B @ Rinv @ B.T, gamma * C.T @ S @ C
    X, info = hm.gare_sign(E, A, G, Q)
    assert info["res"] <= hm.refine_target(371)
    # SciPy's R is (beta R^-1)^-1; its s= is a cross term, so Q is passed densely
    Xr = sla.solve_continuous_are(A, B, Q, np.linalg.inv(beta * Rinv), e=E)
    assert np.linalg.norm(X - Xr) / np.linalg.norm(Xr) < 1e-10


@pytest.mark.parametrize("seed", [0, 2, 3])
def test_random_unstable_pencils_refinement(seed):
    """30 x 30 pencils with ten unstable modes: the extraction alone leaves 1e-8 .. 1e-10 (measured), Newton-Kleinman brings it down;
    the criterion is the scaled residual plus closed-loop stability (SciPy's generalized solver refuses these pencils)."""
    rng = np.random.default_rng(seed)
    n = 30
    E = np.eye(n) + 0.1 * rng.standard_normal((n, n))
    V = rng.standard_normal((n, n))
    lam = np.concatenate([rng.uniform(0.2, 2.0, 10), -rng.uniform(0.2, 3.0, n - 10)])
    A = E @ V @ np.diag(lam) @ np.linalg.inv(V)
    B, C = rng.standard_normal((n, 3)), rng.standard_normal((2, n))
    G, Q = B @ B.T, C.T @ C
    X, info = hm.gare_sign(E, A, G, Q)
    assert info["refinements"] >= 1 and info["res"] < info["res0"]
    assert info["res"] < 1e-10
    assert closed_loop_max_real(E, A, G, X) < 0


def test_loose_tolerance_is_repaired_by_refinement(steel):
    E, A, B, C = steel
    Au = unstable_variant(E, A)
    G, Q = B @ B.T, C.T @ C
    X0, i0 = hm.gare_sign(E, Au, G, Q, tol=1e-3, max_refine=0)
    X, info = hm.gare_sign(E, Au, G, Q, tol=1e-3)
    # measured: 12 iterations, 1.8e-9 after extraction, 3e-15 after one Newton-Kleinman step
    assert i0["refinements"] == 0 and i0["res"] > hm.refine_target(371)
    assert info["refinements"] == 1 and info["res"] <= hm.refine_target(371)
    assert closed_loop_max_real(E, Au, G, X) < 0


def test_imaginary_axis_eigenvalues_do_not_converge():
    E, A, B, C = oscillator_pencil()
    H, K = hm.hamiltonian(E, A, B @ B.T, C.T @ C)
    assert np.abs(sla.eigvals(H, K).real).min() < 1e-8
    with pytest.raises(hm.NotStable):
        hm.gare_sign(E, A, B @ B.T, C.T @ C, maxiters=25)


def test_structure_is_exact(steel):
    E, A, B, C = steel
    n = 40
    E, A, B, C = E[:n, :n], A[:n, :n], B[:n], C[:, :n]
    H, _ = hm.hamiltonian(E, A, B @ B.T, C.T @ C)
    Z = hm.structure(H + 1e-3 * np.random.default_rng(0).standard_normal(H.shape), n)
    J = np.block([[np.zeros((n, n)), np.eye(n)], [-np.eye(n), np.zeros((n, n))]])
    assert np.array_equal(J @ Z, (J @ Z).T)


def test_solve_dispatch_needs_matrix_sign():
    prob = D.GAREProblem(np.eye(2), -np.eye(2), D.lowrank(np.ones((2, 1))), D.lowrank(np.ones((2, 1))))
    assert D.MatrixSign().max_refine == 2
    with pytest.raises(TypeError, match="ndarray"):
        D.residual(prob, "not a solution")
