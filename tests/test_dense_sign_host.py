"""Dense path, host side: dispatch rules of solve_gdre for dense X0 / MatrixSign / Ros3 / Ros4 (all checked before a context is
needed) and the NumPy model of the device's sign-function iteration (tests/_sign_model.py) against the dense oracle."""
import numpy as np
import pytest

import dre_amd as D
import dre_oracle as o
import _sign_model as sm


def _prob(X0):
    return D.GDREProblem(None, None, None, None, X0, (0.0, 1.0))


def test_public_names():
    assert D.MatrixSign().maxiters == 50 and D.MatrixSign().tol is None and D.MatrixSign().max_refine == 2
    assert D.Ros3().inner_alg is None and D.Ros4(D.MatrixSign()).inner_alg == D.MatrixSign()


@pytest.mark.parametrize("alg", [D.Ros1(), D.Ros2(), D.Ros3(), D.Ros4(), D.Ros1(D.ADI())])
def test_dense_x0_needs_matrix_sign(alg):
    with pytest.raises(TypeError, match=r"Ros1\(MatrixSign\(\)\)"):
        D.solve_gdre(_prob(np.eye(3)), alg, dt=1.0)


@pytest.mark.parametrize("alg", [D.Ros1(D.MatrixSign()), D.Ros2(D.MatrixSign())])
def test_matrix_sign_with_lowrank_x0(alg):
    with pytest.raises(TypeError, match="MatrixSign"):
        D.solve_gdre(_prob(D.lowrank(np.ones((3, 1)))), alg, dt=1.0)


@pytest.mark.parametrize("alg", [D.Ros3(), D.Ros4(), D.Ros3(D.MatrixSign()), D.Ros4(D.MatrixSign())])
def test_ros3_ros4_with_lowrank_x0(alg):
    with pytest.raises(TypeError, match="low-rank"):
        D.solve(_prob(D.lowrank(np.ones((3, 1)))), alg, dt=1.0)


@pytest.fixture(scope="module", params=[(371, 0.0), (1357, 3e-3)], ids=["371", "1357conv"])
def pencil(request):
    n, conv = request.param
    d = D.steel_profile(n, convection=conv)
    return d.E.toarray(), d.A.toarray(), d.C.T @ d.C


@pytest.mark.parametrize("tau", [20.0, 100.0])
def test_sign_model_matches_dense_oracle(pencil, tau):
    E, A, R = pencil
    F = A - E / (2.0 * tau)                         # the Ros1 stage matrix with X = 0
    X, info = sm.sign_lyap(F, E, R)
    assert info["iters"] <= 15
    assert info["res"] <= 100 * F.shape[0] * sm.EPS
    assert o.delta(X, o.lyap_dense(F, E, R)) < 1e-12


def test_sign_model_refinement_by_replay(pencil):
    E, A, R = pencil
    F = A - E / 200.0
    m = sm.SignModel(F, E, tol=1e-3)               # a loose stop: the refinement has to recover the accuracy
    X, steps, r0, r = m.solve(R, max_refine=6)
    assert r0 > 100 * F.shape[0] * sm.EPS and 1 <= steps <= 6
    assert r <= 100 * F.shape[0] * sm.EPS
    assert o.delta(X, o.lyap_dense(F, E, R)) < 1e-9          # (refined only down to the 100 n eps residual target)


def test_sign_model_detects_unstable_pencil(pencil):
    E, A, R = pencil
    with pytest.raises(sm.NotStable):
        sm.SignModel(-A, E)                           # (-A, E) is anti-stable: the sign iteration goes to +E
    F = A + 0.5 * np.abs(A).max() * E                 # shifted to the right: a mixed spectrum
    with pytest.raises(sm.NotStable):
        sm.SignModel(F, E)
