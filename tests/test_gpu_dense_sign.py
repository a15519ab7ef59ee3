"""Dense path on the device: the matrix-sign-function GALE solver (solve(GALEProblem, MatrixSign())) and the dense Rosenbrock
methods Ros1..Ros4 (dense_ros{1,2,3,4}.jl) against the dense oracle, the committed dense-oracle fixtures and the low-rank path."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import dre_amd as D
import dre_oracle as o
import _sign_model as sm
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
MS = D.MatrixSign()


def _tiny(symE, symA, n=50, g=4):                     # test/tiny_random.jl:37-46
    rng = np.random.default_rng(100 + 10 * symE + symA)
    sprand = lambda: sp.random(n, n, density=1 / n, random_state=rng, format="csc")
    E = sprand(); E = (E + E.T + n * sp.identity(n)) if symE else (E + n * sp.identity(n))
    A = sprand(); A = (A + A.T - n * sp.identity(n)) if symA else (A - n * sp.identity(n))
    C = (-2) * D.lowrank(rng.random((n, g)), -np.eye(g))
    return E.toarray(), A.toarray(), C


def _rel_res(E, A, C, X):
    return np.linalg.norm(C + A.T @ X @ E + E.T @ X @ A) / np.linalg.norm(C)


@pytest.mark.parametrize("symE,symA", [(True, True), (True, False), (False, True), (False, False)])
def test_gale_tiny_random(ctx, symE, symA):
    E, A, Cl = _tiny(symE, symA)
    Cd = Cl.dense()
    X, info = D.solve_gale_dense(D.GALEProblem(E, A, Cd), MS, return_info=True)
    assert _rel_res(E, A, Cd, X) < 1e-10 and info["res"] < 1e-10
    assert D.delta(X, o.lyap_dense(A, E, Cd)) < 1e-10
    X2 = D.solve(D.GALEProblem(sp.csc_matrix(E), sp.csc_matrix(A), Cl), MS)    # LDLt right-hand side, sparse operands: densified
    assert np.allclose(X2, X, rtol=0, atol=1e-13 * np.abs(X).max())


def test_pivoting_errors_and_recovery(ctx):
    n = 40
    blk = np.array([[0.0, 1.0], [-1.0, -1.0]])        # zero leading diagonal entries: row interchanges are forced
    F = np.kron(np.eye(n // 2), blk)
    E = np.eye(n) + 0.01 * np.diag(np.arange(n) / n)
    R = np.random.default_rng(7).random((n, 3)); R = R @ R.T
    X = D.solve(D.GALEProblem(E, F, R), MS)
    assert D.delta(X, o.lyap_dense(F, E, R)) < 1e-10
    with pytest.raises(D.DREError) as e:              # right-shifted: not c-stable
        D.solve(D.GALEProblem(E, F + 2.0 * E, R), MS)
    assert e.value.code == -7
    Fz = F.copy(); Fz[:, 3] = 0.0
    with pytest.raises(D.DREError) as e:              # a zero column: exactly singular
        D.solve(D.GALEProblem(E, Fz, R), MS)
    assert e.value.code == -4
    Ez, A, C = _tiny(False, False)
    Ez[:, 0] = 0.0
    with pytest.raises(D.DREError) as e:              # singular E
        D.solve(D.GALEProblem(Ez, A, C.dense()), MS)
    assert e.value.code == -4
    E1, A1, C1 = _tiny(False, False)                  # the context is still usable
    X1 = D.solve(D.GALEProblem(E1, A1, C1.dense()), MS)
    assert _rel_res(E1, A1, C1.dense(), X1) < 1e-10


@pytest.fixture(scope="module")
def rail():
    d = D.steel_profile(371)
    L, Dm = D.initial_value(d)
    return d, L, Dm, D.lowrank(L, Dm).dense()


@pytest.mark.parametrize("Ros", [D.Ros1, D.Ros2, D.Ros3, D.Ros4])
def test_rail_smoke(ctx, rail, Ros):                  # test/rail.jl:36-50
    d, L, Dm, X0 = rail
    prob = D.GDREProblem(d.E, d.A, d.B, d.C, X0, (4500.0, 4400.0))
    sol = D.solve(prob, Ros(MS), dt=-100.0)
    assert isinstance(sol, D.DRESolution) and len(sol.X) == 2 and sol.X[0] is prob.X0
    sol = D.solve(prob, Ros(MS), dt=-50.0, save_state=True)
    assert len(sol.t) == len(sol.X) == len(sol.K) == 3 and (np.diff(sol.t) < 0).all()
    for X, K in zip(sol.X, sol.K):
        assert K.shape == (7, 371)
        assert np.abs(K - (d.B.T @ X) @ d.E.toarray()).max() <= 1e-12 * np.abs(K).max()


def _host_iters(d, Kd, t, order):
    """sign iterations of the host model on the stage matrix of every step (the fixture's K(t) feeds the closed loop)"""
    E, A = d.E.toarray(), d.A.toarray()
    g2 = 1.0 + 1.0 / np.sqrt(2.0)
    out = []
    for i in range(1, len(t)):
        tau = t[i - 1] - t[i]
        Acl = A - d.B @ Kd[i - 1]
        F = Acl - E / (2.0 * tau) if order == 1 else g2 * tau * Acl - E / 2.0
        out.append(sm.SignModel(F, E).iters)
    return np.array(out)


@pytest.mark.parametrize("name,Ros,order", [("ros1_371_full", D.Ros1, 1), ("ros2_371_full", D.Ros2, 2)])
def test_full_trajectory_against_dense_fixture(ctx, rail, name, Ros, order):
    d, L, Dm, X0 = rail
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    sol, st = D.solve(D.GDREProblem(d.E, d.A, d.B, d.C, X0, (4500.0, 0.0)), Ros(MS), dt=-100.0, return_stats=True)
    assert len(sol.K) == 46 and np.allclose(sol.t, g["t"])
    for i in range(46):
        assert D.delta(sol.K[i], g["K_dense"][i]) < 1e-10, i
    assert D.delta(sol.X[-1], g["X_dense_end"]) < 1e-10
    assert np.linalg.norm(sol.K[-1] - g["K_dense"][-1]) < np.linalg.norm(g["K_dense"][-1]) * 371 * EPS * 100     # test/rail.jl:56
    assert st["lyapunov_solves"] == 45 * order
    dev_iters = np.array([s["iters"] for s in st["solves"]])[::order]
    assert np.abs(dev_iters - _host_iters(d, g["K_dense"], g["t"], order)).max() <= 1
    assert all(s["res"] <= 100 * 371 * EPS for s in st["solves"])


def test_ros2_convection_1357_against_dense_fixture(ctx):
    g = np.load(os.path.join(GOLDEN, "ros2_1357_proj.npz"))
    d = D.steel_profile(1357, convection=float(g["convection"]))
    L, Dm = D.initial_value(d)
    dt = float(g["dt"])
    prob = D.GDREProblem(d.E, d.A, d.B, d.C, D.lowrank(L, Dm).dense(), (4500.0, 4500.0 + 10 * dt))
    sol = D.solve(prob, D.Ros2(MS), dt=dt)
    assert len(sol.K) == 11
    for i in range(11):
        assert D.delta(sol.K[i], g["K_dense"][i]) < 1e-10, i
    assert np.linalg.norm(sol.K[-1] - g["K_dense"][-1]) < np.linalg.norm(g["K_dense"][-1]) * 1357 * EPS * 100


@pytest.mark.parametrize("Ros,oracle", [(D.Ros3, o.solve_dense_ros3), (D.Ros4, o.solve_dense_ros4)])
def test_ros3_ros4_against_oracle(ctx, rail, Ros, oracle):
    d, L, Dm, X0 = rail
    tspan = (4500.0, 4400.0)
    sol = D.solve(D.GDREProblem(d.E, d.A, d.B, d.C, X0, tspan), Ros(MS), dt=-20.0)
    ref = oracle(o.GDREProblem(d.E, d.A, d.B, d.C, X0, tspan), dt=-20.0)
    assert len(sol.K) == len(ref.K) == 6
    for i in range(6):
        assert D.delta(sol.K[i], ref.K[i]) < 1e-10, i
    assert D.delta(sol.X[-1], ref.X[-1]) < 1e-10


@pytest.mark.parametrize("Ros", [D.Ros1, D.Ros2])
def test_lowrank_vs_dense_both_on_device(ctx, rail, Ros):      # test/rail.jl:52-70
    d, L, Dm, X0 = rail
    tspan = (4500.0, 4400.0)
    shifts = list(np.load(os.path.join(GOLDEN, "heuristic_shifts_371.npy")))
    if Ros is D.Ros2:
        shifts = list((1.0 + 1.0 / np.sqrt(2.0)) * 20.0 * np.array(shifts) - 0.5)
    lr = D.solve(D.GDREProblem(d.E, d.A, d.B, d.C, D.lowrank(L, Dm), tspan), Ros(D.ADI(shifts=D.Shifts.Cyclic(shifts))), dt=-20.0)
    dn = D.solve(D.GDREProblem(d.E, d.A, d.B, d.C, X0, tspan), Ros(MS), dt=-20.0)
    assert np.linalg.norm(lr.K[-1] - dn.K[-1]) < np.linalg.norm(dn.K[-1]) * 371 * EPS * 100


def test_observer_order(ctx, rail):
    d, L, Dm, X0 = rail
    calls = []

    class Obs:
        def observe_gdre_start(self, prob, alg): calls.append(("start", alg))
        def observe_gdre_step(self, t, X, K): calls.append(("step", t, X, K))
        def observe_gdre_done(self): calls.append(("done",))

    alg = D.Ros1(MS)
    sol = D.solve(D.GDREProblem(d.E, d.A, d.B, d.C, X0, (4500.0, 4400.0)), alg, dt=-50.0, save_state=True, observer=Obs())
    assert [c[0] for c in calls] == ["start", "step", "step", "step", "done"] and calls[0][1] is alg
    for i, c in enumerate(calls[1:4]):
        assert c[1] == sol.t[i] and np.array_equal(c[2], sol.X[i]) and np.array_equal(c[3], sol.K[i])


@pytest.mark.parametrize("n,conv", [(371, 0.0), (1357, 3e-3)])
def test_refinement_by_replay_on_device(ctx, n, conv):
    """a loose stopping tolerance leaves the sign iteration's W inaccurate: the replayed residual corrections must recover the accuracy
    (the device side of tests/test_dense_sign_host.py::test_sign_model_refinement_by_replay)"""
    d = D.steel_profile(n, convection=conv)
    E, A, R = d.E.toarray(), d.A.toarray(), d.C.T @ d.C
    F = A - E / 200.0
    X, info = D.solve_gale_dense(D.GALEProblem(E, F, R), D.MatrixSign(tol=1e-3, max_refine=6), return_info=True)
    assert info["res0"] > 100 * n * EPS and 1 <= info["refinements"] <= 6
    assert info["res"] <= 100 * n * EPS
    assert _rel_res(E, F, R, X) <= 100 * n * EPS
    model = sm.SignModel(F, E, tol=1e-3)
    assert abs(info["iters"] - model.iters) <= 1
    Xm = model.solve(R, max_refine=6)[0]
    assert D.delta(X, Xm) < 1e-9
    if n == 371:
        assert D.delta(X, o.lyap_dense(F, E, R)) < 1e-9          # (refined only down to the 100 n eps residual target)


def test_zero_steps_keeps_one_state(ctx, rail):
    d, L, Dm, X0 = rail
    for save_state in (False, True):
        sol = D.solve(D.GDREProblem(d.E, d.A, d.B, d.C, X0, (4500.0, 4450.0)), D.Ros1(MS), dt=-100.0, save_state=save_state)
        assert len(sol.t) == len(sol.K) == len(sol.X) == 1 and sol.X[0] is X0
        assert np.abs(sol.K[0] - (d.B.T @ X0) @ d.E.toarray()).max() <= 1e-12 * np.abs(sol.K[0]).max()
