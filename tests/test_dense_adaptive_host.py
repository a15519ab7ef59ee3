"""Adaptive dense Ros2, the part that needs no device: the ABI level, the exported symbols, the argument errors that `solve` and `solve_batch`
raise before any device call, and the properties of the NumPy model (tests/_adaptive_ros2_model.py) that the device driver follows."""
import math
import os

import numpy as np
import pytest

import dre_amd as D
import _adaptive_ros2_model as am
from conftest import ROOT


def _prob(n=6, X0=None, tspan=(1.0, 0.0)):
    E, A, B, Cm = am.stiff_pencil(n, seed=3)
    return D.GDREProblem(E, A, B, Cm, np.zeros((n, n)) if X0 is None else X0, tspan)


def test_abi_level_symbols_and_error_code():
    lib = D._lib.load()
    assert lib.dre_version() >= 107          # the version that brought the adaptive entry points (include/dre_hip.h); later ones add to it
    for name, nargs in (("dre_dense_gdre_solve_adaptive", 22), ("dre_gdre_result_step_stats", 3)):
        assert hasattr(lib, name)
        assert len(D._lib.PROTOTYPES[name][1]) == nargs
    header = open(os.path.join(ROOT, "include", "dre_hip.h")).read()
    assert "#define DRE_ERR_STEP (-8)" in header


def test_step_control_defaults():
    sc = D.StepControl()
    assert (sc.rtol, sc.atol, sc.dt_min, sc.dt_max, sc.max_steps, tuple(sc.tstops)) == (1e-3, 1e-6, 0.0, math.inf, 10_000, ())


def _no_device(monkeypatch):
    """any device work would start with a context: make that an error of its own"""
    def boom(*a, **k):
        raise AssertionError("a device context was requested")
    monkeypatch.setattr(D.api.dev, "default_context", boom)


@pytest.mark.parametrize("alg", [D.Ros1(D.MatrixSign()), D.Ros3(D.MatrixSign()), D.Ros4(D.MatrixSign()), D.Ros2(), D.Ros2(D.ADI()),
                                 D.Ros2(D.FactoredSign())])
def test_other_methods_and_inner_algorithms_are_a_type_error(monkeypatch, alg):
    _no_device(monkeypatch)
    with pytest.raises(TypeError, match="nothing was run on the device"):
        D.solve(_prob(), alg, dt=-0.1, adaptive=D.StepControl())


def test_a_low_rank_x0_is_a_type_error(monkeypatch):
    _no_device(monkeypatch)
    p = _prob()
    p.X0 = D.lowrank(np.ones((6, 1)), np.eye(1))
    with pytest.raises(TypeError, match="dense X0.*nothing was run on the device"):
        D.solve(p, D.Ros2(D.MatrixSign()), dt=-0.1, adaptive=D.StepControl())


def test_solve_batch_is_a_type_error(monkeypatch):
    _no_device(monkeypatch)
    with pytest.raises(TypeError, match="not batched.*nothing was run on the device"):
        D.solve_batch([_prob(), _prob()], D.Ros2(D.MatrixSign()), dt=-0.1, adaptive=D.StepControl())


@pytest.mark.parametrize("dt,sc", [
    (0.1, D.StepControl()),                                   # wrong sign for tspan (1, 0)
    (0.0, D.StepControl()),
    (-0.1, D.StepControl(rtol=0.0)),
    (-0.1, D.StepControl(atol=0.0)),
    (-0.1, D.StepControl(atol=-1e-9)),
    (-0.1, D.StepControl(dt_min=0.5, dt_max=0.1)),
    (-0.1, D.StepControl(max_steps=0)),
    (-0.1, D.StepControl(tstops=(0.3, 0.6))),                 # not monotone in the direction of integration
    (-0.1, D.StepControl(tstops=(0.5, 0.5))),
    (-0.1, D.StepControl(tstops=(1.0,))),                     # an end of the span
    (-0.1, D.StepControl(tstops=(-0.5,))),
])
def test_control_values_are_a_value_error(monkeypatch, dt, sc):
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match="nothing was run on the device"):
        D.solve(_prob(), D.Ros2(D.MatrixSign()), dt=dt, adaptive=sc)


def test_adaptive_must_be_a_step_control(monkeypatch):
    _no_device(monkeypatch)
    with pytest.raises(TypeError):
        D.solve(_prob(), D.Ros2(D.MatrixSign()), dt=-0.1, adaptive=dict(rtol=1e-3))


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def test_estimator_is_second_order():
    """D is the difference of a second-order and a first-order solution: at X0 = 0 on a mild pencil it falls by about 4 per halving of tau
    (steps well inside the asymptotic range: tau ||E^-1 A|| <= 0.02)"""
    n = 8
    rng = np.random.default_rng(1)
    A = -np.eye(n) + 0.1 * rng.standard_normal((n, n))
    E, B, Cm = np.eye(n), rng.standard_normal((n, 2)), rng.standard_normal((3, n))
    CtC = Cm.T @ Cm
    norms = [np.linalg.norm(am.ros2_step(E, A, B, CtC, np.zeros((n, n)), tau)[1]) for tau in (0.02, 0.01, 0.005, 0.0025)]
    for a, b in zip(norms, norms[1:]):
        assert 3.0 < a / b < 5.0, norms


@pytest.mark.parametrize("tspan,dt0,tstops", [((0.0, 1.0), 0.3, (0.1, 0.37, 0.9)), ((1.0, 0.0), -0.3, (0.9, 0.37, 0.1))])
def test_must_hit_times_are_bitwise_in_t(tspan, dt0, tstops):
    E, A, B, Cm = am.stiff_pencil(12)
    r = am.solve(E, A, B, Cm, np.zeros((12, 12)), tspan, dt0, rtol=1e-2, atol=1e-5, tstops=tstops)
    for s in tstops + (tspan[1],):
        assert s in r.t.tolist()
    d = np.diff(r.t)
    assert (d > 0).all() if tspan[1] > tspan[0] else (d < 0).all()
    assert r.t[0] == tspan[0] and r.t[-1] == tspan[1]
    assert r.accepted == len(r.t) - 1 == len(r.err) and r.rejected >= 1 and (r.err <= 1.0).all()
    assert r.accepted + r.rejected == len(r.trials)


@pytest.mark.parametrize("dt_max", [2.0, 7.0, math.inf])
def test_start_at_the_gare_solution_grows_by_five_until_dt_max(dt_max):
    E, A, B, Cm = am.stiff_pencil(12)
    Xinf = am.stabilizing_solution(E, A, B, Cm)
    K = (B.T @ Xinf) @ E
    AXE = A.T @ Xinf @ E
    assert np.linalg.norm(Cm.T @ Cm + AXE + AXE.T - K.T @ K) <= 1e-12 * (np.linalg.norm(Cm.T @ Cm) + 2 * np.linalg.norm(AXE) + np.linalg.norm(K.T @ K))
    T, dt0 = 50.0, 1e-2
    r = am.solve(E, A, B, Cm, Xinf, (T, 0.0), -dt0, rtol=1e-3, atol=1e-6, dt_max=dt_max)
    assert r.rejected == 0
    assert r.accepted == am.predicted_steps_at_rest(T, dt0, dt_max)
    taus = np.array([tr[1] for tr in r.trials])
    grow = taus[1:] / taus[:-1]
    free = [i for i in range(len(grow)) if taus[i + 1] < 0.999 * dt_max and i + 1 < len(grow) - 1]      # (the last steps follow the must-hit rule)
    assert free and np.allclose(grow[free], 5.0)
    assert np.linalg.norm(r.X[-1] - Xinf) <= 1e-8 * np.linalg.norm(Xinf)


def test_controller_clamps_and_failures():
    assert am.decide(0.0) == (True, 5.0)
    assert am.decide(float("nan")) == (False, 0.2) and am.decide(float("inf")) == (False, 0.2)
    assert am.decide(1e-9)[1] == 5.0 and am.decide(1e9) == (False, 0.2)
    assert am.decide(1.0) == (True, 0.9) and am.decide(1.0 + 1e-12)[0] is False
    n = 4
    E, A, B, Cm = np.eye(n), -np.eye(n), np.ones((n, 1)), np.ones((1, n))
    X0 = np.zeros((n, n))
    # a step function whose error is 4 above tau = 0.1 and 0.25 below: one rejection halves the step (0.9 / 2 = 0.45), the next trial may not grow
    step = lambda X, tau: (X + 1.0, np.full((n, n), (4.0 if tau > 0.1 else 0.25) * (1e-6 + 1e-3 * np.abs(X + 1.0))))
    r = am.solve(E, A, B, Cm, X0, (0.0, 10.0), 0.2, step=step)
    assert [tr[3] for tr in r.trials[:3]] == [False, True, True]
    assert r.trials[1][1] == pytest.approx(0.2 * 0.45) and r.trials[2][1] == pytest.approx(0.09)      # fac = 0.9 / sqrt(0.25) = 1.8 capped at 1
    with pytest.raises(am.StepFailure):
        am.solve(E, A, B, Cm, X0, (0.0, 10.0), 0.2, step=step, dt_min=0.2, dt_max=0.2)
    with pytest.raises(am.StepFailure):
        am.solve(E, A, B, Cm, X0, (0.0, 10.0), 0.2, step=step, max_steps=1)
    nan_step = lambda X, tau: (X * np.nan, X * np.nan)
    with pytest.raises(am.StepFailure):
        am.solve(E, A, B, Cm, X0, (0.0, 1.0), 0.2, step=nan_step, max_steps=50)


@pytest.fixture(scope="module")
def stiff12():
    E, A, B, Cm = am.stiff_pencil(12)
    T = 50.0
    return E, A, B, Cm, T, am.fixed_ros2(E, A, B, Cm, np.zeros((12, 12)), T, 20000)


@pytest.mark.parametrize("rtol", [1e-2, 1e-3, 1e-4])
def test_error_tracks_the_tolerance(stiff12, rtol):
    """the issue's pencil (n = 12, stiff, X0 = 0, horizon 50) against 20 000 fixed Ros2 steps: relative error at most 5 rtol with atol = 1e-3 rtol"""
    E, A, B, Cm, T, Xref = stiff12
    r = am.solve(E, A, B, Cm, np.zeros((12, 12)), (0.0, T), 1e-3, rtol=rtol, atol=1e-3 * rtol, max_steps=100_000)
    err = np.linalg.norm(r.X[-1] - Xref) / np.linalg.norm(Xref)
    print(f"rtol {rtol:g}: accepted {r.accepted} rejected {r.rejected} relative error {err:.3e} = {err / rtol:.2f} rtol")
    assert err <= 5.0 * rtol
