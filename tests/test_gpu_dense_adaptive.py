"""Adaptive dense Ros2 on the device (`solve(prob, Ros2(MatrixSign()), dt=dt0, adaptive=StepControl(...))`, csrc/dense_adaptive.hip) against its
NumPy model (tests/_adaptive_ros2_model.py), against the device's own fixed-step Ros4, and at its edges: must-hit times, saved states, a
start at the GARE solution, DRE_ERR_STEP and the argument errors of the C ABI.

Pencils: seeded and stiff (`stiff_pencil`, stage pencils c-stable for every step tried here), n = 33 and n = 70: n^2 is no multiple of the 256-thread workgroup and n lies on either side
of a 64-lane wave.  tspan runs backwards, (1, 0) with dt0 < 0, as the project's other dense tests do.

Device against model (case 1), measured on an MI355X (n = 33 / n = 70): t 3.3e-12 / 9.1e-13 of the span, err 3.0e-10 / 1.0e-9, K 2.1e-12 /
1.3e-11 and final X 8.8e-16 / 7.0e-15 relative in the Frobenius norm, with equal accept / reject sequences (327 + 25 and 487 + 64 trials).
The asserted tolerances TOL_* are 10 x the larger figure of each pair, for rounding that differs between boxes."""
import ctypes as C

import numpy as np
import pytest

import dre_amd as D
import dre_oracle as o
import _adaptive_ros2_model as am

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
MS = D.MatrixSign()
RTOL, ATOL = 1e-3, 1e-6
TSPAN, DT0, TSTOP = (1.0, 0.0), -0.5, 0.4
SEEDS = {33: 2, 70: 0}              # seeds at which every trial of the model keeps |err - 1| > 1e-3 (asserted below)

# 10 x the measured device-model deviations (module docstring)
TOL_T = 3.4e-11         # relative to the span
TOL_ERR = 1.1e-8        # absolute (err is of order 1); five orders below the asserted decision margin 1e-3
TOL_K = 1.4e-10         # relative, Frobenius norm, the largest over the trajectory
TOL_X = 7.0e-14         # relative, Frobenius norm, the final state


def _rel(a, b):
    return np.linalg.norm(a - b) / np.linalg.norm(b)


class Case:
    """one pencil, its model run and its device run (computed once per size, read by the tests)"""

    def __init__(self, n):
        self.n = n
        self.E, self.A, self.B, self.C = am.stiff_pencil(n, seed=SEEDS[n])
        self.X0 = np.zeros((n, n))
        self.model = am.solve(self.E, self.A, self.B, self.C, self.X0, TSPAN, DT0, rtol=RTOL, atol=ATOL, tstops=(TSTOP,))
        self.prob = D.GDREProblem(self.E, self.A, self.B, self.C, self.X0, TSPAN)
        self.sol, self.stats = D.solve(self.prob, D.Ros2(MS), dt=DT0, adaptive=D.StepControl(rtol=RTOL, atol=ATOL, tstops=(TSTOP,)),
                                       save_state=True, return_stats=True)


@pytest.fixture(scope="module")
def cases(ctx):
    return {}


@pytest.fixture(params=[33, 70])
def case(request, ctx, cases):
    if request.param not in cases:
        cases[request.param] = Case(request.param)
    return cases[request.param]


# ---- 1. device against model ----------------------------------------------------------------------------------------------------------------
def test_device_follows_the_model(case):
    mod, sol, st = case.model, case.sol, case.stats
    errs = np.array([tr[2] for tr in mod.trials])
    assert mod.rejected >= 2 and np.abs(errs - 1.0).min() > 1e-3          # (the accept / reject sequence cannot flip on rounding)
    assert (st["accepted"], st["rejected"]) == (mod.accepted, mod.rejected)
    assert len(sol.t) == len(sol.K) == len(sol.X) == mod.accepted + 1 and len(st["err"]) == mod.accepted
    assert st["lyapunov_solves"] == 2 * (mod.accepted + mod.rejected)
    dev_t = np.abs(sol.t - mod.t).max() / abs(TSPAN[1] - TSPAN[0])
    dev_err = np.abs(st["err"] - mod.err).max()
    dev_K = max(_rel(sol.K[i], mod.K[i]) for i in range(1, len(mod.K)))
    dev_X = _rel(sol.X[-1], mod.X[-1])
    print(f"n = {case.n}: accepted {mod.accepted} rejected {mod.rejected}; device - model: t {dev_t:.3e} err {dev_err:.3e} K {dev_K:.3e} X {dev_X:.3e}")
    assert dev_t <= TOL_T and dev_err <= TOL_ERR and dev_K <= TOL_K and dev_X <= TOL_X


# ---- 2. accuracy ----------------------------------------------------------------------------------------------------------------------------
def test_accuracy_against_fixed_ros4(case):
    ref = D.solve(case.prob, D.Ros4(MS), dt=-1.0 / 400)
    e = _rel(case.sol.X[-1], ref.X[-1])
    print(f"n = {case.n}: ||X_adaptive - X_ros4|| / ||X_ros4|| = {e:.3e} = {e / RTOL:.2f} rtol")
    assert e <= 5.0 * RTOL


# ---- 3. must-hit times ----------------------------------------------------------------------------------------------------------------------
def test_must_hit_times(case):
    t = case.sol.t
    assert t[0] == TSPAN[0] and t[-1] == TSPAN[1] and TSTOP in t.tolist()
    assert (np.diff(t) < 0).all()


def test_several_tstops_forwards(ctx):
    E, A, B, Cm = am.stiff_pencil(33, seed=2)
    stops = (0.01, 0.013, 0.05)
    sol = D.solve(D.GDREProblem(E, A, B, Cm, np.zeros((33, 33)), (0.0, 0.06)), D.Ros2(MS), dt=0.02,
                  adaptive=D.StepControl(rtol=1e-2, atol=1e-4, tstops=stops))
    assert sol.t[0] == 0.0 and sol.t[-1] == 0.06 and all(s in sol.t.tolist() for s in stops)
    assert (np.diff(sol.t) > 0).all()


# ---- 4. save_state --------------------------------------------------------------------------------------------------------------------------
def test_saved_states_and_feedback(case):
    sol = case.sol
    assert sol.X[0] is case.prob.X0
    for X, K in zip(sol.X, sol.K):
        assert X.shape == (case.n, case.n) and K.shape == (2, case.n)
        assert np.abs(K - (case.B.T @ X) @ case.E).max() <= 1e-12 * np.abs(K).max()


def test_without_save_state_first_and_last_only(case):
    seen = []
    obs = type("Obs", (), {"observe_gdre_step": lambda self, t, X, K: seen.append((t, X is not None))})()
    sol, st = D.solve(case.prob, D.Ros2(MS), dt=DT0, adaptive=D.StepControl(rtol=RTOL, atol=ATOL, tstops=(TSTOP,)), return_stats=True, observer=obs)
    assert len(sol.X) == 2 and sol.X[0] is case.prob.X0
    assert np.array_equal(sol.X[1], case.sol.X[-1]) and np.array_equal(sol.t, case.sol.t)       # the same run, state for state
    assert st["accepted"] == case.stats["accepted"] and len(sol.K) == len(sol.t)
    assert [s[0] for s in seen] == sol.t.tolist()                                             # accepted steps only, in order
    assert [s[1] for s in seen] == [True] + [False] * (len(sol.t) - 2) + [True]


# ---- 5. start at the GARE solution ----------------------------------------------------------------------------------------------------------
def test_start_at_the_gare_solution(case):
    n, E, A, B, Cm = case.n, case.E, case.A, case.B, case.C
    Xinf, info = D.solve(D.GAREProblem(E, A, D.lowrank(B, np.eye(2)), D.lowrank(Cm.T.copy(), np.eye(3))), MS, return_info=True)
    T, dt0, dt_max = 50.0, 1e-2, 7.0
    sol, st = D.solve(D.GDREProblem(E, A, B, Cm, Xinf, (T, 0.0)), D.Ros2(MS), dt=-dt0, adaptive=D.StepControl(rtol=RTOL, atol=ATOL, dt_max=dt_max),
                      return_stats=True)
    mod = am.solve(E, A, B, Cm, Xinf, (T, 0.0), -dt0, rtol=RTOL, atol=ATOL, dt_max=dt_max)
    assert st["rejected"] == 0 == mod.rejected
    assert st["accepted"] == mod.accepted == am.predicted_steps_at_rest(T, dt0, dt_max)
    assert np.allclose(sol.t, mod.t, rtol=0, atol=1e-12 * T)
    # X' = L^-1(Res(X)) to first order, L the closed-loop Lyapunov operator: X can move by ||L^-1|| ||Res(Xinf)|| on its way to the exact fixed
    # point, with ||L^-1||_2 = ||H||_2, H the solution for the right-hand side I, and ||Res|| = res S (res: the GARE solver's scaled residual
    # of this X0, at least its target 100 n eps -- at n = 70 the solver stops at 6e-11 --, S = ||Q|| + 2 ||A'XE|| + ||E'XGXE||); every
    # accepted step adds the rounding of its two Lyapunov solves, each bounded by the dense path's residual bound 100 n eps relative to X
    K = (B.T @ Xinf) @ E
    AXE = A.T @ Xinf @ E
    S = np.linalg.norm(Cm.T @ Cm) + 2 * np.linalg.norm(AXE) + np.linalg.norm(K.T @ K)
    H = o.lyap_dense(A - B @ K, E, np.eye(n))
    bound = max(info["res"], 100 * n * EPS) * np.linalg.norm(H, 2) * S + 100 * n * EPS * 2 * st["accepted"] * np.linalg.norm(Xinf)
    moved = np.linalg.norm(sol.X[-1] - Xinf)
    print(f"n = {n}: accepted {st['accepted']}, ||X(0) - Xinf|| = {moved:.3e} (bound {bound:.3e}), GARE residual {info['res']:.3e}")
    assert moved <= bound


# ---- 6. DRE_ERR_STEP ------------------------------------------------------------------------------------------------------------------------
def test_step_failures_leave_the_context_usable(case):
    t, tau, err, ok = case.model.trials[0]
    assert not ok and err > 1.0                                     # the model rejects the first trial, of size tau
    with pytest.raises(D.DREError) as e:
        D.solve(case.prob, D.Ros2(MS), dt=-tau, adaptive=D.StepControl(rtol=RTOL, atol=ATOL, dt_min=tau, dt_max=tau))
    assert e.value.code == -8 and "dt_min" in str(e.value)
    with pytest.raises(D.DREError) as e:
        D.solve(case.prob, D.Ros2(MS), dt=DT0, adaptive=D.StepControl(rtol=RTOL, atol=ATOL, max_steps=1))
    assert e.value.code == -8 and "max_steps" in str(e.value)
    span = (1.0, 0.96)                                              # the context solves a further ordinary problem (steps small enough for
    sol = D.solve(D.GDREProblem(case.E, case.A, case.B, case.C, case.X0, span), D.Ros2(MS), dt=-0.01)      # c-stable stage pencils on a coarse grid)
    ref = o.solve_dense_ros2(o.GDREProblem(case.E, case.A, case.B, case.C, case.X0, span), dt=-0.01)
    assert len(sol.K) == 5 and D.delta(sol.K[-1], ref.K[-1]) < 1e-10


# ---- 7. argument errors through the C ABI ---------------------------------------------------------------------------------------------------
def _abi(ctx, ups, t0=1.0, tf=0.0, dt0=-0.5, order=2, rtol=1e-3, atol=1e-6, dt_min=0.0, dt_max=np.inf, max_steps=100, tstops=()):
    ts = np.array(tstops, dtype=float)
    r = C.c_void_p()
    rc = ctx.lib.dre_dense_gdre_solve_adaptive(ctx.ptr, *[u.ptr for u in ups], t0, tf, dt0, order, rtol, atol, dt_min, dt_max, max_steps,
                                               ts.ctypes.data_as(C.POINTER(C.c_double)), len(ts), 0, 50, 0.0, 2, C.byref(r))
    if r:
        ctx.lib.dre_gdre_result_free(r)
    return rc


def test_argument_errors_through_the_c_abi(ctx):
    n = 12
    E, A, B, Cm = am.stiff_pencil(n, seed=1)
    ups = [ctx.upload(np.asfortranarray(M)) for M in (E, A, B, Cm, np.zeros((n, n)))]
    assert _abi(ctx, ups, tf=0.9, dt0=-0.05, rtol=1e-1, atol=1e-2) == 0
    assert _abi(ctx, ups, order=1) == -1
    assert "Ros2" in ctx.lib.dre_last_error(ctx.ptr).decode()
    for order in (3, 4):
        assert _abi(ctx, ups, order=order) == -1
    assert _abi(ctx, ups, tstops=(0.3, 0.6)) == -1                 # unsorted for tspan (1, 0)
    assert "tstops" in ctx.lib.dre_last_error(ctx.ptr).decode()
    assert _abi(ctx, ups, tstops=(1.0,)) == -1 and _abi(ctx, ups, tstops=(0.0,)) == -1
    assert _abi(ctx, ups, dt0=0.5) == -1 and _abi(ctx, ups, dt0=0.0) == -1
    assert "dt0" in ctx.lib.dre_last_error(ctx.ptr).decode()
    assert _abi(ctx, ups, rtol=0.0) == -1 and _abi(ctx, ups, atol=0.0) == -1 and _abi(ctx, ups, atol=-1.0) == -1
    assert _abi(ctx, ups, dt_min=0.2, dt_max=0.1) == -1 and _abi(ctx, ups, max_steps=0) == -1
    r = C.c_void_p()
    assert ctx.lib.dre_dense_gdre_solve(ctx.ptr, *[u.ptr for u in ups], 1.0, 0.9, -0.05, 2, 0, 50, 0.0, 2, C.byref(r)) == 0
    acc = (C.c_int64 * 2)()
    assert ctx.lib.dre_gdre_result_step_stats(r, acc, None) == -1       # a fixed-step result has no step statistics
    ctx.lib.dre_gdre_result_free(r)
