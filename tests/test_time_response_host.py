"""CPU side of the time response (csrc/time_response.hip): the NumPy model (tests/_time_response_model.py) against the record
tests/golden/time_response.json, closed forms for the scalar systems, the model at block 1 against the sequential recurrence, the convergence
orders against the recorded exact step response, and the argument errors of the Python layer, which are raised before anything touches a
device."""
import os

import numpy as np
import pytest

import dre_amd as D
import _time_response_cases as tc
import _time_response_model as tm

EPS = np.finfo(float).eps


def test_version_is_at_least_117():
    assert D._lib.load().dre_version() >= 117


def test_the_record_is_small_and_covers_every_case():
    assert os.path.getsize(tc.record_path()) + os.path.getsize(tc.arrays_path()) < 1_000_000
    for name, me, ki in tc.ALL:
        Y, md, ld = tc.recorded_case(name, me, ki)
        E, A, B, C = tc.system(name)
        dt, K = tc.GRID[name]
        u, _ = tc.signals(name)
        assert Y.shape == ((u.shape[0], K + 1, C.shape[0]) if ki == "simulate" else (K + 1, C.shape[0], B.shape[1]))
        assert np.isfinite(Y).all() and md.shape == ld.shape == ((u.shape[0],) if ki == "simulate" else ())
        assert tc.recorded()["grid"][name] == [dt, K]
    for name in tc.STEADY:
        assert tc.recorded()["steady"][name]["rho_K"] < 1e-17


def test_the_signals_are_exact_dyadic_rationals():
    u, x0 = tc.signals("pencil33")
    assert u.shape == (3, 128, 7) and x0.shape == (3, 33) and (x0[0] == 0).all()
    assert (u * 2 ** 23 == np.round(u * 2 ** 23)).all() and np.abs(u).max() < 1.0 and len(np.unique(u)) > 2000


@pytest.mark.parametrize("name,me,ki", tc.ALL, ids=lambda v: str(v))
def test_model_against_the_record(name, me, ki):
    """the model at the default block within 10 x the plain recurrence's recorded distance (floored at 2 n eps), and where the record says it was"""
    Y, md, ld = tc.recorded_case(name, me, ki)
    n = tc.system(name)[0].shape[0]
    d = np.asarray(tc.dist(ki, tc.model(name, me, ki), Y))
    print(name, me, ki, "model", d, "recorded", md, "lapack", ld)
    assert (d <= np.maximum(10.0 * ld, 2 * n * EPS)).all()
    assert (d <= np.maximum(2.0 * md, 2 * n * EPS)).all()      # this machine's LAPACK against the recording one's


@pytest.mark.parametrize("L", tc.MODEL_BLOCKS)
def test_the_block_length_does_not_cost_accuracy(L):
    """osc12 (rho(M) = 1 - 1e-7, ||M|| = 2.7) and a pencil at L = 4, 64, 256: the recorded distances of the model at that block stay within 2 x
    the default block's; osc12 at or below 2e-14 relative to the step response it was measured on"""
    for name in ("osc12", "pencil33", "pencil371"):
        for me, ki in tc.present(name):
            r = tc.recorded()["cases"][name][me][ki]
            dl, d0 = np.asarray(r["model_dist_L"][str(L)]), np.asarray(r["model_dist"])
            assert (dl <= 2.0 * np.maximum(d0, EPS)).all(), (name, me, ki, dl, d0)
    E, A, B, C = tc.system("osc12")
    dt, K = tc.GRID["osc12"]
    Y0 = tm.step_response(E, A, B, C, dt, K, "tustin", block=1)
    assert tm.rel_dist(tm.step_response(E, A, B, C, dt, K, "tustin", block=L), Y0) <= 2e-14


@pytest.mark.parametrize("name", ["scalar1", "unstable1"])
@pytest.mark.parametrize("me", tm.METHODS)
def test_closed_forms_of_the_scalars(name, me):
    """y_k = c M^k x_0 (free response), c M^k b / e (impulse) and the geometric sum beta c N (M^k - 1) / (M - 1) (step)"""
    E, A, B, C = tc.system(name)
    e, a, b, c = E[0, 0], A[0, 0], B[0, 0], C[0, 0]
    dt, K = tc.GRID[name]
    th, beta = tm.theta_beta(me, dt)
    M = (2 * e / (e - th * a) - 1) if me == "tustin" else e / (e - th * a)
    N = th * b / (e - th * a)
    k = np.arange(K + 1)
    if name == "unstable1":
        assert M > 1.0
    tol = 4 * (K + 2) * EPS
    step = beta * c * N * (M ** k - 1) / (M - 1)
    Ys = tm.step_response(E, A, B, C, dt, K, me)[:, 0, 0]
    assert np.abs(Ys - step).max() <= tol * np.abs(step).max()
    imp = c * M ** k * b / e
    assert np.abs(tm.impulse_response(E, A, B, C, dt, K, me)[:, 0, 0] - imp).max() <= tol * np.abs(imp).max()
    free = tm.simulate(E, A, B, C, np.zeros((K + 1, 1)), dt, x0=np.array([1.25]), method=me)[:, 0]
    assert np.abs(free - c * M ** k * 1.25).max() <= tol * np.abs(free).max()
    # and the record agrees with the closed form
    assert np.abs(tc.recorded_case(name, me, "step")[0][:, 0, 0] - step).max() <= tol * np.abs(step).max()


@pytest.mark.parametrize("name", ["osc12", "index1_6", "pencil33_m1"])
def test_block_one_is_the_sequential_recurrence(name):
    """at L = 1 the stack is built row by row, G_{k+1} = G_k M: the same numbers as stepping the state, up to the order of the products"""
    E, A, B, C = tc.system(name)
    dt, K = tc.GRID[name]
    K = min(K, 200)
    u, x0 = tc.signals(name)
    n = E.shape[0]
    for me, ki in tc.present(name):
        if ki == "step":
            Y, info = tm.step_response(E, A, B, C, dt, K, me, block=1, return_info=True)
            assert info == dict(block=1, blocks=K + 1, squarings=0)
        elif ki == "impulse":
            Y = tm.impulse_response(E, A, B, C, dt, K, me, block=1)
        else:
            Y = tm.simulate(E, A, B, C, u[1][:K + 1], dt, x0[1], me, block=1)
        Ys = tm.sequential(E, A, B, C, dt, K, me, ki, u[1][:K + 1], x0[1])
        _, md, ld = tc.recorded_case(name, me, ki)
        assert tm.rel_dist(Y, Ys) <= max(10.0 * float(np.max(np.maximum(md, ld))), 2 * n * EPS), (name, me, ki)


def test_default_block_rule():
    # n = 4096: 64 tile columns, L q >= 256; n = 1357: 22, L q >= 768; n = 371: 6, L q >= 2752
    assert tm.default_block(4, 8192, 4096) == 64 and tm.default_block(4, 8192, 1357) == 256 and tm.default_block(4, 8192, 371) == 1024
    # K + 1 = 1025: 1024 and 512 would round the stack up to 2048 and 1536 rows of samples; 256 gives 1280 <= 5/4 * 1025
    assert tm.default_block(4, 1024, 371) == 256 and tm.default_block(4, 1023, 371) == 1024
    assert tm.default_block(5, 127, 33) == 128 and tm.default_block(5, 64, 33) == 16 and tm.default_block(5, 63, 33) == 64
    assert tm.default_block(512, 100, 4096) == 1 and tm.default_block(1, 1, 1) == 2 and tm.default_block(2, 5, 12) == 2
    assert tm.block_in_force(5, 3, 33, 256) == 4 and tm.block_in_force(5, 1000, 33, 4) == 4
    O, nb, sq = tm.markov_stack(np.ones((1, 1)), np.array([[0.5]]), 8, 4)
    assert nb == 3 and sq == 2 and np.array_equal(O[:9, 0], 0.5 ** np.arange(9))


def test_orders_of_the_two_schemes():
    """against the exact (zero-order-hold) step response of pencil33 on T = 6.4: the error falls by 4 per halving of dt under tustin, by 2
    under backward Euler"""
    errs = tc.order_errors(lambda E, A, B, C, dt, K, me: tm.step_response(E, A, B, C, dt, K, me))
    for me, (lo, hi) in (("tustin", (3.6, 4.4)), ("backward_euler", (1.8, 2.2))):
        e = errs[me]
        print(me, e, e[0] / e[1], e[1] / e[2])
        assert lo <= e[0] / e[1] <= hi and lo <= e[1] / e[2] <= hi


def test_step_equals_simulate_with_unit_steps_in_the_model():
    E, A, B, C = tc.system("pencil33_q1")
    dt, K = tc.GRID["pencil33_q1"]
    Y = tm.step_response(E, A, B, C, dt, K, "tustin")
    for c in (0, 6):
        u = np.zeros((K + 1, 7))
        u[:, c] = 1.0          # a unit step held from t_0 on: w_k = 2 under tustin, y_k = 2 sum_{j<k} h_j
        assert tm.rel_dist(tm.simulate(E, A, B, C, u, dt, method="tustin")[:, :, None], Y[:, :, c:c + 1]) <= 100 * 33 * EPS


# ---- argument errors: before anything touches a device ------------------------------------------------------------------------------------
class _NoDevice:
    def __getattr__(self, name):
        raise AssertionError("the device was touched")


def test_argument_errors_of_the_python_layer():
    E, A, B, C = tc.system("pencil33_m1")
    ctx = _NoDevice()
    msg = "nothing was run on the device"
    bad = [dict(dt=0.0), dict(dt=-0.1), dict(dt=np.nan), dict(dt=np.inf), dict(steps=0), dict(steps=-3), dict(method="zoh"), dict(method=None),
           dict(block=0), dict(block=3), dict(block=-4), dict(block=2.0), dict(block=True)]
    for kw in bad:
        args = dict(dt=0.1, steps=10)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            D.step_response(E, A, B, C, ctx=ctx, **args)
        with pytest.raises(ValueError, match=msg):
            D.impulse_response(E, A, B, C, ctx=ctx, **args)
        if "steps" not in kw:
            args.pop("steps")
            with pytest.raises(ValueError, match=msg):
                D.simulate(E, A, B, C, np.zeros((11, 1)), ctx=ctx, **args)
    for kw in (dict(dt="0.1", steps=10), dict(dt=True, steps=10), dict(dt=0.1, steps=2.5), dict(dt=0.1, steps=True)):
        with pytest.raises(TypeError, match=msg):
            D.step_response(E, A, B, C, ctx=ctx, **kw)
        with pytest.raises(TypeError, match=msg):
            D.impulse_response(E, A, B, C, ctx=ctx, **kw)
    for mats in ((E[:7], A, B, C), (E, A[:, :7], B, C), (E, A, B[:7], C), (E, A, B, C[:, :7]), (E, A, B[:, :0], C), (E, A, B, C[:0])):
        with pytest.raises(ValueError, match=msg):
            D.step_response(*mats, 0.1, 10, ctx=ctx)
        with pytest.raises(ValueError, match=msg):
            D.impulse_response(*mats, 0.1, 10, ctx=ctx)
        with pytest.raises(ValueError, match=msg):
            D.simulate(*mats, np.zeros((11, 1)), 0.1, ctx=ctx)
    with pytest.raises(TypeError, match=msg):
        D.step_response("E", A, B, C, 0.1, 10, ctx=ctx)
    with pytest.raises(TypeError, match=msg):
        D.simulate(E, A, B, None, np.zeros((11, 1)), 0.1, ctx=ctx)
    with pytest.raises(ValueError, match="D must be q x m"):
        D.step_response(E, A, B, C, 0.1, 10, D=np.zeros((2, 2)), ctx=ctx)
    with pytest.raises(ValueError, match="D must be q x m"):
        D.simulate(E, A, B, C, np.zeros((11, 1)), 0.1, D=np.zeros((1, 5)), ctx=ctx)
    # simulate's own
    nan_u = np.zeros((11, 1))
    nan_u[3] = np.nan
    for u in (np.zeros(11), np.zeros((11, 2)), np.zeros((2, 11, 3)), np.zeros((1, 11)), np.zeros((1, 1)), np.zeros((2, 2, 11, 1)), nan_u,
              np.full((11, 1), np.inf), np.zeros((0, 11, 1))):
        with pytest.raises(ValueError, match=msg):
            D.simulate(E, A, B, C, u, 0.1, ctx=ctx)
    with pytest.raises(TypeError, match=msg):
        D.simulate(E, A, B, C, "u", 0.1, ctx=ctx)
    with pytest.raises(TypeError, match=msg):
        D.simulate(E, A, B, C, 3.0, 0.1, ctx=ctx)
    for x0 in (np.zeros(32), np.zeros((2, 33)), np.zeros((33, 1)), np.full(33, np.nan), np.full(33, -np.inf)):
        with pytest.raises(ValueError, match=msg):
            D.simulate(E, A, B, C, np.zeros((11, 1)), 0.1, x0=x0, ctx=ctx)
    with pytest.raises(ValueError, match=msg):
        D.simulate(E, A, B, C, np.zeros((3, 11, 1)), 0.1, x0=np.zeros((2, 33)), ctx=ctx)
    with pytest.raises(ValueError, match="q <= 256"):
        D.simulate(np.eye(300), -np.eye(300), np.ones((300, 1)), np.eye(300), np.zeros((3, 1)), 0.1, ctx=ctx)


def test_argument_errors_of_the_reduced_models():
    ctx = _NoDevice()
    msg = "nothing was run on the device"
    rom = D.ReducedModel(np.eye(2), -np.eye(2), np.ones((2, 2)), np.ones((3, 2)), np.array([1.0, 0.5, 0.1]), np.zeros((8, 2)), np.zeros((8, 2)))
    z = np.zeros((2, 2))
    lqg = D.LQGReducedModel(np.eye(2), -np.eye(2), np.ones((2, 2)), np.ones((3, 2)), np.array([1.0, 0.5]), np.zeros((8, 2)), np.zeros((8, 2)), z,
                            np.zeros((2, 3)), z)
    for model in (rom, lqg):
        with pytest.raises(ValueError, match=msg):
            model.step_response(0.0, 10, ctx=ctx)
        with pytest.raises(ValueError, match=msg):
            model.step_response(0.1, 0, ctx=ctx)
        with pytest.raises(ValueError, match=msg):
            model.step_response(0.1, 10, method="euler", ctx=ctx)
        with pytest.raises(ValueError, match="D must be q x m"):
            model.step_response(0.1, 10, D=np.zeros((2, 2)), ctx=ctx)
        with pytest.raises(ValueError, match=msg):
            model.impulse_response(np.nan, 10, ctx=ctx)
        with pytest.raises(ValueError, match=msg):
            model.impulse_response(0.1, 10, block=6, ctx=ctx)
        with pytest.raises(ValueError, match=msg):
            model.simulate(np.zeros((11, 3)), 0.1, ctx=ctx)
        with pytest.raises(ValueError, match=msg):
            model.simulate(np.zeros((11, 2)), 0.1, x0=np.zeros(3), ctx=ctx)
        with pytest.raises(ValueError, match="non-finite"):
            model.simulate(np.full((11, 2), np.nan), 0.1, ctx=ctx)
