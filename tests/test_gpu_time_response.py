"""Time response on the device (step_response, impulse_response, simulate and the reduced models' methods; csrc/time_response.hip) against
the record tests/golden/time_response.json (arrays in time_response_ref.npz): Y from the sequential recurrence in mpmath at 50 digits (n <= 70) or from a refined LU and
numpy.longdouble (n = 371), with the NumPy model's and the plain float64 recurrence's recorded distance to it.

Distance:  max_k ||Y_k - Yref_k||_F / max_k ||Yref_k||_F.   Accuracy bound:  max(10 x max(model's, LAPACK's recorded distance), 2 n eps).
The factor 10 is the project's convention for device against model; the distances come from the record, never from the code under test."""
import numpy as np
import pytest

import dre_amd as D
import _balance_cases as bc
import _lqg_model as lm
import _time_response_cases as tc
import _time_response_model as tm

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps


def _device(ctx, name, me, ki, **kw):
    E, A, B, C = tc.system(name)
    dt, K = tc.GRID[name]
    if ki == "step":
        return D.step_response(E, A, B, C, dt, K, method=me, ctx=ctx, **kw)
    if ki == "impulse":
        return D.impulse_response(E, A, B, C, dt, K, method=me, ctx=ctx, **kw)
    u, x0 = tc.signals(name)
    return D.simulate(E, A, B, C, u, dt, x0=x0, method=me, ctx=ctx, **kw)


# ---- 1. accuracy --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,me,ki", tc.ALL, ids=lambda v: str(v))
def test_accuracy_against_the_record(ctx, name, me, ki):
    Yref, md, ld = tc.recorded_case(name, me, ki)
    Y, info = _device(ctx, name, me, ki, return_info=True)
    assert Y.shape == Yref.shape and Y.dtype == float
    q, K = tc.system(name)[3].shape[0], tc.GRID[name][1]
    assert info["block"] == tm.default_block(q, K, tc.system(name)[0].shape[0]) and info["blocks"] == -(-(K + 1) // info["block"]) and info["method"] == me
    d, bound = np.asarray(tc.dist(ki, Y, Yref)), tc.bound(name, me, ki)
    print(name, me, ki, "device", d, "| model", md, "| lapack", ld, "| bound", bound, "|", info)
    assert (d <= bound).all()


# ---- 2. block edges -----------------------------------------------------------------------------------------------------------------------
def _edge_steps():
    """(block, K): K + 1 in {L, L + 1, 2L - 1, 2L} for the L in force, K = 1, K + 1 a power of two.  The default block follows K (64, 16, 32 and 128
    at K + 1 = 64, 65, 127 and 128): these four are an exact fit, a ragged last block, a block short of one row, and doubling alone"""
    out = []
    for block in (1, 4, None):
        L = block or 64
        for K1 in sorted({L, L + 1, 2 * L - 1, 2 * L, 2, 32}):
            if K1 >= 2:
                out.append((block, K1 - 1))
    return out


@pytest.mark.parametrize("block,K", _edge_steps())
@pytest.mark.parametrize("ki", ["step", "impulse"])
def test_block_edges(ctx, block, K, ki):
    E, A, B, C = tc.system("pencil33")
    dt = tc.GRID["pencil33"][0]
    Yref = tc.recorded_case("pencil33", "tustin", ki)[0][:K + 1]
    f = D.step_response if ki == "step" else D.impulse_response
    Y, info = f(E, A, B, C, dt, K, block=block, ctx=ctx, return_info=True)
    L = tm.block_in_force(5, K, 33, block)
    assert info["block"] == L and info["blocks"] == -(-(K + 1) // L) and info["squarings"] == tm.markov_stack(C, np.eye(33), K, L)[2]
    d = tm.rel_dist(Y, Yref)
    print(ki, "block", block, "K", K, info, "distance", d)
    # a prefix of the recorded response: the bound of the whole response, on the prefix's own scale
    assert d <= tc.bound("pencil33", "tustin", ki)


# ---- 3. simulate --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("me", tm.METHODS)
def test_simulate_scenarios(ctx, me):
    name = "pencil33"
    E, A, B, C = tc.system(name)
    dt, K = tc.GRID[name]
    u, x0 = tc.signals(name)
    Yref, _, _ = tc.recorded_case(name, me, "simulate")
    bound = tc.bound(name, me, "simulate")
    Y3 = D.simulate(E, A, B, C, u, dt, x0=x0, method=me, ctx=ctx)
    assert Y3.shape == (3, K + 1, 5)
    assert (tc.sim_dist(Y3, Yref) <= bound).all()
    Dm = np.arange(35.0).reshape(5, 7) / 35.0
    for s in range(3):
        Y1 = D.simulate(E, A, B, C, u[s], dt, x0=x0[s], method=me, ctx=ctx)
        assert Y1.shape == (K + 1, 5)
        assert tm.rel_dist(Y1, Yref[s]) <= bound[s] and tm.rel_dist(Y3[s], Y1) <= bound[s]
        assert np.array_equal(D.simulate(E, A, B, C, u[s], dt, x0=x0[s], D=Dm, method=me, ctx=ctx), Y1 + u[s] @ Dm.T)
    # without x0: scenario 0 of the record starts from zero
    Y0 = D.simulate(E, A, B, C, u[0], dt, method=me, ctx=ctx)
    assert tm.rel_dist(Y0, Yref[0]) <= bound[0]
    assert np.array_equal(D.simulate(E, A, B, C, u[:1], dt, method=me, ctx=ctx)[0], Y0)
    # one x0 for all scenarios
    Yb = D.simulate(E, A, B, C, u, dt, x0=x0[2], D=Dm, method=me, ctx=ctx)
    assert tm.rel_dist(Yb[2] - u[2] @ Dm.T, Yref[2]) <= bound[2]


@pytest.mark.parametrize("name,me", [("pencil33", "tustin"), ("pencil33", "backward_euler"), ("index1_6", "backward_euler")])
def test_step_response_is_simulate_with_unit_steps(ctx, name, me):
    E, A, B, C = tc.system(name)
    dt, K = tc.GRID[name]
    m = B.shape[1]
    Ys = D.step_response(E, A, B, C, dt, K, method=me, ctx=ctx)
    u = np.zeros((m, K + 1, m))
    for c in range(m):
        u[c, :, c] = 1.0
    Yu = D.simulate(E, A, B, C, u, dt, method=me, ctx=ctx)
    d = tm.rel_dist(Yu.transpose(1, 2, 0), Ys)
    print(name, me, d)
    assert d <= tc.bound(name, me, "step")


# ---- 4. determinism -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ki", tc.KINDS)
def test_the_same_call_twice_gives_the_same_bits(ctx, ki):
    a, b = _device(ctx, "pencil70", "tustin", ki), _device(ctx, "pencil70", "tustin", ki)
    assert np.array_equal(a, b)
    a, b = _device(ctx, "osc12", "backward_euler", ki, block=16), _device(ctx, "osc12", "backward_euler", ki, block=16)
    assert np.array_equal(a, b)


# ---- 5. failures --------------------------------------------------------------------------------------------------------------------------
def test_singular_pencils_and_a_growing_response(ctx):
    one = np.array([[1.0]])
    with pytest.raises(D.DREError) as e:          # P = E - (dt/2) A = 1 - 1 = 0
        D.step_response(one, 2.0 * one, one, one, 1.0, 4, ctx=ctx)
    assert e.value.code == -4 and "singular" in str(e.value)
    E, A, B, C = tc.system("index1_6")
    with pytest.raises(D.DREError) as e:
        D.impulse_response(E, A, B, C, 0.1, 8, method="backward_euler", ctx=ctx)
    assert e.value.code == -4 and "E" in str(e.value)
    E, A, B, C = (np.array(M) for M in tc.system("pencil33"))
    A[4, 9] = np.nan
    with pytest.raises(D.DREError) as e:
        D.step_response(E, A, B, C, 0.05, 8, ctx=ctx)
    assert e.value.code == -4
    with pytest.raises(D.DREError) as e:
        D.simulate(E, A, B, C, np.ones((9, 7)), 0.05, ctx=ctx)
    assert e.value.code == -4
    # the context lives on; the unstable scalar runs and matches its closed form
    E, A, B, C = tc.system("unstable1")
    dt, K = tc.GRID["unstable1"]
    for me in tm.METHODS:
        th, beta = tm.theta_beta(me, dt)
        M = (2 / (1 - th * 0.5) - 1) if me == "tustin" else 1 / (1 - th * 0.5)
        N = th * 1.5 / (1 - th * 0.5)
        k = np.arange(K + 1)
        step = beta * 0.7 * N * (M ** k - 1) / (M - 1)
        Y = D.step_response(E, A, B, C, dt, K, method=me, ctx=ctx)[:, 0, 0]
        assert M > 1 and Y[-1] > Y[1] > 0
        assert np.abs(Y - step).max() <= 4 * (K + 2) * EPS * np.abs(step).max()
        Yi = D.impulse_response(E, A, B, C, dt, K, method=me, ctx=ctx)[:, 0, 0]
        assert np.abs(Yi - 0.7 * 1.5 * M ** k).max() <= 4 * (K + 2) * EPS * np.abs(Yi).max()


def test_the_c_entry_rejects_bad_arguments_before_any_launch(ctx):
    import ctypes as C_
    E, A, B, C = (ctx.upload(np.asfortranarray(M)) for M in tc.system("pencil33"))
    lib, pd = ctx.lib, C_.POINTER(C_.c_double)
    Y = np.full(9 * 35, 7.0)
    U = np.zeros(9 * 7)

    def call(Eh=E, Ah=A, Bh=B, Ch=C, method=0, dt=0.05, K=8, kind=0, Up=None, S=0, X0=None, block=0, Yp=Y.ctypes.data_as(pd)):
        return lib.dre_time_response(ctx.ptr, Eh.ptr if Eh is not None else None, Ah.ptr, Bh.ptr, Ch.ptr, method, dt, K, kind, Up, S, X0, block, Yp, None)
    up = U.ctypes.data_as(pd)
    assert call(K=0) == -1 and b"K >= 1" in lib.dre_last_error(ctx.ptr)
    assert call(dt=0.0) == -1 and call(dt=-1.0) == -1 and call(dt=float("nan")) == -1 and call(dt=float("inf")) == -1
    assert call(method=2) == -1 and call(method=-1) == -1 and call(kind=3) == -1 and call(kind=-1) == -1
    assert call(block=3) == -1 and call(block=-2) == -1 and call(block=48) == -1
    assert call(Bh=C) == -1 and call(Ch=B) == -1 and call(Eh=B) == -1 and call(Ah=C) == -1
    assert call(Eh=None) == -1 and call(Yp=None) == -1
    assert call(kind=2) == -1 and call(kind=2, Up=up, S=0) == -1 and call(kind=0, Up=up, S=1) == -1
    assert (Y == 7.0).all()
    # and it works afterwards, with info
    info = (C_.c_int64 * 4)()
    assert lib.dre_time_response(ctx.ptr, E.ptr, A.ptr, B.ptr, C.ptr, 0, 0.05, 8, 0, None, 0, None, 4, Y.ctypes.data_as(pd), info) == 0
    assert list(info)[:3] == [4, 3, 2] and info[3] > 0
    Yd = Y.reshape(9, 7, 5).transpose(0, 2, 1)
    assert tm.rel_dist(Yd, tc.recorded_case("pencil33", "tustin", "step")[0][:9]) <= tc.bound("pencil33", "tustin", "step")


# ---- 6. cross-checks between device paths -------------------------------------------------------------------------------------------------
def test_the_step_response_settles_on_the_static_gain(ctx):
    """tustin's fixed point is x = -A^-1 B exactly, whatever dt: at dt = 4 and K = 64, rho(M)^K < 1e-17 (recorded), the last sample of the step
    response is the frequency response at omega = 0"""
    name = "pencil33"
    st = tc.recorded()["steady"][name]
    assert st["rho_K"] < 1e-17
    E, A, B, C = tc.system(name)
    Y = D.step_response(E, A, B, C, st["dt"], st["K"], ctx=ctx)
    H0 = D.freq_response(E, A, B, C, [0.0], ctx=ctx)[0].real
    tol = max(10.0 * max(st["model_last_dist"], st["model_dist"]), 2 * 33 * EPS)
    d = np.linalg.norm(Y[-1] - H0) / np.linalg.norm(H0)
    print("||y_K - H(0)|| / ||H(0)|| =", d, "tolerance", tol)
    assert d <= tol
    assert np.linalg.norm(Y[-1] - tc.dec(st["Y_last"])) <= tol * np.linalg.norm(H0)


def test_balanced_truncation_keeps_the_steady_state_within_its_bound(ctx):
    """||y_K - y_r,K||_2 at a K where both have settled is ||H(0) - H_r(0)||_2 <= 2 sum_{i > r} hsv_i, plus the two accuracy bounds times the
    scale"""
    name, r = "pencil70", 12
    st = tc.recorded()["steady"][name]
    E, A, B, C = bc.system(70)
    rom = D.balanced_truncation(E, A, B, C, order=r, ctx=ctx)
    Y = D.step_response(E, A, B, C, st["dt"], st["K"], ctx=ctx)
    Yr = rom.step_response(st["dt"], st["K"], ctx=ctx)
    acc = max(10.0 * max(st["model_dist"], st["lapack_dist"]), 2 * 70 * EPS)
    bound = 2.0 * float(np.sum(rom.hsv[r:][::-1]))
    err = np.linalg.norm(Y[-1] - Yr[-1], 2)
    print("steady-state error", err, "truncation bound", bound, "accuracy terms", acc * (np.linalg.norm(Y[-1]) + np.linalg.norm(Yr[-1])))
    assert err <= bound + acc * (np.linalg.norm(Y[-1]) + np.linalg.norm(Yr[-1]))
    assert err > 0.0


# ---- 7. order -----------------------------------------------------------------------------------------------------------------------------
def test_orders_of_the_two_schemes(ctx):
    errs = tc.order_errors(lambda E, A, B, C, dt, K, me: D.step_response(E, A, B, C, dt, K, method=me, ctx=ctx))
    for me, (lo, hi) in (("tustin", (3.6, 4.4)), ("backward_euler", (1.8, 2.2))):
        e = errs[me]
        print(me, e, e[0] / e[1], e[1] / e[2])
        assert lo <= e[0] / e[1] <= hi and lo <= e[1] / e[2] <= hi


# ---- 8. the reduced models' methods -------------------------------------------------------------------------------------------------------
def test_reduced_model_methods_are_the_free_functions(ctx):
    E, A, B, C = bc.system(33)
    rom = D.balanced_truncation(E, A, B, C, order=8, ctx=ctx)
    lqg = D.lqg_balanced_truncation(*lm.system(33), order=6, ctx=ctx)
    rng = np.random.default_rng(5)
    for model in (rom, lqg):
        r, m, q = model.order, model.Br.shape[1], model.Cr.shape[0]
        u, x0, Dm = rng.standard_normal((2, 41, m)), rng.standard_normal((2, r)), rng.standard_normal((q, m))
        mats = (np.eye(r), model.Ar, model.Br, model.Cr)
        assert np.array_equal(model.step_response(0.1, 40, D=Dm, ctx=ctx), D.step_response(*mats, 0.1, 40, D=Dm, ctx=ctx))
        assert np.array_equal(model.step_response(0.1, 40, method="backward_euler", block=4, ctx=ctx),
                              D.step_response(*mats, 0.1, 40, method="backward_euler", block=4, ctx=ctx))
        assert np.array_equal(model.impulse_response(0.1, 40, ctx=ctx), D.impulse_response(*mats, 0.1, 40, ctx=ctx))
        assert np.array_equal(model.simulate(u, 0.1, x0=x0, D=Dm, ctx=ctx), D.simulate(*mats, u, 0.1, x0=x0, D=Dm, ctx=ctx))
        Y = model.step_response(0.1, 40, ctx=ctx)
        assert Y.shape == (41, q, m) and np.isfinite(Y).all() and np.abs(Y[-1]).max() > 0
