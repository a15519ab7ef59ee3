"""Round 5: the warm-started compression of the dense-X time loop (csrc/warm.hip), the recurrence loop's state without E'L,
option snapshots (dre_ctx_get_option), configs[4] at its stated length through size-independent properties.

Criteria as in the reference's tests: delta(K_hip(t), K_oracle(t)) < 1e-7 (test/cuda.jl:95-99), the oracle's ADI iteration count of every
Lyapunov solve, ||K_dense - K_lr|| < ||K_dense|| n eps 100 against the dense Rosenbrock solver (test/rail.jl:52-70)."""
import os
import warnings

import numpy as np
import pytest

import dre_amd as D
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps


def _shifts(n):
    return list(np.load(os.path.join(GOLDEN, f"heuristic_shifts_{n}.npy")))


def _ros1(n, nsteps, ctx, **kw):
    d = D.steel_profile(n)
    L, Dm = D.initial_value(d)
    prob = D.GDREProblem(d.E, d.A, d.B, d.C, D.lowrank(L, Dm), (4500.0, 4500.0 - 100.0 * nsteps))
    return D.solve_gdre(prob, D.Ros1(D.ADI(shifts=D.Shifts.Cyclic(_shifts(n)), maxiters=200)), dt=-100.0, return_stats=True, ctx=ctx, **kw)


@pytest.mark.parametrize("warm", [1, 2, 0])
def test_warm_started_residual_compression_keeps_every_iteration_count(ctx, warm):      # lyapunov/residual.jl:3-31 -> LDLt.jl:204-225
    """The metric's configuration (SteelProfile(371), Ros1, 45 steps) with the warm-started compression of the Riccati residual (default; 2: with
    16 spare directions in the basis) and without it: the same 746 ADI iterations step by step as the oracle, K(t) within the reference's
    criterion at every step, and the warm path really ran (the widths of the residual factors fall to the numerical rank)."""
    g = np.load(os.path.join(GOLDEN, "ros1_371_full.npz"))
    with ctx.options(dense_warm=warm):
        sol, st = _ros1(371, 45, ctx)
    its = [x["iters"] for x in st["gales"]]
    assert its == [int(v) for v in g["iters"]] and sum(its) == 746
    assert all(x["converged"] for x in st["gales"])
    for i in range(46):
        assert D.delta(sol.K[i], g["K"][i]) < 1e-7, i
    tol = np.linalg.norm(g["K_dense"][-1]) * 371 * EPS * 100
    assert np.linalg.norm(sol.K[-1] - g["K_dense"][-1]) < max(tol, 2 * np.linalg.norm(g["K"][-1] - g["K_dense"][-1]))
    cols = [x["rhs_cols"] for x in st["gales"]]
    if warm and ctx.get_option("dense_x_max_n") >= 371 and ctx.get_option("dense_inverse_max_n") >= 371:
        assert min(cols[12:]) <= 8 and max(cols[12:]) <= 16, cols         # the eigenbasis path reports the rank it kept (where the dense-X loop is on)
    elif not warm:
        assert min(cols[1:]) >= 16 and all(c % 16 == 0 for c in cols[1:]), cols  # the band reduction stops at panel boundaries


def test_warm_compression_in_chained_solves_with_another_step_size(ctx):
    """Two solves in a row, the second started from the first one's X with a step size four times smaller (another operator, another cycle of
    factorisations, a fresh eigenbasis job): the warm path against the same chain without it."""
    d = D.steel_profile(371)
    L, Dm = D.initial_value(d)
    alg = D.Ros1(D.ADI(shifts=D.Shifts.Cyclic(_shifts(371)), maxiters=200))
    Ks = {}
    for warm in (1, 0):
        with ctx.options(dense_warm=warm):
            p1 = D.GDREProblem(d.E, d.A, d.B, d.C, D.lowrank(L, Dm), (4500.0, 2500.0))
            s1 = D.solve_gdre(p1, alg, dt=-100.0, ctx=ctx)
            p2 = D.GDREProblem(d.E, d.A, d.B, d.C, s1.X[-1], (2500.0, 2100.0))
            s2 = D.solve_gdre(p2, alg, dt=-25.0, ctx=ctx)
            Ks[warm] = (s1.K[-1], s2.K[-1])
    assert D.delta(Ks[1][0], Ks[0][0]) < 1e-9 and D.delta(Ks[1][1], Ks[0][1]) < 1e-9


def test_recurrence_loop_state_without_EtL(ctx):                 # ADVICE round 4 (gdre.hip, ros1_recurrence_loop: the `!intact` branch)
    """n = 1357 forced onto the general path (multifrontal solves, residual recurrence) with the factor-form limit c + 64 <= n so tight that the
    ADI compresses X INSIDE a solve: the state published by that branch carried no E'L, and two steps later the deferred tolerance was formed
    from unwritten columns.  The run must agree with the oracle's 45-step fixture on its first steps."""
    g = np.load(os.path.join(GOLDEN, "ros1_1357_full.npz"))
    with ctx.options(dense_inverse_max_n=0, dense_x_max_n=0, compress_factor_min_n=1024, compress_direct_max_n=0):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sol, st = _ros1(1357, 8, ctx)
    its, ref = [x["iters"] for x in st["gales"]], [int(v) for v in g["iters"][:8]]
    assert all(x["converged"] for x in st["gales"])
    assert max(abs(a - b) for a, b in zip(its, ref)) <= 1, (its, ref)
    for i in range(9):
        assert D.delta(sol.K[i], g["K"][i]) < 1e-7, i


def test_options_can_be_read_back(ctx):
    old = ctx.get_option("adi_fan")
    with ctx.options(adi_fan=3, adi_fan_max_coef=17.5):
        assert ctx.get_option("adi_fan") == 3 and ctx.get_option("adi_fan_max_coef") == 17.5
    assert ctx.get_option("adi_fan") == old
    with pytest.raises(D.DREError):
        ctx.get_option("no_such_option")


def test_options_from_the_environment_are_parsed_strictly():
    """DRE_OPTIONS with a typo must fail the context creation instead of silently running the defaults."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import sys; sys.path.insert(0, %r); import dre_amd as D\ntry:\n    D.Context(0)\n    print('CREATED')\nexcept D.DREError as e:\n    print('REFUSED', e)\n" % root
    for bad in ("adi_fan:0", "adi_fan=off", "adi_fan=3x", "=3"):
        out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, DRE_OPTIONS=bad), capture_output=True, text=True, timeout=300).stdout
        assert "REFUSED" in out and "CREATED" not in out, (bad, out)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, DRE_OPTIONS=" adi_fan = 3 , dense_warm=0"), capture_output=True, text=True, timeout=300).stdout
    assert "CREATED" in out, out


def test_config4_ros1_20209_save_state_all_45_steps_properties(ctx):         # lowrank_ros1.jl:50-61, README.md:78,85
    """BASELINE configs[4] at its STATED length: SteelProfile(20209) Ros1, save_state = true, tspan = (4500, 0), dt = -100 — 45 steps.  The oracle
    needs 26 minutes for 12 of them, so the whole run is held to size-independent properties: the first 12 steps equal the oracle's fixture
    (counts, sampled K(t)); every Lyapunov solve converges; at every 5th step K_i = B'X_iE from the downloaded factors of the stored X_i, the
    residual of the step's Lyapunov equation evaluated FROM SCRATCH (dre_gale_residual) is at the tolerance, and the rank of X(t) stays in a
    band; the iteration counts fall monotonically as X(t) approaches the steady state."""
    n = 20209
    d = D.steel_profile(n)
    L, Dm = D.initial_value(d)
    g = np.load(os.path.join(GOLDEN, "ros1_20209_ss12.npz"))
    prob = D.GDREProblem(d.E, d.A, d.B, d.C, D.lowrank(L, Dm), (4500.0, 0.0))
    sol, st = D.solve_gdre(prob, D.Ros1(D.ADI(shifts=D.Shifts.Cyclic(_shifts(n)), maxiters=200)), dt=-100.0, save_state=True, return_stats=True, ctx=ctx)
    its = [x["iters"] for x in st["gales"]]
    assert len(its) == 45 and len(sol.X) == 46 and all(x["converged"] for x in st["gales"])
    assert its[:12] == [int(v) for v in g["iters"]]
    w = np.random.default_rng(1).standard_normal(n)
    for i in range(1, 13):
        K = sol.K[i]
        assert np.linalg.norm(K[:, ::16] - g["K_cols"][i]) < 1e-7 * g["K_norm"][i], i
        assert np.linalg.norm(K @ w - g["K_w"][i]) <= 1e-7 * np.linalg.norm(g["K_w"][i]), i
    assert all(a >= b - 1 for a, b in zip(its[12:], its[13:])), its          # towards the steady state the counts only fall (one borderline decision allowed)
    ranks = [X.rank() for X in sol.X[1:]]
    assert max(ranks) - min(ranks) <= 96 and min(ranks) >= 96, ranks          # (16-column granularity; without the side-stream compression the sketch keeps a few more directions)
    tau = 100.0
    for i in range(5, 46, 5):
        a, Lx, Dx = sol.X[i]
        K = (d.B.T @ Lx) @ (a * Dx) @ (Lx.T @ d.E)
        assert D.delta(K, sol.K[i]) < 1e-9, i
        # the Lyapunov equation of step i (lowrank_ros1.jl:35-49): F = A - E/(2 tau) - B K_{i-1},  rhs = C'C + K_{i-1}'K_{i-1} + E'X_{i-1}E / tau
        a0, L0, D0 = sol.X[i - 1]
        F = D.lr_update((d.A - d.E / (2 * tau)).tocsc(), -1.0, d.B, sol.K[i - 1])
        BtLD = (d.B.T @ L0) @ (a0 * D0)
        G = np.hstack([d.C.T, d.E.T @ L0])
        q = d.C.shape[0]
        S = np.zeros((G.shape[1], G.shape[1])); S[:q, :q] = np.eye(q); S[q:, q:] = BtLD.T @ BtLD + (a0 * D0) / tau
        rhs = D.lowrank(G, S)
        res = D.norm(D.residual(D.GALEProblem(d.E, F, rhs), sol.X[i]))
        assert res <= 50 * n * EPS * D.norm(rhs), (i, res)
    storage = sum(8 * (n * r + r * r) for r in ranks)
    assert 0.5e9 < storage < 3e9                                            # about a gigabyte of X(t)


def test_ros2_on_the_general_path_against_the_oracle_fixture(ctx):           # lowrank_ros2.jl:37-80 at n = 5177
    """SteelProfile(5177) Ros2 LRSIF, Cyclic heuristic real shifts, the first 6 of the fixture's 12 steps: two cold-start Lyapunov solves per step
    on the multifrontal path with fan groups.  The oracle stops every stage solve at maxiters = 200 above its tolerance (the list was computed for
    the Ros1 operator): the HIP path must report the same — 200 iterations, not converged, the warning — and the same K(t)."""
    n, nsteps = 5177, 6
    g = np.load(os.path.join(GOLDEN, "ros2_5177_s12.npz"))
    d = D.steel_profile(n)
    L, Dm = D.initial_value(d)
    prob = D.GDREProblem(d.E, d.A, d.B, d.C, D.lowrank(L, Dm), (4500.0, 4500.0 - 100.0 * nsteps))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        sol, st = D.solve_gdre(prob, D.Ros2(D.ADI(shifts=D.Shifts.Cyclic(_shifts(n)), maxiters=200)), dt=-100.0, return_stats=True, ctx=ctx)
    its = [x["iters"] for x in st["gales"]]
    assert its == [int(v) for v in g["iters_per_solve"][:nsteps].ravel()]
    assert not any(x["converged"] for x in st["gales"])
    w = np.random.default_rng(1).standard_normal(n)
    for i in range(1, nsteps + 1):
        K = sol.K[i]
        assert np.linalg.norm(K[:, ::16] - g["K_cols"][i]) < 1e-7 * g["K_norm"][i], i
        assert np.linalg.norm(K @ w - g["K_w"][i]) <= 1e-7 * np.linalg.norm(g["K_w"][i]), i


def test_ros2_on_the_general_path_with_a_shift_list_made_for_its_operator(ctx):      # lowrank_ros2.jl:37-80, :41 (F = gamma tau A - E / 2 - ...)
    """The same workload with the heuristic list of (E, A) mapped like the spectrum of the Ros2 operator (gamma tau lambda - 1/2): every stage solve of
    the oracle converges (29 - 47 iterations).  The HIP path must converge in the oracle's number of iterations (+-1: the stopping test sits on a
    residual norm that falls by a factor of ~1.5 per iteration, and the compressions inside the solve differ in rounding) and reach its K(t)."""
    n, nsteps = 5177, 12
    g = np.load(os.path.join(GOLDEN, "ros2_5177_conv.npz"))
    d = D.steel_profile(n)
    L, Dm = D.initial_value(d)
    prob = D.GDREProblem(d.E, d.A, d.B, d.C, D.lowrank(L, Dm), (4500.0, 4500.0 - 100.0 * nsteps))
    sol, st = D.solve_gdre(prob, D.Ros2(D.ADI(shifts=D.Shifts.Cyclic(list(g["shifts"])), maxiters=200)), dt=-100.0, return_stats=True, ctx=ctx)
    its = [x["iters"] for x in st["gales"]]
    ref = [int(v) for v in g["iters_per_solve"].ravel()]
    assert all(x["converged"] for x in st["gales"]) and max(ref) < 200
    assert all(abs(a - b) <= 1 for a, b in zip(its, ref)), (its, ref)
    w = np.random.default_rng(1).standard_normal(n)
    for i in range(1, nsteps + 1):
        K = sol.K[i]
        assert np.linalg.norm(K[:, ::16] - g["K_cols"][i]) < 1e-7 * g["K_norm"][i], i
        assert np.linalg.norm(K @ w - g["K_w"][i]) <= 1e-7 * np.linalg.norm(g["K_w"][i]), i


@pytest.mark.parametrize("wide", [1, 0])
def test_recurrence_with_and_without_the_factor_form_limit(ctx, wide):          # gdre.hip ros1_recurrence_loop, engine.hip adi_advance
    """n = 5177, the first 8 steps (residual widths 144 ... 16, 39 ... 29 iterations: up to 5 600 increment columns > n): with `recurrence_wide` the
    increments stay uncompressed inside the solve and the side stream takes a factor with more columns than rows through the sketch compression;
    without it the ADI compresses in the loop and the step falls back to the reference's order.  Both must give the oracle's counts and K(t)."""
    n, nsteps = 5177, 8
    g = np.load(os.path.join(GOLDEN, "ros1_5177_full.npz"))
    with ctx.options(recurrence_wide=wide):
        sol, st = _ros1(n, nsteps, ctx)
    its = [x["iters"] for x in st["gales"]]
    assert its == [int(v) for v in g["iters"][:nsteps]], its
    assert all(x["converged"] for x in st["gales"])
    w = np.random.default_rng(1).standard_normal(n)
    for i in range(1, nsteps + 1):
        K = sol.K[i]
        assert np.linalg.norm(K[:, ::16] - g["K_cols"][i]) < 1e-7 * g["K_norm"][i], i
        assert np.linalg.norm(K @ w - g["K_w"][i]) <= 1e-7 * np.linalg.norm(g["K_w"][i]), i


def test_one_step_runs_leave_no_worker_job_behind(ctx, rail371):          # dense_x.hip: ~DenseXState (found by tools/option_matrix.sh, round 5)
    """A run of ONE time step on the dense-X path: its first dense step used to hand the K-independent base of the group chain to the parked worker
    thread 'for the next step to join' — there is none, the worker outlives the solve (it lives with the context) and went on reading the dead
    frame: a heap corruption that surfaced in a later, unrelated call.  Thirty such runs in a row, each followed by host allocations, must give the
    fixture's K(t_1) every time."""
    d, L, Dm = rail371
    gold = np.load(os.path.join(GOLDEN, "ros1_371.npz"))
    prob = D.GDREProblem(d.E, d.A, d.B, d.C, D.lowrank(L, Dm), (4500.0, 4400.0))
    alg = D.Ros1(D.ADI(shifts=D.Shifts.Cyclic(_shifts(371)), maxiters=200))
    junk = []
    for rep in range(30):
        sol = D.solve(prob, alg, dt=-100.0)
        junk.append(np.random.default_rng(rep).standard_normal(50000))          # churn the host heap between the runs
        assert D.delta(sol.K[-1], gold["K"][1]) < 1e-7, rep
