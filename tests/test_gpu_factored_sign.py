"""Factored sign-function Lyapunov solver on the device (solve(GALEProblem{LDLᵀ}, FactoredSign()), Ros1/Ros2(FactoredSign())) against the
dense MatrixSign() path on the same device, the dense oracle, the NumPy model of the kernel sequence (tests/_factored_sign_model.py) and
the committed Rosenbrock fixtures.

The distance bounds of the GALE tests are not fixed numbers: they are the model's distance for the same input and rtol times MARGIN = 10
(different summation order of the MFMA GEMMs and of the blocked QR).  Measured device values: DESIGN.md §9.2."""
import os

import numpy as np
import pytest

import dre_amd as D
import dre_oracle as o
import _sign_model as sm
import _factored_sign_model as fm
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
MARGIN = 10.0


def _case(n, conv, tau, feedback):
    d = D.steel_profile(n, convection=conv)
    E, A = d.E.toarray(), d.A.toarray()
    B, Cm = np.asarray(d.B, float), np.asarray(d.C, float)
    q = Cm.shape[0]
    rng = np.random.default_rng(0)
    G = np.hstack([Cm.T, E.T @ rng.standard_normal((n, 5))])          # an indefinite rank-11 right-hand side of Ros1's shape
    S = np.zeros((q + 5, q + 5))
    S[:q, :q] = np.eye(q)
    S[q:, q:] = -0.3 * np.eye(5)
    F = A - E / (2.0 * tau)
    Fop = D.ScaledPencil(d.A, 1.0, d.E, -1.0 / (2.0 * tau))
    Fsp = (d.A - d.E / (2.0 * tau)).tocsc()                           # the same operator for residual(), which takes sparse matrices
    if feedback:
        K = 1e-3 * (B.T @ E) / np.linalg.norm(B)                      # a feedback term: F = A - E/(2 tau) - B K as a LowRankUpdate
        F = F - B @ K
        Fop, Fsp = D.lr_update(Fop, -1.0, B, K), D.lr_update(Fsp, -1.0, B, K)
    return d, E, F, (Fop, Fsp), G, S


CASES = [(371, 0.0, 20.0, False), (371, 0.0, 100.0, True), (1357, 3e-3, 100.0, False), (1357, 3e-3, 20.0, True)]


@pytest.mark.parametrize("n,conv,tau,feedback", CASES, ids=["371", "371-feedback", "1357conv", "1357conv-feedback"])
def test_gale_against_matrix_sign_oracle_and_model(ctx, n, conv, tau, feedback):
    d, E, F, (Fop, Fsp), G, S = _case(n, conv, tau, feedback)
    Cl = D.lowrank(G, S)
    alg = D.FactoredSign()
    X, info = D.solve(D.GALEProblem(d.E, Fop, Cl), alg, return_info=True)
    assert isinstance(X, D.LDLt) and X.rank() == info["rank"] <= alg.max_width
    Xd = X.dense()
    R = G @ S @ G.T
    Xms = D.solve(D.GALEProblem(E, F, R), D.MatrixSign())
    Xor = o.lyap_dense(F, E, R)
    m = sm.SignModel(F, E)
    Lm, Dm, st = fm.factored_sign_lyap(m, G, S, fm.default_rtol(n), alg.max_width, alg.max_refine)
    Xm = Lm @ Dm @ Lm.T
    bound_ms, bound_or = MARGIN * o.delta(Xm, m.replay(R)), MARGIN * o.delta(Xm, Xor)
    d_ms, d_or = D.delta(Xd, Xms), D.delta(Xd, Xor)
    res = D.norm(D.residual(D.GALEProblem(d.E, Fsp, Cl), X)) / np.linalg.norm(R)
    print(f"n={n} tau={tau} feedback={feedback}: rank {info['rank']} (model {st['rank']}) peak {info['peak_width']} (model {st['peak_width']}) "
          f"compressions {info['compressions']} refinements {info['refinements']} (model {st['refinements']}) res0 {info['res0']:.2e} "
          f"res {info['res']:.2e} (model {st['res0']:.2e} / {st['res']:.2e}) independent res {res:.2e} "
          f"d_MatrixSign {d_ms:.2e} (bound {bound_ms:.2e}) d_oracle {d_or:.2e} (bound {bound_or:.2e})")
    assert d_ms < bound_ms and d_or < bound_or
    assert info["iters"] == m.iters
    assert abs(info["rank"] - st["rank"]) <= 2
    # the solver's own residual is the factored one; residual(GALEProblem, LDLᵀ) evaluates it independently
    target = 100 * n * EPS + 10 * fm.default_rtol(n)
    assert res <= MARGIN * max(st["res"], target) and info["res"] <= MARGIN * max(st["res"], target)


def test_rtol_sweep_is_monotone(ctx):
    n = 371
    d, E, F, _, G, S = _case(n, 0.0, 100.0, False)
    R = G @ S @ G.T
    Xor = o.lyap_dense(F, E, R)
    m = sm.SignModel(F, E)
    ranks, errs = [], []
    for rtol in (1e-14, None, 1e-10):
        X, info = D.solve(D.GALEProblem(E, F, D.lowrank(G, S)), D.FactoredSign(rtol=rtol, max_refine=0), return_info=True)
        _, _, st = fm.factored_sign_lyap(m, G, S, rtol, 256, 0)
        print(f"rtol {rtol}: rank {info['rank']} (model {st['rank']}) err {D.delta(X.dense(), Xor):.2e} res {info['res']:.2e}")
        assert abs(info["rank"] - st["rank"]) <= 2
        ranks.append(info["rank"]); errs.append(D.delta(X.dense(), Xor))
    assert ranks[0] > ranks[1] > ranks[2] and errs[0] < errs[1] < errs[2]


def test_two_right_hand_sides_share_one_factorisation(ctx):
    d, E, F, _, G, S = _case(371, 0.0, 20.0, False)
    G2, S2 = G[:, :3] + 0.5 * G[:, 3:6], np.diag([1.0, -2.0, 0.5])
    sign = D.SignFactorization(E, F, ctx=ctx)
    L1, D1, i1 = sign.solve_lr(G, S)
    L2, D2, i2 = sign.solve_lr(G2, S2)
    sign.close()
    for (L, Dm, i), (g, s) in zip([(L1, D1, i1), (L2, D2, i2)], [(G, S), (G2, S2)]):
        X, info = D.solve(D.GALEProblem(E, F, D.lowrank(g, s)), D.FactoredSign(), return_info=True)
        assert info["rank"] == i["rank"] and info["iters"] == i["iters"] == sign.iters
        assert D.delta(L @ Dm @ L.T, X.dense()) < 100 * EPS


def test_width_cap_at_r_and_never_reached_agree(ctx):
    n = 371
    d, E, F, _, G, S = _case(n, 0.0, 20.0, False)
    G, S = G[:, [0, 8]], np.diag([1.0, -0.3])          # rank 2: 2 * 2^iters <= 4096, so the large cap is never reached before the final compression
    R = G @ S @ G.T
    m = sm.SignModel(F, E)
    assert 2 * 2 ** m.iters <= 4096
    Xrep = m.replay(R)
    r = G.shape[1]
    out = {}
    for cap in (r, 4096):
        X, info = D.solve(D.GALEProblem(E, F, D.lowrank(G, S)), D.FactoredSign(max_width=cap), return_info=True)
        Lm, Dm, st = fm.factored_sign_lyap(m, G, S, None, cap, 1)
        bound = MARGIN * o.delta(Lm @ Dm @ Lm.T, Xrep)
        dist = D.delta(X.dense(), Xrep)
        print(f"max_width {cap}: rank {info['rank']} peak {info['peak_width']} compressions {info['compressions']} distance {dist:.2e} (bound {bound:.2e})")
        assert dist < bound
        out[cap] = (X.dense(), info, bound)
    assert out[r][1]["compressions"] >= m.iters and out[4096][1]["peak_width"] == 2 * 2 ** m.iters
    assert D.delta(out[r][0], out[4096][0]) < out[r][2] + out[4096][2]


class _Hooks:
    def __init__(self):
        self.events = []

    def observe_gdre_start(self, prob, alg):
        self.events.append("start")

    def observe_gdre_step(self, t, X, K):
        self.events.append(("step", float(t), X is not None))

    def observe_gdre_done(self):
        self.events.append("done")

    def observe_gale_step(self, *a):
        self.events.append("gale_step")


class _StateHooks(_Hooks):
    needs_state = True


@pytest.mark.parametrize("Ros,fixture", [(D.Ros1, "ros1_371.npz"), (D.Ros2, "ros2_371.npz")], ids=["ros1", "ros2"])
def test_rosenbrock_371(ctx, rail371, Ros, fixture):
    d, L, Dm = rail371
    n = 371
    g = np.load(os.path.join(GOLDEN, fixture))
    X0 = D.lowrank(L, Dm)
    tspan = (4500.0, 4000.0)
    hooks = _Hooks()
    sol, st = D.solve(D.GDREProblem(d.E, d.A, d.B, d.C, X0, tspan), Ros(D.FactoredSign()), dt=-100.0, save_state=True, observer=hooks,
                      return_stats=True)
    ref = D.solve(D.GDREProblem(d.E, d.A, d.B, d.C, X0.dense(), tspan), Ros(D.MatrixSign()), dt=-100.0)
    assert len(sol.K) == len(ref.K) == 6 and len(sol.X) == 6
    for i in range(6):
        err, nk = np.linalg.norm(sol.K[i] - ref.K[i]), np.linalg.norm(ref.K[i])
        print(f"{Ros.__name__} step {i}: ||dK|| / ||K|| = {err / nk:.2e} (bound {100 * n * EPS:.2e}) rank {sol.X[i].rank()}")
        assert err < 100 * n * EPS * nk                                 # test/rail.jl:52-70
    for i in range(len(g["K"])):
        assert D.delta(sol.K[i], g["K"][i]) < 1e-7                      # the fixtures' tolerance (tests/test_gpu_gdre.py)
    assert all(isinstance(X, D.LDLt) for X in sol.X) and st["ranks"] == [X.rank() for X in sol.X]
    per_step = 1 if Ros is D.Ros1 else 2
    assert st["lyapunov_solves"] == 5 * per_step and all(s["rank"] >= 1 and s["iters"] >= 1 for s in st["solves"])
    # the same hook order as the host-driven ADI path (observe_gdre_*), and no per-iteration hooks
    adi_hooks = _StateHooks()
    shifts = g["shifts"] if "shifts" in g.files else np.load(os.path.join(GOLDEN, "heuristic_shifts_371.npy"))
    D.solve(D.GDREProblem(d.E, d.A, d.B, d.C, X0, tspan), Ros(D.ADI(shifts=D.Shifts.Cyclic(list(shifts)))), dt=-100.0, save_state=True,
            observer=adi_hooks)
    assert hooks.events == [e for e in adi_hooks.events if e != "gale_step"]
    assert hooks.events[0] == "start" and hooks.events[-1] == "done" and len(hooks.events) == 8


def test_ros1_5177_against_the_lowrank_fixture(ctx):
    """the first Ros1 steps at SteelProfile(5177) (tournament panel) against the sampled K columns of the low-rank fixture, as
    tests/test_gpu_dense_large.py checks the dense path: 1e-7 K_norm"""
    d = D.steel_profile(5177)
    L, Dm = D.initial_value(d)
    g = np.load(os.path.join(GOLDEN, "ros1_5177.npz"))
    sol, st = D.solve(D.GDREProblem(d.E, d.A, d.B, d.C, D.lowrank(L, Dm), (4500.0, 4200.0)), D.Ros1(D.FactoredSign()), dt=-100.0,
                      save_state=True, return_stats=True)
    assert len(sol.K) == 4 and np.allclose(sol.t, g["t"])
    print("n = 5177 ranks of X per step:", st["ranks"], "solves:", st["solves"])
    for i, K in enumerate(sol.K):
        err = np.linalg.norm(K[:, ::16] - g["K_cols"][i])
        print(f"step {i}: sampled ||dK|| / K_norm = {err / g['K_norm'][i]:.2e}")
        assert err < 1e-7 * g["K_norm"][i]


def test_failure_paths(ctx):
    n = 40
    rng = np.random.default_rng(3)
    E = np.eye(n) + 0.01 * np.diag(np.arange(n) / n)
    F = -np.eye(n) + 0.1 * rng.standard_normal((n, n)) / np.sqrt(n)
    G = rng.standard_normal((n, 4))
    C4 = D.lowrank(G, np.diag([1.0, -1.0, 2.0, 0.5]))
    X = D.solve(D.GALEProblem(E, F, C4), D.FactoredSign())
    assert D.delta(X.dense(), o.lyap_dense(F, E, C4.dense())) < 1e-10
    with pytest.raises(D.DREError) as e:                                # right-shifted: not c-stable
        D.solve(D.GALEProblem(E, F + 2.0 * E, C4), D.FactoredSign())
    assert e.value.code == -7
    for bad in (D.FactoredSign(max_width=3), D.FactoredSign(max_width=0), D.FactoredSign(rtol=0.0), D.FactoredSign(rtol=1.0),
                D.FactoredSign(max_refine=-1), D.FactoredSign(max_width=5000)):
        with pytest.raises(D.DREError) as e:
            D.solve(D.GALEProblem(E, F, C4), bad)
        assert e.value.code == -1, bad
    X0, info = D.solve(D.GALEProblem(E, F, D.lowrank(np.zeros((n, 0)), np.zeros((0, 0)))), D.FactoredSign(), return_info=True)
    assert X0.rank() == 0 and info["rank"] == 0 and info["compressions"] == 0
    X1, info = D.solve(D.GALEProblem(E, F, D.lowrank(G[:, :1])), D.FactoredSign(), return_info=True)
    assert D.delta(X1.dense(), o.lyap_dense(F, E, G[:, :1] @ G[:, :1].T)) < 1e-10
    assert D.solve(D.GALEProblem(E, F, D.lowrank(G)), D.FactoredSign()).rank() >= 4     # the context still works after the errors


def test_memory_check_before_any_kernel(ctx):
    n = 8000
    E, A = np.eye(n), -np.eye(n)
    # the kept sequence is maxiters n x n matrices: (1000 + 7) n^2 doubles = 515 GB, far above the device's memory
    with pytest.raises(D.DREError) as e:
        D.solve(D.GALEProblem(E, A, D.lowrank(np.ones((n, 1)))), D.FactoredSign(maxiters=1000))
    assert e.value.code == -3
