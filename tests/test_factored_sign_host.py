"""Factored sign-function solver, host side: the dispatch rules of FactoredSign (checked before a context is needed) and the NumPy model of
SignLyap::solve_lr (tests/_factored_sign_model.py) against the dense replay of `_sign_model`, the dense oracle and the dense Rosenbrock oracle.

Bounds: the truncation at rtol max|lambda| perturbs W_k by at most rtol ||W_k|| per compression and there are at most `iters` + 1 of them, each
carried to X through the remaining (contractive, once scaled) recursion and E^-1; the model run behind DESIGN.md §9.2 gave a distance to the
dense replay of 17 .. 89 rtol and a residual of 10 .. 850 rtol without refinement.  The tests ask for 200 rtol + 1e-12 (1e-12: the dense
replay's own distance to the oracle, tests/test_dense_sign_host.py) and, for the residual, 2000 rtol + 100 n eps."""
import numpy as np
import pytest

import dre_amd as D
import dre_oracle as o
import _sign_model as sm
import _factored_sign_model as fm

EPS = sm.EPS


def _prob(X0):
    return D.GDREProblem(None, None, None, None, X0, (0.0, 1.0))


def test_tag_is_a_value_and_not_a_matrix_sign():
    a = D.FactoredSign()
    assert (a.maxiters, a.tol, a.rtol, a.max_width, a.max_refine) == (50, None, None, 256, 1)
    assert a == D.FactoredSign(50) and hash(a) == hash(D.FactoredSign(max_width=256)) and a != D.FactoredSign(rtol=1e-10)
    assert len({a, D.FactoredSign(), D.FactoredSign(max_refine=0)}) == 2
    assert not isinstance(a, D.MatrixSign) and not isinstance(D.MatrixSign(), D.FactoredSign)


@pytest.mark.parametrize("alg", [D.Ros1(D.FactoredSign()), D.Ros2(D.FactoredSign()), D.Ros3(D.FactoredSign()), D.Ros4(D.FactoredSign())])
def test_dense_x0_names_matrix_sign(alg):
    with pytest.raises(TypeError, match=r"MatrixSign\(\)"):
        D.solve(_prob(np.eye(3)), alg, dt=1.0)


@pytest.mark.parametrize("alg", [D.Ros3(D.FactoredSign()), D.Ros4(D.FactoredSign())])
def test_ros3_ros4_stay_dense_only(alg):
    with pytest.raises(TypeError, match="low-rank"):
        D.solve(_prob(D.lowrank(np.ones((3, 1)))), alg, dt=1.0)


def test_dense_right_hand_side_names_matrix_sign():
    with pytest.raises(TypeError, match=r"MatrixSign\(\)"):
        D.solve(D.GALEProblem(np.eye(3), -np.eye(3), np.eye(3)), D.FactoredSign())


def test_matrix_sign_dispatch_is_unchanged():
    with pytest.raises(TypeError, match="MatrixSign"):
        D.solve_gdre(_prob(D.lowrank(np.ones((3, 1)))), D.Ros1(D.MatrixSign()), dt=1.0)


def _rhs(E, Cm, n):
    q = Cm.shape[0]
    G = np.hstack([Cm.T, E.T @ np.random.default_rng(0).standard_normal((n, 5))])
    S = np.zeros((q + 5, q + 5))
    S[:q, :q] = np.eye(q)
    S[q:, q:] = -0.3 * np.eye(5)
    return G, S


@pytest.fixture(scope="module", params=[(371, 0.0), (1357, 3e-3)], ids=["371", "1357conv"])
def pencil(request):
    n, conv = request.param
    d = D.steel_profile(n, convection=conv)
    E = d.E.toarray()
    G, S = _rhs(E, np.asarray(d.C), n)
    return n, E, d.A.toarray(), G, S


@pytest.mark.parametrize("tau", [20.0, 100.0])
def test_model_against_dense_replay_and_oracle(pencil, tau):
    n, E, A, G, S = pencil
    F = A - E / (2.0 * tau)
    m = sm.SignModel(F, E)
    R = G @ S @ G.T
    Xrep, Xor = m.replay(R), o.lyap_dense(F, E, R)
    nR = np.linalg.norm(R)
    prev_rank = None
    for rtol in (1e-14, n * EPS, 1e-10):
        L, Dm, st = fm.factored_sign_lyap(m, G, S, rtol, 256, 0)
        X = L @ Dm @ L.T
        res = np.linalg.norm(m.residual(X, R)) / nR
        print(f"n={n} tau={tau} rtol={rtol:.1e}: rank {st['rank']} peak {st['peak_width']} d_replay {o.delta(X, Xrep):.2e} d_oracle {o.delta(X, Xor):.2e} "
              f"res {res:.2e} (factored {st['res']:.2e})")
        assert o.delta(X, Xrep) < 200 * rtol + 1e-12 and o.delta(X, Xor) < 200 * rtol + 1e-12
        assert res < 2000 * rtol + 100 * n * EPS
        assert abs(st["res"] - res) <= 0.05 * res + 10 * n * EPS          # the factored residual norm is the residual norm
        # cap logic: a compression happens only above the cap, so no factor is wider than twice the cap or twice the rank it came from
        assert st["rank"] <= 256 and G.shape[1] < st["peak_width"] <= 512 and st["compressions"] >= 1
        assert np.allclose(Dm, np.diag(np.diag(Dm))) and (np.diag(Dm) < 0).any() and (np.diag(Dm) > 0).any()      # diagonal, indefinite
        assert prev_rank is None or st["rank"] < prev_rank
        prev_rank = st["rank"]
    # the default rule refines where the residual exceeds 100 n eps + 10 rtol, and the refined residual is below the unrefined one
    L, Dm, st = fm.factored_sign_lyap(m, G, S)
    target = 100 * n * EPS + 10 * n * EPS
    assert st["refinements"] == (1 if st["res0"] > target else 0) and st["res"] <= st["res0"]
    assert o.delta(L @ Dm @ L.T, Xor) < 200 * n * EPS + 1e-12


def test_model_edge_cases():
    d = D.steel_profile(371)
    E, A = d.E.toarray(), d.A.toarray()
    F = A - E / 40.0
    m = sm.SignModel(F, E)
    L, Dm, st = fm.factored_sign_lyap(m, np.zeros((371, 0)), np.zeros((0, 0)))
    assert L.shape == (371, 0) and Dm.shape == (0, 0) and st["rank"] == 0 and st["compressions"] == 0
    g = np.asarray(d.C)[:1].T                                            # rank 1
    L, Dm, st = fm.factored_sign_lyap(m, g, np.eye(1), 1e-14, 1, 0)      # cap = r = 1: a compression in every iteration
    assert st["compressions"] >= m.iters
    assert o.delta(L @ Dm @ L.T, o.lyap_dense(F, E, g @ g.T)) < 200 * 1e-14 + 1e-12
    L0, D0, _ = fm.factored_sign_lyap(m, np.zeros((371, 2)), np.eye(2))   # a zero right-hand side of positive width
    assert L0.shape[1] == 0
    with pytest.raises(ValueError):
        fm.factored_sign_lyap(m, np.ones((371, 3)), np.eye(3), None, 2)
    for bad in (0.0, 1.0, -1e-3):
        with pytest.raises(ValueError):
            fm.FactoredReplay(m, bad)


def _lowrank_rosenbrock(d, L, Dm, order, nsteps, tau, rtol):
    """lowrank_ros1.jl / lowrank_ros2.jl with the Lyapunov solves done by the factored model (one SignModel per step)"""
    E, A, B, Cm = d.E.toarray(), d.A.toarray(), np.asarray(d.B, float), np.asarray(d.C, float)
    q, gamma = Cm.shape[0], 1.0 + 1.0 / np.sqrt(2.0)
    ranks = []
    for _ in range(nsteps):
        BtLD, EtL = (B.T @ L) @ Dm, E.T @ L
        K = BtLD @ EtL.T
        r = L.shape[1]
        if order == 1:
            m = sm.SignModel(A - E / (2.0 * tau) - B @ K, E)
            G = np.hstack([Cm.T, EtL])
            S = np.zeros((q + r,) * 2)
            S[:q, :q] = np.eye(q)
            S[q:, q:] = BtLD.T @ BtLD + Dm / tau
            G, lam = fm.compress(G, S, rtol)
            L, Dm, _ = fm.factored_sign_lyap(m, G, np.diag(lam), rtol)
        else:
            m = sm.SignModel(gamma * tau * A - 0.5 * E - gamma * tau * (B @ K), E)
            G = np.hstack([Cm.T, A.T @ L, EtL])
            S = np.zeros((q + 2 * r,) * 2)
            S[:q, :q] = np.eye(q)
            S[q:q + r, q + r:] = Dm
            S[q + r:, q:q + r] = Dm
            S[q + r:, q + r:] = -(BtLD.T @ BtLD)
            G, lam = fm.compress(G, S, rtol)
            T1, D1, _ = fm.factored_sign_lyap(m, G, np.diag(lam), rtol)
            BtT1D1 = (B.T @ T1) @ D1
            T2, D2, _ = fm.factored_sign_lyap(m, E.T @ T1, tau * tau * (BtT1D1.T @ BtT1D1) + (2.0 - 1.0 / gamma) * D1, rtol)
            cat = np.hstack([L, T1, T2])
            p, p1, p2 = L.shape[1], T1.shape[1], T2.shape[1]
            Dc = np.zeros((p + p1 + p2,) * 2)
            Dc[:p, :p] = Dm
            Dc[p:p + p1, p:p + p1] = (2.0 - 1.0 / (2.0 * gamma)) * tau * D1
            Dc[p + p1:, p + p1:] = (-tau / 2.0) * D2
            L, lam = fm.compress(cat, Dc, rtol)
            Dm = np.diag(lam)
        ranks.append(L.shape[1])
    return (B.T @ L @ Dm) @ (E.T @ L).T, ranks


@pytest.mark.parametrize("order", [1, 2])
def test_five_rosenbrock_steps_against_the_dense_oracle(order):
    n = 371
    d = D.steel_profile(n)
    L0, D0 = D.initial_value(d)
    tspan = (4500.0, 4000.0)
    ref = o.solve(o.GDREProblem(d.E, d.A, d.B, d.C, o.lowrank(L0, D0).dense(), tspan), o.Ros1() if order == 1 else o.Ros2(), dt=-100.0)
    K, ranks = _lowrank_rosenbrock(d, np.asarray(L0, float), np.asarray(D0, float), order, 5, 100.0, n * EPS)
    err, nk = np.linalg.norm(K - ref.K[-1]), np.linalg.norm(ref.K[-1])
    print(f"Ros{order}: ||dK_end|| / ||K_end|| = {err / nk:.2e} (bound {100 * n * EPS:.2e}), ranks {ranks}")
    assert err < 100 * n * EPS * nk                                       # test/rail.jl:52-70


def test_julia_shims_carry_the_tag_and_the_calls():
    """extends the static shim check (tests/test_julia_shim_static.py counts the ccall arguments of every call, these included)"""
    import os
    import re
    from conftest import ROOT
    jdir = os.path.join(ROOT, "differentialriccatiequations.jl_amd", "julia")
    main, ext = open(os.path.join(jdir, "DREHip.jl")).read(), open(os.path.join(jdir, "DREHipExt.jl")).read()
    called = set(re.findall(r"ccall\(\(:(dre_sign_[a-z_]+),", main))
    assert called == {"dre_sign_create", "dre_sign_info", "dre_sign_solve_lr", "dre_sign_solve_dense", "dre_sign_free"}
    assert "struct FactoredSign" in main and "FactoredSign, SignFactorization" in main[main.index("\nexport"):]
    assert "struct HipFactoredSign" in ext and "HipFactoredSign" in ext[ext.index("export"):ext.index("\n", ext.index("export"))]
    fields = lambda src, name: re.findall(r"(\w+)::", src[src.index("struct " + name):].split("end")[0])
    assert fields(main, "FactoredSign") == fields(ext, "HipFactoredSign") == ["maxiters", "tol", "rtol", "max_width", "max_refine"]
