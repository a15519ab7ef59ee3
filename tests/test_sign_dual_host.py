"""Dual solves on a kept sign factorisation, the part that needs no device: the NumPy model (tests/_sign_dual_model.py) against the oracle on
non-symmetric pencils (tests/_sign_dual_cases.py), the ABI level and symbols, the argument errors that are raised before any device work, and
the Julia shim (static)."""
import os
import re

import numpy as np
import pytest

import dre_amd as D
import dre_oracle as o
import _sign_dual_cases as cs
import _sign_dual_model as dm
import _factored_sign_model as fm
from conftest import ROOT

EPS = np.finfo(float).eps


@pytest.mark.parametrize("n", [33, 70, 371])
def test_fixture_pencils_are_c_stable_and_non_symmetric(n):
    E, F, _, _ = cs.pencil(n)
    assert cs.stable(F, E) < 0.0
    assert np.linalg.cond(E) <= 1e3
    assert np.linalg.norm(E - E.T) > 0.05 * np.linalg.norm(E) and np.linalg.norm(F - F.T) > 1e-3 * np.linalg.norm(F)


@pytest.mark.parametrize("n", [33, 70, 371])
def test_dual_and_primal_models_against_the_oracle_on_one_pencil(n):
    """each replay solves ITS equation, and the two solutions are far apart: the fixture tells them from each other.  Bound: both the model and
    the oracle (one step of refinement) leave a relative residual of at most 100 n eps; the error is that times the condition of the Lyapunov
    operator, for which 1e3 is allowed (the fixtures have cond(E) <= 1e3 by construction).  The wrong equation's solution is O(1) away, more
    than eight orders above that bound."""
    m = cs.model(n)
    R = cs.rhs(n)[2]
    Y, _, _, resY = cs.model_dual(n)
    X, _, _, resX = m.solve(R)
    Yo, Xo = cs.oracle(n), cs.oracle(n, None, False)
    bound = 100 * n * EPS * 1e3
    dY, dX, apart = o.delta(Y, Yo), o.delta(X, Xo), o.delta(Xo, Yo)
    print(f"n={n}: iters {m.iters}; dual model-oracle {dY:.2e} (res {resY:.2e}); primal model-oracle {dX:.2e} (res {resX:.2e}); "
          f"bound {bound:.2e}; ||X - Y|| / max = {apart:.2e}; primal model against the dual oracle {o.delta(X, Yo):.2e}")
    assert resY <= 100 * n * EPS and resX <= 100 * n * EPS
    assert dY < bound and dX < bound
    assert apart > 0.1 and o.delta(X, Yo) > 1e3 * bound and o.delta(Y, Xo) > 1e3 * bound
    # the dual of the kept sequence is the primal of the transposed pencil
    Yt = cs.model_of_transposed_pencil(n).solve(R)[0]
    assert o.delta(Y, Yt) < bound


def test_dual_model_refines_after_a_loose_sign_iteration():
    n = 70
    R = cs.rhs(n)[2]
    Y0, s0, r00, _ = dm.solve_t(cs.model(n, 1e-3), R, 0)
    Y1, s1, r0, r1 = dm.solve_t(cs.model(n, 1e-3), R, 1)
    assert (s0, s1) == (0, 1) and r00 == r0 > 100 * n * EPS and r1 < 1e-2 * r0
    assert o.delta(Y1, cs.oracle(n)) < 1e-2 * o.delta(Y0, cs.oracle(n))


@pytest.mark.parametrize("cols,cap,max_refine", [((0,), 256, 1), ((0, 8), 2, 1), ((0, 8), 256, 0), (None, 256, 1), (None, 11, 0)],
                         ids=["r1", "r2-cap2", "r2-norefine", "r11", "r11-cap11-norefine"])
def test_factored_dual_model_reproduces_the_dense_one(cols, cap, max_refine):
    """§9.2's bounds: distance 200 rtol + 1e-12 to the dense replay, residual 2000 rtol + 100 n eps; S is indefinite whenever column 8 is in"""
    n = 371
    m = cs.model(n)
    G, S, R = cs.rhs(n, None if cols is None else list(cols))
    rtol = fm.default_rtol(n)
    L, Dm, st = dm.factored_sign_lyap_t(m, G, S, rtol, cap, max_refine)
    Yd = dm.replay_t(m, R)
    dist = o.delta(L @ Dm @ L.T, Yd)
    res = np.linalg.norm(dm.residual_t(m, L @ Dm @ L.T, R)) / np.linalg.norm(R)
    print(f"cols {cols} cap {cap} max_refine {max_refine}: rank {st['rank']} peak {st['peak_width']} compressions {st['compressions']} "
          f"refinements {st['refinements']} res0 {st['res0']:.2e} res {st['res']:.2e} independent res {res:.2e} distance {dist:.2e}")
    assert dist < 200 * rtol + 1e-12
    assert st["res"] < 2000 * rtol + 100 * n * EPS and res < 2000 * rtol + 100 * n * EPS
    assert np.count_nonzero(np.abs(Dm - np.diag(np.diag(Dm)))) == 0
    if cols is None or 8 in cols:
        assert (np.diag(S) < 0).any() and (np.diag(Dm) < 0).any() and (np.diag(Dm) > 0).any()
    if cap == 2:
        assert st["compressions"] >= m.iters


def test_abi_level_and_symbols():
    lib = D._lib.load()
    assert lib.dre_version() >= 109
    for name, sibling in (("dre_sign_solve_dense_t", "dre_sign_solve_dense"), ("dre_sign_solve_lr_t", "dre_sign_solve_lr")):
        assert hasattr(lib, name)
        assert D._lib.PROTOTYPES[name] == D._lib.PROTOTYPES[sibling]
    header = open(os.path.join(ROOT, "include", "dre_hip.h")).read()
    for name in ("dre_sign_solve_dense_t", "dre_sign_solve_lr_t"):
        assert re.search(r"\bint " + name + r"\(", header)
    assert "solve_gale_pair" in D.__all__


def _no_device(monkeypatch):
    """any device work would start with a context: make that an error of its own"""
    def boom(*a, **k):
        raise AssertionError("a device context was requested")
    monkeypatch.setattr(D.api.dev, "default_context", boom)


def test_pair_argument_errors_come_before_any_device_work(monkeypatch):
    _no_device(monkeypatch)
    E, F, G, S = cs.pencil(33)
    R, Cl = G @ S @ G.T, D.lowrank(G, S)
    for alg in (D.ADI(), None, "MatrixSign"):
        with pytest.raises(TypeError, match="MatrixSign\\(\\) or FactoredSign\\(\\).*nothing was run on the device"):
            D.solve_gale_pair(E, F, R, R, alg)
    for C_obs, C_ctr in ((R, Cl), (Cl, R), (R, R)):
        with pytest.raises(TypeError, match="FactoredSign\\(\\) takes low-rank right-hand sides.*nothing was run on the device"):
            D.solve_gale_pair(E, F, C_obs, C_ctr, D.FactoredSign())
    for C_obs, C_ctr in ((R, [[1.0]]), ("R", R), (None, Cl)):
        with pytest.raises(TypeError, match="MatrixSign\\(\\) takes ndarray or LDL.*nothing was run on the device"):
            D.solve_gale_pair(E, F, C_obs, C_ctr, D.MatrixSign())


def test_transposed_must_be_a_bool():
    """checked before the library is called: the object below has neither a context nor a handle"""
    s = object.__new__(D.SignFactorization)
    for call in (lambda: s.solve_dense(np.eye(3), transposed="yes"), lambda: s.solve_lr(np.ones((3, 1)), np.eye(1), transposed=1)):
        with pytest.raises(TypeError, match="transposed must be a bool.*nothing was run on the device"):
            call()


def test_julia_shim_carries_the_keyword_and_the_two_calls():
    """static, as tests/test_julia_shim_static.py (which counts the ccall arguments of these calls too): solve_dense / solve_lr take `transposed`
    and pass it on; the two dual entry points are called with the argument types of their siblings"""
    jdir = os.path.join(ROOT, "differentialriccatiequations.jl_amd", "julia")
    main, dual = open(os.path.join(jdir, "DREHip.jl")).read(), open(os.path.join(jdir, "DREHipSignDual.jl")).read()
    assert 'include("DREHipSignDual.jl")' in main
    for fn in ("solve_lr", "solve_dense"):
        sig = re.search(r"^function " + fn + r"\(s::SignFactorization,[^\n]*\)$", main, flags=re.M).group(0)
        assert "transposed::Bool=false" in sig
        body = main[main.index(sig):]
        body = body[:body.index("\nend")]
        assert re.search(r"transposed && return " + fn + r"_t\(s, ", body)
        assert re.search(r"^function " + fn + r"_t\(s::SignFactorization,", dual, flags=re.M)

    def types(src, name):
        m = re.search(r"ccall\(\(:" + name + r", LIB\), Cint,\s*\(([^)]*)\)", src)
        return [t.strip() for t in m.group(1).split(",") if t.strip()]
    assert types(dual, "dre_sign_solve_dense_t") == types(main, "dre_sign_solve_dense")
    assert types(dual, "dre_sign_solve_lr_t") == types(main, "dre_sign_solve_lr")
