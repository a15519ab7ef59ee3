"""LQG balanced truncation, host side: the NumPy model of the pair solve and of lqg_balance (tests/_lqg_model.py) against the SciPy reference
chain on the four generated systems and against its record (tests/golden/lqg_model.json), the ABI level and symbols, the Julia shim (static)
and the argument errors that are raised before any device work.

Bounds.  X, Y: 1e-10 relative against solve_continuous_are, the bound of tests/test_dense_gare_host.py for the same comparison (two
backward-stable solvers on problems whose condition is at most 1e3).  mu against sqrt(eig(Y E'X E)): sqrt(n eps) mu_1 for the whole list (a
perturbation of order n eps in an eigenvalue of Y E'X E moves its square root by at most the square root of that), 1e3 n eps mu_1 for the
leading r, which the reduced model is made of.  The reduced Riccati residuals with Sigma_r: 100 n eps scaled as the full ones, times the
condition bound 1e3 of the balancing transformation."""
import os
import re

import numpy as np
import pytest
import scipy.linalg as sla

import dre_amd as D
import _lqg_model as lm
from conftest import ROOT

EPS = np.finfo(float).eps
GENERATED = sorted(lm.GENERATED)


@pytest.mark.parametrize("n", GENERATED)
def test_model_against_the_reference_and_the_record(n):
    E, A, B, C = lm.system(n)
    r, rec = lm.ORDERS[n], lm.recorded()[str(n)]
    assert (B.shape[1], C.shape[0]) == (rec["m"], rec["q"]) == lm.GENERATED[n][:2]
    if n > 1:
        assert B.shape[1] != C.shape[0] and not np.allclose(E, E.T) and not np.allclose(A, A.T)
        assert (sla.eigvals(A, E).real > 0).sum() == 2
    X, Y, info = lm.model_xy(n)
    Xr, Yr = lm.reference_xy(n)
    live = lm.record_case(n)
    print(f"n={n}: " + " ".join(f"{k} {v:.3e}" if isinstance(v, float) else f"{k} {v}" for k, v in live.items()))
    # one iteration, no refinement needed, residuals at the target
    assert info["iters"] == rec["iters"] and info["regulator"]["refinements"] == info["filter"]["refinements"] == 0
    assert info["regulator"]["res"] <= 100 * n * EPS and info["filter"]["res"] <= 100 * n * EPS
    assert lm.rel(X, Xr) < 1e-10 and lm.rel(Y, Yr) < 1e-10
    # the filter's solution from Z_inf' is the regulator's solver on the transposed problem
    Yt, _ = lm.hm.gare_sign(E.T, A.T, C.T @ C, B @ B.T)
    assert lm.rel(Y, Yt) < 1e-10
    # the LQG characteristic values
    ch, ref = lm.chain(n, r), lm.reference(n, r)
    mu_direct = np.sort(np.sqrt(np.abs(sla.eigvals(Yr @ E.T @ Xr @ E).real)))[::-1]
    k = min(len(ch["mu"]), n)
    assert np.abs(ch["mu"][:k] - mu_direct[:k]).max() <= np.sqrt(n * EPS) * mu_direct[0]
    assert np.abs(ch["mu"][:r] - mu_direct[:r]).max() <= 1e3 * n * EPS * mu_direct[0]
    # both reduced Riccati equations hold with Sigma_r, the controller is made of the reduced matrices
    for red in (ch, ref):
        assert max(lm.riccati_residuals(red)) <= 100 * n * EPS * 1e3
        Sig = np.diag(red["mu"][:r])
        assert np.array_equal(red["Kr"], red["Br"].T @ Sig) and np.array_equal(red["Lr"], Sig @ red["Cr"].T)
        assert red["eye_err"] <= 100 * n * EPS
    # the bound on the normalised right coprime factors, and the stabilising reduced controller
    err = lm.coprime_error(E, A, B, C, X, ch)
    assert err <= ch["bound"] + 1e3 * EPS and ch["bound"] == lm.bound(ch["mu"], r)
    assert lm.closed_loop_abscissa(E, A, B, C, ch) < 0 < live["open_loop"]
    # the record is this model's run (another BLAS sums in another order: rounding-level figures within a factor of 3)
    for key in ("iters", "refinements_x", "refinements_y", "order", "r_o", "r_c"):
        assert live[key] == rec[key], key
    assert abs(live["rank"] - rec["rank"]) <= 2
    for key in ("x_err", "y_err", "mu", "eye", "transfer"):
        assert live[key] <= 3 * rec[key] + n * EPS and rec[key] <= 3 * live[key] + n * EPS, key
    for key in ("bound", "err", "abscissa", "abscissa_ref", "open_loop"):
        assert live[key] == pytest.approx(rec[key], rel=1e-6, abs=1e-12), key
    if n > 2:
        assert live["tol_order"] == rec["tol_order"] == r - 1 and live["tol"] == pytest.approx(rec["tol"], rel=1e-6)


def test_the_record_and_the_recorded_reference():
    rec, gold = lm.recorded(), lm.golden()
    assert set(rec) == {str(n) for n in lm.SIZES}
    r = rec["371"]
    assert r["iters"] == 14 and r["refinements_x"] == r["refinements_y"] == 0 and r["order"] == 16
    assert r["err"] <= r["bound"] and r["abscissa_ref"] < 0 < r["open_loop"]
    assert gold["mu_371"].ndim == 1 and (np.diff(gold["mu_371"]) <= 0).all() and gold["Hr_371"].shape == (len(lm.OMEGA_371), r["q"], r["m"])


def test_order_rule_and_transposed_extraction():
    mu = np.array([10.0, 1.0, 0.1, 1e-3, 1e-6])
    nu = mu / np.sqrt(1 + mu * mu)
    assert np.allclose(lm.nu(mu), nu) and lm.bound(mu, 3) == 2.0 * (nu[4] + nu[3])
    assert lm.choose_order(mu, 5, 2.1e-6) == 4 and lm.choose_order(mu, 5, 1.9e-6) == 5 and lm.choose_order(mu, 3, 1e-12) == 3
    assert lm.choose_order(mu, 5, 10.0) == 0 and lm.choose_order(mu, 5, 0.0) == 5
    assert lm.choose_order(mu, 5, lm.clear_tol(mu, 2)) == 2
    # a wrong transposition in the dual extraction shows on a nonsymmetric pencil: the structured Z_inf gives the same Y with and without it
    # only when both blocks are read consistently
    E, A, B, C = lm.system(12)
    Z, _, _ = lm.hm.sign_iteration(E, A, B @ B.T, C.T @ C)
    Y = lm.extract_t(Z, E)
    assert lm.residual_f(E, A, B @ B.T, C.T @ C, Y)[1] <= 100 * 12 * EPS
    assert lm.residual_f(E, A, B @ B.T, C.T @ C, lm.hm.extract(Z, E))[1] > 1e-3          # X is not Y
    assert lm.residual_f(E, A, C.T @ C, B @ B.T, Y)[1] > 1e-3                             # G and Q exchanged


# ---- the interfaces ---------------------------------------------------------------------------------------------------------------------
def test_abi_level_and_symbols():
    lib = D._lib.load()
    assert lib.dre_version() >= 113
    header = open(os.path.join(ROOT, "include", "dre_hip.h")).read()
    for name, nargs in (("dre_dense_gare_solve_pair", 14), ("dre_lqg_balance", 20)):
        assert hasattr(lib, name) and len(D._lib.PROTOTYPES[name][1]) == nargs
        proto = re.search(r"\bint " + name + r"\(dre_ctx\* ctx, ([^;]*)\);", header)
        assert proto and re.sub(r"/\*.*?\*/", "", proto.group(1)).count(",") == nargs - 2
    for name in ("solve_gare_pair", "lqg_balanced_truncation", "lqg_characteristic_values", "lqg_error", "LQGReducedModel"):
        assert name in D.__all__ and callable(getattr(D, name))
    rom = D.LQGReducedModel(*(np.zeros((2, 2)) for _ in range(4)), np.zeros(2), *(np.zeros((2, 2)) for _ in range(5)))
    assert rom.order == 2 and rom.K is None
    Ac, Lr, Kr = rom.controller()
    assert Ac is rom.Ac and Lr is rom.Lr and Kr is rom.Kr


def test_julia_shim_carries_the_two_calls():
    """static, as tests/test_julia_shim_static.py (which counts the ccall arguments of these calls too)"""
    jdir = os.path.join(ROOT, "differentialriccatiequations.jl_amd", "julia")
    main, lqg = open(os.path.join(jdir, "DREHip.jl")).read(), open(os.path.join(jdir, "DREHipLQG.jl")).read()
    assert 'include("DREHipLQG.jl")' in main and main.index('include("DREHipFreq.jl")') < main.index('include("DREHipLQG.jl")')
    for fn, call in (("solve_gare_pair", "dre_dense_gare_solve_pair"), ("lqg_balanced_truncation", "dre_lqg_balance")):
        assert re.search(r"^function " + fn + r"\(", lqg, flags=re.M) and len(re.findall(r"ccall\(\(:" + call + r", LIB\), Cint,", lqg)) == 1
    for fn in ("lqg_error", "lqg_characteristic_values", "controller"):
        assert re.search(r"^(function )?" + fn + r"\(", lqg, flags=re.M) and fn in lqg[lqg.index("\nexport "):]


def test_argument_errors_come_before_any_device_work(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a device context was requested")
    monkeypatch.setattr(D.api.dev, "default_context", boom)
    E, A, B, C = lm.system(33)
    for fn in (D.lqg_balanced_truncation, D.lqg_characteristic_values, D.solve_gare_pair):
        for alg in (D.FactoredSign(), D.ADI(), None):
            with pytest.raises(TypeError, match="alg = MatrixSign\\(\\).*nothing was run on the device"):
                fn(E, A, B, C, alg)
        with pytest.raises(TypeError, match="C must be a matrix.*nothing was run on the device"):
            fn(E, A, B, "C")
        with pytest.raises(ValueError, match="E and A must be n x n.*nothing was run on the device"):
            fn(E, A, B, C.T)
        with pytest.raises(ValueError, match="n, m and q must be at least 1.*nothing was run on the device"):
            fn(E, A, B[:, :0], C)
    for order in (8.0, "8", True):
        with pytest.raises(TypeError, match="order must be None or an int.*nothing was run on the device"):
            D.lqg_balanced_truncation(E, A, B, C, order=order)
    with pytest.raises(ValueError, match="order must be at least 1.*nothing was run on the device"):
        D.lqg_balanced_truncation(E, A, B, C, order=0)
    for tol in (-1.0, float("nan"), None):
        with pytest.raises(ValueError, match="tol must be a finite non-negative number.*nothing was run on the device"):
            D.lqg_balanced_truncation(E, A, B, C, tol=tol)
    with pytest.raises(ValueError, match="Rinv must be 3 x 3.*nothing was run on the device"):
        D.solve_gare_pair(E, A, B, C, Rinv=np.eye(2))
    with pytest.raises(ValueError, match="S must be 2 x 2.*nothing was run on the device"):
        D.solve_gare_pair(E, A, B, C, S=np.eye(3))
    rom = D.LQGReducedModel(*(np.zeros((2, 2)) for _ in range(4)), np.zeros(2), *(np.zeros((2, 2)) for _ in range(5)))
    with pytest.raises(TypeError, match="rom must be an LQGReducedModel.*nothing was run on the device"):
        D.lqg_error(E, A, B, C, "rom", lm.OMEGA)
    with pytest.raises(ValueError, match="the reduced model has \\(m, q\\).*nothing was run on the device"):
        D.lqg_error(E, A, B, C, rom, lm.OMEGA)
    with pytest.raises(ValueError, match="omega has a non-finite entry.*nothing was run on the device"):
        D.lqg_error(E, A, B, C, rom, [1.0, np.inf])
