"""Device SVD and balanced truncation, the part that needs no device: the NumPy model of the SVD (tests/_svd_jacobi_model.py) against
numpy.linalg.svd and its record, the balanced-truncation chain in NumPy (factored sign models + SVD model + the steps of csrc/balance.hip)
against the reference (oracle.lyap_dense Gramians, eigh factors, numpy.linalg.svd) on the systems of tests/_balance_cases.py, the properties of
the reference alone, the ABI level and symbols, the Julia shim (static) and the argument errors that are raised before any device work."""
import os
import re

import numpy as np
import pytest

import dre_amd as D
import _balance_cases as bc
import _svd_jacobi_model as sv
from conftest import ROOT

EPS = np.finfo(float).eps


# ---- the SVD model ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sv.CASES))
def test_model_against_numpy_and_the_record(name):
    A, r, rec = sv.case(name), sv.run(name), sv.recorded()[name]
    m, w = A.shape
    print(f"{name}: {m} x {w} sweeps {r['sweeps']} rounds {r['rounds']} rank {r['rank']} " + " ".join(f"{k} {e:.2e}" for k, e in zip(sv.MEASURES, r["err"])))
    assert 1 <= r["sweeps"] <= sv.MAX_SWEEPS and rec["shape"] == [m, w]
    # a backward-stable method that applies r rounds of orthogonal 32-column updates: each measure stays below (rounds + 1) * 32 eps, the
    # orthogonality measures (Frobenius norms over k columns) below sqrt(k) times that
    cap = (r["rounds"] + 1) * 32 * EPS
    e_sig, e_v, e_res, e_u = r["err"]
    assert e_sig <= cap and e_res <= cap and e_v <= cap * np.sqrt(min(m, w)) and e_u <= cap * np.sqrt(min(m, w))
    # the record is this model's run (other BLAS builds sum in another order: a sweep or two more or less, figures within a factor of 3)
    assert abs(r["sweeps"] - rec["sweeps"]) <= 2 and r["rank"] == rec["rank"]
    for live, key in zip(r["err"], sv.MEASURES):
        assert live <= 3 * rec[key] + m * EPS and rec[key] <= 3 * live + m * EPS
    s = r["s"]
    assert (s >= 0).all() and (np.diff(s) <= 0).all() and not r["U"][:, r["rank"]:].any()


def test_record_lists_every_case_and_the_model_refuses_non_finite_input():
    assert set(sv.recorded()) == set(sv.CASES) | {"balance"}
    A = sv.case("random40x33").copy()
    A[3, 7] = np.inf
    with pytest.raises(ValueError):
        sv.svd(A)
    assert sv.padded_width(1) == sv.padded_width(32) == 32 and sv.padded_width(33) == 48
    assert sv.run("rank5_50x40")["rank"] == 5 and sv.run("zero")["rank"] == 0 and sv.run("zero")["sweeps"] == 1


def test_order_rule():
    s = np.array([1.0, 0.5, 0.1, 1e-3, 1e-6])
    assert sv.choose_order(s, 5, 2.1e-6) == 4 and sv.choose_order(s, 5, 1.9e-6) == 5 and sv.choose_order(s, 3, 1e-12) == 3
    assert sv.choose_order(s, 5, 10.0) == 0 and sv.choose_order(s, 5, 0.0) == 5
    Z, dropped, neg = sv.sqrt_factor(np.eye(3), np.array([4.0, -1e-9, 0.0]))
    assert Z.shape == (3, 1) and Z[0, 0] == 2.0 and dropped == 2 and neg == 1e-9
    assert np.array_equal(sv.sqrt_factor(np.eye(2), np.diag([4.0, 9.0]))[0], np.diag([2.0, 3.0]))


# ---- balanced truncation: the reference alone ----------------------------------------------------------------------------------------------
RANKS = {33: (33, 31), 70: (57, 39), 371: (118, 106)}      # numerical ranks of the controllability / observability Gramian


@pytest.mark.parametrize("n", bc.SIZES)
def test_reference_properties(n):
    """with the reference alone at r = 4, 8, 12: the a-priori bound max_w ||H(iw) - H_r(iw)||_2 <= 2 sum_{i > r} sigma_i holds at the 60
    frequencies (bound / error between 1.99, at n = 33 and r = 8, and 5.2), (A_r, I) is c-stable; the Gramians have
    different numerical ranks (except at n = 33), so that Z_o'E Z_c is rectangular"""
    E, A, Bm, Cm = bc.system(n)
    H = bc.full_transfer(n)
    ref0 = bc.reference(n, 8)
    assert (ref0["r_c"], ref0["r_o"]) == RANKS[n] and ref0["M"].shape == RANKS[n][::-1] and ref0["dropped"] == 0
    for r in bc.ORDERS:
        ref = bc.reference(n, r)
        err, bound = bc.max_norm2(H - bc.reduced_transfer(ref)), ref["bound"]
        print(f"n={n} r={r}: max ||H - H_r|| {err:.3e} bound {bound:.3e} (ratio {bound / err:.2f}) ||W'ET - I|| {ref['eye_err']:.2e} "
              f"max Re lambda(A_r) {np.linalg.eigvals(ref['Ar']).real.max():.3e}")
        assert err <= bound          # (a theorem; the ratio is printed, not asserted)
        assert np.linalg.eigvals(ref["Ar"]).real.max() < 0.0


@pytest.mark.parametrize("n", bc.SIZES)
def test_reference_projections_are_biorthogonal_to_5e14(n):
    """||W'ET - I||_F <= 5.1e-14 for the reference at r = 4, 8, 12.  The reference carries its matrix products in extended precision
    (tests/_balance_cases.py: _reference_balance), so that the measure shows the SVD's backward error scaled by sigma_1 / sigma_r and not
    the rounding of the products: with all products in double it is 5.4e-14 at n = 33 and 7.7e-14 at n = 70 for r = 12, with them in
    extended precision at most 1.5e-14 on the three systems."""
    for r in bc.ORDERS:
        ref = bc.reference(n, r)
        print(f"n={n} r={r}: ||W'ET - I||_F = {ref['eye_err']:.2e}")
    for r in bc.ORDERS:
        assert bc.reference(n, r)["eye_err"] <= 5.1e-14


@pytest.mark.parametrize("n", bc.SIZES)
def test_numpy_chain_against_the_reference_and_the_record(n):
    """the device's path restated in NumPy.  The two chains get their Gramians from different solvers (sign-function replays, truncated at
    n eps, against Bartels-Stewart), each with errors of order n eps ||P||: a Hankel singular value moves by at most
    sqrt(n eps) sigma_1 for that (the square root of a perturbed eigenvalue of P Q), the leading ones, which the reduced model is made of, by
    n eps cond sigma_1 with cond <= 1e3 the condition of the fixtures (tests/_sign_dual_cases.py)"""
    rec, gold = sv.recorded()["balance"][str(n)], bc.golden()
    ref, ch = bc.reference(n, 8), bc.chain(n, 8)
    assert (rec["ref_r_o"], rec["ref_r_c"]) == (ref["r_o"], ref["r_c"]) and (rec["r_o"], rec["r_c"], rec["rank"]) == (ch["r_o"], ch["r_c"], ch["rank"])
    assert ch["sweeps"] <= sv.MAX_SWEEPS and abs(ch["sweeps"] - rec["sweeps"]) <= 2
    tol = rec["tol"]
    for lab, r in (("order8", 8), ("tol", rec["tol_order"])):
        sig, eye, tr = bc.chain_errors(n, r)
        print(f"n={n} {lab}: sigma {sig:.2e} eye {eye:.2e} transfer {tr:.2e}")
        assert sig <= np.sqrt(n * EPS) and eye <= 100 * n * EPS and tr <= 100 * n * EPS * 1e3
        for live, key in ((sig, "sigma_"), (eye, "eye_"), (tr, "transfer_")):
            assert live <= 3 * rec[key + lab] and rec[key + lab] <= 3 * live
        red = bc.chain(n, r)
        assert np.linalg.eigvals(red["Ar"]).real.max() < 0.0
        assert bc.max_norm2(bc.full_transfer(n) - bc.reduced_transfer(red)) <= bc.reference(n, r)["bound"]
    # the order rule, decided by a clear margin at the recorded tolerance, gives the same order in both chains
    assert tol == pytest.approx(bc.clear_tol(ref["hsv"]), rel=1e-6)
    for r in (rec["tol_order"], rec["tol_order"] - 1):
        assert not 0.9 <= bc.tail_ratio(ref["hsv"], r, tol) <= 1.1
    assert bc.reference(n, 0, tol)["order"] == bc.chain(n, 0, tol)["order"] == rec["tol_order"]
    # the recorded reference is the live one
    k = len(ref["hsv"])
    assert gold[f"hsv_{n}"].shape == (k,) and np.abs(gold[f"hsv_{n}"] - ref["hsv"]).max() <= np.sqrt(n * EPS) * ref["hsv"][0]
    assert np.abs(gold[f"hsv_{n}"][:12] - ref["hsv"][:12]).max() <= 1e3 * n * EPS * ref["hsv"][0]
    assert bc.max_norm2(gold[f"H_{n}"] - bc.full_transfer(n)) <= 1e3 * n * EPS * bc.max_norm2(bc.full_transfer(n))
    assert float(gold[f"h0_{n}"]) == pytest.approx(bc.h0_norm(n), rel=1e-9)
    for lab, r in (("order8", 8), ("tol", rec["tol_order"])):
        assert bc.max_norm2(gold[f"Hr_{lab}_{n}"] - bc.reduced_transfer(bc.reference(n, r))) <= 1e3 * n * EPS * bc.h0_norm(n)
    if n == 371:
        assert np.array_equal(sv.hankel371(), ref["M"]) or np.linalg.norm(sv.hankel371() - ref["M"]) <= np.sqrt(n * EPS) * np.linalg.norm(ref["M"])


# ---- the interfaces ---------------------------------------------------------------------------------------------------------------------
def test_abi_level_and_symbols():
    lib = D._lib.load()
    assert lib.dre_version() >= 110
    header = open(os.path.join(ROOT, "include", "dre_hip.h")).read()
    for name, nargs in (("dre_svd_jacobi", 7), ("dre_balance_lr", 19)):
        assert hasattr(lib, name) and len(D._lib.PROTOTYPES[name][1]) == nargs
        assert re.search(r"\bint " + name + r"\(dre_ctx\* ctx, ", header)
    for name in ("svd_jacobi", "balanced_truncation", "hankel_singular_values", "ReducedModel"):
        assert name in D.__all__ and callable(getattr(D, name))


def test_julia_shim_carries_the_two_calls():
    """static, as tests/test_julia_shim_static.py (which counts the ccall arguments of these calls too)"""
    jdir = os.path.join(ROOT, "differentialriccatiequations.jl_amd", "julia")
    main, bal = open(os.path.join(jdir, "DREHip.jl")).read(), open(os.path.join(jdir, "DREHipBalance.jl")).read()
    assert 'include("DREHipBalance.jl")' in main
    for fn, call in (("svd_jacobi", "dre_svd_jacobi"), ("balanced_truncation", "dre_balance_lr")):
        assert re.search(r"^function " + fn + r"\(", bal, flags=re.M) and len(re.findall(r"ccall\(\(:" + call + r", LIB\), Cint,", bal)) == 1


def _no_device(monkeypatch):
    """any device work would start with a context: make that an error of its own"""
    def boom(*a, **k):
        raise AssertionError("a device context was requested")
    monkeypatch.setattr(D.api.dev, "default_context", boom)


def test_argument_errors_come_before_any_device_work(monkeypatch):
    _no_device(monkeypatch)
    E, A, Bm, Cm = bc.system(33)
    for fn in (D.balanced_truncation, D.hankel_singular_values):
        for alg in (D.ADI(), None, "FactoredSign"):
            with pytest.raises(TypeError, match="FactoredSign\\(\\) or MatrixSign\\(\\).*nothing was run on the device"):
                fn(E, A, Bm, Cm, alg)
        with pytest.raises(TypeError, match="C must be a matrix.*nothing was run on the device"):
            fn(E, A, Bm, "C")
        with pytest.raises(ValueError, match="E and A must be n x n.*nothing was run on the device"):
            fn(E, A, Bm, Cm.T)
        with pytest.raises(ValueError, match="E and A must be n x n.*nothing was run on the device"):
            fn(E, A[:, :30], Bm, Cm)
    for order in (8.0, "8", True):
        with pytest.raises(TypeError, match="order must be None or an int.*nothing was run on the device"):
            D.balanced_truncation(E, A, Bm, Cm, order=order)
    with pytest.raises(ValueError, match="order must be at least 1.*nothing was run on the device"):
        D.balanced_truncation(E, A, Bm, Cm, order=0)
    for tol in (-1.0, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="tol must be a finite non-negative number.*nothing was run on the device"):
            D.balanced_truncation(E, A, Bm, Cm, tol=tol)
    with pytest.raises(ValueError, match="a matrix is expected.*nothing was run on the device"):
        D.svd_jacobi(np.ones(4))
    for tol in (0.0, -1e-3, float("nan")):
        with pytest.raises(ValueError, match="tol must be positive and finite.*nothing was run on the device"):
            D.svd_jacobi(np.eye(3), tol=tol)
