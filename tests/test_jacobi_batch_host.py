"""Batched block Jacobi and ensemble balanced truncation, the part that needs no device: the argument errors that are raised before a context
is touched, the two records of tests/_jacobi_batch_cases.py against their live regeneration, zero padding in the NumPy model of the SVD, and
the three prototypes in the header, the ctypes table and the Julia shim (tests/test_abi.py and tests/test_julia_shim_static.py then cover
export, binding and the ccall argument counts by themselves)."""
import os
import re

import numpy as np
import pytest

import dre_amd as D
import _balance_cases as bc
import _jacobi_batch_cases as jc
import _svd_jacobi_model as sv
from conftest import ROOT

EPS = np.finfo(float).eps
NOTHING = ".*nothing was run on the device"


@pytest.fixture
def no_device(monkeypatch):
    """any device work would start with a context: make that an error of its own"""
    def boom(*a, **k):
        raise AssertionError("a device context was requested")
    monkeypatch.setattr(D.api.dev, "default_context", boom)


# ---- argument errors ---------------------------------------------------------------------------------------------------------------------------
def test_eig_batch_argument_errors_come_before_any_device_work(no_device):
    S = np.eye(4)
    with pytest.raises(ValueError, match="empty list" + NOTHING):
        D.sym_eigh_batch([])
    with pytest.raises(TypeError, match="a list of matrices is expected" + NOTHING):
        D.sym_eigh_batch(S)
    with pytest.raises(ValueError, match="member 1: a square matrix is expected" + NOTHING):
        D.sym_eigh_batch([S, np.ones((4, 3))])
    with pytest.raises(ValueError, match="member 1 has shape \\(5, 5\\), member 0 has \\(4, 4\\)" + NOTHING):
        D.sym_eigh_batch([S, np.eye(5)])
    A = np.eye(4)
    A[0, 1] = 1e-3
    with pytest.raises(ValueError, match="member 2 is not symmetric" + NOTHING):
        D.sym_eigh_batch([S, S, A])
    for tol in (0.0, -1.0):
        with pytest.raises(ValueError, match="tol must be positive" + NOTHING):
            D.sym_eigh_batch([S], tol=tol)
    with pytest.raises(ValueError, match='errors must be "raise" or "return"' + NOTHING):
        D.sym_eigh_batch([S], errors="ignore")
    assert [(w.shape, V.shape) for w, V in D.sym_eigh_batch([np.zeros((0, 0))] * 2)] == [((0,), (0, 0))] * 2


def test_svd_batch_argument_errors_come_before_any_device_work(no_device):
    A = np.ones((4, 3))
    with pytest.raises(ValueError, match="empty list" + NOTHING):
        D.svd_jacobi_batch([])
    with pytest.raises(ValueError, match="member 1: a matrix is expected" + NOTHING):
        D.svd_jacobi_batch([A, np.ones(4)])
    with pytest.raises(ValueError, match="member 1 has shape \\(3, 4\\), member 0 has \\(4, 3\\)" + NOTHING):
        D.svd_jacobi_batch([A, A.T])
    for tol in (0.0, -1e-3, float("nan")):
        with pytest.raises(ValueError, match="tol must be positive and finite" + NOTHING):
            D.svd_jacobi_batch([A], tol=tol)
    with pytest.raises(ValueError, match='errors must be "raise" or "return"' + NOTHING):
        D.svd_jacobi_batch([A], errors=None)


def test_balance_batch_argument_errors_come_before_any_device_work(no_device):
    s33, s70 = jc.systems(33)[0], jc.systems(70)[0]
    E, A, Bm, Cm = s33
    fn = D.balanced_truncation_batch
    with pytest.raises(ValueError, match="empty list" + NOTHING):
        fn([])
    with pytest.raises(TypeError, match="the batched route is the dense one" + NOTHING):
        fn([s33], D.FactoredSign())
    for alg in (D.ADI(), None, "MatrixSign"):
        with pytest.raises(TypeError, match="takes alg = MatrixSign\\(\\)" + NOTHING):
            fn([s33], alg)
    with pytest.raises(TypeError, match="member 1 must be a tuple \\(E, A, B, C\\)" + NOTHING):
        fn([s33, (E, A, Bm)])
    with pytest.raises(TypeError, match="member 1: C must be a matrix" + NOTHING):
        fn([s33, (E, A, Bm, "C")])
    with pytest.raises(ValueError, match="member 0: E and A must be n x n" + NOTHING):
        fn([(E, A, Bm, Cm.T)])
    with pytest.raises(ValueError, match="member 1 has \\(n, m, q\\) = \\(70, 7, 5\\), member 0 has \\(33, 7, 5\\)" + NOTHING):
        fn([s33, s70])
    with pytest.raises(ValueError, match="member 1 has \\(n, m, q\\) = \\(33, 6, 5\\)" + NOTHING):
        fn([s33, (E, A, Bm[:, :6], Cm)])
    for order in (8.0, "8", True):
        with pytest.raises(TypeError, match="order must be None or an int" + NOTHING):
            fn([s33], order=order)
    with pytest.raises(ValueError, match="order must be at least 1" + NOTHING):
        fn([s33], order=0)
    for tol in (-1.0, float("nan"), None):
        with pytest.raises(ValueError, match="tol must be a finite non-negative number" + NOTHING):
            fn([s33], tol=tol)
    with pytest.raises(ValueError, match='errors must be "raise" or "return"' + NOTHING):
        fn([s33], errors="skip")
    big = np.zeros((4097, 4097))
    with pytest.raises(ValueError, match="orders 1 .. 4096, got n = 4097" + NOTHING):
        fn([(big, big, np.zeros((4097, 1)), np.zeros((1, 4097)))])


# ---- the records ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", jc.SIZES)
def test_the_records_are_the_live_reference_and_chain(n):
    """the recorded reference against its regeneration (the bounds of tests/test_svd_balance_host.py for the same quantities); the recorded
    chain figures within a factor of 3 of the live ones (other BLAS builds sum in another order)"""
    gold, live, rec_all, rec_live = jc.golden(), jc.golden_arrays(), jc.recorded(), jc.record()
    assert set(gold) == set(live) and set(rec_all) == set(rec_live) == {f"{m}_{i}" for m in jc.SIZES for i in range(len(jc.SHIFTS))}
    for i in range(len(jc.SHIFTS)):
        key, rec, now = f"{n}_{i}", rec_all[f"{n}_{i}"], rec_live[f"{n}_{i}"]
        s1, h0 = live[f"hsv_{key}"][0], float(live[f"h0_{key}"])
        assert gold[f"hsv_{key}"].shape == live[f"hsv_{key}"].shape
        assert np.abs(gold[f"hsv_{key}"] - live[f"hsv_{key}"]).max() <= np.sqrt(n * EPS) * s1
        assert np.abs(gold[f"hsv_{key}"][:12] - live[f"hsv_{key}"][:12]).max() <= 1e3 * n * EPS * s1
        assert bc.max_norm2(gold[f"H_{key}"] - live[f"H_{key}"]) <= 1e3 * n * EPS * bc.max_norm2(live[f"H_{key}"])
        assert float(gold[f"h0_{key}"]) == pytest.approx(h0, rel=1e-9)
        for lab in ("order8", "tol"):
            assert gold[f"Hr_{lab}_{key}"].shape == live[f"Hr_{lab}_{key}"].shape
            assert bc.max_norm2(gold[f"Hr_{lab}_{key}"] - live[f"Hr_{lab}_{key}"]) <= 1e3 * n * EPS * h0
        for k in ("ref_r_o", "ref_r_c", "r_o", "r_c", "rank", "padded_shape", "tol_order"):
            assert rec[k] == now[k], k
        assert rec["tol"] == pytest.approx(now["tol"], rel=1e-6) and abs(rec["sweeps"] - now["sweeps"]) <= 2
        for lab in ("order8", "tol"):
            for k in ("sigma_", "eye_", "transfer_"):
                assert now[k + lab] <= 3 * rec[k + lab] and rec[k + lab] <= 3 * now[k + lab], k + lab
        # the systems are what the docstring says: c-stable variants, a tolerance decided by more than 10 % on both sides
        E, A, _, _ = jc.systems(n)[i]
        assert np.linalg.eigvals(np.linalg.solve(E, A)).real.max() < 0.0
        for r in (rec["tol_order"], rec["tol_order"] - 1):
            assert not 0.9 <= bc.tail_ratio(gold[f"hsv_{key}"], r, rec["tol"]) <= 1.1
    assert len({rec_all[f"{n}_{i}"]["tol"] for i in range(len(jc.SHIFTS))}) == 1
    if n == 70:
        assert len({(rec_all[f"{n}_{i}"]["r_o"], rec_all[f"{n}_{i}"]["r_c"]) for i in range(len(jc.SHIFTS))}) >= 2


# ---- zero padding in the model ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", jc.SIZES)
def test_zero_padding_leaves_a_members_singular_values_and_reduced_model(n):
    """a member of the stack sees its M with zero rows and columns added: zero rows add nothing to a Gram matrix and zero columns are never
    rotated (h_rr h_cc > 0 fails), so the model on the padded M gives the unpadded singular values within m eps sigma_1 (m the padded longer
    dimension, the sum length of a Gram entry), zeros for the padding, and the reduced model within the recorded chain distance"""
    i = len(jc.SHIFTS) - 1                                    # the member with the smallest ranks at n = 70: padded on both sides
    own = jc.chain(n, i, jc.ORDER)
    M = own["M"]
    shape = (M.shape[0] + 5, M.shape[1] + 19)
    Mp = np.zeros(shape)
    Mp[:M.shape[0], :M.shape[1]] = M
    k = min(M.shape)
    s0, (Up, sp, Vp, stp) = sv.svd(M)[1], sv.svd(Mp)
    assert np.abs(sp[:k] - s0).max() <= max(shape) * EPS * s0[0]
    # the padding takes no part in the triplets that count: exactly zero in the padded rows of U and V (a zero column keeps its unit vector,
    # which belongs to a zero singular value beyond the rank)
    assert not Up[M.shape[0]:, :stp["rank"]].any() and not Vp[M.shape[1]:, :stp["rank"]].any()
    assert stp["rank"] <= k
    pad = jc.chain(n, i, jc.ORDER, shape=shape)
    rec = jc.recorded()[f"{n}_{i}"]
    assert pad["order"] == own["order"] == jc.ORDER and (pad["r_o"], pad["r_c"]) == M.shape
    d = bc.max_norm2(bc.reduced_transfer(pad) - bc.reduced_transfer(own)) / jc.h0_norm(n, i)
    print(f"n={n}: padded {shape} against {M.shape}: sigma {np.abs(sp[:k] - s0).max() / s0[0]:.2e} transfer {d:.2e} (chain {rec['transfer_order8']:.2e})")
    assert d <= rec["transfer_order8"] and pad["eye_err"] <= 3 * rec["eye_order8"]


# ---- the interfaces ------------------------------------------------------------------------------------------------------------------------------
CALLS = (("dre_sym_eig_jacobi_batched", 8), ("dre_svd_jacobi_batched", 9), ("dre_balance_lr_batched", 21))


def test_abi_level_prototypes_and_exports():
    lib = D._lib.load()
    assert lib.dre_version() >= 111
    header = open(os.path.join(ROOT, "include", "dre_hip.h")).read()
    for name, nargs in CALLS:
        assert hasattr(lib, name) and len(D._lib.PROTOTYPES[name][1]) == nargs
        assert re.search(r"\bint " + name + r"\(dre_ctx\* ctx, int batch, ", header)
    for name in ("sym_eigh_batch", "svd_jacobi_batch", "balanced_truncation_batch"):
        assert name in D.__all__ and callable(getattr(D, name))


def test_julia_shim_carries_the_three_calls():
    """static, as tests/test_julia_shim_static.py (which counts the ccall arguments of these calls too)"""
    jdir = os.path.join(ROOT, "differentialriccatiequations.jl_amd", "julia")
    main, jl = open(os.path.join(jdir, "DREHip.jl")).read(), open(os.path.join(jdir, "DREHipBatchJacobi.jl")).read()
    assert 'include("DREHipBatchJacobi.jl")' in main
    for fn, (call, _) in zip(("sym_eigh_batch", "svd_jacobi_batch", "balance_lr_batch"), CALLS):
        assert re.search(r"^function " + fn + r"\(", jl, flags=re.M) and len(re.findall(r"ccall\(\(:" + call + r", LIB\), Cint,", jl)) == 1
