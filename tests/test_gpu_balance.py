"""Balanced truncation on the device (balanced_truncation, hankel_singular_values; csrc/balance.hip on top of csrc/svd_jacobi.hip) on the
systems of tests/_balance_cases.py, against the recorded reference (oracle.lyap_dense Gramians, eigh factors, numpy.linalg.svd:
tests/golden/balance_reference.npz) and the NumPy chain's recorded distance from it (tests/golden/svd_jacobi_model.json, "balance").

Bounds: max_i |sigma_i - sigma_i^ref| / sigma_1, ||W'ET - I||_F and max_w ||H_r^device(iw) - H_r^ref(iw)||_2 / ||H(0)||_2 are each at most
MARGIN = 10 times the NumPy chain's value for the same input.  The a-priori bound max_w ||H - H_r|| <= 2 sum_{i > r} sigma_i^ref is a theorem
(the reference meets it with a factor >= 2): a condition, not a tolerance."""
import numpy as np
import pytest

import dre_amd as D
import _balance_cases as bc
import _svd_jacobi_model as sv

pytestmark = pytest.mark.gpu
MARGIN = 10.0
REC = sv.recorded()["balance"]
ALGS = {"factored": D.FactoredSign(), "dense": D.MatrixSign()}
CASES = [(33, "factored"), (33, "dense"), (70, "factored"), (70, "dense"), (371, "factored")]


@pytest.mark.parametrize("how", ["order8", "tol"])
@pytest.mark.parametrize("n,alg", CASES)
def test_reduced_model_against_the_reference(ctx, n, alg, how):
    E, A, Bm, Cm = bc.system(n)
    gold, rec = bc.golden(), REC[str(n)]
    hsv_ref, H, h0, Hr_ref = gold[f"hsv_{n}"], gold[f"H_{n}"], float(gold[f"h0_{n}"]), gold[f"Hr_{how}_{n}"]
    if how == "order8":
        red, info = D.balanced_truncation(E, A, Bm, Cm, ALGS[alg], order=8, ctx=ctx, return_info=True)
        r = 8
    else:
        # the reference's rule is decided by a clear margin at this tolerance
        tol, r = rec["tol"], rec["tol_order"]
        for rr in (r, r - 1):
            assert not 0.9 <= bc.tail_ratio(hsv_ref, rr, tol) <= 1.1
        assert bc.tail_ratio(hsv_ref, r, tol) <= 1.0 < bc.tail_ratio(hsv_ref, r - 1, tol)
        red, info = D.balanced_truncation(E, A, Bm, Cm, ALGS[alg], tol=tol, ctx=ctx, return_info=True)
    assert info["order"] == red.order == r and info["factorizations"] == 1
    assert red.Ar.shape == (r, r) and red.Br.shape == (r, Bm.shape[1]) and red.Cr.shape == (Cm.shape[0], r) and red.T.shape == red.W.shape == (n, r)
    assert np.array_equal(red.Er, np.eye(r))
    k = min(len(hsv_ref), len(red.hsv))
    e_sig = float(np.abs(red.hsv[:k] - hsv_ref[:k]).max() / hsv_ref[0])
    e_eye = float(np.linalg.norm(red.W.T @ E @ red.T - np.eye(r)))
    Hr = bc.reduced_transfer(dict(order=r, Ar=red.Ar, Br=red.Br, Cr=red.Cr))
    e_tr = bc.max_norm2(Hr - Hr_ref) / h0
    err_full, bound = bc.max_norm2(H - Hr), 2.0 * float(np.sum(hsv_ref[r:][::-1]))
    print(f"n={n} {alg} {how}: r {r} rank {info['rank']} r_c {info['r_c']} r_o {info['r_o']} dropped {info['dropped']} sweeps {info['svd_sweeps']} "
          f"sigma {e_sig:.2e} (chain {rec['sigma_' + how]:.2e}) eye {e_eye:.2e} (chain {rec['eye_' + how]:.2e}; reported {info['eye_err']:.2e}) "
          f"transfer {e_tr:.2e} (chain {rec['transfer_' + how]:.2e}) max ||H - H_r|| {err_full:.3e} bound {bound:.3e}")
    assert e_sig <= MARGIN * rec["sigma_" + how]
    assert e_eye <= MARGIN * rec["eye_" + how] and info["eye_err"] <= MARGIN * rec["eye_" + how]
    assert e_tr <= MARGIN * rec["transfer_" + how]
    assert err_full <= bound
    assert np.linalg.eigvals(red.Ar).real.max() < 0.0
    assert (np.diff(red.hsv) <= 0).all() and (red.hsv >= 0).all()


def test_an_order_above_the_numerical_rank_is_invalid_and_the_context_lives(ctx):
    E, A, Bm, Cm = bc.system(33)
    with pytest.raises(D.DREError) as e:
        D.balanced_truncation(E, A, Bm, Cm, order=34, ctx=ctx)
    assert e.value.code == -1 and "numerical rank" in str(e.value)
    hsv = D.hankel_singular_values(E, A, Bm, Cm, ctx=ctx)
    ref = bc.golden()["hsv_33"]
    k = min(len(hsv), len(ref))
    assert np.abs(hsv[:k] - ref[:k]).max() / ref[0] <= MARGIN * REC["33"]["sigma_order8"]


def test_shape_errors_of_the_c_entry_come_back_as_invalid(ctx):
    E, A, Bm, Cm = (ctx.upload(M) for M in bc.system(33))
    L, d = ctx.upload(np.ones((33, 3))), ctx.upload(np.ones((3, 1)))
    out = [D.api.C.c_void_p() for _ in range(6)]
    refs = [D.api.C.byref(p) for p in out]
    bad_d, bad_l = ctx.upload(np.ones((2, 1))), ctx.upload(np.ones((32, 3)))
    for args in ((E, A, Bm, Cm, L, bad_d, L, d), (E, A, Bm, Cm, bad_l, d, L, d), (E, A, Cm, Cm, L, d, L, d), (E, A, Bm, Bm, L, d, L, d)):
        assert ctx.lib.dre_balance_lr(ctx.ptr, *(a.ptr for a in args), 0, 1e-8, *refs, None, None) == -1
    assert ctx.lib.dre_balance_lr(ctx.ptr, *(a.ptr for a in (E, A, Bm, Cm, L, d, L, d)), -1, 1e-8, *refs, None, None) == -1
    # a vector and a diagonal matrix are the same D
    ii = (D.api.C.c_int64 * 6)()
    res = []
    for dm in (d, ctx.upload(np.eye(3))):
        assert ctx.lib.dre_balance_lr(ctx.ptr, *(a.ptr for a in (E, A, Bm, Cm, L, dm, L, dm)), 0, 1e-8, *refs, ii, None) == 0
        res.append([D.DenseMatrix(ctx, D.api.C.c_void_p(p.value)).numpy() for p in out])
    assert all(np.array_equal(a, b) for a, b in zip(*res))
