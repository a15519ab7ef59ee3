"""Ensemble balanced truncation on the device (balanced_truncation_batch: one dre_dense_gale_solve_batched of 2B members, one
dre_sym_eig_jacobi_batched of the 2B Gramians, one dre_balance_lr_batched) on the ensembles of tests/_jacobi_batch_cases.py: the systems of
tests/_balance_cases.py at n = 33 and 70 with two shifted variants each, whose Gramians have different numerical ranks.

Reference per member: tests/_balance_cases.py's own chain (oracle.lyap_dense Gramians, eigh factors, numpy.linalg.svd), recorded in
tests/golden/balance_batch_reference.npz.  Bounds, those of tests/test_gpu_balance.py: max_i |sigma_i - sigma_i^ref| / sigma_1, ||W'ET - I||_F
and max_w ||H_r^device(iw) - H_r^ref(iw)||_2 / ||H(0)||_2 are each at most MARGIN = 10 times the value of the NumPy restatement of the batched
route for the same member (tests/golden/balance_batch_model.json; tests/test_jacobi_batch_host.py keeps both records honest).  The a-priori
bound max_w ||H - H_r|| <= 2 sum_{i > r} sigma_i^ref is a theorem: a condition, not a tolerance."""
import numpy as np
import pytest

import dre_amd as D
import _balance_cases as bc
import _jacobi_batch_cases as jc

pytestmark = pytest.mark.gpu
MARGIN = 10.0
REC = jc.recorded()
INFO_KEYS = {"primal", "dual", "factorizations", "order", "rank", "r_c", "r_o", "dropped", "svd_sweeps", "eye_err", "bound", "neg_max", "padded_shape"}


def check_member(n, i, how, red, info, systems=None):
    """the bounds of one member against its recorded reference and chain"""
    E, A, Bm, Cm = (systems or jc.systems(n))[i]
    gold, rec = jc.golden(), REC[f"{n}_{i}"]
    hsv_ref, H, h0, Hr_ref = gold[f"hsv_{n}_{i}"], gold[f"H_{n}_{i}"], float(gold[f"h0_{n}_{i}"]), gold[f"Hr_{how}_{n}_{i}"]
    r = jc.ORDER if how == "order8" else rec["tol_order"]
    assert set(info) == INFO_KEYS
    assert info["order"] == red.order == r
    assert red.Ar.shape == (r, r) and red.Br.shape == (r, Bm.shape[1]) and red.Cr.shape == (Cm.shape[0], r) and red.T.shape == red.W.shape == (n, r)
    assert np.array_equal(red.Er, np.eye(r))
    e_sig, e_eye, e_tr = jc.errors_against(hsv_ref, Hr_ref, h0, red.hsv, np.linalg.norm(red.W.T @ E @ red.T - np.eye(r)),
                                           dict(order=r, Ar=red.Ar, Br=red.Br, Cr=red.Cr))
    Hr = bc.reduced_transfer(dict(order=r, Ar=red.Ar, Br=red.Br, Cr=red.Cr))
    err_full, bound = bc.max_norm2(H - Hr), 2.0 * float(np.sum(hsv_ref[r:][::-1]))
    print(f"n={n} member {i} {how}: r {r} rank {info['rank']} r_c {info['r_c']} r_o {info['r_o']} padded {info['padded_shape']} sweeps {info['svd_sweeps']} "
          f"sigma {e_sig:.2e} (chain {rec['sigma_' + how]:.2e}) eye {e_eye:.2e} (chain {rec['eye_' + how]:.2e}; reported {info['eye_err']:.2e}) "
          f"transfer {e_tr:.2e} (chain {rec['transfer_' + how]:.2e}) max ||H - H_r|| {err_full:.3e} bound {bound:.3e}")
    assert e_sig <= MARGIN * rec["sigma_" + how]
    assert e_eye <= MARGIN * rec["eye_" + how] and info["eye_err"] <= MARGIN * rec["eye_" + how]
    assert e_tr <= MARGIN * rec["transfer_" + how]
    assert err_full <= bound
    assert np.linalg.eigvals(red.Ar).real.max() < 0.0
    assert (np.diff(red.hsv) <= 0).all() and (red.hsv >= 0).all()


# ---- 1. reference values; 2. a batch of three systems with different Gramian ranks ---------------------------------------------------------
@pytest.mark.parametrize("how", ["order8", "tol"])
@pytest.mark.parametrize("n", jc.SIZES)
def test_reduced_models_against_the_reference(ctx, n, how):
    systems = jc.systems(n)
    if how == "order8":
        out = D.balanced_truncation_batch(systems, order=jc.ORDER, ctx=ctx, return_info=True)
    else:
        # one tolerance for the batch at which every member's reference rule is decided by more than 10 % on both sides
        tol = REC[f"{n}_0"]["tol"]
        assert all(REC[f"{n}_{i}"]["tol"] == tol for i in range(len(systems)))
        for i in range(len(systems)):
            hsv_ref, r = jc.golden()[f"hsv_{n}_{i}"], REC[f"{n}_{i}"]["tol_order"]
            for rr in (r, r - 1):
                assert not 0.9 <= bc.tail_ratio(hsv_ref, rr, tol) <= 1.1
            assert bc.tail_ratio(hsv_ref, r, tol) <= 1.0 < bc.tail_ratio(hsv_ref, r - 1, tol)
        out = D.balanced_truncation_batch(systems, tol=tol, ctx=ctx, return_info=True)
    assert len(out) == len(systems)
    ranks = {(info["r_o"], info["r_c"]) for _, info in out}
    if n == 70:
        assert len(ranks) >= 2                    # the Gramian ranks differ inside the batch: the padding is exercised
    for i, (red, info) in enumerate(out):
        assert info["padded_shape"] == (max(x[1]["r_o"] for x in out), max(x[1]["r_c"] for x in out))
        check_member(n, i, how, red, info)


# ---- 2. the padding contract ---------------------------------------------------------------------------------------------------------------------
def test_a_member_depends_on_the_batch_through_the_padded_shape_only(ctx):
    s = jc.systems(33)[0]
    two = D.balanced_truncation_batch([s, s], order=jc.ORDER, ctx=ctx)
    one = D.balanced_truncation_batch([s], order=jc.ORDER, ctx=ctx)
    for a in (two[1], one[0]):
        for name in ("Ar", "Br", "Cr", "hsv", "T", "W"):
            assert np.array_equal(getattr(two[0], name), getattr(a, name)), name


# ---- 3. per-member failure -----------------------------------------------------------------------------------------------------------------------
def test_an_unstable_member_fails_alone(ctx):
    systems = list(jc.systems(33))
    E, A, Bm, Cm = systems[1]
    bad = [systems[0], (E, -A, Bm, Cm), systems[2]]
    out = D.balanced_truncation_batch(bad, order=jc.ORDER, errors="return", ctx=ctx, return_info=True)
    assert isinstance(out[1], D.DREError) and out[1].code == -7
    for i in (0, 2):
        check_member(33, i, "order8", *out[i])
    with pytest.raises(D.DREError) as e:
        D.balanced_truncation_batch(bad, order=jc.ORDER, ctx=ctx)
    assert e.value.code == -7


def test_an_order_above_the_numerical_rank_is_the_members_invalid(ctx):
    systems = jc.systems(33)
    out = D.balanced_truncation_batch(systems, order=34, errors="return", ctx=ctx)
    assert all(isinstance(x, D.DREError) and x.code == -1 and "numerical rank" in str(x) for x in out)
    assert [f"member {i}" in str(x) for i, x in enumerate(out)] == [True] * 3
    # through the C entry it is the member's status, not the call's; and the context lives
    red = D.balanced_truncation_batch(systems[:1], order=jc.ORDER, ctx=ctx)[0]
    ref = jc.golden()["hsv_33_0"]
    k = min(len(red.hsv), len(ref))
    assert np.abs(red.hsv[:k] - ref[:k]).max() / ref[0] <= MARGIN * REC["33_0"]["sigma_order8"]
