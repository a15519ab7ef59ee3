"""Device SVD (svd_jacobi, csrc/svd_jacobi.hip) against numpy.linalg.svd and the NumPy model of the kernel sequence (tests/_svd_jacobi_model.py).

Bounds: each of the four error measures is at most max(MARGIN = 10 times the MODEL's recorded value for the same input, m eps) with m the longer
dimension (tests/golden/svd_jacobi_model.json; tests/test_svd_balance_host.py keeps that record honest); sweeps between 1 and the model's + 2.
The shapes: the inputs of the model's record plus m = 33 and 35 with w = 32 (the K tail of the MFMA loop), 300 x 32 (several row slabs) and
33 x 40 (a wide input, the transposed entry).  The 106 x 118 matrix Z_o'E Z_c of the n = 371 pencil is wide as well."""
import numpy as np
import pytest

import dre_amd as D
import _svd_jacobi_model as sv

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
MARGIN = 10.0
REC = sv.recorded()


@pytest.mark.parametrize("name", list(sv.CASES))
def test_against_numpy_within_ten_times_the_model(ctx, name):
    A, rec = sv.case(name), REC[name]
    m, w = A.shape
    k = min(m, w)
    U, s, V, st = D.svd_jacobi(A, ctx=ctx, return_stats=True)
    assert U.shape == (m, k) and s.shape == (k,) and V.shape == (w, k)
    err = sv.errors(A, U, s, V)
    print(f"{name}: {m} x {w} sweeps {st['sweeps']} (model {rec['sweeps']}) rounds {st['rounds']} rank {st['rank']} (model {rec['rank']}) "
          + " ".join(f"{key} {e:.2e} (model {rec[key]:.2e})" for key, e in zip(sv.MEASURES, err)))
    for key, e in zip(sv.MEASURES, err):
        assert e <= max(MARGIN * rec[key], max(m, w) * EPS), key
    assert 1 <= st["sweeps"] <= rec["sweeps"] + 2
    assert (s >= 0).all() and (np.diff(s) <= 0).all()
    if name in ("rank5_50x40", "zero"):
        assert st["rank"] == rec["rank"]
    # U's columns beyond the numerical rank are exactly zero (the wide inputs here have full rank)
    assert not U[:, st["rank"]:].any() and (np.abs(U[:, :st["rank"]]).max(axis=0) > 0).all()
    # twice the same bits
    U2, s2, V2 = D.svd_jacobi(A, ctx=ctx)
    assert np.array_equal(U, U2) and np.array_equal(s, s2) and np.array_equal(V, V2)


def test_nan_is_a_clean_invalid_and_the_context_lives(ctx):
    A = sv.case("random40x33").copy()
    A[7, 21] = np.nan
    with pytest.raises(D.DREError) as e:
        D.svd_jacobi(A, ctx=ctx)
    assert e.value.code == -1 and "non-finite" in str(e.value)
    assert str(e.value).startswith("libdre_hip error -1: svd_jacobi:") and "member" not in str(e.value)
    A = sv.case("random70x17")
    U, s, V = D.svd_jacobi(A, ctx=ctx)
    assert sv.errors(A, U, s, V)[2] <= max(MARGIN * REC["random70x17"]["residual"], 70 * EPS)


def test_limits_are_checked_before_any_launch(ctx):
    big = ctx.zeros(4097, 4097)
    U, S, V = (D.api.C.c_void_p() for _ in range(3))
    rc = ctx.lib.dre_svd_jacobi(ctx.ptr, big.ptr, 0.0, D.api.C.byref(U), D.api.C.byref(S), D.api.C.byref(V), None)
    assert rc == -1
    # and the context lives
    A = sv.case("one_column")
    U, s, V = D.svd_jacobi(A, ctx=ctx)
    assert abs(s[0] - np.linalg.norm(A)) <= 23 * EPS * s[0]
