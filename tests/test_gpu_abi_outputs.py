"""The output slots of the C ABI on a call that fails after its argument checks (csrc/abi_out.hpp), at n = 2 and batch = 3.

Single calls: every slot is preset to a sentinel pointer; the call must return its error, dre_last_error the text of the solver that refused,
and every slot must still hold the sentinel.  The failing input is an exactly singular E = diag(1, 0) where the call takes an E and inverts it
(dre_dense_gale_solve, dre_dense_gare_solve_pair).  The others get an operand the solver itself rejects: dre_sign_solve_dense and
dre_sylvester_solve work on a kept factorisation (a singular E is refused when the handle is made) and get a 3 x 3 right-hand side,
dre_balance_lr never inverts E and gets a B of three rows, dre_svd_jacobi has neither an E nor, at this size, a shape it refuses, and gets a
matrix with a NaN entry, which its first sweep reports.

Batched calls: the middle member's E is singular.  Slots 0 and 2 hold live handles of finite matrices, slot 1 is null, status is
[0, DRE_ERR_SINGULAR, 0]; dre_dense_gale_solve_batched returns DRE_OK, dre_dense_gare_solve_batched the failed member's code (by design).

The messages are those of the solver sources (dense_sign.hip, dense_are.hip, dense_sylvester.hip, svd_jacobi.hip, balance.hip, dense_batch.hip,
dense_are_batch.hip), written out here.  No call faults: a zero pivot and a refused operand are ordinary reported errors."""
import ctypes as C

import numpy as np
import pytest

import dre_amd.device as dev

pytestmark = pytest.mark.gpu

ERR_INVALID, ERR_SINGULAR = -1, -4
SENTINEL = 0x5E5E5E50
I2 = np.eye(2)
E_SINGULAR = np.diag([1.0, 0.0])
E_REGULAR = np.diag([1.0, 2.0])
NULL = C.c_void_p()


def _slots(k):
    return [C.c_void_p(SENTINEL) for _ in range(k)]


def _refused(ctx, rc, code, msg, slots):
    err = (ctx.lib.dre_last_error(ctx.ptr) or b"").decode()
    print(f"rc {rc}, dre_last_error {err!r}, slots {[hex(s.value or 0) for s in slots]}")
    assert rc == code and rc != 0
    assert err == msg
    assert all(s.value == SENTINEL for s in slots)


def _take(ctx, arr, b):
    """Member b of a batched call's output array as a matrix the test owns (and frees)."""
    assert arr[b], b
    return dev.DenseMatrix(ctx, C.c_void_p(arr[b])).numpy()


def test_output_slots_of_failed_calls(ctx):
    lib, up = ctx.lib, ctx.upload
    ii, dd = (C.c_int64 * 16)(), (C.c_double * 16)()
    Es, Er, F, R, R3 = up(E_SINGULAR), up(E_REGULAR), up(-I2), up(I2), up(np.eye(3))
    B, Ct = up(np.array([[1.0], [0.5]])), up(np.array([[0.5], [1.0]]))

    s = _slots(1)
    rc = lib.dre_dense_gale_solve(ctx.ptr, Es.ptr, F.ptr, R.ptr, 50, 0.0, 2, C.byref(s[0]), ii, dd)
    _refused(ctx, rc, ERR_SINGULAR, "dense path: E is singular (zero pivot in the Gauss-Jordan inversion)", s)

    s = _slots(2)          # (max_refine = 0: with refinement the Lyapunov solver of the Newton steps inverts E first, under its own name)
    rc = lib.dre_dense_gare_solve_pair(ctx.ptr, Es.ptr, F.ptr, B.ptr, NULL, Ct.ptr, NULL, 50, 0.0, 0, C.byref(s[0]), C.byref(s[1]), ii, dd)
    _refused(ctx, rc, ERR_SINGULAR, "dense GARE: E is singular (zero pivot in the Gauss-Jordan inversion)", s)

    sign = C.c_void_p()
    ctx.chk(lib.dre_sign_create(ctx.ptr, Er.ptr, F.ptr, 50, 0.0, C.byref(sign)))
    try:
        s = _slots(1)
        rc = lib.dre_sign_solve_dense(ctx.ptr, sign, R3.ptr, 2, C.byref(s[0]), ii, dd)
        _refused(ctx, rc, ERR_INVALID, "dense path: R and X must be n x n", s)
    finally:
        lib.dre_sign_free(ctx.ptr, sign)

    sylv = C.c_void_p()
    ctx.chk(lib.dre_sylvester_create(ctx.ptr, Er.ptr, F.ptr, NULL, F.ptr, 50, 0.0, C.byref(sylv)))
    try:
        s = _slots(1)
        rc = lib.dre_sylvester_solve(ctx.ptr, sylv, R3.ptr, 0, 2, C.byref(s[0]), ii, dd)
        _refused(ctx, rc, ERR_INVALID, "dense Sylvester: C and X must be n x m", s)
    finally:
        lib.dre_sylvester_destroy(ctx.ptr, sylv)

    s = _slots(3)
    Anan = up(np.array([[1.0, 2.0], [np.nan, 4.0]]))          # (kept in a name: a temporary's finaliser would free the handle before the call)
    rc = lib.dre_svd_jacobi(ctx.ptr, Anan.ptr, 0.0, C.byref(s[0]), C.byref(s[1]), C.byref(s[2]), ii)
    _refused(ctx, rc, ERR_INVALID, "svd_jacobi: the matrix has non-finite entries", s)

    s = _slots(6)
    B3, Cq, L, Dg = up(np.ones((3, 1))), up(np.ones((1, 2))), up(I2), up(np.ones((2, 1)))
    rc = lib.dre_balance_lr(ctx.ptr, Es.ptr, F.ptr, B3.ptr, Cq.ptr, L.ptr, Dg.ptr, L.ptr, Dg.ptr, 0, 1e-8, *[C.byref(x) for x in s], ii, dd)
    _refused(ctx, rc, ERR_INVALID, "balance_lr: B must have n rows and C n columns", s)

    _batched_calls_with_a_failed_member(ctx)


def _batched_calls_with_a_failed_member(ctx):
    lib, up = ctx.lib, ctx.upload
    keep = [up(M) for M in (E_REGULAR, E_SINGULAR, -I2, I2, np.array([[1.0], [0.5]]), np.array([[0.5], [1.0]]))]
    Er, Es, F, R, B, Ct = [k.ptr for k in keep]
    arr = lambda *p: (C.c_void_p * 3)(*p)
    ii, dd = (C.c_int64 * 6)(), (C.c_double * 6)()

    X, st = arr(SENTINEL, SENTINEL, SENTINEL), (C.c_int32 * 3)(9, 9, 9)
    rc = lib.dre_dense_gale_solve_batched(ctx.ptr, 3, arr(Er, Es, Er), arr(F, F, F), arr(R, R, R), 50, 0.0, 2, X, ii, dd, st)
    err = (lib.dre_last_error(ctx.ptr) or b"").decode()
    print(f"gale batched: rc {rc}, status {list(st)}, dre_last_error {err!r}")
    assert rc == 0 and list(st) == [0, ERR_SINGULAR, 0]
    assert err == "batched dense path, member 1: E is singular (zero pivot in the Gauss-Jordan inversion)"
    assert lib.dre_batch_member_error(ctx.ptr, 1).decode() == err and lib.dre_batch_member_error(ctx.ptr, 0) == b""
    assert X[1] is None
    X0, X2 = _take(ctx, X, 0), _take(ctx, X, 2)
    assert X0.shape == X2.shape == (2, 2) and np.isfinite(X0).all() and np.array_equal(X0, X2)
    # F'XE + E'XF = -R with F = -I, E = diag(1, 2), R = I: X = diag(1/2, 1/4)
    assert np.allclose(X0, np.diag([0.5, 0.25]), rtol=0, atol=1e-12)

    X, st = arr(SENTINEL, SENTINEL, SENTINEL), (C.c_int32 * 3)(9, 9, 9)
    rc = lib.dre_dense_gare_solve_batched(ctx.ptr, 3, arr(Er, Es, Er), arr(F, F, F), arr(B, B, B), None, arr(Ct, Ct, Ct), None, 50, 0.0, 0, X, ii, dd,
                                          st)
    err = (lib.dre_last_error(ctx.ptr) or b"").decode()
    print(f"gare batched: rc {rc}, status {list(st)}, dre_last_error {err!r}")
    assert rc == ERR_SINGULAR and list(st) == [0, ERR_SINGULAR, 0]
    assert err == "batched dense GARE, member 1: E is singular (zero pivot in the Gauss-Jordan inversion)"
    assert X[1] is None
    X0, X2 = _take(ctx, X, 0), _take(ctx, X, 2)
    assert X0.shape == X2.shape == (2, 2) and np.isfinite(X0).all() and np.array_equal(X0, X2)
