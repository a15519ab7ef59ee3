"""Batched block Jacobi on the device (sym_eigh_batch, svd_jacobi_batch; csrc/sym_jacobi.hip, csrc/svd_jacobi.hip) against the single solvers.

The contract is bitwise: every output array of every member of a batch equals what svd_jacobi / sym_eigh(method="jacobi") returns for that
member alone (numpy.array_equal), and so do the sweeps, rounds and rank.  The members of a batch (tests/_jacobi_batch_cases.py) need different
numbers of sweeps, so the workgroups of a finished member return at entry while the others go on.  The accuracy bound of the single SVD
(10 times the model's recorded value, tests/test_gpu_svd_jacobi.py) is carried by that equality and asserted once explicitly.

Limits through the raw C entries: the 4097 x 4097 member is the SVD's (its shorter dimension is limited to 4096); the eigensolver's single
call has no such limit (its order limit is the 32-bit index limit), so its refused arguments are batch = 0, two orders in one batch and a
member that is not square."""
import ctypes as C

import numpy as np
import pytest

import dre_amd as D
import _jacobi_batch_cases as jc
import _svd_jacobi_model as sv

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
MARGIN = 10.0
_single = {}


def single_svd(ctx, m, w):
    if ("svd", m, w) not in _single:
        _single["svd", m, w] = [D.svd_jacobi(A, ctx=ctx, return_stats=True) for A in jc.svd_members(m, w)]
    return _single["svd", m, w]


def single_eig(ctx, q):
    if ("eig", q) not in _single:
        _single["eig", q] = [D.sym_eigh(A, ctx=ctx, return_stats=True) for A in jc.eig_members(q)]
    return _single["eig", q]


def same(got, want):
    """every array bitwise, the stats dict equal"""
    assert len(got) == len(want)
    for g, x in zip(got, want):
        if isinstance(x, dict):
            assert g == x
        else:
            assert g.shape == x.shape and np.array_equal(g, x)
    return True


# ---- 1. bitwise equality with the single solver ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,w", jc.SVD_SHAPES)
def test_svd_batch_is_bitwise_the_single_solver(ctx, m, w):
    want = single_svd(ctx, m, w)
    got = D.svd_jacobi_batch(jc.svd_members(m, w), ctx=ctx, return_stats=True)
    sweeps = [x[3]["sweeps"] for x in want]
    print(f"{m} x {w}: sweeps {sweeps} ranks {[x[3]['rank'] for x in want]}")
    for g, x in zip(got, want):
        assert same(g, x)
    k = min(m, w)
    assert got[2][3] == dict(sweeps=1, rounds=want[2][3]["rounds"], rank=0) and not got[2][1].any()       # the zero member: one sweep
    assert all(g[0].shape == (m, k) and g[1].shape == (k,) and g[2].shape == (w, k) for g in got)
    if k > 1:
        assert len(set(sweeps)) >= 2 and max(sweeps) > 1          # the members leave the iteration at different sweeps


@pytest.mark.parametrize("q", jc.EIG_ORDERS)
def test_eig_batch_is_bitwise_the_single_solver(ctx, q):
    want = single_eig(ctx, q)
    got = D.sym_eigh_batch(jc.eig_members(q), ctx=ctx, return_stats=True)
    sweeps = [x[2]["sweeps"] for x in want]
    print(f"q = {q}: sweeps {sweeps}")
    for g, x in zip(got, want):
        assert same(g, x)
    assert got[2][2]["sweeps"] == 0 and np.array_equal(got[2][0], np.linspace(1.0, 2.0, q))               # the diagonal member: no sweep
    if q > 1:
        assert len(set(sweeps)) >= 2 and max(sweeps) >= 1
    for (w_, V, _), A in zip(got, jc.eig_members(q)):
        assert (np.diff(w_) >= 0).all()
        assert np.abs(w_ - np.linalg.eigvalsh(A)).max() <= 10 * max(q, 32) * EPS * np.linalg.norm(A)


# ---- 2. independence of the batch ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,w", [(40, 33), (33, 40)])
def test_svd_members_do_not_depend_on_the_batch(ctx, m, w):
    mem, want = jc.svd_members(m, w), single_svd(ctx, m, w)
    rev = D.svd_jacobi_batch(mem[::-1], ctx=ctx, return_stats=True)
    for g, x in zip(rev, want[::-1]):
        assert same(g, x)
    many = D.svd_jacobi_batch((mem * 5)[:17], ctx=ctx, return_stats=True)
    assert len(many) == 17
    for b, g in enumerate(many):
        assert same(g, want[b % 4])
    for b in (0, 3):
        assert same(D.svd_jacobi_batch([mem[b]], ctx=ctx, return_stats=True)[0], want[b])


@pytest.mark.parametrize("q", [33, 70])
def test_eig_members_do_not_depend_on_the_batch(ctx, q):
    mem, want = jc.eig_members(q), single_eig(ctx, q)
    rev = D.sym_eigh_batch(mem[::-1], ctx=ctx, return_stats=True)
    for g, x in zip(rev, want[::-1]):
        assert same(g, x)
    many = D.sym_eigh_batch((mem * 5)[:17], ctx=ctx, return_stats=True)
    assert len(many) == 17
    for b, g in enumerate(many):
        assert same(g, want[b % 4])
    for b in (0, 3):
        assert same(D.sym_eigh_batch([mem[b]], ctx=ctx, return_stats=True)[0], want[b])


# ---- 3. a failed member is dropped -----------------------------------------------------------------------------------------------------------
def test_a_non_finite_svd_member_fails_alone(ctx):
    mem, want = list(jc.svd_members(40, 33)), single_svd(ctx, 40, 33)
    bad = mem[1].copy()
    bad[7, 21] = np.nan
    got = D.svd_jacobi_batch([mem[0], bad, mem[2], mem[3]], errors="return", ctx=ctx, return_stats=True)
    assert isinstance(got[1], D.DREError) and got[1].code == -1 and "non-finite" in str(got[1]) and "member 1" in str(got[1])
    for b in (0, 2, 3):
        assert same(got[b], want[b])
    with pytest.raises(D.DREError) as e:
        D.svd_jacobi_batch([mem[0], bad, mem[2], mem[3]], ctx=ctx)
    assert e.value.code == -1 and "non-finite" in str(e.value)
    for g, x in zip(D.svd_jacobi_batch(mem, ctx=ctx, return_stats=True), want):          # the context solves a following batch
        assert same(g, x)


def test_a_non_finite_eig_member_fails_alone(ctx):
    mem, want = list(jc.eig_members(33)), single_eig(ctx, 33)
    bad = mem[0].copy()
    bad[5, 5] = np.nan
    got = D.sym_eigh_batch([bad, mem[1], mem[2], mem[3]], errors="return", ctx=ctx, return_stats=True)
    assert isinstance(got[0], D.DREError) and got[0].code == -1 and "non-finite" in str(got[0]) and "member 0" in str(got[0])
    for b in (1, 2, 3):
        assert same(got[b], want[b])
    with pytest.raises(D.DREError) as e:
        D.sym_eigh_batch([bad, mem[1], mem[2], mem[3]], ctx=ctx)
    assert e.value.code == -1 and "non-finite" in str(e.value)
    for g, x in zip(D.sym_eigh_batch(mem, ctx=ctx, return_stats=True), want):
        assert same(g, x)


# ---- 4. limits before any launch -------------------------------------------------------------------------------------------------------------
def _arr(hs):
    return (C.c_void_p * len(hs))(*[h.ptr for h in hs])


def _last_error(ctx):
    return ctx.lib.dre_last_error(ctx.ptr).decode()


def test_limits_of_the_c_entries_come_before_any_launch(ctx):
    lib = ctx.lib
    a, b, big = ctx.upload(np.eye(5)), ctx.upload(np.ones((6, 5))), ctx.zeros(4097, 4097)
    out = [(C.c_void_p * 2)() for _ in range(3)]
    st = (C.c_int32 * 2)()
    assert lib.dre_svd_jacobi_batched(ctx.ptr, 0, _arr([a]), 0.0, *out, None, st) == -1
    assert lib.dre_svd_jacobi_batched(ctx.ptr, 2, _arr([a, b]), 0.0, *out, None, st) == -1 and "one shape" in _last_error(ctx)
    assert lib.dre_svd_jacobi_batched(ctx.ptr, 2, _arr([big, big]), 0.0, *out, None, st) == -1 and "4096" in _last_error(ctx)
    assert lib.dre_svd_jacobi_batched(ctx.ptr, 1, None, 0.0, *out, None, st) == -1
    assert lib.dre_sym_eig_jacobi_batched(ctx.ptr, 0, _arr([a]), 0.0, out[0], out[1], None, st) == -1
    assert lib.dre_sym_eig_jacobi_batched(ctx.ptr, 2, _arr([a, ctx.upload(np.eye(6))]), 0.0, out[0], out[1], None, st) == -1
    assert lib.dre_sym_eig_jacobi_batched(ctx.ptr, 2, _arr([b, b]), 0.0, out[0], out[1], None, st) == -1
    assert lib.dre_sym_eig_jacobi_batched(ctx.ptr, 1, _arr([a]), 0.0, None, out[1], None, st) == -1
    assert all(not p for o in out for p in o)
    # the context lives
    rng = np.random.default_rng(77)
    As = [rng.standard_normal((9, 4)) for _ in range(3)]
    for A, (U, s, V) in zip(As, D.svd_jacobi_batch(As, ctx=ctx)):
        assert np.abs(s - np.linalg.svd(A, compute_uv=False)).max() <= 32 * EPS * s[0] and np.linalg.norm(A - (U * s) @ V.T) <= 32 * EPS * np.linalg.norm(A)
    Ss = [A.T @ A for A in As]
    for S, (w_, V) in zip(Ss, D.sym_eigh_batch(Ss, ctx=ctx)):
        assert np.abs(w_ - np.linalg.eigvalsh(S)).max() <= 32 * EPS * np.linalg.norm(S) and np.linalg.norm(S @ V - V * w_) <= 32 * 4 * EPS * np.linalg.norm(S)


# ---- 5. accuracy, once explicitly --------------------------------------------------------------------------------------------------------------
def test_accuracy_of_a_batch_of_model_cases(ctx):
    """the 40 x 33 case of the model's record inside a batch: the bounds of tests/test_gpu_svd_jacobi.py"""
    name = "random40x33"
    A, rec = sv.case(name), sv.recorded()[name]
    got = D.svd_jacobi_batch([np.zeros(A.shape), A, jc.svd_members(40, 33)[3], A], ctx=ctx, return_stats=True)
    for U, s, V, st in (got[1], got[3]):
        err = sv.errors(A, U, s, V)
        print(name, st, " ".join(f"{key} {e:.2e} (model {rec[key]:.2e})" for key, e in zip(sv.MEASURES, err)))
        for key, e in zip(sv.MEASURES, err):
            assert e <= max(MARGIN * rec[key], 40 * EPS), key
        assert 1 <= st["sweeps"] <= rec["sweeps"] + 2 and st["rank"] == rec["rank"]
    assert same(got[1], got[3])
