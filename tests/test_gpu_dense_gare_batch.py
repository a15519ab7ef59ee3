"""Batched dense GARE on the device (csrc/dense_are_batch.hip): `solve_batch` on a list of GAREProblem against the single-problem
`solve(GAREProblem, MatrixSign())` of the same member on the same device, the Kleinman-Newton fixture and the NumPy model
(tests/_hamiltonian_sign_model.py).  The n = 371 bounds are those of tests/test_gpu_dense_gare.py; every figure is printed before it is
asserted.

Measured on one MI355X (test_smallest_shapes, batched residual / single residual per regular member, bound max(100 n eps, 10 x single)):
n = 37: 3.983e-12 / 3.983e-12, 5.422e-13 / 5.422e-13, 6.305e-13 / 6.305e-13, 1.542e-13 / 1.542e-13; n = 70: 5.648e-14 / 5.648e-14,
1.671e-13 / 1.671e-13, 1.131e-12 / 1.131e-12, 1.216e-13 / 1.216e-13."""
import ctypes as C
import os

import numpy as np
import pytest

import dre_amd as D
import _hamiltonian_sign_model as hm
from conftest import GOLDEN
from test_dense_gare_host import closed_loop_max_real, oscillator_pencil, spd, steel_dense, unstable_variant

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
N = 371


def _are(E, A, B, C, beta=1.0, Rinv=None, gamma=1.0, S=None):
    Rinv = np.eye(B.shape[1]) if Rinv is None else Rinv
    S = np.eye(C.shape[0]) if S is None else S
    return D.GAREProblem(E, A, beta * D.lowrank(B, Rinv), gamma * D.lowrank(np.ascontiguousarray(C.T), S))


def _dense_gq(are):
    (b, B, R), (g, Ct, S) = are.G, are.Q
    return b * B @ R @ B.T, g * Ct @ S @ Ct.T


@pytest.fixture(scope="module")
def steel():
    E, A, B, C = steel_dense(N)
    return E, A, B, C, unstable_variant(E, A)


def _regular_members(n):
    probs = []
    for s in range(4):
        rng = np.random.default_rng(100 + s)
        E = np.eye(n) + 0.1 * rng.standard_normal((n, n))
        V = np.eye(n) + 0.3 * rng.standard_normal((n, n)) / np.sqrt(n)
        lam = np.concatenate([rng.uniform(0.2, 1.0, 3), -rng.uniform(0.5, 3.0, n - 3)])
        A = E @ V @ np.diag(lam) @ np.linalg.inv(V)
        B = rng.standard_normal((n, 2))
        Cm = rng.standard_normal((2, n))
        probs.append(_are(E, A, B, Cm))
    return probs


@pytest.fixture(scope="module")
def small37():
    """the four regular n = 37 members and their full-batch solutions (shared, never modified)"""
    probs = _regular_members(37)
    full = D.solve_batch(probs, D.MatrixSign(maxiters=25))
    return probs, full


# ---- 1. steel ensemble ------------------------------------------------------------------------------------------------------------------
def test_steel_ensemble_371(ctx, steel):
    E, A, B, Cm, Au = steel
    members = [_are(E, A, B, Cm), _are(E, Au, B, Cm), _are(E, A, B, Cm, 2.5, spd(B.shape[1], 1), 0.7, spd(Cm.shape[0], 2)), _are(E, A, 0.5 * B, Cm)]
    out = D.solve_batch(members, D.MatrixSign(), return_stats=True)
    assert len(out) == 4
    g = np.load(os.path.join(GOLDEN, "gare_371.npz"))
    bound = 100 * N * EPS
    for b, p in enumerate(members):
        X, info = out[b]
        Xs, si = D.solve(p, D.MatrixSign(), return_info=True)
        dl = D.delta(X, Xs)
        print(f"steel member {b}: res {info['res']:.3e} (single {si['res']:.3e}, bound {bound:.3e}), delta to single {dl:.3e}, "
              f"iters {info['iters']} (single {si['iters']}), refinements {info['refinements']} (single {si['refinements']})")
        assert info["res"] <= bound
        assert dl < 1e-10
        assert abs(info["iters"] - si["iters"]) <= 1
        assert np.array_equal(X, X.T)
    dk = D.delta(out[0][1]["K"], g["K_dense"])
    print(f"steel member 0: delta(K, fixture) {dk:.3e}")
    assert dk < 1e-7
    G, _ = _dense_gq(members[1])
    mr = closed_loop_max_real(E, Au, G, out[1][0])
    print(f"unstable member: max Re of the closed loop {mr:.3e}")
    assert mr < 0


# ---- 2. smallest shapes -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [37, 70])
def test_smallest_shapes(ctx, n):
    probs = _regular_members(n)
    Eo, Ao, Bo, Co = oscillator_pencil(n=n)
    alg = D.MatrixSign(maxiters=25)
    out = D.solve_batch(probs + [_are(Eo, Ao, Bo, Co)], alg, errors="return", return_stats=True)
    assert len(out) == 5
    for b, p in enumerate(probs):
        assert not isinstance(out[b], D.DREError), out[b]
        X, info = out[b]
        _, si = D.solve(p, alg, return_info=True)
        G, Q = _dense_gq(p)
        Xm, mi = hm.gare_sign(p.E, p.A, G, Q, maxiters=25)
        bound = max(100 * n * EPS, 10 * si["res"])
        mr = closed_loop_max_real(p.E, p.A, G, X)
        dm = D.delta(X, Xm)
        print(f"n = {n} member {b}: res batched {info['res']:.3e} / single {si['res']:.3e} (bound {bound:.3e}), iters {info['iters']} / "
              f"{si['iters']} / model {mi['iters']}, refinements {info['refinements']} / {si['refinements']} / model {mi['refinements']}, "
              f"max Re closed loop {mr:.3e}, delta to the model {dm:.3e}")
        assert info["res"] <= bound
        assert mr < 0
        assert dm < 1e-8
    print(f"n = {n} member 4: {out[4]!r}")
    assert isinstance(out[4], D.DREError) and out[4].code == -7 and "member 4" in str(out[4])
    with pytest.raises(D.DREError) as e:
        D.solve_batch(probs + [_are(Eo, Ao, Bo, Co)], alg)
    assert e.value.code == -7


# ---- 3. independence --------------------------------------------------------------------------------------------------------------------
def test_a_member_does_not_see_the_others(ctx, small37):
    p, full = small37
    alg = D.MatrixSign(maxiters=25)
    pair = D.solve_batch([p[3], p[1]], alg)
    one = D.solve_batch([p[1]], alg)
    assert np.array_equal(full[1], pair[1]) and np.array_equal(full[1], one[0])
    assert np.array_equal(full[3], pair[0])


# ---- 4. a member with singular E --------------------------------------------------------------------------------------------------------
def test_a_singular_member_is_dropped_and_the_others_go_on(ctx, small37):
    p, full = small37
    Es = p[2].E.copy()
    Es[:, 5] = 0.0
    bad = D.GAREProblem(Es, p[2].A, p[2].G, p[2].Q)
    out = D.solve_batch([p[0], p[1], bad, p[3]], D.MatrixSign(maxiters=25), errors="return")
    print(f"singular member: {out[2]!r}")
    assert isinstance(out[2], D.DREError) and out[2].code == -4 and "member 2" in str(out[2])
    for b in (0, 1, 3):
        assert np.array_equal(out[b], full[b]), b
    X, info = D.solve(p[2], D.MatrixSign(maxiters=25), return_info=True)        # the context solves a further ordinary problem
    assert np.isfinite(X).all() and info["iters"] >= 1


# ---- 5. refinement subset ---------------------------------------------------------------------------------------------------------------
def test_refinement_of_a_subset(ctx, steel):
    E, A, B, Cm, Au = steel
    members = [_are(E, A, B, Cm), _are(E, Au, B, Cm)]
    out = D.solve_batch(members, D.MatrixSign(tol=1e-3), return_stats=True)
    bound = 100 * N * EPS
    for b in range(2):
        X, info = out[b]
        print(f"tol = 1e-3 member {b}: iters {info['iters']}, refinements {info['refinements']}, res0 {info['res0']:.3e}, res {info['res']:.3e} "
              f"(bound {bound:.3e})")
    for b in range(2):
        X, info = out[b]
        if info["refinements"] >= 1:
            assert info["res"] < info["res0"]
        assert info["res"] <= bound
    assert out[1][1]["refinements"] >= 1            # the unstable member stops at about 2e-9: test_newton_kleinman_refinement


# ---- 6. limits --------------------------------------------------------------------------------------------------------------------------
def _gare_abi(ctx, ups, batch, maxiters=50, max_refine=2):
    E, A, B, Ct = ups
    k = max(batch, 1)
    arrs = [(C.c_void_p * k)(*([u.ptr] * batch)) for u in (E, A, B)] + [None] + [(C.c_void_p * k)(*([Ct.ptr] * batch))] + [None]
    xs = (C.c_void_p * k)()
    st = np.zeros(k, dtype=np.int32)
    ii, dd = np.zeros(2 * k, dtype=np.int64), np.zeros(2 * k)
    rc = ctx.lib.dre_dense_gare_solve_batched(ctx.ptr, batch, *arrs, maxiters, 0.0, max_refine, xs, ii.ctypes.data_as(C.POINTER(C.c_int64)),
                                              dd.ctypes.data_as(C.POINTER(C.c_double)), st.ctypes.data_as(C.POINTER(C.c_int32)))
    got = [D.device.DenseMatrix(ctx, C.c_void_p(x)) for x in xs if x]          # (owning wrappers: the results are freed with them)
    return rc, len(got)


def test_limits(ctx, steel):
    n = 12
    rng = np.random.default_rng(5)
    mats = (np.eye(n), -np.eye(n) + 0.1 * rng.standard_normal((n, n)), rng.standard_normal((n, 2)), rng.standard_normal((n, 3)))
    ups = [ctx.upload(np.asfortranarray(M)) for M in mats]
    assert _gare_abi(ctx, ups, 2) == (0, 2)
    assert _gare_abi(ctx, ups, 0)[0] == -1
    assert _gare_abi(ctx, ups, 2, maxiters=0)[0] == -1
    assert _gare_abi(ctx, ups, 2, maxiters=1001)[0] == -1
    assert _gare_abi(ctx, ups, 2, max_refine=-1)[0] == -1
    # 2n = 4098 is beyond the register panel: refused before any allocation
    nb = 2049
    big = [ctx.upload(np.asfortranarray(M)) for M in (np.eye(nb), -np.eye(nb), np.ones((nb, 1)), np.ones((nb, 1)))]
    ctx.sync()
    before = ctx.info()["pool_bytes"]
    assert _gare_abi(ctx, big, 2)[0] == -1
    msg = ctx.lib.dre_last_error(ctx.ptr).decode()
    print(msg)
    assert "register panel" in msg and "4098" in msg
    assert ctx.info()["pool_bytes"] == before
    del big
    # a batch whose memory formula exceeds the device: refused up front, nothing allocated
    import torch
    total = torch.cuda.get_device_properties(0).total_memory
    E, A, B, Cm, Au = steel
    ups371 = [ctx.upload(np.asfortranarray(M)) for M in (E, A, B, np.ascontiguousarray(Cm.T))]
    ctx.sync()
    per_member = 24 * N * N * 8                          # the single path's own count alone
    batch = int(total // per_member) + 1
    assert batch <= 65535
    before = ctx.info()["pool_bytes"]
    assert _gare_abi(ctx, ups371, batch)[0] == -3
    assert ctx.info()["pool_bytes"] == before
    out = D.solve_batch([_are(E, A, B, Cm)], D.MatrixSign())
    assert len(out) == 1 and np.isfinite(out[0]).all()
