"""Batched dense path on the device (csrc/dense_batch.hip): an ensemble of same-size problems in shared launches through
`dense_invert_batch` and `solve_batch`, against the single-problem path, the dense oracle and the committed dense-oracle fixtures.

The bounds are those of tests/test_gpu_dense_large.py (inversion) and tests/test_gpu_dense_sign.py (GALE, Ros1 / Ros2); every figure is
printed before it is asserted."""
import ctypes as C
import os

import numpy as np
import pytest

import dre_amd as D
import dre_oracle as o
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
MS = D.MatrixSign()
N = 371
TOL_K = 100 * N * EPS            # test/rail.jl:56
TAUS = (100.0, 50.0, 25.0, 10.0)


@pytest.fixture(scope="module")
def rail():
    d = D.steel_profile(N)
    L, Dm = D.initial_value(d)
    return d, d.E.toarray(), d.A.toarray(), D.lowrank(L, Dm).dense()


def _check_inverse(A, X, ld):
    n = A.shape[0]
    r = np.linalg.norm(A @ X - np.eye(n)) / (np.linalg.norm(A) * np.linalg.norm(X))
    s, ldn = np.linalg.slogdet(A)
    print(f"inverse: residual {r:.3e} (bound {100 * n * EPS:.3e}), logdet {ld!r} vs {ldn!r}")
    assert r <= 100 * n * EPS, r
    assert s != 0 and abs(ld - ldn) <= 1e-12 * abs(ldn)


def _rel2(a, b):
    return np.linalg.norm(a - b, 2) / np.linalg.norm(b, 2)


# ---- 1. batched inversion ------------------------------------------------------------------------------------------------------------
def test_batched_inversion(ctx, rail):
    d, E, A, X0 = rail
    Z = A.copy(); Z[:, 17] = 0.0
    regular = [E, A, A - E / (2 * 100.0), A - E / (2 * 10.0)]
    with pytest.raises(D.DREError) as e:
        D.dense_invert_batch(regular + [Z])
    assert e.value.code == -4 and "member 4" in str(e.value)
    # per-member status through the ABI: the four regular members are inverted, the fifth reports DRE_ERR_SINGULAR
    ups = [ctx.upload(np.asfortranarray(M)) for M in regular + [Z]]
    piv, ld, st = np.zeros((5, N), dtype=np.int32), np.zeros(5), np.zeros(5, dtype=np.int32)
    arr = (C.c_void_p * 5)(*[u.ptr for u in ups])
    ctx.chk(ctx.lib.dre_dense_invert_batched(ctx.ptr, 5, arr, piv.ctypes.data_as(C.POINTER(C.c_int32)), ld.ctypes.data_as(C.POINTER(C.c_double)),
                                             st.ctypes.data_as(C.POINTER(C.c_int32))))
    assert list(st) == [0, 0, 0, 0, -4]
    for b, M in enumerate(regular):
        X = ups[b].numpy()
        _check_inverse(M, X, float(ld[b]))
        Xs, ps, lds = D.dense_invert(M)
        assert np.array_equal(piv[b], ps), b
    assert np.array_equal(ups[4].numpy(), Z)              # a singular member is left as it came
    out = D.dense_invert_batch(regular)
    for b, (X, p, l) in enumerate(out):
        assert np.array_equal(p, piv[b]) and l == ld[b] and np.array_equal(X, ups[b].numpy())


# ---- 2. batched GALE -------------------------------------------------------------------------------------------------------------------
def _gale_members(E, A):
    rng = np.random.default_rng(11)
    probs = []
    for tau in TAUS:
        G = rng.standard_normal((N, 5))
        probs.append(D.GALEProblem(E, A - E / (2 * tau), G @ G.T))
    return probs


def test_batched_gale(ctx, rail):
    d, E, A, X0 = rail
    probs = _gale_members(E, A)
    bad = D.GALEProblem(E, -A, probs[0].C)
    out = D.solve_batch(probs + [bad], MS, errors="return", return_stats=True)
    assert len(out) == 5
    for b, p in enumerate(probs):
        X, info = out[b]
        dl = D.delta(X, o.lyap_dense(p.A, p.E, p.C))
        print(f"gale member {b}: delta {dl:.3e}, res {info['res']:.3e} (bound {100 * N * EPS:.3e}), iters {info['iters']}, refinements {info['refinements']}")
        assert dl < 1e-10
        assert info["res"] <= 100 * N * EPS
    assert isinstance(out[4], D.DREError) and out[4].code == -7
    with pytest.raises(D.DREError) as e:
        D.solve_batch(probs + [bad], MS)
    assert e.value.code == -7 and "member 4" in str(e.value)


# ---- 3. batched Ros1 / Ros2 ------------------------------------------------------------------------------------------------------------
def _gdre_members(rail, tspan):
    d, E, A, X0 = rail
    return [D.GDREProblem(E, A, s * d.B, d.C, X0, tspan) for s in (1.0, 0.5, 2.0, 3.0)]


@pytest.mark.parametrize("name,Ros,order", [("ros1_371_full", D.Ros1, 1), ("ros2_371_full", D.Ros2, 2)])
def test_batched_rosenbrock_five_steps(ctx, rail, name, Ros, order):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    probs = _gdre_members(rail, (4500.0, 4000.0))
    out = D.solve_batch(probs, Ros(MS), dt=-100.0, return_stats=True)
    sol0, st0 = out[0]
    assert len(sol0.K) == 6 and np.allclose(sol0.t, g["t"][:6])
    for i in range(6):
        dl = D.delta(sol0.K[i], g["K_dense"][i])
        print(f"{name} member 0 step {i}: delta to the fixture {dl:.3e}")
        assert dl < 1e-10, i
    for b, p in enumerate(probs):
        sol, st = out[b]
        ref, rst = D.solve(p, Ros(MS), dt=-100.0, return_stats=True)
        r = _rel2(sol.K[-1], ref.K[-1])
        print(f"{name} member {b}: ||K - K_single||_2 / ||K_single||_2 = {r:.3e} (bound {TOL_K:.3e})")
        assert len(sol.K) == 6 and len(sol.X) == 2 and sol.X[0] is p.X0
        assert r <= TOL_K
        assert st["lyapunov_solves"] == 5 * order == rst["lyapunov_solves"]
        it = np.array([s["iters"] for s in st["solves"]]); rit = np.array([s["iters"] for s in rst["solves"]])
        res = max(s["res"] for s in st["solves"])
        print(f"    iters {it.tolist()} single {rit.tolist()}, max res {res:.3e}")
        assert np.abs(it - rit).max() <= 1
        assert res <= 100 * N * EPS


# ---- 4. independence --------------------------------------------------------------------------------------------------------------------
def test_a_member_does_not_see_the_others(ctx, rail):
    p = _gdre_members(rail, (4500.0, 4300.0))
    alg = D.Ros1(MS)
    full = D.solve_batch(p, alg, dt=-100.0)
    pair = D.solve_batch([p[3], p[1]], alg, dt=-100.0)
    one = D.solve_batch([p[1]], alg, dt=-100.0)
    for a, b in ((full[1], pair[1]), (full[1], one[0]), (full[3], pair[0])):
        assert len(a.K) == len(b.K) == 3
        for Ka, Kb in zip(a.K, b.K):
            assert np.array_equal(Ka, Kb)
        assert np.array_equal(a.X[-1], b.X[-1])
    d, E, A, X0 = rail
    gp = _gale_members(E, A)
    gfull = D.solve_batch(gp, MS)
    gpair = D.solve_batch([gp[3], gp[1]], MS)
    gone = D.solve_batch([gp[1]], MS)
    assert np.array_equal(gfull[1], gpair[1]) and np.array_equal(gfull[1], gone[0]) and np.array_equal(gfull[3], gpair[0])


# ---- 5. a member failing in the middle of the ensemble ---------------------------------------------------------------------------------
def test_a_failing_member_is_dropped_and_the_others_go_on(ctx, rail):
    d, E, A, X0 = rail
    p = _gdre_members(rail, (4500.0, 4200.0))
    bad = D.GDREProblem(E, -A, d.B, d.C, X0, (4500.0, 4200.0))
    alg = D.Ros1(MS)
    out = D.solve_batch([p[0], bad, p[2]], alg, dt=-100.0, errors="return", save_state=True)
    assert isinstance(out[1], D.DREError) and out[1].code == -7 and "member 1" in str(out[1])
    part = out[1].partial
    assert len(part.t) == len(part.K) == 1 and len(part.X) == 1          # it failed in the first step: K(t_0) is what it produced
    for b, q in ((0, p[0]), (2, p[2])):
        ref = D.solve(q, alg, dt=-100.0, save_state=True)
        assert len(out[b].K) == 4 and len(out[b].X) == 4
        for i in range(4):
            r = _rel2(out[b].K[i], ref.K[i])
            print(f"member {b} step {i}: ||K - K_single|| / ||K_single|| = {r:.3e} (bound {TOL_K:.3e})")
            assert r <= TOL_K
    with pytest.raises(D.DREError) as e:
        D.solve_batch([p[0], bad, p[2]], alg, dt=-100.0)
    assert e.value.code == -7
    sol = D.solve(p[1], alg, dt=-100.0)                                   # the context solves a further ordinary problem
    assert len(sol.K) == 4 and np.isfinite(sol.K[-1]).all()


# ---- 6. limits ------------------------------------------------------------------------------------------------------------------------------
def _gdre_abi(ctx, ups, batch, order, maxiters=50):
    arrs = [(C.c_void_p * max(batch, 1))(*([u.ptr] * batch)) for u in ups]
    rs = (C.c_void_p * max(batch, 1))()
    st = np.zeros(max(batch, 1), dtype=np.int32)
    rc = ctx.lib.dre_dense_gdre_solve_batched(ctx.ptr, batch, *arrs, 1.0, 0.0, -0.5, order, 0, maxiters, 0.0, 2, rs, st.ctypes.data_as(C.POINTER(C.c_int32)))
    for r in rs:
        if r:
            ctx.lib.dre_gdre_result_free(C.c_void_p(r))
    return rc


def test_limits(ctx, rail):
    with pytest.raises(D.DREError) as e:
        D.dense_invert_batch([np.eye(4097)])
    assert e.value.code == -1
    n, m, q = 12, 2, 3
    rng = np.random.default_rng(5)
    mats = (np.eye(n), -np.eye(n) + 0.1 * rng.standard_normal((n, n)), rng.standard_normal((n, m)), rng.standard_normal((q, n)), np.zeros((n, n)))
    ups = [ctx.upload(np.asfortranarray(M)) for M in mats]
    assert _gdre_abi(ctx, ups, 2, 1) == 0
    assert _gdre_abi(ctx, ups, 2, 3) == -1
    msg = ctx.lib.dre_last_error(ctx.ptr).decode()
    assert "Ros1 and Ros2" in msg, msg
    assert _gdre_abi(ctx, ups, 2, 4) == -1
    assert _gdre_abi(ctx, ups, 0, 1) == -1
    # a batch whose memory formula exceeds the device: refused up front, nothing allocated
    import torch
    total = torch.cuda.get_device_properties(0).total_memory
    d, E, A, X0 = rail
    big = [ctx.upload(np.asfortranarray(M)) for M in (E, A, d.B, d.C, X0)]
    ctx.sync()
    per_member = (50 + 10) * N * N * 8                   # the sign solver's own stacks alone
    batch = int(total // per_member) + 1
    assert batch <= 65535
    before = ctx.info()["pool_bytes"]
    assert _gdre_abi(ctx, big, batch, 1) == -3
    assert ctx.info()["pool_bytes"] == before
    out = D.solve_batch(_gdre_members(rail, (4500.0, 4400.0))[:2], D.Ros1(MS), dt=-100.0)
    assert len(out) == 2 and len(out[0].K) == 2
