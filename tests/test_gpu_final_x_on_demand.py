"""The final X of a dense-X run is factored on demand (context option `final_x_lazy`).

A Ros1 run without save_state carries X as a dense symmetric matrix; K(t) is complete when the step loop ends and nothing K(t) depends on
needs the LDLᵀ form of the last X.  With `final_x_lazy=1` (default) the result keeps the dense matrix and `dre_gdre_result_X` converts it at
the first request; `final_x_lazy=0` converts inside the solve as before and is the reference of every test here.

All runs: SteelProfile(371), Ros1, Cyclic shifts of tests/golden/heuristic_shifts_371.npy, dt = -100, 6 time steps (the dense-X path is
reached at the first step), plus the 1-step run whose only dense step defers its group-base job to the parked thread.  The C ABI is driven
directly (as bench.py does): the tests need a result handle that outlives the next solve, which `solve_gdre` does not expose.

Tolerance of the X comparison.  Both modes run the same conversion code on the same dense matrix, so the factors are expected to agree to
the last bit; what is asserted is the bound that the number format gives for the comparison itself: X is rebuilt on the host as
alpha L D Lᵀ, two products with inner dimension r <= n, each entry with a relative error of at most ~ r eps against the product of the
norms of its factors (L has orthonormal columns, so that product is ||D||_F ~ ||X||_F).  Hence  ||X_1 - X_0||_F <= 2 n eps ||X_0||_F."""
import ctypes as C
import os

import numpy as np
import pytest

import dre_amd as D
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
N = 371
T0, DT = 4500.0, -100.0


class _Setup:
    """pencil, B, C, ADI options on the session context (built once), X0 per scale"""

    def __init__(self, ctx, rail):
        self.ctx, self.lib = ctx, ctx.lib
        self.d, self.L, self.Dm = rail
        self.pencil = D.Pencil(self.d.E, self.d.A, ctx)
        self.Bd, self.Cd = ctx.upload(self.d.B), ctx.upload(self.d.C)
        shifts = list(np.load(os.path.join(GOLDEN, "heuristic_shifts_371.npy")))
        self.opt, self._keep = D.device.make_adi_options(shift_kind=0, shifts=shifts, maxiters=100)
        self.m = self.d.B.shape[1]
        self._x0 = {}
        self._ref = {}

    def x0(self, scale):
        if scale not in self._x0:
            self._x0[scale] = D.DeviceLDLt.create(self.ctx, self.pencil, self.L, self.Dm * scale, 1.0)
        return self._x0[scale]

    def solve(self, nsteps, scale=1.0):
        r = C.c_void_p()
        self.ctx.chk(self.lib.dre_gdre_solve(self.ctx.ptr, self.pencil.ptr, self.Bd.ptr, self.Cd.ptr, self.x0(scale).ptr, T0, T0 + DT * nsteps, DT,
                                             1, 0, C.byref(self.opt), C.byref(r)))
        return r

    def info(self, r):
        ii = (C.c_int64 * 7)()
        self.lib.dre_gdre_result_info(r, ii)
        return list(ii)

    def K(self, r):
        nt = self.info(r)[0]
        Kall = np.zeros((nt, N, self.m))
        self.ctx.chk(self.lib.dre_gdre_result_K_all(self.ctx.ptr, r, Kall.ctypes.data_as(C.POINTER(C.c_double))))
        return Kall

    def iters(self, r):
        out = []
        for j in range(self.info(r)[4]):
            gi = (C.c_int64 * 4)(); gd = (C.c_double * 2)()
            assert self.lib.dre_gdre_result_gale(r, j, gi, gd) == 0
            out.append(int(gi[0]))
        return out

    def X(self, r):
        """the final X of the result: (rank, alpha, L, D)"""
        xp = C.c_void_p()
        self.ctx.chk(self.lib.dre_gdre_result_X(r, self.info(r)[1] - 1, C.byref(xp)))
        h = D.DeviceLDLt(self.ctx, xp, self.pencil)
        rank = h.info()[1]
        a, L, Dm = h.destructure()
        return rank, a, L, Dm

    def free(self, r):
        self.lib.dre_gdre_result_free(r)

    def eager(self, nsteps, scale=1.0, **opts):
        """K(t), iteration counts and final X of the run with final_x_lazy=0: computed once per configuration, never modified"""
        key = (nsteps, scale, tuple(sorted(opts.items())))
        if key not in self._ref:
            with self.ctx.options(final_x_lazy=0, **opts):
                r = self.solve(nsteps, scale)
                try:
                    K, its, info, X = self.K(r), self.iters(r), self.info(r), self.X(r)
                finally:
                    self.free(r)
            for a in (K, X[2], X[3]):
                a.setflags(write=False)
            self._ref[key] = dict(K=K, its=its, info=info, X=X)
        return self._ref[key]


@pytest.fixture(scope="module")
def S(ctx, rail371):
    return _Setup(ctx, rail371)


def _dense(X):
    _, a, L, Dm = X
    return a * (L @ Dm @ L.T)


def _same_x(X1, X0):
    assert X1[0] == X0[0], (X1[0], X0[0])                       # the same rank
    A1, A0 = _dense(X1), _dense(X0)
    diff, ref = np.linalg.norm(A1 - A0), np.linalg.norm(A0)
    bit = X1[2].shape == X0[2].shape and np.array_equal(X1[2], X0[2]) and np.array_equal(X1[3], X0[3]) and X1[1] == X0[1]
    print(f"final X: rank {X1[0]}, ||X_lazy - X_eager||_F / ||X_eager||_F = {diff / ref:.3e}, factors bit-identical: {bit}")
    assert diff <= 2 * N * EPS * ref, (diff, ref)


def _on_dense_path(ctx):
    """the option sets of tools/option_matrix.sh that switch the dense-X loop off leave nothing to defer"""
    return ctx.get_option("dense_x_max_n") >= N and ctx.get_option("dense_inverse_max_n") >= N and ctx.get_option("dense_x_max_k") == 0


def _launches(ctx):
    return sum(v["launches"] for v in ctx.prof_stats().values())


@pytest.mark.parametrize("nsteps", [6, 1])
def test_lazy_and_eager_give_the_same_k_counts_and_final_x(ctx, S, nsteps):
    ref = S.eager(nsteps)
    with ctx.options(final_x_lazy=1):
        r = S.solve(nsteps)
        try:
            assert S.info(r) == ref["info"]                      # dre_gdre_result_info: the same counts, X not yet requested
            K, its = S.K(r), S.iters(r)
            X = S.X(r)
        finally:
            S.free(r)
    assert len(its) == nsteps and its == ref["its"], (its, ref["its"])
    assert K.shape == (nsteps + 1, N, S.m) and np.array_equal(K, ref["K"])          # bit-identical K(t)
    _same_x(X, ref["X"])


def test_second_fetch_runs_no_kernel_and_returns_the_same_factors(ctx, S):
    ref = S.eager(6)
    with ctx.options(final_x_lazy=1):
        r = S.solve(6)
        try:
            ctx.sync()
            ctx.prof_reset(); ctx.prof_enable(True)
            try:
                xp1 = C.c_void_p()
                ctx.chk(S.lib.dre_gdre_result_X(r, 1, C.byref(xp1)))
                h1 = D.DeviceLDLt(ctx, xp1, S.pencil)
                first = _launches(ctx)
                ctx.prof_reset()
                xp2 = C.c_void_p()
                ctx.chk(S.lib.dre_gdre_result_X(r, 1, C.byref(xp2)))
                h2 = D.DeviceLDLt(ctx, xp2, S.pencil)
                second = _launches(ctx)
            finally:
                ctx.prof_enable(False); ctx.prof_reset()
            print(f"kernel launches of the first fetch {first}, of the second {second}")
            if _on_dense_path(ctx):
                assert first > 0                                  # the conversion ran at the first request, not inside the solve
            assert second == 0
            assert h1.info() == h2.info()
            X1 = (h1.info()[1],) + h1.destructure()
            X2 = (h2.info()[1],) + h2.destructure()
        finally:
            S.free(r)
    assert X1[1] == X2[1] and np.array_equal(X1[2], X2[2]) and np.array_equal(X1[3], X2[3])
    _same_x(X1, ref["X"])


def test_eager_mode_converts_inside_the_solve(ctx, S):
    """the reference mode really is the earlier behaviour: with final_x_lazy=0 the first fetch finds the factors ready"""
    with ctx.options(final_x_lazy=0):
        r = S.solve(6)
        try:
            ctx.sync()
            ctx.prof_reset(); ctx.prof_enable(True)
            try:
                xp = C.c_void_p()
                ctx.chk(S.lib.dre_gdre_result_X(r, 1, C.byref(xp)))
                h = D.DeviceLDLt(ctx, xp, S.pencil)
                n_first = _launches(ctx)
            finally:
                ctx.prof_enable(False); ctx.prof_reset()
            assert n_first == 0 and h.info()[0] == N
        finally:
            S.free(r)


@pytest.mark.parametrize("nsteps", [6, 1])
def test_kept_result_survives_a_second_solve_on_the_same_context(ctx, S, nsteps):
    """the dense buffer belongs to the result: a later solve (other X0, same sizes: the pool would hand the block out again) cannot recycle it"""
    ref1, ref2 = S.eager(nsteps), S.eager(nsteps, scale=3.0)
    with ctx.options(final_x_lazy=1):
        r1 = S.solve(nsteps)
        try:
            r2 = S.solve(nsteps, scale=3.0)
            try:
                K2, its2, X2 = S.K(r2), S.iters(r2), S.X(r2)
            finally:
                S.free(r2)
            K1, its1, X1 = S.K(r1), S.iters(r1), S.X(r1)          # only now: after the second solve ran and its result is gone
        finally:
            S.free(r1)
    assert not np.array_equal(ref1["K"][-1], ref2["K"][-1])       # (the two runs do differ)
    assert np.array_equal(K1, ref1["K"]) and its1 == ref1["its"]
    assert np.array_equal(K2, ref2["K"]) and its2 == ref2["its"]
    _same_x(X1, ref1["X"])
    _same_x(X2, ref2["X"])


@pytest.mark.parametrize("nsteps", [6, 1])
def test_result_freed_without_x_then_next_solve_matches(ctx, S, nsteps):
    ref = S.eager(nsteps)
    with ctx.options(final_x_lazy=1):
        r = S.solve(nsteps)
        K_a = S.K(r)
        S.free(r)                                                 # X never requested: only the dense buffer goes back
        r = S.solve(nsteps)
        try:
            K_b, its, X = S.K(r), S.iters(r), S.X(r)
        finally:
            S.free(r)
    assert np.array_equal(K_a, ref["K"]) and np.array_equal(K_b, ref["K"]) and its == ref["its"]
    _same_x(X, ref["X"])


def test_run_forced_off_the_dense_path_still_returns_its_final_x(ctx, S):
    """dense_x_max_k below the residual width: the second step refuses, the loop converts X there (eagerly, the next step needs the factors)
    and ends on the factored path; final_x_lazy=1 has nothing to defer and must hand out the same X"""
    ref = S.eager(6, dense_x_max_k=16)
    with ctx.options(final_x_lazy=1, dense_x_max_k=16):
        r = S.solve(6)
        try:
            assert S.info(r) == ref["info"]
            K, its, X = S.K(r), S.iters(r), S.X(r)
        finally:
            S.free(r)
    assert np.array_equal(K, ref["K"]) and its == ref["its"]
    _same_x(X, ref["X"])


def test_option_is_readable_and_defaults_to_on(ctx):
    assert ctx.get_option("final_x_lazy") in (0.0, 1.0)
    if "final_x_lazy" not in os.environ.get("DRE_OPTIONS", ""):
        assert ctx.get_option("final_x_lazy") == 1.0
    with ctx.options(final_x_lazy=0):
        assert ctx.get_option("final_x_lazy") == 0.0
