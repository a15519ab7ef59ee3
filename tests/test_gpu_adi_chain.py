"""The dense-inverse ADI chain (csrc/dense.hip: adi_fast_build, adi_fast_pack_r, adi_fast_iter, adi_group_pack, adi_group_iter) on its own, through
dre_adi_chain_probe, at the smallest shapes at which each piece can go wrong.

Every comparison is ONE-STEP consistent: iteration j is held against the model (tests/_adi_chain_model.py) applied to the DEVICE's own effective stack
and the DEVICE's own R_(j-1), so the bounds do not compound.  The bounds are derived, not measured — a product over K = n terms on the matrix cores is a
chain of n / 4 fused multiply-adds per K-quarter plus a fixed-order sum of the four quarters, i.e. at most (n / 4 + 3) roundings per entry against the
componentwise product of the absolute values; the tests allow 2 (n + 8) eps of it (eps = 2^-52), twice that where the reference itself is float64:
    |V - V_ref|      <= 2 (n + 8) eps |Seff_top| |R|
    |R+ - R+_ref|    <= 2 (n + 8) eps (|R| + 2 |mu| |Seff_bot| |R|)
    |G - G_ref|      <= 2 (n + 8) eps |R|'|R|
    |nrm^2 - ref^2|  <= 2 (n + 2 k + 8) eps alpha^2 sum_ij (|T| |R|'|R|)_ij (|R|'|R| |T|)_ij
    build            <= 2 (m + 8) eps (|[N; E'N]| + |WKS| |U'N|)          (m multiply-adds and one subtraction per entry)
    group            <= 2 (n + 8) eps |Om_i| |R_in|  and  |Pi_i| |R_in|   (one product of the group's input residual per output)
Padding of the packed arrays is exactly 0.0; guard rows, the spare column block and everything behind the last launched iteration are still NaN."""
import hashlib

import numpy as np
import pytest

import dre_amd as D
import _adi_chain_model as M
import _adi_chain_probe as P

pytestmark = pytest.mark.gpu
EPS = M.EPS


# ---- operands ---------------------------------------------------------------------------------------------------------------------------
_pencils, _stacks, _memo = {}, {}, {}


def _pencil(n):
    if n not in _pencils:
        rng = np.random.default_rng(1000 + n)
        _pencils[n] = (np.eye(n) + 0.1 * rng.standard_normal((n, n)) / np.sqrt(n) * 3.0, -(2.0 * np.eye(n) + 0.1 * rng.standard_normal((n, n)) / np.sqrt(n) * 3.0))
    return _pencils[n]


def _stack(n, mu, m):
    """([N; E'N; U'N], WKS or None) of the stable dense pencil E = I + 0.1 G1, A = -(2 I + 0.1 G2) (G scaled by 3 / sqrt(n): a spectral radius of about 0.3 at every order, so the
    pencil stays stable and the residual norms contract) with a rank-m update, N = inv(A' + mu E')"""
    key = (n, mu, m)
    if key not in _stacks:
        E, A = _pencil(n)
        N = np.linalg.inv(A.T + mu * E.T)
        top = np.vstack([N, E.T @ N])
        if m == 0:
            _stacks[key] = (top, None)
        else:
            rng = np.random.default_rng(7 * n + m)
            U, Vt = 0.3 * rng.standard_normal((n, m)), 0.3 * rng.standard_normal((m, n))
            S = np.eye(m) + U.T @ N @ Vt.T
            _stacks[key] = (np.vstack([top, U.T @ N]), top @ Vt.T @ np.linalg.inv(S))
    return _stacks[key]


def _shifts(count):
    return [float(v) for v in np.linspace(-3.0, -0.3, count)] if count > 1 else [-1.1]


def _R0(n, k, seed=0):
    return np.random.default_rng(31 * n + k + seed).standard_normal((n, k))


def _T(k, diag):
    rng = np.random.default_rng(5 * k + diag)
    if diag:
        return np.diag(rng.standard_normal(k) + np.where(np.arange(k) % 2, 1.5, -1.5))          # indefinite
    T = rng.standard_normal((k, k))
    return (T + T.T) / 2.0 - 0.2 * np.eye(k)                                                       # dense, symmetric, indefinite


def _h(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.digest()


def _step(S, skey, R, mu):
    key = ("s", skey, mu, _h(R))
    if key not in _memo:
        if len(_memo) > 400:
            _memo.clear()
        _memo[key] = M.step(S, R, mu)
    return _memo[key]


def _norm2(R, T, alpha):
    key = ("n", _h(R, T), alpha)
    if key not in _memo:
        _memo[key] = M.norm2(R, T, alpha)
    return _memo[key]


def _within(got, ref, bound, what):
    err = np.abs(got - ref)
    bad = ~(err <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} entries outside the bound, worst ratio {float(np.max(err[bad] / np.maximum(bound[bad], 1e-300))):.3g}"


def _all_nan(a):
    return bool(np.all(np.isnan(a)))


def _device_seff(out, nstack, n):
    """the effective stacks as the device packed them, with the padding checked to be exactly zero"""
    res = []
    for s in range(nstack):
        S, pad = M.unpack_a(out.packs[s], n, 2)
        assert np.all(pad == 0.0), "padding of the packed stack"
        assert not np.isnan(S).any()
        res.append(S)
    return res


# ---- the fast chain ---------------------------------------------------------------------------------------------------------------------
def run_fast(ctx, n, k, *, m=2, nshift=2, nit=3, mode=-1, nt=-1, tdiag=0, alpha=1.0, abstol=0.0, maxiters=1 << 20, base_it=0, ld=None, T=None, R0=None):
    mus = _shifts(nshift)
    st = [_stack(n, mu, m) for mu in mus]
    R0 = _R0(n, k) if R0 is None else R0
    T = _T(k, tdiag) if T is None else T
    out = P.probe(ctx, P.FAST, n, k, [s[0] for s in st], m=m, wks=[s[1] for s in st] if m else None, mu=mus, R0=R0, T=T, nit=nit, mode=mode, nt=nt,
                  tdiag=tdiag, alpha=alpha, abstol=abstol, maxiters=maxiters, base_it=base_it, ld=ld)
    out.mus, out.R0, out.T, out.alpha, out.n, out.k, out.nit, out.base_it, out.m = mus, R0, T, alpha, n, k, nit, base_it, m
    out.abstol_in, out.maxiters = abstol, maxiters
    return out


def check_fast(out, steps=True):
    """everything one run of the fast chain must satisfy; returns the model's norms of the device's residuals"""
    n, k, nit, base_it, mus = out.n, out.k, out.nit, out.base_it, out.mus
    S = _device_seff(out, len(mus), n)
    skeys = [_h(s) for s in S]
    # the norms of the device's own residuals, and what the decision rule makes of them
    nr = [_norm2(out.R[j - 1][:n], out.T, out.alpha) if not np.isnan(out.R[j - 1][:n]).any() else None for j in range(1, nit + 1)]
    norms_ref = []
    for v in nr:
        if v is None:
            break
        norms_ref.append(float(np.sqrt(max(v[0], 0.0))))
    iters, done, acc = M.decide(norms_ref, base_it, out.abstol_in, out.maxiters)
    assert (out.iters, out.done) == (iters, done), f"iters/done {out.iters}/{out.done}, model {iters}/{done}; norms {norms_ref[:acc + 2]}"
    # a decision arrives two launches late: iterations up to acc + 2 ran, nothing behind them
    launched = nit if not done else min(nit, acc + 2)
    assert len(norms_ref) >= launched
    for buf, name in ((out.V, "V"), (out.R, "R")):
        assert _all_nan(buf[:, n:, :]), f"{name}: guard rows written"
        assert _all_nan(buf[launched:]), f"{name}: written behind the last launched iteration or in the spare block"
        assert not np.isnan(buf[:launched, :n, :]).any(), f"{name}: NaN inside the launched region"
    # packed residuals: bit for bit the packed column-major ones, padding exactly zero (mode 0); untouched in mode 1
    if out.mode == 0:
        assert np.array_equal(out.Rp[0], M.pack_r(out.R0)), "packed R0"
        for j in range(1, launched + 1):
            assert np.array_equal(out.Rp[j], M.pack_r(out.R[j - 1][:n])), f"packed residual of iteration {j}"
        assert _all_nan(out.Rp[launched + 1:])
    else:
        assert _all_nan(out.Rp)
    # iterations against the model, one step at a time
    if steps:
        for j in range(1, launched + 1):
            pos = (j - 1) % len(mus)
            Rprev = out.R0 if j == 1 else out.R[j - 2][:n]
            s = _step(S[pos], skeys[pos], Rprev, mus[pos])
            _within(out.V[j - 1][:n], s["V"], M.bound_step(n, s["aV"], s["f"]), f"V of iteration {j}")
            _within(out.R[j - 1][:n], s["Rn"], M.bound_step(n, s["aR"], s["f"]), f"R of iteration {j}")
    # norms: ring entries of the accepted iterations, nothing else
    ring = np.full(M.RING, np.nan)
    for j in range(1, acc + 1):
        ref2, op, f = nr[j - 1]
        got = out.norms[(base_it + j) & 511]
        assert abs(got * got - ref2) <= M.bound_norm2(n, k, op, f), f"norm of iteration {j}: {got!r} against {np.sqrt(max(ref2, 0.0))!r}"
        ring[(base_it + j) & 511] = got
    assert np.array_equal(ring, out.norms, equal_nan=True), "ring entries outside the accepted iterations"
    assert out.abstol == out.abstol_in
    assert out.res_norm == out.norms[(base_it + acc) & 511]
    # the Gram matrices still held after a chain that ran to its end
    if not done:
        for j in ([nit - 1, nit] if nit >= 2 else [nit]):
            G, aG, f = M.gram(out.R[j - 1][:n])
            _within(out.G[(base_it + j) & 1], G, M.bound_step(n, aG, f), f"Gram matrix of iteration {j}")
    return norms_ref


COMBOS = ((0, 1.0), (0, -0.37), (1, 1.0), (1, -0.37))          # (tdiag, alpha)


def _sweep(ctx, n, ks, mode, nts, combos=COMBOS, nit=3):
    for k in ks:
        first = None
        for nt in nts:
            for ci, (tdiag, alpha) in enumerate(combos):
                out = run_fast(ctx, n, k, mode=mode, nt=nt, tdiag=tdiag, alpha=alpha, nit=nit)
                assert (out.mode, out.nt) == (mode, nt)
                # T and alpha only enter the norm: the iterates of the other combinations must be the same bits, the model steps are then shared
                check_fast(out, steps=ci == 0)
                if ci == 0:
                    first = out
                else:
                    assert np.array_equal(out.V, first.V, equal_nan=True) and np.array_equal(out.R, first.R, equal_nan=True)


@pytest.mark.parametrize("n", [1, 3, 12, 16, 29, 30, 31, 32, 100, 400])
def test_fast_mode0_every_tile_width(ctx, n):
    """K-split tile workgroups: waves with an empty K range (n <= 12), n mod 16 in {0, 13, 14, 15} with an odd tile count at nt = 2 and a single tile at
    nt = 4 (the tile index that had no clamp), k not a multiple of 16, and at n = 400 a per-wave K range of 25 = 2 KB + 1 for the double-buffered batches"""
    _sweep(ctx, n, (1, 15, 16, 17, 48, 97), 0, (1, 2, 4))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 70])
def test_fast_mode1_every_tile_width(ctx, n):
    """LDS-staged strips: one K-chunk of 64 and its edges, every compiled tile width (only nt = 2 is picked today)"""
    _sweep(ctx, n, (1, 17, 128, 144), 1, (1, 2, 4), combos=COMBOS[:2])
    _sweep(ctx, n, (17,), 1, (2,), combos=COMBOS[2:])


@pytest.mark.parametrize("n,k,want", [(371, 35, (0, 1)), (371, 144, (0, 2)), (1357, 48, (0, 2)), (784, 128, (1, 2)), (752, 352, (0, 4))])
def test_pick_table(ctx, n, k, want):
    """adi_fast_pick left alone: the variant each production shape takes (the coverage claims of this file rest on them), checked like every other run"""
    out = run_fast(ctx, n, k, m=1, nshift=1, nit=2)
    assert (out.mode, out.nt) == want
    check_fast(out)


def test_limits(ctx):
    out = run_fast(ctx, 40, 512, nit=3)
    check_fast(out)
    with pytest.raises(D.DREError) as e:
        run_fast(ctx, 40, 513, nit=1)
    assert e.value.code == P.ERR_INVALID and "too wide" in str(e.value)
    check_fast(run_fast(ctx, 40, 5, nit=1))          # the context stays usable


@pytest.mark.parametrize("mode", [0, 1])
def test_pipeline_and_decisions(ctx, mode):
    n, k = 61, 17
    kw = dict(mode=mode, nt=2)
    for nit in (1, 2, 3, 9):
        out = run_fast(ctx, n, k, nit=nit, **kw)
        check_fast(out)
        assert (out.iters, out.done) == (nit, 0)          # the last two norms come from the flush launches
        assert not np.isnan(out.norms[1:nit + 1]).any()
    norms = check_fast(run_fast(ctx, n, k, nit=9, **kw))
    assert all(b < a for a, b in zip(norms, norms[1:])), "the residual norms of the test pencil must contract for the thresholds below to mean anything"
    for jstar in (4, 5):          # in the middle of the chunk
        tol = float(np.sqrt(norms[jstar - 2] * norms[jstar - 1]))          # between the norms after iterations jstar - 1 and jstar
        out = run_fast(ctx, n, k, nit=9, abstol=tol, **kw)
        check_fast(out)
        assert (out.iters, out.done) == (jstar, 1) and out.res_norm == out.norms[jstar]
        again = run_fast(ctx, n, k, nit=9, abstol=tol, **kw)          # after a run that ended early: the ticket word and the control block start afresh
        for name in ("V", "R", "Rp", "G", "norms"):
            assert np.array_equal(getattr(out, name), getattr(again, name), equal_nan=True), name
        assert (again.iters, again.done, again.res_norm) == (out.iters, out.done, out.res_norm)
    out = run_fast(ctx, n, k, nit=9, abstol=0.0, maxiters=5, **kw)
    check_fast(out)
    assert (out.iters, out.done) == (5, 1)
    out = run_fast(ctx, n, k, nit=12, base_it=505, **kw)          # the ring wraps at 512
    check_fast(out)
    assert (out.iters, out.done) == (517, 0)
    assert not np.isnan(out.norms[[506 & 511, 511, 0, 517 & 511]]).any() and _all_nan(out.norms[6:506])
    # a leading dimension above n + 2 changes nothing but the stride
    wide = run_fast(ctx, n, k, nit=3, ld=n + 11, **kw)
    check_fast(wide)
    assert np.array_equal(wide.R[:, :n], run_fast(ctx, n, k, nit=3, **kw).R[:, :n], equal_nan=True)


# ---- the build --------------------------------------------------------------------------------------------------------------------------
def _check_build(ctx, n, m, nshift, wks_null=None):
    mus = _shifts(nshift)
    st = [_stack(n, mu, m) for mu in mus]
    out = P.probe(ctx, P.BUILD, n, 0, [s[0] for s in st], m=m, wks=[s[1] for s in st] if m else None, wks_null=wks_null)
    for i, (stack, wks) in enumerate(st):
        S, pad = M.unpack_a(out.packs[i], n, 2)
        assert np.all(pad == 0.0), "padding of the packed stack"
        plain = m == 0 or (wks_null is not None and wks_null[i])
        ref, op = M.seff(stack, None if plain else wks, n)
        if plain:
            assert np.array_equal(S, stack[:2 * n]), f"shift {i}: a stack without correction is copied"
        else:
            _within(S, ref, 2.0 * (m + 8) * EPS * op, f"effective stack of shift {i}")
            assert not np.array_equal(S, stack[:2 * n])


@pytest.mark.parametrize("n", [1, 5, 16, 17, 61])
def test_build(ctx, n):
    """m = 1 .. 8 with every WKS present: matrix cores; m = 9, m = 0 or a missing WKS: scalar kernel; 17 shifts: two batches of at most 16"""
    for m in (0, 1, 3, 8, 9):
        _check_build(ctx, n, m, 2)
    _check_build(ctx, n, 3, 3, wks_null=[0, 1, 0])
    _check_build(ctx, n, 3, 17)
    _check_build(ctx, n, 9, 17)


# ---- the group chain --------------------------------------------------------------------------------------------------------------------
_gops = {}


def _group_ops(n, g, ncyc):
    """one group stack per start position of a cycle of ncyc shifts, from the model's effective stacks (no low-rank part)"""
    key = (n, g, ncyc)
    if key not in _gops:
        mus = _shifts(ncyc)
        Ss = [M.seff(*_stack(n, mu, 0), n)[0] for mu in mus]
        _gops[key] = (mus, Ss, [M.group_ops(Ss[p:p + g], mus[p:p + g]) for p in range(0, ncyc, g)])
    return _gops[key]


def run_group(ctx, n, k, g, NG, *, two_starts=False, abstol=0.0, maxiters=1 << 20, alpha=1.0):
    ncyc = 2 * g if two_starts else g
    mus, Ss, ops = _group_ops(n, g, ncyc)
    R0, T = _R0(n, k, 3), _T(k, 0)
    out = P.probe(ctx, P.GROUP, n, k, ops, g=g, mu=mus, R0=R0, T=T, nit=g * NG, alpha=alpha, abstol=abstol, maxiters=maxiters)
    out.n, out.k, out.g, out.NG, out.ops, out.mus, out.Ss, out.R0, out.T, out.alpha, out.abstol_in, out.maxiters = n, k, g, NG, ops, mus, Ss, R0, T, alpha, abstol, maxiters
    return out


def check_group(out):
    n, k, g, NG = out.n, out.k, out.g, out.NG
    nit = g * NG
    for s, op in enumerate(out.ops):          # the packed group stacks: the operands bit for bit, zero padding
        back, pad = M.unpack_a(out.packs[s], n, 2 * g)
        assert np.array_equal(back, op) and np.all(pad == 0.0)
    norms_ref, nr = [], []
    for j in range(1, nit + 1):
        Rj = out.R[j - 1][:n]
        if np.isnan(Rj).any():
            break
        nr.append(_norm2(Rj, out.T, out.alpha))
        norms_ref.append(float(np.sqrt(max(nr[-1][0], 0.0))))
    iters, done, acc = M.decide(norms_ref, 0, out.abstol_in, out.maxiters)
    assert (out.iters, out.done) == (iters, done), f"iters/done {out.iters}/{out.done}, model {iters}/{done}"
    # the decisions for the residuals of launch L are taken by launch L + 2, whose own strips still run
    groups = NG if not done else min(NG, (acc - 1) // g + 3)
    launched = groups * g
    assert len(norms_ref) >= launched
    for buf, name in ((out.V, "V"), (out.R, "R")):
        assert _all_nan(buf[:, n:, :]) and _all_nan(buf[launched:]), f"{name}: written outside its region"
        assert not np.isnan(buf[:launched, :n, :]).any()
    assert np.array_equal(out.Rp[0], M.pack_r(out.R0))
    for j in range(1, launched + 1):
        assert np.array_equal(out.Rp[j], M.pack_r(out.R[j - 1][:n])), f"packed residual of iteration {j}"
    assert _all_nan(out.Rp[launched + 1:])
    for L in range(groups):
        Rin = out.R0 if L == 0 else out.R[L * g - 1][:n]
        op = out.ops[((L * g) % len(out.mus)) // g]
        ref, exact = M._mm(op, Rin)
        ref = np.asarray(ref, dtype=np.float64)
        bound = M.bound_step(n, np.abs(op) @ np.abs(Rin), 1.0 if exact else 2.0)
        for i in range(g):
            _within(out.V[L * g + i][:n], ref[i * n:(i + 1) * n], bound[i * n:(i + 1) * n], f"V of iteration {L * g + i + 1}")
            _within(out.R[L * g + i][:n], ref[(g + i) * n:(g + i + 1) * n], bound[(g + i) * n:(g + i + 1) * n], f"R of iteration {L * g + i + 1}")
    ring = np.full(M.RING, np.nan)
    for j in range(1, acc + 1):
        ref2, opn, f = nr[j - 1]
        got = out.norms[j]
        assert abs(got * got - ref2) <= M.bound_norm2(n, k, opn, f), f"norm of iteration {j}"
        ring[j] = got
    assert np.array_equal(ring, out.norms, equal_nan=True), "a later iteration of the deciding launch left a ring entry"
    assert out.res_norm == out.norms[acc]
    if not done:          # the Gram matrices of the last group, still in their slots
        for i in range(g):
            G, aG, f = M.gram(out.R[(NG - 1) * g + i][:n])
            _within(out.G[(NG & 1) * g + i], G, M.bound_step(n, aG, f), f"Gram matrix of iteration {(NG - 1) * g + i + 1}")
    return norms_ref


@pytest.mark.parametrize("n", [12, 29, 32, 100])
@pytest.mark.parametrize("g", [2, 3, 5, 6])
def test_group_chain(ctx, n, g):
    for k in (1, 17, 48, 256):
        check_group(run_group(ctx, n, k, g, 1))
        check_group(run_group(ctx, n, k, g, 3, two_starts=True))          # Gpack alternates between the two start positions


@pytest.mark.parametrize("g", [3, 5])
def test_group_stop_in_the_middle_of_a_group(ctx, g):
    n, k = 29, 17
    norms = check_group(run_group(ctx, n, k, g, 3, two_starts=True))
    assert all(b < a for a, b in zip(norms, norms[1:]))
    for jstar in (g + 2, 2):          # second iteration of the second and of the first group
        tol = float(np.sqrt(norms[jstar - 2] * norms[jstar - 1]))          # between the norms after iterations jstar - 1 and jstar
        out = run_group(ctx, n, k, g, 3, two_starts=True, abstol=tol)
        check_group(out)
        assert (out.iters, out.done) == (jstar, 1) and _all_nan(out.norms[jstar + 1:])
    out = run_group(ctx, n, k, g, 3, two_starts=True, maxiters=g + 1)
    check_group(out)
    assert (out.iters, out.done) == (g + 1, 1)


def test_group_refusals(ctx):
    for k, g, text in ((257, 2, "too wide"), (17, 7, "g must lie")):
        with pytest.raises(D.DREError) as e:
            P.probe(ctx, P.GROUP, 12, k, [np.zeros((2 * g * 12, 12))], g=g, mu=[-1.0] * g, R0=np.zeros((12, k)), T=np.eye(k), nit=g)
        assert e.value.code == P.ERR_INVALID and text in str(e.value)


@pytest.mark.parametrize("n,k,g", [(29, 17, 3), (100, 48, 5)])
def test_group_and_fast_chain_agree(ctx, n, k, g):
    """The same g shifts through both chains from the same R0.  The group chain forms R_i = Pi_i R0 in one product (bound as above, plus eps |Pi_i| |R0| for
    the single rounding of the operator, inside the same allowance); the fast chain compounds: e_R(i) <= b_R(i) + |I - 2 mu_i Seff_bot| e_R(i - 1),
    e_V(i) <= b_V(i) + |Seff_top| e_R(i - 1).  The two results may differ by the sum."""
    mus, Ss, ops = _group_ops(n, g, g)
    R0, T = _R0(n, k, 3), _T(k, 0)
    grp = run_group(ctx, n, k, g, 1)
    fast = P.probe(ctx, P.FAST, n, k, Ss, mu=mus, R0=R0, T=T, nit=g)
    for i in range(g):
        assert np.array_equal(M.unpack_a(fast.packs[i], n, 2)[0], Ss[i])
    eR = np.zeros((n, k))
    gb = M.bound_step(n, np.abs(ops[0]) @ np.abs(R0))
    for i in range(g):
        Rprev = R0 if i == 0 else fast.R[i - 1][:n]
        s = M.step(Ss[i], Rprev, mus[i])
        eV = M.bound_step(n, s["aV"], s["f"]) + np.abs(Ss[i][:n]) @ eR
        eR = M.bound_step(n, s["aR"], s["f"]) + np.abs(np.eye(n) - 2.0 * mus[i] * Ss[i][n:]) @ eR
        _within(fast.V[i][:n], grp.V[i][:n], eV + gb[i * n:(i + 1) * n], f"V of iteration {i + 1}")
        _within(fast.R[i][:n], grp.R[i][:n], eR + gb[(g + i) * n:(g + i + 1) * n], f"R of iteration {i + 1}")


# ---- fixed-order sums -------------------------------------------------------------------------------------------------------------------
def test_every_variant_is_deterministic(ctx):
    def same(a, b):
        for name in ("V", "R", "Rp", "G", "norms", "packs"):
            assert np.array_equal(getattr(a, name), getattr(b, name), equal_nan=True), name
    for mode, nt in ((0, 1), (0, 2), (0, 4), (1, 2)):
        same(run_fast(ctx, 100, 97, mode=mode, nt=nt, nit=5), run_fast(ctx, 100, 97, mode=mode, nt=nt, nit=5))
    same(run_group(ctx, 100, 48, 3, 3, two_starts=True), run_group(ctx, 100, 48, 3, 3, two_starts=True))
