"""The kernels of the warm-started compression (csrc/warm.hip: k_warm_project, k_warm_z, k_warm_zapply, k_warm_small in its three instantiations and
three modes, k_warm_finish) on their own, through dre_warm_probe, at the smallest shapes at which each piece can go wrong, and the launch sequence of
the dense-X time loop's compression (warm_chain_jacobi) as a whole.

Every comparison is ONE-STEP consistent: a stage is held against the model (tests/_warm_model.py) applied to the DEVICE's own inputs of that stage,
so the bounds do not compound.  The bounds are derived, not measured (eps = 2^-52):
    matrix cores, K terms      |C - C_ref| <= 2 (K + 8) eps |A| |B|            (W_2 = Res Z: K = n;  R = B Wk: K = q)
    scalar chains, K terms     |c - c_ref| <= (K + 2) eps sum |a| |b|           (Z_1 = Y_f - Q P_f: K = q;  Z = Z_1 C: K = 16;  a slab share: K = rows)
    whitening C of PROJECT     C'GC = I on the live pivots within 16 eps kappa(G_live), G = the device's own slab shares summed in slab order
    small eigenproblem         8 (s na + m) eps ||L^-T||_2^2 ||H||_2, s sweeps and na active coordinates as the kernel reports them in tols[3]: a plane
                               rotation is orthogonal to a few ulp and a column meets at most na - 1 of them per sweep; for the dimensionless
                               identities (Uc'G Uc = I, U'U = I) ||G||_2 resp. 1 stands in the place of ||H||_2
    probe estimate             |est^2 - ref| <= (2 ||D||_F ||E||_F + ||E||_F^2) / 16 + (n / 16 + 80) eps est^2,  D = Y_p - B P_p, E = 2 (q + 8) eps (|Y_p| + |B| |P_p|)
The inputs come from tests/_warm_cases.py; tests/test_warm_host.py asserts on the CPU that each family meets its stated condition (gaps, distances from
thresholds), so no assertion here rests on a borderline input.  No bound in this file was loosened after a GPU run."""
import numpy as np
import pytest

import dre_amd as D
import _warm_cases as K
import _warm_model as M
import _warm_probe as P

pytestmark = pytest.mark.gpu
EPS = M.EPS


def _within(got, ref, bound, what):
    err = np.abs(got - ref)
    bad = ~(err <= bound)
    assert not bad.any(), f"{what}: {int(bad.sum())} entries outside the bound, worst ratio {float(np.max(err[bad] / np.maximum(bound[bad], 1e-300))):.3g}"


def _all_nan(a):
    return bool(np.all(np.isnan(a)))


def _same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def _pad(n):
    return 0 if n in (371, 1024, 4112) else 3          # the library's own leading dimension at the headline sizes, spare rows to watch elsewhere


# ---- PROJECT ------------------------------------------------------------------------------------------------------------------------------
def _check_project(ctx, kind, n, q):
    Q, Yf, Pf, live = K.project_inputs(kind, n, q)
    pad = _pad(n)
    o = P.probe(ctx, P.PROJECT, n=n, q=q, ldpad=pad, Q=Q, Yf=Yf, Pf=Pf)
    assert o.ticket[0] == 0
    Z1 = o.Z1_out[:n]
    assert _all_nan(o.Z1_out[n:])
    ref, bound, _, _, _ = M.project(Q, Yf, Pf)
    _within(Z1, ref, bound + EPS * np.abs(ref), "Z1")
    shares, sb = M.slab_shares(Z1)
    assert o.slab.shape == shares.shape == (M.project_slabs(n), 16, 16)
    _within(o.slab, shares, sb + EPS * np.abs(shares), "slab shares")
    G = M.sum_slabs(o.slab)
    Cw = o.Cw_out
    assert np.all(np.isfinite(Cw)) and np.array_equal(Cw, np.triu(Cw))
    _, lv, _ = M.chol_c(G)
    assert np.array_equal(lv, live)
    dead = np.flatnonzero(~live)
    assert np.all(Cw[dead, :] == 0.0) and np.all(Cw[:, dead] == 0.0)
    idx = np.flatnonzero(live)
    if idx.size:
        Gl = G[np.ix_(idx, idx)]
        Cl = Cw[np.ix_(idx, idx)]
        assert np.all(np.diag(Cl) > 0.0)
        defect = np.abs(M.mm(M.mm(Cl.T, Gl), Cl) - np.eye(idx.size))
        assert np.max(defect) <= 16 * EPS * np.linalg.cond(Gl), float(np.max(defect))
    # a second call on the same ticket block
    o2 = P.probe(ctx, P.PROJECT, n=n, q=q, ldpad=pad, Q=Q, Yf=Yf, Pf=Pf)
    assert o2.ticket[0] == 0 and _same(o2.Z1_out, o.Z1_out) and _same(o2.Cw_out, o.Cw_out) and _same(o2.slab, o.slab)
    return o


@pytest.mark.parametrize("n", K.PROJECT_N)
@pytest.mark.parametrize("q", K.PROJECT_Q)
def test_project(ctx, n, q):
    _check_project(ctx, "plain", n, q)


@pytest.mark.parametrize("kind,n,q", K.PROJECT_DEAD)
def test_project_dead_pivots(ctx, kind, n, q):
    o = _check_project(ctx, kind, n, q)
    if kind == "allzero":
        assert np.all(o.Cw_out == 0.0) and np.all(o.Z1_out[:n] == 0.0) and np.all(o.slab == 0.0)


# ---- Z / ZAPPLY -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", K.Z_N)
def test_z(ctx, n):
    Z1, Cw, Res = K.z_inputs(n)
    o = P.probe(ctx, P.Z, n=n, q=17, ldpad=_pad(n), Z1=Z1, Cw=Cw, Res=Res)
    assert _same(o.Zb, o.Zy)
    for a in (o.Zb, o.Zy, o.W2):
        assert _all_nan(a[n:]) and np.all(np.isfinite(a[:n]))
    zref, zb = M.zapply(Z1, Cw)
    Zd = o.Zb[:n]
    _within(Zd, zref, zb + EPS * np.abs(zref), "Z")
    assert np.all(Zd[:, 7] == 0.0)
    wref = M.mm(Res, Zd)
    _within(o.W2[:n], wref, M.mfma_bound(Res, Zd) + EPS * np.abs(wref), "W2")
    o2 = P.probe(ctx, P.Z, n=n, q=64, ldpad=_pad(n), Z1=Z1, Cw=Cw, Res=Res)          # the views at the far end of the buffers
    assert _same(o2.Zb, o.Zb) and _same(o2.Zy, o.Zy) and _same(o2.W2, o.W2)


@pytest.mark.parametrize("n", K.ZAPPLY_N)
def test_zapply(ctx, n):
    Z1, Cw, _ = K.z_inputs(n, False)
    o = P.probe(ctx, P.ZAPPLY, n=n, q=64, ldpad=_pad(n), Z1=Z1, Cw=Cw)
    assert _same(o.Zb, o.Zy) and _all_nan(o.Zb[n:])
    zref, zb = M.zapply(Z1, Cw)
    _within(o.Zb[:n], zref, zb + EPS * np.abs(zref), "Z")
    if n <= 1024:          # the two kernels form Z by the same chain
        Res = np.zeros((n, n))
        assert _same(P.probe(ctx, P.Z, n=n, q=64, ldpad=_pad(n), Z1=Z1, Cw=Cw, Res=Res).Zb, o.Zb)


# ---- SMALL ------------------------------------------------------------------------------------------------------------------------------
def _decode_tols3(t):
    """tols[3] = sweeps + 1e-4 rounds + 1e-7 na"""
    s = int(t + 1e-9)
    rest = (t - s) * 1e4
    rounds = int(rest + 1e-5)
    na = int(round((rest - rounds) * 1e3))
    return s, rounds, na


def _kl_qn(J, m, slack=0):
    kl = min(m, 16 * ((J + 15) // 16)) + slack
    return kl, min(m, kl + 16)


def _check_small(ctx, q, m, Cc, info, branch="abs", nparts=64, expect_na=None, kl=None):
    kw = K.small_tols(branch, nparts)
    r = M.small(Cc, q, m, kw["parts"], kw["reltol"], kw["abstol"], kw["frac"], kw["budget_frac"])
    J = r["J"]
    assert J == info["nkeep"]
    kl_, qn = _kl_qn(J, m)
    kl = kl_ if kl is None else kl
    o = P.probe(ctx, P.SMALL, q=q, m=m, kl=kl, qn=qn, mode=0, Cc=Cc, **kw)
    t = o.tols
    assert o.ticket[1] == 0
    np_ = max(nparts if kw["parts"] is not None else 1, 1)
    for i, ref in enumerate((r["at"], r["tolc"], r["nc"])):
        assert abs(t[i] - ref) <= np_ * EPS * abs(ref), (i, t[i], ref)
    s, rounds, na = _decode_tols3(t[3])
    assert 0 <= na <= m and 0 <= s <= 24
    if expect_na is not None:
        assert na == expect_na
    assert t[5] == 0.0 and t[6] == 0.0 and int(t[4]) == J and t[4] == float(J)
    H, G, LT, Mm = r["H"], r["G"], r["LT"], r["M"]
    nlt2 = np.linalg.norm(LT, 2) ** 2
    c = 8.0 * (s * na + m) * EPS * nlt2
    T, Uc = o.T, o.Uc
    assert np.all(np.isfinite(T)) and np.all(np.isfinite(Uc)) and np.array_equal(T, T.T)
    assert np.all(T[J:, :] == 0.0) and np.all(T[:, J:] == 0.0)
    UJ = Uc[:, :J]
    assert np.max(np.abs(M.mm(M.mm(UJ.T, H), UJ) - T[:J, :J])) <= c * np.linalg.norm(H, 2)
    assert np.max(np.abs(M.mm(M.mm(Uc.T, G), Uc) - np.eye(qn))) <= c * np.linalg.norm(G, 2)
    # tols[7] = ||M||_F^2 - ||T_J||_F^2, plus ||M[D, D]||_F^2 for the deflated coordinates D, which the kernel's figure 2 sum ||row||^2 counts twice
    # (_warm_model.deflate): exact when nothing is deflated, an upper bound otherwise
    Dset, _ = M.deflate(Mm, r["budget"])
    assert len(Dset) == m - na
    twice = float(np.sum(Mm[np.ix_(Dset, Dset)] ** 2))
    d2 = float(np.sum(np.asarray(Mm, dtype=M.LD) ** 2) - np.sum(np.asarray(T[:J, :J], dtype=M.LD) ** 2))
    print(f"small q={q} m={m} na={na} s={s}: dropped^2 {d2:.6e} + twice-counted {twice:.3e} against tols[7] {t[7]:.6e}, budget {r['budget']:.3e}")
    assert abs(d2 + twice - t[7]) <= c * np.linalg.norm(H, 2) * np.linalg.norm(Mm), (d2, twice, t[7])
    assert d2 <= t[7] + c * np.linalg.norm(H, 2) * np.linalg.norm(Mm) and t[7] <= r["budget"]
    assert np.max(np.abs(M.mm(G, o.Cp) - r["P"])) <= 8.0 * m * EPS * nlt2 * np.linalg.norm(G, 2) * np.max(np.abs(r["P"]))
    # the kept eigenvalues are those of the pencil
    lamT = np.linalg.eigvalsh(T[:J, :J])
    lamT = lamT[np.argsort(-np.abs(lamT), kind="stable")]
    # (Rayleigh-Ritz: the coupling that was dropped is at most sqrt(budget), the gap to the dropped spectrum at least half the smallest kept eigenvalue)
    assert np.max(np.abs(np.sort(lamT) - np.sort(r["lam"][:J]))) <= c * np.linalg.norm(H, 2) + 2.0 * r["budget"] / np.min(np.abs(r["lam"][:J]))
    return o, r


@pytest.mark.parametrize("q,m", K.SMALL_QM)
def test_small_mode0(ctx, q, m):
    Cc, info = K.small_inputs(q, m)
    o, r = _check_small(ctx, q, m, Cc, info, "abs", expect_na=m)
    _check_small(ctx, q, m, Cc, info, "rel", nparts={32: 300, 33: 1500}.get(m, 64), expect_na=m)          # (more partial sums than threads: a second pass)
    kl, qn = _kl_qn(r["J"], m)
    o3 = P.probe(ctx, P.SMALL, q=q, m=m, kl=kl, qn=qn, mode=0, Cc=Cc, **K.small_tols("abs"))
    assert _same(o3.T, o.T) and _same(o3.Uc, o.Uc) and _same(o3.Cp, o.Cp) and _same(o3.tols[:8], o.tols[:8])


@pytest.mark.parametrize("q,m", ((16, 32), (48, 64), (49, 65), (64, 80)))
@pytest.mark.parametrize("na0", (14, 15))
def test_small_deflation_leaves_an_even_or_an_odd_active_count(ctx, q, m, na0):
    Cc, info = K.small_inputs(q, m, family="block", na0=na0)
    o, r = _check_small(ctx, q, m, Cc, info, expect_na=na0)
    # the deflated coordinates come behind the active ones as unit vectors of M's coordinates: Uc = L^-T e_i there
    qn = o.Uc.shape[1]
    W = np.linalg.solve(r["LT"], o.Uc[:, na0:qn])
    assert np.all(np.abs(W).max(axis=0) > 0.999) and np.max(np.abs(np.abs(W).sum(axis=0) - 1.0)) <= 1e-12


@pytest.mark.parametrize("q,m,d", ((32, 48, 4), (49, 65, 0)))
def test_small_dead_fresh_direction(ctx, q, m, d):
    """a zero column of Z gets a unit pivot and stays decoupled: the same J, T and Uc as with a live direction of unit norm that couples to nothing"""
    Cd, info = K.small_inputs(q, m, dead=d)
    Cl, _ = K.small_inputs(q, m, decouple=d)
    od, r = _check_small(ctx, q, m, Cd, info)
    ol, _ = _check_small(ctx, q, m, Cl, info)
    assert _same(od.T, ol.T) and _same(od.Uc, ol.Uc) and od.tols[4] == ol.tols[4] and od.tols[7] == ol.tols[7]
    assert np.all(od.Cp[q + d] == 0.0)


def test_small_rejections(ctx):
    q, m = 16, 32
    Cc, info = K.small_inputs(q, m)
    kw = K.small_tols("abs")
    J = info["nkeep"]
    o = P.probe(ctx, P.SMALL, q=q, m=m, kl=J - 3, qn=J + 5, mode=0, Cc=Cc, **kw)          # the model's J > kl
    assert o.tols[5] == 1.0 and o.tols[4] == float(J - 3) and o.ticket[1] == 0
    assert np.all(np.isfinite(o.T)) and np.all(np.isfinite(o.Uc))
    kw2 = K.small_tols("rel")
    parts = kw2["parts"].copy(); parts[17] = np.nan
    o = P.probe(ctx, P.SMALL, q=q, m=m, kl=16, qn=32, mode=0, Cc=Cc, **{**kw2, "parts": parts})
    assert o.tols[5] == 1.0 and o.ticket[1] == 0
    Cb, _ = K.small_inputs(q, m, kappa_s=1e12)
    o = P.probe(ctx, P.SMALL, q=q, m=m, kl=16, qn=32, mode=0, Cc=Cb, **kw)              # Newton-Schulz gives up after six iterations
    assert o.tols[5] == 1.0 and o.ticket[1] == 0
    o = P.probe(ctx, P.SMALL, q=q, m=m, kl=16, qn=32, mode=1, Cc=Cb, **kw)
    assert o.tols[5] == 1.0 and o.ticket[1] == 0
    o = P.probe(ctx, P.SMALL, q=q, m=m, kl=16, qn=32, mode=0, Cc=Cc, **kw)              # and the context's next call is none the worse
    assert o.tols[5] == 0.0 and o.tols[4] == float(J)


@pytest.mark.parametrize("q,m", ((16, 32), (33, 49), (64, 80), (64, 64)))
def test_small_mode1(ctx, q, m):
    Cc, info = K.small_inputs(q, m)
    kw = K.small_tols("rel")
    r = M.small(Cc, q, m, kw["parts"], kw["reltol"], kw["abstol"], kw["frac"], kw["budget_frac"])
    o = P.probe(ctx, P.SMALL, q=q, m=m, kl=16, qn=32, mode=1, Cc=Cc, **kw)
    t = o.tols
    assert o.ticket[1] == 0 and _all_nan(o.T) and _all_nan(o.Uc)
    for i, ref in enumerate((r["at"], r["tolc"], r["nc"])):
        assert abs(t[i] - ref) <= 64 * EPS * abs(ref)
    assert abs(t[3] - np.sqrt(kw["budget_frac"]) * t[1]) <= 4 * EPS * t[1] and abs(t[7] - kw["budget_frac"] * t[1] ** 2) <= 4 * EPS * t[1] ** 2
    assert t[4] == 0.0 and t[5] == 0.0 and t[6] == 0.0
    LT, H = r["LT"], r["H"]
    kS = np.linalg.cond(r["S"]) if r["S"].size else 1.0
    nlt2 = np.linalg.norm(LT, 2) ** 2
    assert np.max(np.abs(o.LTout - LT)) <= 16 * (m + 16) * EPS * kS * np.linalg.norm(LT, 2)
    assert np.array_equal(o.LTout[:, :q], np.eye(m)[:, :q]) and np.all(o.LTout[q:, :q] == 0.0)
    assert np.max(np.abs(o.Mout - r["M"])) <= 16 * (m + 16) * EPS * kS * nlt2 * np.linalg.norm(H, 2)
    assert np.max(np.abs(M.mm(r["G"], o.Cp) - r["P"])) <= 8.0 * m * EPS * nlt2 * np.linalg.norm(r["G"], 2) * np.max(np.abs(r["P"]))


# ---- EIG --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,nzero,kind", K.EIG_CASES)
def test_eig(ctx, m, nzero, kind):
    S = K.eig_input(m, nzero, kind)
    U = P.probe(ctx, P.EIG, m=m, S=S).U
    na = m - nzero
    c = 8.0 * (8 * na + m) * EPS
    assert np.all(np.isfinite(U))
    assert np.max(np.abs(M.mm(U.T, U) - np.eye(m))) <= c
    zero_rows = np.flatnonzero(np.sum(np.abs(S), axis=1) == 0.0)
    tail = U[:, na:]
    assert np.all((tail == 0.0) | (tail == 1.0)) and np.array_equal(np.sort(np.argmax(tail, axis=0)), zero_rows) and np.all(tail.sum(axis=0) == 1.0)
    assert np.all(U[zero_rows, :na] == 0.0)
    A = M.mm(M.mm(U.T, S), U)
    nS = np.linalg.norm(S)
    d = np.abs(np.diag(A))[:na]
    assert np.all(d[:-1] - d[1:] >= -2.0 * c * np.linalg.norm(S, 2))
    if (m, nzero, kind) not in K.EIG_SLOW:
        assert np.linalg.norm(A - np.diag(np.diag(A))) <= 1e-10 * nS
    assert _same(P.probe(ctx, P.EIG, m=m, S=S).U, U)


# ---- FINISH -----------------------------------------------------------------------------------------------------------------------------
def _check_finish(ctx, n, q, kl, side, tols5=0.0, nan_yp=False):
    B, Wk, Yp, Pp, tols = K.finish_inputs(n, q, kl, side)
    tols = tols.copy(); tols[5] = tols5
    if nan_yp:
        Yp = Yp.copy(); Yp[n // 2, 3] = np.nan
    pad = _pad(n)
    o = P.probe(ctx, P.FINISH, n=n, q=q, kl=kl, ldpad=pad, Q=B, Wk=Wk, Yp=Yp, Pp=Pp, tols_in=tols)
    assert o.ticket[1] == 0
    R = o.R
    assert _all_nan(R[n:]) and _all_nan(R[:, kl:]) and R.shape[1] == 16 * ((kl + 15) // 16)
    ref, est2, rej = M.finish(B, Wk, Yp, Pp, tols[1], tols5, tols[7])
    _within(R[:n, :kl], ref, M.mfma_bound(B, Wk) + EPS * np.abs(ref), "R")
    t = o.tols
    assert _same(t[[0, 2, 3, 4, 8, 9, 10, 11]], tols[[0, 2, 3, 4, 8, 9, 10, 11]]) and t[1] == tols[1] and t[7] == tols[7]
    if nan_yp:
        assert np.isnan(t[6]) and t[5] == 1.0
    else:
        Dm = Yp - M.mm(B, Pp)
        E = 2.0 * (q + 8) * EPS * (np.abs(Yp) + M.amm(B, Pp))
        nE, nD = np.linalg.norm(E), np.linalg.norm(Dm)
        assert abs(t[6] - est2) <= (2.0 * nD * nE + nE * nE) / 16.0 + (n / 16 + 80) * EPS * est2, (t[6], est2)
        assert t[5] == (1.0 if rej else 0.0)
        assert abs(float(np.sum(o.slab)) / 16.0 - t[6]) <= (n / 16 + 80) * EPS * est2
    o2 = P.probe(ctx, P.FINISH, n=n, q=q, kl=kl, ldpad=pad, Q=B, Wk=Wk, Yp=Yp, Pp=Pp, tols_in=tols)
    assert o2.ticket[1] == 0 and _same(o2.R, R) and _same(o2.tols, t) and _same(o2.slab, o.slab)


@pytest.mark.parametrize("n,q,kl", K.FINISH_CASES)
def test_finish(ctx, n, q, kl):
    _check_finish(ctx, n, q, kl, "accept")
    _check_finish(ctx, n, q, kl, "reject")


def test_finish_keeps_an_earlier_rejection_and_rejects_a_nan(ctx):
    _check_finish(ctx, 97, 33, 20, "accept", tols5=1.0)
    _check_finish(ctx, 97, 33, 20, "accept", nan_yp=True)
    _check_finish(ctx, 4112, 33, 20, "accept", nan_yp=True)


# ---- CHAIN ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,qb", K.CHAIN_CASES)
def test_chain(ctx, n, qb):
    kw = dict(abstol=K.CHAIN_AT, reltol=0.0, frac=1.0, budget_frac=K.BF)
    Res, basis, kl, qn, info = K.chain_inputs(n, qb, 3)
    parts = np.full(((n + 15) // 16) ** 2, 0.25)
    o = P.probe(ctx, P.CHAIN, n=n, q=qb, kl=kl, qn=qn, Res=Res, basis=basis, parts=parts, **kw)
    t = o.tols
    tolc = K.CHAIN_AT
    assert o.ticket == [0, 0]
    assert t[0] == K.CHAIN_AT and t[1] == tolc and abs(t[2] - np.sqrt(np.sum(parts))) <= parts.size * EPS * t[2]
    assert t[5] == 0.0, ("rejected", t)
    J = int(t[4])
    assert J == info["kd"]                         # every dominant direction, those the basis had and the three the fresh directions caught
    assert 2.0 * t[6] + t[7] <= tolc ** 2 / 4.0
    assert np.array_equal(o.basis_out[:, :32 + qb], basis)
    Bm = o.basis_out[:, 32:]
    R, T = o.R[:, :kl], o.T
    assert np.all(np.isfinite(o.R)) and np.all(T[J:, :] == 0.0) and np.all(T[:, J:] == 0.0)
    assert np.linalg.norm(Res - R @ T @ R.T) <= tolc
    s, rounds, na = _decode_tols3(t[3])
    m = qb + 16
    G = M.mm(Bm.T, Bm)
    live = np.diag(G)[qb:] > 0.5
    keep = np.concatenate([np.ones(qb, dtype=bool), live])
    kG = np.linalg.cond(G[np.ix_(keep, keep)])
    # the eigenproblem's bound (||L^-T||_2^2 ||G||_2 = kappa(G)), the Gram product B'B the kernel worked with (K = n) and R = B Uc (K = m)
    c = (8.0 * (s * na + m) + 4.0 * (m + 8)) * EPS * kG + 4.0 * (n + 8) * EPS * kG / np.linalg.norm(G, 2) * np.linalg.norm(Bm) ** 2
    RtR = M.mm(o.R[:, :J].T, o.R[:, :J])
    assert np.max(np.abs(RtR - np.eye(J))) <= c, (float(np.max(np.abs(RtR - np.eye(J)))), c)
    o2 = P.probe(ctx, P.CHAIN, n=n, q=qb, kl=kl, qn=qn, Res=Res, basis=basis, parts=parts, **kw)
    assert o2.ticket == [0, 0] and _same(o2.R, o.R) and _same(o2.T, o.T) and _same(o2.basis_out, o.basis_out) and _same(o2.tols[:8], o.tols[:8])
    assert _same(o2.Uc, o.Uc) and _same(o2.Cp, o.Cp)
    # more missing directions than the 16 fresh ones can catch: rejected through the probe's estimate
    Res, basis, kl, qn, info = K.chain_inputs(n, qb, 24)
    o = P.probe(ctx, P.CHAIN, n=n, q=qb, kl=kl, qn=qn, Res=Res, basis=basis, parts=parts, **kw)
    assert o.ticket == [0, 0] and o.tols[5] == 1.0 and 2.0 * o.tols[6] >= 4.0 * tolc ** 2


def test_bad_arguments_leave_the_context_usable(ctx):
    Z1, Cw, _ = K.z_inputs(97, False)
    with pytest.raises(D.DREError) as e:
        P.probe(ctx, P.Z, n=1025, q=16, Z1=np.zeros((1025, 16)), Cw=Cw, Res=np.zeros((1025, 1025)))
    assert e.value.code == P.ERR_INVALID
    with pytest.raises(D.DREError) as e:
        P.probe(ctx, P.SMALL, q=16, m=31, kl=16, qn=16, Cc=np.zeros((31, 80)))
    assert e.value.code == P.ERR_INVALID
    o = P.probe(ctx, P.ZAPPLY, n=97, q=16, Z1=Z1, Cw=Cw)
    assert np.all(np.isfinite(o.Zb))
