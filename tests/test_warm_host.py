"""The NumPy model of the warm-started compression (tests/_warm_model.py) against independent facts, the conditions of the GPU tests' input families
(tests/_warm_cases.py) and the argument checks of dre_warm_probe.  No device is needed."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest
import scipy.linalg

import _warm_cases as K
import _warm_model as M
import _warm_probe as P


# ---- the model against independent facts ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,n,q", [("plain", 97, 17), ("dup", 97, 17), ("zero", 111, 16), ("allzero", 97, 16)])
def test_project_whitens_the_live_columns_and_zeroes_the_dead_ones(kind, n, q):
    Q, Yf, Pf, live = K.project_inputs(kind, n, q)
    Z1, bound, G, Cm, lv = M.project(Q, Yf, Pf)
    assert np.array_equal(lv, live)
    assert np.allclose(Z1, (np.eye(n) - Q @ Q.T) @ Yf, atol=1e-13)
    assert np.array_equal(Cm, np.triu(Cm))
    Zw = Z1 @ Cm
    ZtZ = Zw.T @ Zw
    idx = np.flatnonzero(live)
    if idx.size:
        kappa = np.linalg.cond(G[np.ix_(idx, idx)])
        assert np.max(np.abs(ZtZ[np.ix_(idx, idx)] - np.eye(idx.size))) <= 16 * M.EPS * kappa
    dead = np.flatnonzero(~live)
    assert np.all(Zw[:, dead] == 0.0) and np.all(ZtZ[dead, :] == 0.0) and np.all(ZtZ[:, dead] == 0.0)
    assert np.all(Cm[dead, :] == 0.0) and np.all(Cm[:, dead] == 0.0) and np.all(np.isfinite(Cm))


def test_slab_sum_is_sequential_in_slab_order():
    rng = np.random.default_rng(3)
    slab = rng.standard_normal((37, 16, 16)) * np.logspace(0, -12, 37)[:, None, None]
    G = M.sum_slabs(slab)
    ref = np.zeros((16, 16))
    for b in range(37):
        ref += slab[b]
    assert np.array_equal(G, ref)
    assert M.project_rows(4096) == 16 and M.project_rows(4112) == 32 and M.project_slabs(4112) == 129 and M.project_slabs(4097) == 129


@pytest.mark.parametrize("q,m", [(16, 32), (33, 49), (64, 80), (16, 16)])
def test_small_model_solves_the_generalized_eigenproblem(q, m):
    Cc, info = K.small_inputs(q, m)
    r = M.small(Cc, q, m, None, 0.0, K.AT, K.FRAC, K.BF)
    LT, G, H = r["LT"], r["G"], r["H"]
    assert np.max(np.abs(LT.T @ G @ LT - np.eye(m))) <= 64 * M.EPS * np.linalg.cond(G)
    ref = scipy.linalg.eigh(H, G, eigvals_only=True)
    ref = ref[np.argsort(-np.abs(ref), kind="stable")]
    assert np.max(np.abs(np.sort(ref) - np.sort(r["lam"]))) <= 1e-12 * np.max(np.abs(ref))
    assert np.max(np.abs(np.sort(r["lam"]) - np.sort(info["lam"]))) <= 1e-12
    assert np.max(np.abs(G @ r["Cp"] - r["P"])) <= 1e-12 * np.max(np.abs(r["P"]))
    assert r["J"] == info["nkeep"]
    assert r["tolc"] == K.FRAC * K.AT and r["budget"] == K.BF * (K.FRAC * K.AT) ** 2


def test_the_J_rule_against_brute_force():
    rng = np.random.default_rng(11)
    for trial in range(200):
        k = int(rng.integers(1, 12))
        lam = rng.standard_normal(k) * 10.0 ** rng.integers(-3, 1, k)
        budget = float(10.0 ** rng.uniform(-6, 1))
        defl2 = float(rng.choice([0.0, 0.1 * budget]))
        J, d2 = M.optimal_J(lam, budget, defl2)
        a2 = np.sort(lam ** 2)[::-1]
        brute = min(j for j in range(k + 1) if defl2 + float(np.sum(a2[j:][::-1])) <= budget * (1 + 1e-12) or j == k)
        assert J == brute or abs(defl2 + float(np.sum(a2[J:])) - budget) <= 1e-9 * budget


def test_deflation_figure_counts_the_deflated_block_twice():
    Cc, info = K.small_inputs(48, 64, family="block", na0=15)
    r = M.small(Cc, 48, 64, None, 0.0, K.AT, K.FRAC, K.BF)
    Mm = r["M"]
    D, defl2 = M.deflate(Mm, r["budget"])
    keep = np.setdiff1d(np.arange(64), D)
    assert len(D) == 64 - 15 and 2.0 * defl2 <= 0.5 * r["budget"]
    left = np.linalg.norm(Mm) ** 2 - np.linalg.norm(Mm[np.ix_(keep, keep)]) ** 2
    assert abs(defl2 - (left + np.linalg.norm(Mm[np.ix_(D, D)]) ** 2)) <= 1e-12 * np.linalg.norm(Mm) ** 2
    assert len(M.deflate(M.small(K.small_inputs(48, 64)[0], 48, 64, None, 0.0, K.AT, K.FRAC, K.BF)["M"], r["budget"])[0]) == 0


def test_tolerances_take_either_branch():
    for branch in ("abs", "rel"):
        kw = K.small_tols(branch)
        at, tolc, nc, budget = M.tolerances(kw["parts"], kw["reltol"], kw["abstol"], kw["frac"], kw["budget_frac"])
        assert abs(at - K.AT) <= 4 * M.EPS * K.AT and abs(tolc - K.FRAC * K.AT) <= 4 * M.EPS * K.AT
        assert (nc == 0.0) == (branch == "abs")


def test_finish_model():
    B, Wk, Yp, Pp, tols = K.finish_inputs(97, 33, 20)
    R, est2, rej = M.finish(B, Wk, Yp, Pp, tols[1], tols[5], tols[7])
    assert np.allclose(R, B @ Wk, rtol=0, atol=1e-13) and not rej
    assert abs(est2 - np.linalg.norm(Yp - B @ Pp) ** 2 / 16) <= 1e-6 * est2
    assert M.finish(B, Wk, Yp, Pp, tols[1], 1.0, tols[7])[2]


def test_jacobi_model_converges_to_the_eigenvalues():
    S = K.eig_input(17, 0)
    assert M.jacobi_sweeps(S) <= 8
    assert M.jacobi_sweeps(np.diag(np.arange(1.0, 6.0))) == 0


# ---- the conditions of the GPU tests' inputs ----------------------------------------------------------------------------------------------
def test_project_pivots_keep_their_distance_from_the_floor():
    cases = [("plain", n, q) for n in K.PROJECT_N for q in K.PROJECT_Q] + list(K.PROJECT_DEAD)
    for kind, n, q in cases:
        ratios, live = K.project_pivots(kind, n, q)
        assert np.all(ratios[live] >= 1e4), (kind, n, q, ratios)
        assert np.all(ratios[~live] <= 1e-4), (kind, n, q, ratios)


def _small_families():
    fam = [dict(q=q, m=m) for q, m in K.SMALL_QM]
    fam += [dict(q=q, m=m, family="block", na0=na0) for (q, m), na0 in itertools.product(((16, 32), (48, 64), (49, 65), (64, 80)), (14, 15))]
    fam += [dict(q=32, m=48, dead=4), dict(q=32, m=48, decouple=4), dict(q=49, m=65, dead=0), dict(q=49, m=65, decouple=0)]
    return fam


def test_small_spectra_have_their_gap():
    for kw in _small_families():
        kept, rest, r = K.small_gap(**kw)
        assert kept >= 100.0 and rest <= 0.01, (kw, kept, rest)
        assert r["J"] == 11
        if r["S"].size:
            assert np.linalg.cond(r["S"]) <= 4.0
    Cc, _ = K.small_inputs(16, 32, kappa_s=1e12)
    assert np.linalg.cond(M.small(Cc, 16, 32, None, 0.0, K.AT, K.FRAC, K.BF)["S"]) >= 1e11


def test_finish_cases_sit_a_factor_four_from_the_threshold():
    for n, q, kl in K.FINISH_CASES:
        for side in ("accept", "reject"):
            B, Wk, Yp, Pp, tols = K.finish_inputs(n, q, kl, side)
            _, est2, rej = M.finish(B, Wk, Yp, Pp, tols[1], tols[5], tols[7])
            ratio = (2.0 * est2 + tols[7]) / tols[1] ** 2
            assert rej == (side == "reject")
            assert ratio <= 0.2501 if side == "accept" else ratio >= 3.999, (n, q, kl, side, ratio)


def test_eig_inputs_converge_within_six_model_sweeps():
    slow = [c for c in K.EIG_CASES if M.jacobi_sweeps(K.eig_input(*c)) > 6]
    assert 6 * len(slow) <= len(K.EIG_CASES), slow
    assert sorted(slow) == sorted(K.EIG_SLOW)


def test_chain_inputs():
    for n, qb in K.CHAIN_CASES:
        for r in (3, 24):
            Res, basis, kl, qn, info = K.chain_inputs(n, qb, r)
            Q = basis[:, 32:]
            assert basis.shape == (n, 32 + qb) and np.max(np.abs(Q.T @ Q - np.eye(qb))) <= 1e-13
            budget, tolc = K.BF * K.CHAIN_AT ** 2, K.CHAIN_AT
            lam = info["lam"]
            assert np.min(np.abs(lam[:info["kd"]])) >= 100.0 * np.sqrt(budget) and float(np.sum(lam[info["kd"]:] ** 2)) <= budget / 100.0
            # what no 16 fresh directions can reach: the r - 16 smallest of the missing dominant eigenvalues at least
            missed = np.sort(np.abs(lam[info["missing"]]))[:max(r - 16, 0)]
            if r == 24:
                assert 2.0 * float(np.sum(missed ** 2)) >= 4.0 * tolc ** 2 and info["kd"] - r + 16 > 0
            else:
                assert info["kd"] <= kl and len(info["missing"]) == 3


# ---- the C surface ------------------------------------------------------------------------------------------------------------------------
def test_probe_refuses_bad_arguments_before_it_needs_a_device():
    import dre_amd as D
    lib = D._lib.load()
    assert lib.dre_version() >= 120
    z16 = np.zeros((8, 16))

    def msg(stage, **kw):
        a, keep = P.make_args(stage, outputs=False, **kw)
        rc = lib.dre_warm_probe(None, C.byref(a))
        assert rc == P.ERR_INVALID
        return lib.dre_last_error(None).decode()

    proj = dict(n=8, q=4, Q=np.zeros((8, 4)), Yf=z16, Pf=np.zeros((4, 16)))
    small = dict(q=16, m=32, kl=16, qn=32, Cc=np.zeros((32, 80)))
    fin = dict(n=8, q=4, kl=3, Q=np.zeros((8, 4)), Wk=np.zeros((4, 3)), Yp=z16, Pp=np.zeros((4, 16)), tols_in=np.zeros(12))
    zin = dict(n=8, q=4, Z1=z16, Cw=np.zeros((16, 16)), Res=np.zeros((8, 8)))
    chain = dict(n=96, q=16, kl=16, qn=32, Res=np.zeros((96, 96)), basis=np.zeros((96, 48)))
    for stage, kw in ((P.PROJECT, proj), (P.SMALL, small), (P.SMALL, {**small, "mode": 1}), (P.SMALL, {**small, "m": 16, "qn": 16}), (P.FINISH, fin), (P.Z, zin),
                      (P.ZAPPLY, {**zin, "Res": None}), (P.EIG, dict(m=80, S=np.zeros((80, 80)))), (P.CHAIN, chain), (P.FINISH, {**fin, "q": 80, "Q": np.zeros((8, 80)),
                      "Wk": np.zeros((80, 3)), "Pp": np.zeros((80, 16))})):
        assert "context missing" in msg(stage, **kw)
    assert "unknown stage" in msg(7) and "unknown stage" in msg(-1)
    assert "n must lie" in msg(P.PROJECT, **{**proj, "n": 0})
    for q in (0, 65):
        assert "q must lie in 1 .. 64" in msg(P.PROJECT, **{**proj, "q": q})
        assert "q must lie in 1 .. 64" in msg(P.SMALL, **{**small, "q": q})
        assert "q must lie in 1 .. 64" in msg(P.CHAIN, **{**chain, "q": q})
    assert "q must lie in 1 .. 80" in msg(P.FINISH, **{**fin, "q": 81})
    assert "m must be q or q + 16" in msg(P.SMALL, **{**small, "m": 31})
    assert "qn must lie" in msg(P.SMALL, **{**small, "qn": 33})
    assert "kl must lie in 1 .. qn" in msg(P.SMALL, **{**small, "kl": 0})
    assert "kl must lie in 1 .. qn" in msg(P.SMALL, **{**small, "kl": 33, "qn": 32})
    assert "kl must lie in 1 .. 80" in msg(P.FINISH, **{**fin, "kl": 81})
    assert "n above 1024" in msg(P.Z, **{**zin, "n": 1025})
    assert "n above 1024" in msg(P.CHAIN, **{**chain, "n": 1025})
    assert "mode must be 0 or 1" in msg(P.SMALL, **{**small, "mode": 2})
    assert "Q, Yf or Pf missing" in msg(P.PROJECT, **{**proj, "Pf": None})
    assert "Z1, Cw or Res missing" in msg(P.Z, **{**zin, "Res": None})
    assert "Z1 or Cw missing" in msg(P.ZAPPLY, **{**zin, "Cw": None})
    assert "Cc missing" in msg(P.SMALL, **{**small, "Cc": None})
    assert "S missing" in msg(P.EIG, m=16)
    assert "m must lie in 1 .. 80" in msg(P.EIG, m=81, S=np.zeros((81, 81)))
    assert "missing" in msg(P.FINISH, **{**fin, "tols_in": None})
    assert "Res or basis missing" in msg(P.CHAIN, **{**chain, "basis": None})
    assert "ldpad" in msg(P.PROJECT, **{**proj, "ldpad": 65})
    assert lib.dre_warm_probe(None, None) == P.ERR_INVALID


def test_widest_problem_is_accepted_and_the_next_q_refused():
    """m = 80 (q = 64) is the widest problem and passes the argument checks.  The probe's own `m above 80` requirement mirrors warm_small's
    DRE_REQUIRE and cannot fire on its own: m is q or q + 16 and q is at most 64, so a wider problem is refused by the bound on q, whose message
    this test names."""
    import dre_amd as D
    lib = D._lib.load()
    a, keep = P.make_args(P.SMALL, outputs=False, q=64, m=80, kl=16, qn=32, Cc=np.zeros((80, 128)))
    assert lib.dre_warm_probe(None, C.byref(a)) == P.ERR_INVALID and "context missing" in lib.dre_last_error(None).decode()
    a, keep = P.make_args(P.SMALL, outputs=False, q=65, m=81, kl=16, qn=32, Cc=np.zeros((81, 129)))
    assert lib.dre_warm_probe(None, C.byref(a)) == P.ERR_INVALID and "q must lie in 1 .. 64" in lib.dre_last_error(None).decode()


def test_probe_adds_no_kernel_and_launches_only_through_the_entry_points():
    from conftest import ROOT
    api = open(os.path.join(ROOT, "differentialriccatiequations.jl_amd", "csrc", "api_probe.hip")).read()
    start = api.index("int dre_warm_probe(")
    end = api.find("// ---- dre_", start)          # the next probe's banner, or the end of the file
    body = api[start:end if end >= 0 else len(api)]
    assert "hipLaunchKernelGGL" not in body and "<<<" not in body and "__global__" not in body
    called = set(re.findall(r"\b(warm_[a-z_]+|gemm[a-z_]*|copy_mat|fill_[a-z]+)\s*\(", body))
    assert called == {"warm_project", "warm_z", "warm_zapply", "warm_small", "warm_eig", "warm_finish", "warm_chain_jacobi", "warm_project_slabs"}
    # one owner for the chain's launch sequence: the time loop goes through the same function
    dx = open(os.path.join(ROOT, "differentialriccatiequations.jl_amd", "csrc", "dense_x.hip")).read()
    body = dx[dx.index("Compressed DenseStep::compress_warm()"):dx.index("Compressed DenseStep::compress_cold()")]
    assert "warm_chain_jacobi(ctx, w)" in body and "warm_chain_front(ctx, w)" in body
    assert not re.search(r"\bwarm_(project|z)\s*\(", body)
