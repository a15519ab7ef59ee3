"""Whole-device block Jacobi eigensolver (sym_eigh(A, "jacobi"), context option sym_eig_method) against numpy.linalg.eigh, the NumPy model of
the kernel sequence (tests/_block_jacobi_model.py), the library's Householder + QL solver and, through the compression, FactoredSign.

Bounds: each error measure is at most MARGIN = 10 times the MODEL's value for the same input (tests/golden/block_jacobi_model.json, the
model's recorded run; tests/test_sym_jacobi_host.py keeps that record honest), sweep counts within one of the model's."""
import numpy as np
import pytest

import dre_amd as D
import dre_oracle as o
import _sign_model as sm
import _factored_sign_model as fm
import _block_jacobi_model as bm

pytestmark = pytest.mark.gpu
EPS = np.finfo(float).eps
MARGIN = 10.0
CASES = bm.cases()
REC = bm.recorded()


@pytest.mark.parametrize("name", list(CASES))
def test_against_numpy_within_ten_times_the_model(ctx, name):
    S, rec = CASES[name], REC[name]
    w, V, st = D.sym_eigh(S, "jacobi", ctx=ctx, return_stats=True)
    q = S.shape[0]
    assert w.shape == (q,) and V.shape == (q, q) and (np.diff(w) >= 0).all()
    e_eig, e_res, e_orth = bm.errors(S, w, V)
    print(f"{name}: order {q} sweeps {st['sweeps']} (model {rec['sweeps']}) rounds {st['rounds']} eig {e_eig:.2e} (model {rec['eig_err']:.2e}) "
          f"residual {e_res:.2e} (model {rec['residual']:.2e}) orth {e_orth:.2e} (model {rec['orth']:.2e})")
    assert e_eig <= MARGIN * rec["eig_err"] and e_res <= MARGIN * rec["residual"] and e_orth <= MARGIN * rec["orth"]
    assert abs(st["sweeps"] - rec["sweeps"]) <= 1
    if name == "diagonal":
        assert st["sweeps"] <= 1
    if name == "rank3":
        # truncation rule of the compressions, |lambda| > rtol max |lambda|: the three eigenvalues are O(1) of the largest, the 93 others are
        # rounding noise below the eigenvalue bound above (MARGIN * model = 4e-14 ||A||_2); rtol = 1e-10 lies between with room on both sides
        assert int((np.abs(w) > 1e-10 * np.abs(w).max()).sum()) == 3


def test_nan_is_a_clean_invalid_and_the_context_lives(ctx):
    S = CASES["random33"].copy()
    S[4, 20] = S[20, 4] = np.nan
    with pytest.raises(D.DREError) as e:
        D.sym_eigh(S, "jacobi", ctx=ctx)
    assert e.value.code == -1 and "non-finite" in str(e.value)
    assert str(e.value).startswith("libdre_hip error -1: sym_eig_jacobi:") and "member" not in str(e.value)
    w, V = D.sym_eigh(CASES["random17"], "jacobi", ctx=ctx)
    assert bm.errors(CASES["random17"], w, V)[0] <= MARGIN * REC["random17"]["eig_err"]


def test_option_round_trips_and_rejects_other_values(ctx):
    before = ctx.get_option("sym_eig_method")
    try:
        ctx.set_option("sym_eig_method", 1)
        assert ctx.get_option("sym_eig_method") == 1.0
        ctx.set_option("sym_eig_method", 0)
        assert ctx.get_option("sym_eig_method") == 0.0
        for bad in (2, -1, 0.5):
            with pytest.raises(D.DREError) as e:
                ctx.set_option("sym_eig_method", bad)
            assert e.value.code == -1 and "sym_eig_method" in str(e.value)
            assert ctx.get_option("sym_eig_method") == 0.0
    finally:
        ctx.set_option("sym_eig_method", before)


@pytest.mark.parametrize("n", [33, 130])
def test_same_answer_as_the_householder_ql_solver(ctx, n):
    S, rec = CASES[f"random{n}"], REC[f"random{n}"]
    wj, Vj = D.sym_eigh(S, "jacobi", ctx=ctx)
    wq, Vq = D.sym_eigh(S, "ql", ctx=ctx)
    assert wq.shape == wj.shape                      # (full rank: the early-terminating reduction keeps everything)
    n2, nf = np.abs(np.linalg.eigvalsh(S)).max(), np.linalg.norm(S)
    d_eig = np.abs(wj - wq).max() / n2
    # invariant subspaces, not vectors: the eigenvalues below the widest gap of the middle half of the spectrum.  Davis-Kahan: each solver's
    # projector is within sqrt(2) ||residual||_F / gap (+ its loss of orthogonality) of the exact one; both solvers get the Jacobi bound
    k = n // 4 + int(np.argmax(np.diff(wq[n // 4:3 * n // 4]))) + 1
    gap = wq[k] - wq[k - 1]
    bound = 2 * (np.sqrt(2) * MARGIN * rec["residual"] * nf / gap + MARGIN * rec["orth"])
    d_sub = np.linalg.norm(Vj[:, :k] @ Vj[:, :k].T - Vq[:, :k] @ Vq[:, :k].T)
    print(f"n={n}: eigenvalues differ by {d_eig:.2e} ||A||_2 (bound {MARGIN * rec['eig_err']:.2e}); subspace of the {k} lowest (gap {gap:.2e}): "
          f"{d_sub:.2e} (bound {bound:.2e})")
    assert d_eig <= MARGIN * rec["eig_err"]
    assert d_sub <= bound


def test_default_path_is_untouched_by_a_jacobi_call(ctx):
    S = CASES["random130"]
    before = ctx.get_option("sym_eig_method")
    try:
        ctx.set_option("sym_eig_method", 0)
        w0, V0 = D.sym_eigh(S, "ql", ctx=ctx)
        D.sym_eigh(S, "jacobi", ctx=ctx)
        w1, V1 = D.sym_eigh(S, "ql", ctx=ctx)
        ctx.set_option("sym_eig_method", 1)          # "ql" names the Householder + QL solver whatever the compressions are set to use
        w2, V2 = D.sym_eigh(S, "ql", ctx=ctx)
        assert ctx.get_option("sym_eig_method") == 1.0
    finally:
        ctx.set_option("sym_eig_method", before)
    assert np.array_equal(w0, w1) and np.array_equal(V0, V1)
    assert np.array_equal(w0, w2) and np.array_equal(V0, V2)


def test_factored_sign_through_the_compression(ctx):
    """the smallest pencil of tests/test_gpu_factored_sign.py (n = 371, tau = 20, no feedback) with the compressions' eigensolver switched"""
    n, tau = 371, 20.0
    d = D.steel_profile(n)
    E, A = d.E.toarray(), d.A.toarray()
    Cm = np.asarray(d.C, float)
    q = Cm.shape[0]
    G = np.hstack([Cm.T, E.T @ np.random.default_rng(0).standard_normal((n, 5))])
    S = np.zeros((q + 5, q + 5))
    S[:q, :q] = np.eye(q)
    S[q:, q:] = -0.3 * np.eye(5)
    F = A - E / (2.0 * tau)
    Fop = D.ScaledPencil(d.A, 1.0, d.E, -1.0 / (2.0 * tau))
    Fsp = (d.A - d.E / (2.0 * tau)).tocsc()
    Cl = D.lowrank(G, S)
    R = G @ S @ G.T
    out = {}
    before = ctx.get_option("sym_eig_method")
    try:
        for method in (0, 1):
            ctx.set_option("sym_eig_method", method)
            X, info = D.solve(D.GALEProblem(d.E, Fop, Cl), D.FactoredSign(), return_info=True)
            res = D.norm(D.residual(D.GALEProblem(d.E, Fsp, Cl), X)) / np.linalg.norm(R)
            out[method] = (X.dense(), info["rank"], res)
    finally:
        ctx.set_option("sym_eig_method", before)
    # that file's own bound for the distance to MatrixSign(): MARGIN times the model's distance for the same input
    m = sm.SignModel(F, E)
    Lm, Dm, _ = fm.factored_sign_lyap(m, G, S, fm.default_rtol(n), D.FactoredSign().max_width, D.FactoredSign().max_refine)
    bound = MARGIN * o.delta(Lm @ Dm @ Lm.T, m.replay(R))
    dist = D.delta(out[1][0], out[0][0])
    print(f"rank {out[0][1]} / {out[1][1]}, distance {dist:.2e} (bound {bound:.2e}), residual {out[0][2]:.2e} / {out[1][2]:.2e}")
    assert out[0][1] == out[1][1]
    assert dist <= bound
    assert out[1][2] <= 2.0 * out[0][2]
