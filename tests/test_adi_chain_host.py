"""The model of the dense-inverse ADI chain (tests/_adi_chain_model.py) against the reference arithmetic of oracle/dre_oracle.py, its packed layouts and
group operators against their definitions, and the argument checks of dre_adi_chain_probe.  No device is needed."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import dre_oracle as O
import _adi_chain_model as M
import _adi_chain_probe as P


def _pencil(n, seed):
    rng = np.random.default_rng(seed)
    E = np.eye(n) + 0.1 * rng.standard_normal((n, n))
    A = -(2.0 * np.eye(n) + 0.1 * rng.standard_normal((n, n)))
    return E, A, rng


def _stack(E, A, mu, U=None, Vt=None, alpha_lr=1.0):
    """([N; E'N; U'N], WKS) for F = A + inv(alpha_lr) U Vt:  N = inv(A' + mu E'),  WKS = [N; E'N] Vt' inv(alpha_lr I + U'N Vt')  (smw.jl:20-43)"""
    N = np.linalg.inv(A.T + mu * E.T)
    top = np.vstack([N, E.T @ N])
    if U is None:
        return top, None
    S = alpha_lr * np.eye(U.shape[1]) + U.T @ N @ Vt.T
    return np.vstack([top, U.T @ N]), top @ Vt.T @ np.linalg.inv(S)


def test_model_step_is_the_reference_adi_step():
    """One model iteration on a 12 x 12 dense pencil with a rank-2 update equals adi_single_step of the oracle (adi.jl:149-179 with the
    Sherman-Morrison-Woodbury solve) in V, in the residual and in the norm, to 1e-12 relative."""
    n, m, k, mu, alpha = 12, 2, 3, -0.7, -0.37
    E, A, rng = _pencil(n, 1)
    U, Vt = rng.standard_normal((n, m)), rng.standard_normal((m, n))
    R0 = rng.standard_normal((n, k))
    T = rng.standard_normal((k, k)); T = T + T.T
    prob = O.GALEProblem(sp.csc_matrix(E), O.LowRankUpdate(sp.csc_matrix(A), 1.5, U, Vt), None)
    res = alpha * O.lowrank(R0.copy(), T)
    c = O.ADICache(prob, O.ADI(shifts=O.Cyclic([mu])), None, O._CyclicIterator([mu]), 0.0, res.zero(), res.zero(), res, O.norm(res))
    O.adi_single_step(c, mu)
    _, V_ref, _ = c.increment.destructure()
    _, R_ref, _ = c.residual.destructure()
    nrm_ref = O.norm(c.residual)
    stack, wks = _stack(E, A, mu, U, Vt, 1.5)
    S, _ = M.seff(stack, wks, n)
    s = M.step(S, R0, mu)
    rel = lambda a, b: np.linalg.norm(a - b) / np.linalg.norm(b)
    assert rel(s["V"], V_ref) <= 1e-12
    assert rel(s["Rn"], R_ref) <= 1e-12
    assert abs(M.norm(s["Rn"], T, alpha) - nrm_ref) <= 1e-12 * nrm_ref
    assert abs(M.norm(R0, T, alpha) - O.norm(alpha * O.lowrank(R0, T))) <= 1e-12 * M.norm(R0, T, alpha)


@pytest.mark.parametrize("n", [1, 15, 16, 17])
def test_packed_stack_round_trip(n):
    rng = np.random.default_rng(n)
    for nblk in (2, 6):
        Mx = rng.standard_normal((nblk * n, n))
        flat = M.pack_a(Mx, n)
        assert flat.size == nblk * M.nstrip(n) * M.kst(n) * 64
        back, pad = M.unpack_a(flat, n, nblk)
        assert np.array_equal(back, Mx) and np.all(pad == 0.0) and pad.size == flat.size - Mx.size
        # the documented index, entry by entry
        ns, ks = M.nstrip(n), M.kst(n)
        for b, r, c in ((0, 0, 0), (nblk - 1, n - 1, n - 1), (1, n // 2, n - 1)):
            s, t = r // 16, c // 4
            lane = 16 * (c % 4) + (r % 16)
            assert flat[((b * ns + s) * ks + t) * 64 + lane] == Mx[b * n + r, c]


@pytest.mark.parametrize("n", [1, 15, 16, 17])
@pytest.mark.parametrize("k", [1, 16, 17])
def test_packed_residual_round_trip(n, k):
    R = np.random.default_rng(100 * n + k).standard_normal((n, k))
    flat = M.pack_r(R)
    assert flat.size == M.rpack_doubles(n, k)
    back, pad = M.unpack_r(flat, n, k)
    assert np.array_equal(back, R) and np.all(pad == 0.0) and pad.size == flat.size - R.size
    ct = (k + 15) // 16
    for r, c in ((0, 0), (n - 1, k - 1), (n // 2, k - 1)):
        lane = 16 * (r % 4) + (c % 16)
        assert flat[((r // 4) * ct + c // 16) * 64 + lane] == R[r, c]


@pytest.mark.parametrize("g", [2, 3, 6])
def test_group_operators_reproduce_sequential_iterations(g):
    n, k = 13, 5
    E, A, rng = _pencil(n, 7 + g)
    mus = np.linspace(-3.0, -0.3, g)
    Ss = [M.seff(*_stack(E, A, mu), n)[0] for mu in mus]
    ops = M.group_ops(Ss, mus)
    assert ops.shape == (2 * g * n, n)
    R = rng.standard_normal((n, k))
    R0 = R.copy()
    for i, (S, mu) in enumerate(zip(Ss, mus)):
        s = M.step(S, R, mu)
        V_i, R_i = ops[i * n:(i + 1) * n] @ R0, ops[(g + i) * n:(g + i + 1) * n] @ R0
        assert np.linalg.norm(V_i - s["V"]) <= 1e-12 * np.linalg.norm(s["V"])
        assert np.linalg.norm(R_i - s["Rn"]) <= 1e-12 * np.linalg.norm(R0)
        R = s["Rn"]


def test_decision_rule():
    assert M.decide([3.0, 2.0, 1.0, 0.5], 0, 1.5, 100) == (3, 1, 3)
    assert M.decide([3.0, 2.0, 1.0, 0.5], 10, 0.0, 12) == (12, 1, 2)
    assert M.decide([3.0, 2.0], 4, 0.0, 100) == (6, 0, 2)
    assert M.decide([3.0, 1.5], 0, 1.5, 100) == (2, 1, 2)          # "at or below"


# ---- the C surface ---------------------------------------------------------------------------------------------------------------------
def _refuse(lib, a):
    rc = lib.dre_adi_chain_probe(None, C.byref(a))
    return rc, lib.dre_last_error(None).decode()


def test_probe_refuses_bad_arguments_before_it_needs_a_device():
    """Every argument error of the header is DRE_ERR_INVALID with its own message; arguments that pass are told apart by the message about the
    missing context (the checks run in front of the first use of the context, so no launch can precede them)."""
    import dre_amd as D
    lib = D._lib.load()
    assert lib.dre_version() >= 116
    n, k = 5, 3
    st = [np.zeros((2 * n, n))]
    base = dict(R0=np.zeros((n, k)), T=np.eye(k), nit=2, outputs=False)
    gst = lambda g, cnt=1: [np.zeros((2 * g * n, n))] * cnt

    def msg(kind, n_, k_, stacks, **kw):
        a, keep = P.make_args(kind, n_, k_, stacks, **{**base, **kw})
        rc, text = _refuse(lib, a)
        assert rc == P.ERR_INVALID
        return text

    assert "context missing" in msg(P.FAST, n, k, st)
    assert "context missing" in msg(P.FAST, n, 512, st, R0=np.zeros((n, 512)), T=np.eye(512))
    assert "context missing" in msg(P.GROUP, n, 256, gst(2), g=2, mu=(-1.0, -2.0), R0=np.zeros((n, 256)), T=np.eye(256))
    assert "context missing" in msg(P.GROUP, n, k, gst(6), g=6, nit=12, mu=(-1.0,) * 6)
    assert "context missing" in msg(P.FAST, n, k, st, mode=1, nt=4, nit=480)
    assert "context missing" in msg(P.BUILD, n, 0, st)
    assert "k must be at least 1" in msg(P.FAST, n, 0, st)
    assert "too wide" in msg(P.FAST, n, 513, st)
    assert "too wide" in msg(P.GROUP, n, 257, gst(2), g=2, mu=(-1.0, -2.0))
    for g in (1, 7):
        assert "g must lie in 2 .. 6" in msg(P.GROUP, n, k, gst(max(g, 1)), g=g, nit=2 * g, mu=(-1.0,) * g)
    assert "multiple of g" in msg(P.GROUP, n, k, gst(3), g=3, nit=4, mu=(-1.0,) * 3)
    assert "start position" in msg(P.GROUP, n, k, gst(2, 2), g=2, mu=(-1.0, -2.0))
    assert "start position" in msg(P.GROUP, n, k, gst(2), g=2, mu=(-1.0, -2.0, -3.0))
    for nt in (0, 3, 8):
        assert "nt must be 1, 2 or 4" in msg(P.FAST, n, k, st, mode=0, nt=nt)
    assert "mode must be 0 or 1" in msg(P.FAST, n, k, st, mode=2, nt=1)
    assert "picked together" in msg(P.FAST, n, k, st, mode=-1, nt=2)
    assert "nit must lie in 1 .. 480" in msg(P.FAST, n, k, st, nit=481)
    assert "nit must lie in 1 .. 480" in msg(P.FAST, n, k, st, nit=0)
    assert "ld must be at least n + 2" in msg(P.FAST, n, k, st, ld=n + 1)
    assert "outside [0, nstack)" in msg(P.FAST, n, k, st, cycle=[0, 1], mu=(-1.0, -2.0))
    assert "needs wks" in msg(P.FAST, n, k, st, m=2)
    assert "n must lie" in msg(P.FAST, 0, k, st)
    assert "base_it" in msg(P.FAST, n, k, st, base_it=-1)
    assert "R0 or T missing" in msg(P.FAST, n, k, st, R0=None)
    assert "unknown kind" in msg(3, n, k, st)
    assert lib.dre_adi_chain_probe(None, None) == P.ERR_INVALID


def test_probe_adds_no_kernel_and_launches_only_through_the_chain():
    """The body of dre_adi_chain_probe holds no launch of its own: every kernel it starts is started by one of the five production entry points."""
    import os
    import re
    from conftest import ROOT
    api = open(os.path.join(ROOT, "differentialriccatiequations.jl_amd", "csrc", "api_probe.hip")).read()
    start = api.index("int dre_adi_chain_probe(")
    end = api.find("// ---- dre_", start)          # the next probe's banner, or the end of the file
    body = api[start:end if end >= 0 else len(api)]
    assert "hipLaunchKernelGGL" not in body and "<<<" not in body and "__global__" not in body
    called = set(re.findall(r"\b(adi_[a-z_]+|gemm[a-z_]*|copy_mat|fill_mat|residual_norm[a-z_]*|dense_adi_step)\s*\(", body))
    assert called == {"adi_fast_build", "adi_fast_pack_r", "adi_fast_iter", "adi_group_pack", "adi_group_iter", "adi_fast_pick", "adi_fast_nstrip",
                      "adi_fast_kst", "adi_fast_pack_doubles", "adi_fast_rpack_doubles"}
