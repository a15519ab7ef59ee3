"""Block Jacobi eigensolver, the part that needs no device: the exported symbol and its binding, the option's registration, the argument errors
that `sym_eigh` raises before any device call, and the NumPy model (tests/_block_jacobi_model.py) against numpy.linalg.eigh.

The model's figures (eigenvalue error / ||A||_2, residual / ||A||_F, loss of orthogonality, sweeps) are what the device test's bounds are made
of; they are recorded in tests/golden/block_jacobi_model.json.  Every case, the order-352 one included, is repeated here and compared with the record.
(The option's round trip and its rejection of 2 and -1 need a context, hence a device: tests/test_gpu_sym_jacobi.py.)"""
import os
import re

import numpy as np
import pytest

import dre_amd as D
import _block_jacobi_model as bm
from conftest import ROOT

EPS = np.finfo(float).eps
LIVE = list(bm.cases())


def test_symbol_is_exported_bound_and_declared():
    lib = D._lib.load()
    assert hasattr(lib, "dre_sym_eig_jacobi")
    assert len(D._lib.PROTOTYPES["dre_sym_eig_jacobi"][1]) == 6
    header = open(os.path.join(ROOT, "include", "dre_hip.h")).read()
    assert re.search(r"int dre_sym_eig_jacobi\(dre_ctx\* ctx, const dre_dense\* S, double tol, dre_dense\*\* values, dre_dense\*\* vectors, int64_t\* stats\);", header)
    assert '"sym_eig_method"' in header
    assert "sym_eigh" in D.__all__ and callable(D.sym_eigh)


def _no_device(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a device context was requested")
    monkeypatch.setattr(D.api.dev, "default_context", boom)


@pytest.mark.parametrize("A,kw", [
    (np.ones((3, 4)), {}),
    (np.ones(5), {}),
    (np.array([[1.0, 2.0], [2.0 + 1e-10, 1.0]]), {}),
    (np.eye(3), dict(method="qr")),
    (np.eye(3), dict(method="ql", tol=-1.0)),
    (np.eye(3), dict(tol=0.0)),
])
def test_argument_errors_before_any_device_call(monkeypatch, A, kw):
    _no_device(monkeypatch)
    with pytest.raises(ValueError, match="nothing was run on the device"):
        D.sym_eigh(A, **kw)


def test_asymmetry_within_100_eps_is_accepted(monkeypatch):
    """the check is relative to max |A|: rounding-level asymmetry passes it and reaches the device call"""
    _no_device(monkeypatch)
    A = np.array([[1.0, 2.0], [2.0 * (1 + 10 * EPS), 1.0]])
    with pytest.raises(AssertionError, match="a device context was requested"):
        D.sym_eigh(A)


def test_schedule_is_a_tournament():
    for p in (2, 3, 4, 9, 22):
        rounds = bm.schedule(p)
        assert len(rounds) == p - 1 + (p & 1)
        met = set()
        for pairs, sit in rounds:
            blocks = [b for pr in pairs for b in pr] + ([sit] if sit >= 0 else [])
            assert sorted(blocks) == list(range(p)) and (sit >= 0) == bool(p & 1)        # disjoint, everyone placed, one sits out iff p is odd
            assert all(i < j for i, j in pairs)
            met |= set(pairs)
        assert len(met) == p * (p - 1) // 2
    assert bm.padded_order(1) == bm.padded_order(32) == 32 and bm.padded_order(33) == 48 and bm.padded_order(352) == 352


@pytest.mark.parametrize("name", LIVE)
def test_model_against_numpy_and_the_record(name):
    r, rec = bm.run(name), bm.recorded()[name]
    S, (e_eig, e_res, e_orth) = r["S"], r["err"]
    q = S.shape[0]
    print(f"{name}: order {q} sweeps {r['sweeps']} rounds {r['rounds']} eig {e_eig:.2e} residual {e_res:.2e} orth {e_orth:.2e}")
    # a backward-stable solver that applies r rounds of orthogonal 32-column updates: each measure stays below (rounds + 1) * 32 eps
    cap = (r["rounds"] + 1) * 32 * EPS
    assert e_eig <= cap and e_res <= cap and e_orth <= cap * np.sqrt(q)
    assert r["sweeps"] <= bm.MAX_SWEEPS and rec["order"] == q
    # the record is this model's run (other BLAS builds sum in another order: a sweep more or less, figures within a factor of 3)
    assert abs(r["sweeps"] - rec["sweeps"]) <= 1
    for live, key in ((e_eig, "eig_err"), (e_res, "residual"), (e_orth, "orth")):
        assert live <= 3 * rec[key] and rec[key] <= 3 * live or max(live, rec[key]) == 0.0
    if name in ("diagonal", "random1"):
        assert r["sweeps"] == 0 and r["err"] == (0.0, 0.0, 0.0)
    if name == "rank3":
        assert int((np.abs(r["w"]) > 1e-10 * np.abs(r["w"]).max()).sum()) == 3


def test_record_lists_every_case():
    assert set(bm.recorded()) == set(bm.cases())


def test_model_rejects_non_finite_input_and_honours_tol():
    A = bm.random_indefinite(33)
    A[3, 7] = A[7, 3] = np.nan
    with pytest.raises(ValueError):
        bm.solve(A)
    S = bm.random_indefinite(48)
    w, V, loose, _ = bm.solve(S, tol=1e-3)
    T = V.T @ S @ V
    assert loose <= bm.run("random48")["sweeps"] and np.linalg.norm(T - np.diag(np.diag(T))) <= 1e-3 * np.linalg.norm(S) * (1 + 1e-8)
    assert np.linalg.norm(T - np.diag(np.diag(T))) > 48 * EPS * np.linalg.norm(S)          # (it stopped early: the default would have gone on)
