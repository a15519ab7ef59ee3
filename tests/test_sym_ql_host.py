"""Host side of the Householder + QL tests: the NumPy model (tests/_sym_ql_model.py) against its recorded run (tests/golden/sym_ql_model.json) and
against LAPACK, the conditions the device tests' bounds rest on, and the C surface of dre_sym_eig_probe.  No device is needed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _sym_ql_model as M
from conftest import ROOT

REC = M.recorded()
CASES = M.cases()
FIGURES = ("a1", "a2", "a3", "b1", "b2", "b3", "c", "eig_err", "residual", "orth")
LIVE = [n for n in CASES if REC.get(n, {}).get("order", 1 << 30) <= M.HOST_MAX_ORDER]
_RUNS = {}


def live(name):
    if name not in _RUNS:
        _RUNS[name] = M.run_case(name)
    return _RUNS[name]


def test_the_record_holds_every_case():
    assert set(REC) == set(CASES)
    assert len(LIVE) >= 40


@pytest.mark.parametrize("name", LIVE)
def test_model_reproduces_its_record(name):
    """The figures within a factor of four: another BLAS, or another number of its threads, sums in another order (the device tests have a
    margin of ten).  The same rounding moves the counts: where the reduction runs to the end they are exact, where it stops early the
    remainder it tests is itself rounding noise once the rank is exhausted, so jdim may move by a column or two inside its window; the
    numbers of sweeps and rotations follow T_j."""
    got, rec = live(name), REC[name]
    assert set(got) == set(rec) and got["order"] == rec["order"]
    floor = rec["order"] * M.EPS / M.MARGIN
    for k in FIGURES:
        assert got[k] <= 4.0 * rec[k] + floor and rec[k] <= 4.0 * got[k] + floor, (k, got[k], rec[k])
    slack = 0 if rec["jdim"] in (0, rec["order"]) else 2
    for k in ("jdim", "nref", "tau0"):
        assert abs(got[k] - rec[k]) <= slack, (k, got[k], rec[k])
    for k in ("nsweeps", "nrot"):
        assert abs(got[k] - rec[k]) <= 0.1 * rec[k] + 2 + slack * rec["order"], (k, got[k], rec[k])
    if rec["residues"] == list(range(16)):
        assert got["residues"] == list(range(16)) and got["below8"] > 0 and got["from9to15"] > 0


def test_the_yardstick_is_sound():
    """every recorded figure of the model is rounding noise of the size LAPACK's own solvers leave: below 20 q eps; where the reduction
    stopped early, the three figures that see the dropped part may add the tolerance it stopped at (relative to ||S||_F)"""
    for name, rec in REC.items():
        dropped = max(4 * M.EPS, CASES[name][1].get("abs_tol_rel", 0.0), 1.0 if name.startswith("stop_edge") else 0.0) if rec["jdim"] < rec["order"] else 0.0
        for k in FIGURES:
            assert 0.0 <= rec[k] <= 20 * max(rec["order"], 8) * M.EPS + (dropped if k in ("a3", "eig_err", "residual") else 0.0), (name, k, rec[k])


def test_model_against_numpy_eigh_on_a_full_run():
    S = M.dense(129)
    r = M.solve(S)
    B = M.backtransform(r["V"], r["tau"], r["nref"], r["Z"])
    ref = np.linalg.eigvalsh(S)
    assert np.abs(np.sort(r["w"]) - ref).max() <= 100 * M.EPS * np.abs(ref).max()
    assert np.linalg.norm(S @ B - B * r["w"]) <= 100 * M.EPS * np.linalg.norm(S)
    # dorgqr and the reflector-by-reflector product in np.longdouble give the same orthogonal factor
    Ql, Qd = M.form_q(r["V"], r["tau"], r["nref"], 129, np.longdouble), M.form_q_lapack(r["V"], r["tau"], r["nref"], 129)
    assert np.abs((Ql - Qd).astype(float)).max() <= 100 * M.EPS
    t = M.tridiag(M.low_rank(300, 8)[0])
    Ql, Qd = M.form_q(t["V"], t["tau"], t["nref"], t["jdim"], np.longdouble), M.form_q_lapack(t["V"], t["tau"], t["nref"], t["jdim"])
    assert t["jdim"] < 20 and np.abs((Ql - Qd).astype(float)).max() <= 100 * M.EPS


# ---- the conditions of the device tests' bounds ---------------------------------------------------------------------------------------------
def test_sweep_lengths_cover_every_residue_at_every_order_of_the_ql_cases():
    """the read-ahead of k_tql_replay: two register batches of eight rotations; sweep lengths of every residue mod 16, below 8 and from 9 to 15"""
    for q in M.QL_ORDERS:
        for kind in ("dense", "spectrum"):
            rec = REC[f"{kind}{q}"]
            assert rec["jdim"] == q and rec["nref"] == max(q - 1, 0), (kind, q)          # nothing stops early in these
            if q >= 63:
                assert rec["residues"] == list(range(16)) and rec["below8"] > 0 and rec["from9to15"] > 0 and rec["longest"] == q - 1, (kind, q)


def test_slab_heights_at_the_switches():
    assert [M.slab_rows(j) for j in (129, 300, 301, 600, 601, 1200, 1201, 2048)] == [64, 64, 32, 32, 16, 16, 8, 8]
    assert all(M.slab_rows(j) * j * 8 <= 150 * 1024 for j in range(129, 2049))


def test_jdim_windows_are_narrow_and_above_the_rank():
    for (q, r) in M.LOW_RANK:
        rec = REC[f"lowrank{q}_r{r}"]
        assert rec["jdim_tight"] - rec["jdim_loose"] <= 10 and r <= rec["jdim_loose"] <= rec["jdim"] <= rec["jdim_tight"] < q, (q, r, rec)
    for name in LIVE:
        rec = REC[name]
        if 0 < rec["jdim"] < rec["order"] and "jdim_loose" not in rec:
            S = CASES[name][0]()
            lo, hi = M.tridiag(S, 16.0, want_v=False)["jdim"], M.tridiag(S, 1.0, want_v=False)["jdim"]
            assert hi - lo <= M.window_width_max(name) and lo <= rec["jdim"] <= hi, (name, lo, rec["jdim"], hi)


def test_stop_rule_cases_do_what_their_names_say():
    S, lam = M.low_rank(1000, 20)
    nf = np.linalg.norm(S)
    assert 1e-18 * nf < 4 * M.EPS * nf < 1e-6 * nf          # the floor loses once and wins once
    assert REC["floor_loses"] == {**REC["lowrank1000_r20"]} and REC["floor_wins"] == REC["abs_tol"]
    assert REC["abs_tol"]["jdim"] <= REC["lowrank1000_r20"]["jdim"]
    assert REC["floor_coarse"] == REC["abs_tol_coarse"] and 10 <= REC["abs_tol_coarse"]["jdim"] <= REC["lowrank1000_r20"]["jdim_loose"] - 5
    # counts of kept eigenvalues are asserted at 1e-10 max |lambda|: in a gap of more than four decades, two on either side, between the
    # smallest |lambda| and the largest error the device tests allow an eigenvalue
    for q, r in M.LOW_RANK:
        lam, rec = M.low_rank_spectrum(r), REC[f"lowrank{q}_r{r}"]          # (the spectrum does not depend on the order)
        assert np.abs(lam).min() >= 1e2 * 1e-10 and 1e-10 >= 1e2 * M.MARGIN * (rec["eig_err"] + rec["orth"])
    assert REC["zero1"]["jdim"] == REC["zero6"]["jdim"] == 0 and REC["padded9"]["jdim"] == 5
    # the factor 2 of the stop rule decides these two: with e^2 in the place of 2 e^2 the reduction would stop one column earlier
    tr = []
    tol = M.stop_edge_tol(S)
    j = M.tridiag(S, abs_tol=tol, want_v=False, trace=tr)["jdim"]
    assert j == REC["stop_edge"]["jdim"] == 11 and tr[10][0] + tr[10][1] ** 2 < 0.97 * tol ** 2 and tr[10][0] + 2 * tr[10][1] ** 2 > 1.03 * tol ** 2
    assert REC["stop_edge2"]["jdim"] == 2 and 0.8 ** 2 < 1.0 < 2 * 0.8 ** 2


def test_block_tridiagonal_inputs_have_the_blocks_the_issue_asks_for():
    for q, at in M.BLOCKTRI.items():
        T, sizes = M.block_tridiagonal(q, at)
        ends = np.cumsum(sizes)
        assert ends[-1] == q and 1 <= min(sizes) and max(sizes) <= 41 and at not in ends          # a block holds both at - 1 and at
        assert (np.diag(T) != 0).all() and np.array_equal(T, T.T) and not np.triu(T, 2).any()
        e = np.diag(T, -1)
        assert (e[ends[:-1] - 1] == 0).all() and np.count_nonzero(e) == q - len(sizes)
        rec = REC[f"blocktri{q}"]
        assert (rec["jdim"], rec["nref"], rec["tau0"]) == (q, q - 1, q - 1) and rec["nrot"] < 4e5 and rec["a1"] == rec["a2"] == 0.0


def test_deflate_asymmetry_is_mirrored():
    """k_tql<true> (j <= 128) has 1e-3 built in; the host generator above takes the caller's value"""
    t = M.tridiag(M.dense(100), want_v=False)
    a, b = M.ql(t["d"], t["e"], t["snorm"], 1.0), M.ql(t["d"], t["e"], t["snorm"], 1e-3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert REC["dense100_deflate1"] == REC["dense100_deflate1e-3"]


# ---- the C surface -----------------------------------------------------------------------------------------------------------------------------
def test_probe_prototype_matches_the_header_and_the_version():
    import dre_amd as D
    lib = D._lib.load()
    assert lib.dre_version() >= 114 and hasattr(lib, "dre_sym_eig_probe")
    txt = open(os.path.join(ROOT, "include", "dre_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    decl = re.search(r"int\s+dre_sym_eig_probe\s*\(([^;]*)\)\s*;", txt).group(1)
    params = [p.strip() for p in decl.split(",")]
    res, args = D._lib.PROTOTYPES["dre_sym_eig_probe"]
    assert res is C.c_int and len(args) == len(params) == 18
    for p, a in zip(params, args):
        if "**" in p:
            assert a is D._lib._pvp, p
        elif p.startswith("double "):
            assert a is C.c_double, p
        elif p.startswith("int "):
            assert a is C.c_int, p
    # the source refuses before it launches: the checks stand in front of the copy of S and the call of sym_eig, the finite check of
    # sym_eig in front of the QL stage
    api = open(os.path.join(ROOT, "differentialriccatiequations.jl_amd", "csrc", "api_probe.hip")).read()
    start = api.index("int dre_sym_eig_probe(")
    end = api.find("// ---- dre_", start)          # the next probe's banner, or the end of the file
    body = api[start:end if end >= 0 else len(api)]
    assert body.index("square matrix expected") < body.index("order above 8192") < body.index("copy_mat") < body.index("sym_eig(c, A")
    assert body.index("sym_eig(c, A") < body.index("outside [0, jdim)") < body.index("sym_eig_backtransform")
    assert "c->sym_eig_method = 0" in body and "~Method0" in body
    qr = open(os.path.join(ROOT, "differentialriccatiequations.jl_amd", "csrc", "qr_band.hip")).read()
    body = qr[qr.index("SymEig sym_eig(Ctx* ctx"):qr.index("__global__ __launch_bounds__(256) void k_backtransform")]
    assert body.index("k_tridiag, dim3(1)") < body.index("sym_eig: non-finite input") < body.index("(k_tql<true>), dim3(1)")
