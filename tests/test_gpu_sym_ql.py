"""The Householder + QL eigensolver (csrc/qr_band.hip: sym_eig) stage by stage through dre_sym_eig_probe, at every order and input at which the
chain takes another path, plus one run of every case through the public dre_sym_eig.

    stage A  k_tridiag          a1 = ||Q'SQ - T||_F / ||S||_F, a2 = ||Q'Q - I||_F, a3 = ||S - Q T Q'||_F / ||S||_F with Q formed on the host from the
                                downloaded (V, tau): np.longdouble up to order 600, LAPACK's dorgqr above
    stage B  k_tql<true> (j <= 128), host_tql_log + k_tql_replay (j <= 2048, slabs of 64 / 32 / 16 / 8 rows), k_tql<false> (above)
                                on the device's own T_j: b1 eigenvalues against scipy's eigh_tridiagonal, b2 residual, b3 orthogonality
    stage C  k_backtransform    ||B - Q_j Z(:, ids)||_F against the host product

Bounds: every measure is at most max(MARGIN x the MODEL's figure for the same case, q eps), MARGIN = 10 (tests/_sym_ql_model.py, recorded in
tests/golden/sym_ql_model.json; tests/test_sym_ql_host.py keeps the record honest).  The device's own output is never the yardstick.
A case is run once per session (`run`) and its figures are shared by the tests of the stages, so that a failure names its kernel."""
import time

import numpy as np
import pytest

import dre_amd as D
import _sym_ql_model as M
import _sym_ql_probe as P

pytestmark = pytest.mark.gpu
EPS = M.EPS
MARGIN = M.MARGIN
CASES = M.cases()
REC = M.recorded()
KEEP_ARRAYS_MAX = 2600          # the arrays of a run stay in memory up to this order (stage C variants, determinism, scaling)
_RUNS = {}


def bound(name, key, q=None):
    q = REC[name]["order"] if q is None else q
    return max(MARGIN * REC[name][key], q * EPS)


def tri_args(args):
    return {k: v for k, v in args.items() if k != "deflate"}          # (the reduction does not see deflate)


def measure_device(S, r, keep):
    """every figure of a probe result r for the input S; with keep the arrays stay attached"""
    q, j = r.q, r.jdim
    fig = dict(jdim=j, nref=r.nref, snorm=r.snorm, snorm_err=abs(r.snorm - np.linalg.norm(S)) / max(np.linalg.norm(S), np.finfo(float).tiny))
    V, tau = r.V, r.tau
    fig["tau0"] = int(np.sum(tau[:r.nref] == 0.0))
    fig["tau_tail_zero"] = bool((tau[r.nref:] == 0.0).all())
    fig["v_cols_zero"] = bool(not V[:, r.nref:].any())                                   # no reflector from nref on
    fig["v_upper_zero"] = bool(not np.triu(V[:, :r.nref]).any())                         # zero on and above the diagonal ...
    idx = np.arange(r.nref)
    fig["v_unit"] = bool((V[idx + 1, idx] == 1.0).all()) if r.nref else True            # ... and the unit entry just below it
    Q = M.orthogonal_factor(V, tau, r.nref, j)
    fig["a1"], fig["a2"], fig["a3"] = M.stage_a(S, Q, r.d, r.e)
    fig["shapes"] = (r.d.shape, r.e.shape, r.tau.shape, V.shape, None if r.Z is None else r.Z.shape, None if r.w is None else r.w.shape,
                     None if r.B is None else r.B.shape)
    if r.Z is not None:
        fig["b1"], fig["b2"], fig["b3"] = M.stage_b(r.d, r.e, r.w, r.Z)
        fig["c"] = M.stage_c(r.B, Q, r.Z)
    out = dict(fig=fig, w=r.w)
    if keep:
        out.update(r=r, Q=Q)
    return out


def run(ctx, name):
    """the device's run of a named case (once per session): probe with every column back-transformed"""
    if name not in _RUNS:
        build, kw = CASES[name]
        S = build()
        args = M.solver_args(S, kw)
        q = S.shape[0]
        t0 = time.perf_counter()
        r = P.probe(ctx, S, ids="all", **args)
        ms = (time.perf_counter() - t0) * 1e3
        out = measure_device(S, r, q <= KEEP_ARRAYS_MAX)
        out.update(S=S, args=args, q=q, ms=ms, normF=float(np.linalg.norm(S)))
        f = out["fig"]
        print(f"{name}: q {q} jdim {f['jdim']} nref {f['nref']} tau0 {f['tau0']}; probe with upload and download {ms:.0f} ms; " +
              " ".join(f"{k} {f[k]:.2e} (model {REC[name][k]:.2e})" for k in ("a1", "a2", "a3", "b1", "b2", "b3", "c") if k in f))
        _RUNS[name] = out
    return _RUNS[name]


QL_CASES = [f"{kind}{q}" for q in M.QL_ORDERS for kind in ("dense", "spectrum")]
BLOCKTRI_CASES = [f"blocktri{q}" for q in M.BLOCKTRI]
LOWRANK_CASES = [f"lowrank{q}_r{r}" for q, r in M.LOW_RANK]
STOP_CASES = ["abs_tol", "floor_wins", "floor_loses", "abs_tol_coarse", "floor_coarse", "stop_edge", "stop_edge2", "padded9"]
HARD_CASES = [f"{k}{q}" for q in M.HARD_ORDERS for k in M.HARD]
DEFLATE_CASES = [f"dense{q}_deflate{v}" for q in (100, 160) for v in ("1", "1e-3")]
ALL_CASES = QL_CASES + BLOCKTRI_CASES + LOWRANK_CASES + STOP_CASES + HARD_CASES + DEFLATE_CASES
TRUE_RANK = {"padded9": 5, "rank364": 3, "rank3160": 3, "floor_loses": 20,
             **{f"lowrank{q}_r{r}": r for q, r in M.LOW_RANK}}


def test_the_case_list_is_the_record():
    assert set(ALL_CASES) | {"zero1", "zero6"} == set(CASES) == set(REC)


# ---- stage A: k_tridiag ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES)
def test_stage_a_tridiagonalisation(ctx, name):
    R, rec = run(ctx, name), REC[name]
    f, q = R["fig"], R["q"]
    j = f["jdim"]
    assert f["shapes"][:4] == ((j,), (max(j - 1, 0),), (q,), (q, q))
    assert f["snorm_err"] <= q * EPS
    assert f["a1"] <= bound(name, "a1") and f["a2"] <= bound(name, "a2")
    # what the early stop drops is ||S22||_F^2 + 2 e_(j-1)^2 <= tol^2 by construction, on top of the reduction's own error
    tol = M.stop_tol(f["snorm"], R["args"].get("tolfac", 4.0), R["args"].get("abs_tol", -1.0), R["args"].get("floor_mode", 0))
    assert f["a3"] <= (tol / R["normF"] if j < q else 0.0) + bound(name, "a1")
    # untouched regions of V and tau, the unit entries
    assert f["tau_tail_zero"] and f["v_cols_zero"] and f["v_upper_zero"] and f["v_unit"]
    # jdim and nref: the model's window (stop rule at 4 tolfac and at tolfac / 4), at least the true rank
    if "jdim_loose" in rec:
        lo, hi = rec["jdim_loose"], rec["jdim_tight"]
    elif rec["jdim"] == q:
        lo = hi = q
    else:
        S, a = R["S"], tri_args(R["args"])
        tf = a.pop("tolfac", 4.0)
        lo, hi = M.tridiag(S, 4.0 * tf, want_v=False, **a)["jdim"], M.tridiag(S, tf / 4.0, want_v=False, **a)["jdim"]
    assert hi - lo <= M.window_width_max(name) and lo <= j <= hi and j >= TRUE_RANK.get(name, 0), (lo, j, hi)
    assert f["nref"] == (q - 1 if j == q else j)          # (j == q: the `j == q - 1` exit, no reflector for the last column)
    if j == rec["jdim"]:
        assert f["tau0"] == rec["tau0"]          # tau == 0 exactly where the model has it (positions: below, for the orders the model repeats live)
    if q <= M.HOST_MAX_ORDER and j == rec["jdim"]:
        m = M.tridiag(R["S"], want_v=False, **tri_args(R["args"]))
        assert np.array_equal(m["tau"] == 0.0, R["r"].tau == 0.0)


def test_already_tridiagonal_input_takes_the_tau_zero_path_everywhere(ctx):
    for name in BLOCKTRI_CASES + ["wilkinson64", "wilkinson160", "diagonal64", "diagonal160"]:
        R = run(ctx, name)
        q = R["q"]
        assert R["fig"]["jdim"] == q and R["fig"]["nref"] == q - 1 and R["fig"]["tau0"] == q - 1, name
        if "r" in R:          # no reflector does anything: T is the input, Q the identity, the back-transformation copies Z
            r, S = R["r"], R["S"]
            assert np.array_equal(r.d, np.diag(S)) and np.array_equal(r.e, np.diag(S, -1)) and np.array_equal(r.B, r.Z), name


# ---- stage B: the three QL variants ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES)
def test_stage_b_ql(ctx, name):
    R = run(ctx, name)
    f = R["fig"]
    j = f["jdim"]
    assert f["shapes"][4:6] == ((j, j), (j,))
    assert f["b1"] <= bound(name, "b1") and f["b2"] <= bound(name, "b2") and f["b3"] <= bound(name, "b3")


def test_every_ql_variant_and_slab_height_has_run(ctx):
    """names the path of every row of the table: the variant and the slab height follow from jdim alone (sym_eig), and the record shows that the
    sweeps of each order have lengths of every residue mod 16, below 8 and from 9 to 15 (the read-ahead edges of k_tql_replay)"""
    want = {1: ("lds", 0), 2: ("lds", 0), 3: ("lds", 0), 63: ("lds", 0), 65: ("lds", 0), 127: ("lds", 0), 128: ("lds", 0), 129: ("replay", 64),
            300: ("replay", 64), 301: ("replay", 32), 600: ("replay", 32), 601: ("replay", 16), 1200: ("replay", 16), 1201: ("replay", 8),
            2048: ("replay", 8), 2049: ("global", 0), 2600: ("global", 0)}
    seen = {}
    for name in QL_CASES + BLOCKTRI_CASES:
        j = run(ctx, name)["fig"]["jdim"]
        assert j == REC[name]["order"], name          # nothing stopped early: the QL stage ran at the order of the input
        seen[j] = ("lds", 0) if j <= M.LDS_QL_MAX else ("replay", M.slab_rows(j)) if j <= M.REPLAY_MAX else ("global", 0)
        if j >= 63 and name in QL_CASES:
            rec = REC[name]
            assert rec["residues"] == list(range(16)) and rec["below8"] > 0 and rec["from9to15"] > 0, name
    assert seen == want


# ---- stage C: k_backtransform ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES)
def test_stage_c_backtransformation_of_every_column(ctx, name):
    R = run(ctx, name)
    f = R["fig"]
    assert f["shapes"][6] == (R["q"], f["jdim"])
    assert f["c"] <= bound(name, "c")


STAGE_C_CASES = ("dense3", "dense65", "dense129", "graded_alt160", "rank3160", "lowrank1000_r20", "wilkinson160")


@pytest.mark.parametrize("name", STAGE_C_CASES)
def test_stage_c_subsets_of_columns_and_the_pure_reflector_form(ctx, name):
    """one column, five in descending order, 4k + 1, 4k + 2 and 4k + 3 columns (one wave per column, four per workgroup), repeats; with
    want_eig = False the unit vectors take the place of Z's columns: B = Q_j(:, ids)"""
    R = run(ctx, name)
    r, Q, j, q = R["r"], R["Q"], R["fig"]["jdim"], R["q"]
    rng = np.random.default_rng(j)
    lists = [[j - 1], list(range(j - 1, -1, -1))[:5], list(rng.integers(0, j, 4 * min(j // 4, 3) + 1)), list(range(min(j, 6))),
             list(rng.permutation(j)[:min(j, 7)])]
    for ids in lists:
        ids = np.asarray(ids)
        r2 = P.probe(ctx, R["S"], ids=ids, want_v=False, **R["args"])
        assert r2.B.shape == (q, len(ids))
        assert np.array_equal(r2.Z, r.Z) and np.array_equal(r2.tau, r.tau)          # same run: the columns can be compared with the first call's
        assert np.array_equal(r2.B, r.B[:, ids]), ids          # a column does not depend on its place in the list
        assert M.stage_c(r2.B, Q, r.Z[:, ids]) <= bound(name, "c")
        r3 = P.probe(ctx, R["S"], want_eig=False, ids=ids, want_v=False, **R["args"])
        assert r3.Z is None and r3.w is None and r3.jdim == j
        # both sides apply the same reflectors to unit vectors, one in float64: rounding of the size of the orthogonality figure a2
        assert float(np.linalg.norm((r3.B.astype(Q.dtype) - Q[:, ids]).astype(float))) <= bound(name, "a2")


# ---- end to end: the public dre_sym_eig -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL_CASES)
def test_public_entry_end_to_end(ctx, name):
    R, rec = run(ctx, name), REC[name]
    S, q = R["S"], R["q"]
    if R["args"].get("abs_tol", -1.0) > 0 or R["args"].get("floor_mode", 0) or R["args"].get("deflate", 1e-3) != 1e-3:
        # (the public entry has tolfac only: the other arguments go through the probe, sorted here as the public entry sorts)
        r = R["r"]
        assert r.B is not None
        order = np.argsort(r.w, kind="stable")
        w, U = r.w[order], r.B[:, order]
    else:
        w, U = P.public(ctx, S)
    j = len(w)
    assert U.shape == (q, j) and j == R["fig"]["jdim"] and (np.diff(w) >= 0).all()
    e1, e2, e3 = M.end_to_end(S, w, U)
    print(f"{name}: eig {e1:.2e} (model {rec['eig_err']:.2e}) residual {e2:.2e} (model {rec['residual']:.2e}) orth {e3:.2e} (model {rec['orth']:.2e})")
    if j == rec["jdim"] or j == q:
        assert e1 <= bound(name, "eig_err") and e2 <= bound(name, "residual") and e3 <= bound(name, "orth")
    else:          # (the model stopped at another j inside the window: what it dropped is below tol either way)
        tol = M.stop_tol(R["fig"]["snorm"], 4.0) / R["normF"]
        assert e1 <= tol + bound(name, "eig_err") and e2 <= tol + bound(name, "residual") and e3 <= bound(name, "orth")
    if name in TRUE_RANK and name.startswith("lowrank"):
        # reference eigenvalues from the r x r problem (B has orthonormal columns: they are lambda); the kept ones lie above a threshold in
        # a gap of more than four decades, two on either side (tests/test_sym_ql_host.py): |lambda_r| = 0.5^(r-1) >= 1.9e-6 above, the bound below.
        # Weyl: eigenvalues move by at most ||U diag(w) U' - S||_2 (<= e1 ||S||_F) plus the loss of orthogonality times ||S||_2
        lam = M.low_rank_spectrum(TRUE_RANK[name])
        keep = np.abs(w) > 1e-10 * np.abs(w).max()
        assert int(keep.sum()) == len(lam)
        assert np.abs(w[keep] - np.sort(lam)).max() <= (bound(name, "eig_err") + bound(name, "orth")) * R["normF"]
    if name in ("rank364", "rank3160"):
        assert int((np.abs(w) > 1e-10 * np.abs(w).max()).sum()) == 3          # (three eigenvalues of order one, the rest rounding noise)


# ---- the stop rule ---------------------------------------------------------------------------------------------------------------------------
def test_stop_rule_three_ways_to_form_the_tolerance(ctx):
    base, a0, fw, fl, ac, fc = (run(ctx, n) for n in ("lowrank1000_r20", "abs_tol", "floor_wins", "floor_loses", "abs_tol_coarse", "floor_coarse"))
    # the floor loses against tolfac eps ||S||: the run is the default run, bit for bit; it wins: the run with abs_tol alone
    for k in ("d", "e", "tau", "V", "w", "Z", "B"):
        assert np.array_equal(getattr(fl["r"], k), getattr(base["r"], k)), k
        assert np.array_equal(getattr(fw["r"], k), getattr(a0["r"], k)), k
        assert np.array_equal(getattr(fc["r"], k), getattr(ac["r"], k)), k
    # |lambda_k| = 0.5^k: 1e-6 ||S||_F stops no later than 4 eps ||S||_F, 1e-3 ||S||_F ten columns earlier (the window of each is checked in stage A)
    assert a0["fig"]["jdim"] <= base["fig"]["jdim"] and 10 <= ac["fig"]["jdim"] <= base["fig"]["jdim"] - 5
    # and what it drops is what it was allowed to drop, not less by orders of magnitude: the coarse run really stopped at 1e-3 ||S||_F
    assert 1e-5 <= ac["fig"]["a3"] <= 1e-3 + bound("abs_tol_coarse", "a1")


def test_without_eigenvectors_the_reduction_is_the_same_bits(ctx):
    R = run(ctx, "lowrank1000_r20")
    r0 = P.probe(ctx, R["S"], want_eig=False)
    r = R["r"]
    assert r0.Z is None and r0.w is None and r0.B is None
    assert (r0.jdim, r0.nref, r0.snorm) == (r.jdim, r.nref, r.snorm)
    assert np.array_equal(r0.d, r.d) and np.array_equal(r0.e, r.e) and np.array_equal(r0.tau, r.tau) and np.array_equal(r0.V, r.V)


def test_stop_rule_counts_the_coupling_entry_twice(ctx):
    """tol^2 lies between ||S22||^2 + e^2 and ||S22||^2 + 2 e^2 at one j: the reduction must go on there (the dropped part of
    S - Q_j T_j Q_j' holds e twice)"""
    for name, j in (("stop_edge", 11), ("stop_edge2", 2)):
        assert REC[name]["jdim"] == REC[name]["jdim_loose"] == REC[name]["jdim_tight"] == j
        assert run(ctx, name)["fig"]["jdim"] == j, name


@pytest.mark.parametrize("q", [1, 6])
def test_zero_matrix_gives_nothing(ctx, q):
    r = P.probe(ctx, np.zeros((q, q)))
    assert (r.jdim, r.nref, r.snorm) == (0, 0, 0.0) and REC[f"zero{q}"]["jdim"] == 0
    assert r.d.shape == (0,) and r.e.shape == (0,) and r.w is None and r.Z is None and r.B is None
    assert r.V.shape == (q, q) and not r.V.any() and not r.tau.any()
    w, U = P.public(ctx, np.zeros((q, q)))
    assert w.shape == (0,) and U.shape == (q, 0)


@pytest.mark.parametrize("q", [2, 65])
def test_last_column_exit(ctx, q):
    R = run(ctx, f"dense{q}")
    r = R["r"]
    assert (r.jdim, r.nref) == (q, q - 1) and r.tau[q - 1] == 0.0
    # the last diagonal entry is read from the reduced matrix, not computed: Q'SQ has it at (q - 1, q - 1) within the bound of a1
    Q = R["Q"]
    t = float((Q[:, -1] @ R["S"].astype(Q.dtype) @ Q[:, -1]))
    assert abs(t - r.d[-1]) <= bound(f"dense{q}", "a1") * R["normF"]


# ---- deflate, scaling, determinism -------------------------------------------------------------------------------------------------------------
def test_deflate_is_ignored_up_to_128_and_honoured_above(ctx):
    a, b = run(ctx, "dense100_deflate1"), run(ctx, "dense100_deflate1e-3")
    for k in ("d", "e", "tau", "V", "w", "Z", "B"):          # k_tql<true> has its constant built in: documented behaviour
        assert np.array_equal(getattr(a["r"], k), getattr(b["r"], k)), k
    a, b = run(ctx, "dense160_deflate1"), run(ctx, "dense160_deflate1e-3")
    assert np.array_equal(a["r"].d, b["r"].d) and np.array_equal(a["r"].e, b["r"].e)          # (the same T: only the QL stage sees deflate)
    for R, name in ((a, "dense160_deflate1"), (b, "dense160_deflate1e-3")):
        assert R["fig"]["b1"] <= bound(name, "b1") and R["fig"]["b2"] <= bound(name, "b2") and R["fig"]["b3"] <= bound(name, "b3")


@pytest.mark.parametrize("q", [100, 160])
@pytest.mark.parametrize("k", [200, -200])
def test_scaling_by_a_power_of_two(ctx, q, k):
    """every operation of k_tridiag commutes with 2^k in this range, and so do sqrt and division in the host generator (j > 128);
    k_tql<true> uses rsqrt, which need not: there the bounds of the unscaled case apply"""
    name = f"dense{q}_deflate1e-3"
    R = run(ctx, name)
    r, s = R["r"], 2.0 ** k
    r2 = P.probe(ctx, R["S"] * s, ids="all")
    assert (r2.jdim, r2.nref) == (r.jdim, r.nref) and r2.snorm == r.snorm * s
    assert np.array_equal(r2.tau, r.tau) and np.array_equal(r2.V, r.V) and np.array_equal(r2.d, r.d * s) and np.array_equal(r2.e, r.e * s)
    if q > M.LDS_QL_MAX:
        assert np.array_equal(r2.Z, r.Z) and np.array_equal(r2.w, r.w * s) and np.array_equal(r2.B, r.B)
    else:
        b1, b2, b3 = M.stage_b(r2.d, r2.e, r2.w, r2.Z)
        assert b1 <= bound(name, "b1") and b2 <= bound(name, "b2") and b3 <= bound(name, "b3")
        assert M.stage_c(r2.B, R["Q"], r2.Z) <= bound(name, "c")


@pytest.mark.parametrize("name", ["dense100_deflate1e-3", "dense129", "graded_alt160"])
def test_determinism(ctx, name):
    R = run(ctx, name)
    r = R["r"]
    r2 = P.probe(ctx, R["S"], ids="all", **R["args"])
    assert (r2.jdim, r2.nref, r2.snorm) == (r.jdim, r.nref, r.snorm)
    for k in ("d", "e", "tau", "V", "w", "Z", "B"):
        assert np.array_equal(getattr(r2, k), getattr(r, k)), k
    w, U = P.public(ctx, R["S"])
    order = np.argsort(r.w, kind="stable")
    assert np.array_equal(w, r.w[order]) and np.array_equal(U, r.B[:, order])          # the public entry is the same chain, sorted


# ---- what is refused ---------------------------------------------------------------------------------------------------------------------------
def _refused(ctx, call, *words):
    with pytest.raises(D.DREError) as e:
        call()
    assert e.value.code == P.ERR_INVALID
    for w in words:
        assert w in str(e.value), str(e.value)


def _still_works(ctx):
    R = run(ctx, "dense65")
    r = P.probe(ctx, R["S"], ids=np.arange(65))
    assert np.array_equal(r.B, R["r"].B)
    w, U = P.public(ctx, R["S"])
    e1, e2, e3 = M.end_to_end(R["S"], w, U)
    assert e1 <= bound("dense65", "eig_err") and e2 <= bound("dense65", "residual") and e3 <= bound("dense65", "orth")


def test_argument_validation(ctx):
    S = run(ctx, "dense65")["S"]
    _refused(ctx, lambda: P.probe(ctx, np.zeros((4, 5))), "dre_sym_eig_probe", "square")
    _refused(ctx, lambda: P.probe(ctx, S, ids=[65]), "ids")
    _refused(ctx, lambda: P.probe(ctx, S, ids=[0, -1]), "ids")
    _refused(ctx, lambda: P.probe(ctx, run(ctx, "rank364")["S"], ids=[10]), "ids")          # inside [0, q) but not inside [0, jdim)
    _refused(ctx, lambda: P.probe(ctx, S, tolfac=0.0), "tolfac")
    _still_works(ctx)


def test_order_above_8192_is_refused_before_any_launch(ctx):
    Sd = ctx.zeros(8193, 8193)
    ctx.prof_reset()
    ctx.prof_enable(True)
    try:
        _refused(ctx, lambda: P.probe(ctx, Sd), "8192")
        launched = {k: v for k, v in ctx.prof_stats().items() if v["launches"]}
    finally:
        ctx.prof_enable(False)
    assert not launched, launched
    _still_works(ctx)


@pytest.mark.parametrize("kind", ["nan_off_diagonal", "inf_on_diagonal", "squares_overflow"])
def test_non_finite_input_is_a_clean_invalid(ctx, kind):
    """sym_eig reads ||S||_F back right after the reduction and refuses a non-finite value before any QL launch (and before the public entry
    sorts eigenvalues that may be NaN); finite entries whose squares overflow count as non-finite.  Error codes: nothing faults."""
    S = M.dense(65).copy()
    if kind == "nan_off_diagonal":
        S[7, 40] = S[40, 7] = np.nan
    elif kind == "inf_on_diagonal":
        S[12, 12] = np.inf
    else:
        S *= 1e200
        assert np.isfinite(S).all()
    _refused(ctx, lambda: P.probe(ctx, S), "sym_eig", "non-finite")
    _refused(ctx, lambda: P.public(ctx, S), "sym_eig", "non-finite")
    _still_works(ctx)
