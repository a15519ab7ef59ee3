"""Host checks of the dense generalized Sylvester solver (no GPU): the NumPy model tests/_sylvester_model.py against SciPy and against its
record tests/golden/sylvester_model.json, the decision rule csrc/sylvester_decide.hpp compiled with g++ into a stand-alone program, the
failure cases on the model, the H2 formula against the Gramian of the error system, and the Python argument checks, which raise before a
context is needed."""
import os
import subprocess

import numpy as np
import pytest
import scipy.linalg as sla

import dre_amd as D
import _sylvester_model as sm
from conftest import ROOT

EPS = np.finfo(float).eps
LD = np.longdouble
CSRC = os.path.join(ROOT, "differentialriccatiequations.jl_amd", "csrc")
REC = sm.recorded()


def _same_size(live, rec, k, keys):
    for key in keys:
        assert live[key] <= 3 * rec[key] + k * EPS and rec[key] <= 3 * live[key] + k * EPS, (key, live[key], rec[key])


@pytest.mark.parametrize("n,m", sm.SIZES)
def test_model_against_scipy_and_the_record(n, m):
    E, A, F, B, C, C2 = sm.system(n, m)
    assert not np.array_equal(E, np.eye(n)) and not np.array_equal(F, np.eye(m)) and (n == 1 or not np.array_equal(E, E.T)) and (m == 1 or not np.array_equal(F, F.T))
    live, rec = sm.record_size(n, m), REC["sizes"][sm.key(n, m)]
    k, target = max(n, m), sm.refine_target(n, m)
    print((n, m), live)
    # the two pencils are c-stable with different spectral abscissae
    aL, aR = sla.eigvals(A, E).real.max(), sla.eigvals(B, F).real.max()
    assert aL <= -sm.ALPHA_LEFT + 1e-9 and aR <= -sm.ALPHA_RIGHT + 1e-9
    # the residuals, in double and in extended precision, hold the solver's own target with room; SciPy's standard form agrees
    for key in ("res", "res_ext", "res_t", "res_t_ext", "res2_ext"):
        assert live[key] <= target / 10, key
    for key in ("x_err", "y_err", "x2_err", "t_err"):
        assert live[key] <= 100 * k * EPS, key
    assert 2 <= live["iters"] <= 8 and live["replay_equal"]
    # ... and the record is this run's
    for key in ("iters", "refinements", "refinements_t", "replay_equal"):
        assert live[key] == rec[key], key
    _same_size(live, rec, k, ("res", "res_ext", "res_t", "res_t_ext", "res2_ext", "x_err", "y_err", "x2_err", "t_err"))


@pytest.mark.parametrize("n", (sm.H2_GPU_N, sm.STEEL_N))
def test_lyapunov_tie_on_the_model(n):
    """GSYLEProblem(E, A, E', A', R) with a symmetric R is the Lyapunov equation A X E' + E X A' = -R: X is symmetric to rounding"""
    live, rec = sm.record_lyapunov(n), REC["lyapunov"][str(n)]
    print(n, live)
    assert live["iters"] == rec["iters"]
    assert live["asym"] <= n * EPS
    _same_size(live, rec, n, ("x_err",))
    assert live["x_err"] <= (1e-10 if n == sm.STEEL_N else 100 * n * EPS)


def test_failure_cases_on_the_model():
    for name, (ops, (exc, side)) in sm.failure_cases().items():
        with pytest.raises(exc) as e:
            sm.solve(*ops)
        print(name, "->", e.value)
        if side is not None:
            assert e.value.side == side and sm.SIDE_NAMES[side] in str(e.value)
        assert sm.run_failure(name) == REC["failures"][name], name
    # a singular F is refused by name, before the iteration
    with pytest.raises(sm.Singular, match="F is singular"):
        sm.solve(*sm.failure_cases()["singular_F"][0])
    # the kept factorisation refuses the non-finite right-hand side in both directions
    E, A, F, B, Cn = sm.failure_cases()["non_finite_C"][0]
    s = sm.SignSylvester(E, F)
    s.factor(A, B)
    for transposed in (False, True):
        with pytest.raises(sm.NonFiniteRhs):
            s.solve(Cn, transposed)
    # C = 0 returns X = 0 exactly
    for transposed in (False, True):
        X, info = sm.solve(E, A, F, B, np.zeros((12, 5)), transposed)
        assert np.array_equal(X, np.zeros((12, 5))) and info["res"] == 0.0 and info["refinements"] == 0
    # running out of iterations names a side too
    with pytest.raises(sm.NotStable) as e:
        sm.solve(E, A, F, B, np.ones((12, 5)), maxiters=2)
    assert e.value.done == sm.OUT_OF_ITERS and e.value.side in (sm.SIDE_LEFT, sm.SIDE_RIGHT)


def test_h2_formula_on_the_model():
    """err^2 = ||H||^2 - 2 <H, H_r> + ||H_r||^2 against tr(C_e P_e C_e') of the block-diagonal error system (n = 60, r = 6, m = 2, q = 3)"""
    full, rom = sm.h2_case("model")
    assert (full[0].shape[0], rom[1].shape[0], full[2].shape[1], full[3].shape[0]) == tuple(sm.H2_SIZES[k] for k in ("n", "r", "m", "q"))
    live = sm.h2_error(full, rom)
    ref2, refn2 = sm.h2_reference(full, rom), sm.h2_reference(full)
    rec = REC["h2"]["model"]
    print(live, ref2, refn2, rec)
    assert abs(live["norm2"] - refn2) <= 100 * 60 * EPS * refn2
    # the formula cancels: its accuracy is relative to ||H||^2 + ||H_r||^2, not to err^2
    assert abs(live["err2"] - ref2) <= 100 * live["floor"]
    assert live["err"] == np.sqrt(live["err2"]) and live["floor"] == EPS * (live["norm2"] + live["norm2_r"])
    assert abs(live["err2"] - ref2) <= 3 * rec["err2_diff"] + live["floor"] and rec["floor"] == pytest.approx(live["floor"], rel=1e-9)
    # the system as its own reduced model: err^2 at the floor
    own = sm.h2_error(full, full)
    assert abs(own["err2"]) <= 10 * own["floor"] and own["err"] <= np.sqrt(10 * own["floor"])
    for name in ("gpu", "steel"):
        live_n, rec_n = sm.record_h2(name), REC["h2"][name]
        print(name, live_n)
        assert live_n["norm2"] == pytest.approx(rec_n["norm2"], rel=1e-9) and live_n["err2_ref"] == pytest.approx(rec_n["err2_ref"], rel=1e-6)
        assert live_n["err2_diff"] <= 3 * rec_n["err2_diff"] + 10 * live_n["floor"]


DECIDE_SRC = r"""
#include <cstdio>
#include <limits>
#include "sylvester_decide.hpp"

using namespace dre;

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double tol = 1e-13;
    // eA eB dA dB dC singular_left singular_right
    const double cases[][7] = {
        {1e-14, 1e-15, 1e-9, 1e-9, 1e-9, 0, 0},      // converged
        {1e-13, 1e-13, 0.0, 0.0, 0.5, 0, 0},         // converged at tol exactly; the step of C does not decide
        {1e-14, 1e-3, 1e-9, 0.1, 1e-9, 0, 0},        // the right side still runs
        {1e-3, 1e-14, 0.1, 1e-9, 1e-9, 0, 0},        // the left side still runs
        {0.5, 1e-14, 1e-9, 1e-9, 1e-9, 0, 0},        // the left side stagnates
        {1e-14, 0.5, 1e-9, 1e-9, 1e-9, 0, 0},        // the right side stagnates
        {0.5, 0.5, 1e-9, 1e-9, 1e-9, 0, 0},          // both stagnate: the left is named
        {0.5, 0.5, 1e-8, 2e-8, 1e-9, 0, 0},          // a step at STAG_STEP stagnates, one above it runs on
        {2e-4, 1e-4, 1e-9, 1e-9, 0.0, 0, 0},         // a distance at STAG_DIST does not stagnate, one above it does
        {1e-4, 1e-4, 1e-9, 1e-9, 0.0, 0, 0},         // small steps close to the limit: running
        {0.5, 0.5, 0.5, 0.5, 0.5, 1, 0},             // singular A_k
        {0.5, 0.5, 0.5, 0.5, 0.5, 0, 1},             // singular B_k
        {nan, nan, nan, nan, nan, 1, 1},             // both singular: the left is named, before anything else
        {nan, 0.5, 0.5, 0.5, 0.5, 0, 0},             // non-finite on the left
        {0.5, 0.5, inf, 0.5, 0.5, 0, 0},
        {0.5, inf, 0.5, 0.5, 0.5, 0, 0},             // non-finite on the right
        {0.5, 0.5, 0.5, nan, 0.5, 0, 0},
        {1e-14, 1e-14, 1e-9, 1e-9, nan, 0, 0},       // only the step of C: the right-hand side, even on converged pencils
        {nan, nan, 0.5, 0.5, nan, 0, 0},             // everything: the left is named
    };
    for (const auto& c : cases) {
        const SylvDecision d = sylvester_decide(c[0], c[1], c[2], c[3], c[4], (int)c[5], (int)c[6], tol);
        std::printf("%d %d\n", d.done, d.side);
    }
    std::printf("tol %.17g %.17g %.17g %.17g\n", sylvester_default_tol(33, 1, 0.0), sylvester_default_tol(7, 130, -1.0), sylvester_default_tol(7, 130, 1e-3),
                sylvester_refine_target(257, 40));
    std::printf("step %.17g %.17g %.17g\n", sylvester_rel_step(0.0, 0.0), sylvester_rel_step(1.0, 4.0), sylvester_rel_step(0.0, 4.0));
    std::printf("consts %.17g %.17g %d %d %d %d %d %d\n", SYLV_STAG_STEP, SYLV_STAG_DIST, SYLV_RUNNING, SYLV_CONVERGED, SYLV_STAGNATED, SYLV_NON_FINITE,
                SYLV_SINGULAR, SYLV_OUT_OF_ITERS);
    return 0;
}
"""
DECIDE_CASES = [
    ((1e-14, 1e-15, 1e-9, 1e-9, 1e-9, 0, 0), (sm.CONVERGED, sm.SIDE_NONE)),
    ((1e-13, 1e-13, 0.0, 0.0, 0.5, 0, 0), (sm.CONVERGED, sm.SIDE_NONE)),
    ((1e-14, 1e-3, 1e-9, 0.1, 1e-9, 0, 0), (sm.RUNNING, sm.SIDE_NONE)),
    ((1e-3, 1e-14, 0.1, 1e-9, 1e-9, 0, 0), (sm.RUNNING, sm.SIDE_NONE)),
    ((0.5, 1e-14, 1e-9, 1e-9, 1e-9, 0, 0), (sm.STAGNATED, sm.SIDE_LEFT)),
    ((1e-14, 0.5, 1e-9, 1e-9, 1e-9, 0, 0), (sm.STAGNATED, sm.SIDE_RIGHT)),
    ((0.5, 0.5, 1e-9, 1e-9, 1e-9, 0, 0), (sm.STAGNATED, sm.SIDE_LEFT)),
    ((0.5, 0.5, 1e-8, 2e-8, 1e-9, 0, 0), (sm.STAGNATED, sm.SIDE_LEFT)),
    ((2e-4, 1e-4, 1e-9, 1e-9, 0.0, 0, 0), (sm.STAGNATED, sm.SIDE_LEFT)),
    ((1e-4, 1e-4, 1e-9, 1e-9, 0.0, 0, 0), (sm.RUNNING, sm.SIDE_NONE)),
    ((0.5, 0.5, 0.5, 0.5, 0.5, 1, 0), (sm.SINGULAR, sm.SIDE_LEFT)),
    ((0.5, 0.5, 0.5, 0.5, 0.5, 0, 1), (sm.SINGULAR, sm.SIDE_RIGHT)),
    ((np.nan, np.nan, np.nan, np.nan, np.nan, 1, 1), (sm.SINGULAR, sm.SIDE_LEFT)),
    ((np.nan, 0.5, 0.5, 0.5, 0.5, 0, 0), (sm.NON_FINITE, sm.SIDE_LEFT)),
    ((0.5, 0.5, np.inf, 0.5, 0.5, 0, 0), (sm.NON_FINITE, sm.SIDE_LEFT)),
    ((0.5, np.inf, 0.5, 0.5, 0.5, 0, 0), (sm.NON_FINITE, sm.SIDE_RIGHT)),
    ((0.5, 0.5, 0.5, np.nan, 0.5, 0, 0), (sm.NON_FINITE, sm.SIDE_RIGHT)),
    ((1e-14, 1e-14, 1e-9, 1e-9, np.nan, 0, 0), (sm.NON_FINITE, sm.SIDE_RHS)),
    ((np.nan, np.nan, 0.5, 0.5, np.nan, 0, 0), (sm.NON_FINITE, sm.SIDE_LEFT)),
]


def test_decision_header_stand_alone(tmp_path):
    """csrc/sylvester_decide.hpp without HIP on a table of cases (converged, each side stagnating, each side singular, non-finite, the default
    tolerance): every row is pinned, and the model's decide gives the same"""
    cpp = tmp_path / "decide.cpp"
    cpp.write_text(DECIDE_SRC)
    exe = tmp_path / "decide"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(cpp), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    assert len(lines) == len(DECIDE_CASES) + 3, r.stdout
    for ln, (args, want) in zip(lines, DECIDE_CASES):
        got = tuple(int(v) for v in ln.split())
        model = sm.decide(*args[:5], bool(args[5]), bool(args[6]), 1e-13)
        assert got == want == model, (args, got, want, model)
    tol = [float(v) for v in lines[-3].split()[1:]]
    assert tol == [sm.default_tol(33, 1, None), sm.default_tol(7, 130, -1.0), 1e-3, sm.refine_target(257, 40)]
    assert tol[0] == 10 * 33 * EPS and tol[1] == 10 * 130 * EPS and tol[3] == 100 * 257 * EPS
    assert [float(v) for v in lines[-2].split()[1:]] == [0.0, 0.5, 0.0] == [sm.rel_step(0.0, 0.0), sm.rel_step(1.0, 4.0), sm.rel_step(0.0, 4.0)]
    consts = lines[-1].split()[1:]
    assert [float(v) for v in consts[:2]] == [sm.STAG_STEP, sm.STAG_DIST]
    assert [int(v) for v in consts[2:]] == [sm.RUNNING, sm.CONVERGED, sm.STAGNATED, sm.NON_FINITE, sm.SINGULAR, sm.OUT_OF_ITERS]
    # the header's constants are the Lyapunov solver's
    body = open(os.path.join(CSRC, "dense_sign_body.hpp")).read()
    assert "STAG_STEP = 1e-8;" in body and "STAG_DIST = 1e-4;" in body and "SCALE_OFF = 1e-2;" in body
    assert (sm.SCALE_OFF, sm.STAG_STEP, sm.STAG_DIST) == (1e-2, 1e-8, 1e-4)


def test_python_argument_checks_raise_before_a_context_is_needed():
    I2, I3 = np.eye(2), np.eye(3)
    C23 = np.ones((2, 3))
    good = D.GSYLEProblem(I2, -I2, I3, -I3, C23)
    Bm, Cm = np.ones((2, 1)), np.ones((1, 2))
    rom = D.ReducedModel(np.eye(1), -np.eye(1), np.ones((1, 1)), np.ones((1, 1)), np.ones(2), np.ones((2, 1)), np.ones((2, 1)))
    bad_calls = [
        (TypeError, lambda: D.solve(good, D.Doubling())),
        (TypeError, lambda: D.solve(good, D.FactoredSign())),
        (TypeError, lambda: D.solve_gsyle_dense(D.GALEProblem(I2, I2, I2), D.MatrixSign())),
        (TypeError, lambda: D.solve(good, D.MatrixSign(), transposed=1)),
        (ValueError, lambda: D.solve(good, D.MatrixSign(maxiters=0))),
        (ValueError, lambda: D.solve(good, D.MatrixSign(max_refine=-1))),
        (ValueError, lambda: D.solve(D.GSYLEProblem(I2, -I2, I3, -I3, C23.T), D.MatrixSign())),
        (ValueError, lambda: D.solve(D.GSYLEProblem(I3, -I2, I3, -I3, C23), D.MatrixSign())),
        (ValueError, lambda: D.solve(D.GSYLEProblem(I2, -I2, I2, -I3, C23), D.MatrixSign())),
        (ValueError, lambda: D.solve(D.GSYLEProblem(None, np.ones((2, 3)), None, -I3, C23), D.MatrixSign())),
        (ValueError, lambda: D.solve(D.GSYLEProblem(None, -I2, None, np.ones(3), C23), D.MatrixSign())),
        (ValueError, lambda: D.gsyle_residual_dense(good, C23.T)),
        (TypeError, lambda: D.gsyle_residual_dense(good, C23, transposed="yes")),
        (TypeError, lambda: D.gsyle_residual_dense(D.GDALEProblem(I2, I2, I2), C23)),
        (ValueError, lambda: D.SylvesterFactorization(I2, -I2, I3, np.ones((3, 2)))),
        (ValueError, lambda: D.SylvesterFactorization(I3, -I2, I3, -I3)),
        (ValueError, lambda: D.SylvesterFactorization(I2, -I2, I3, -I3, maxiters=0)),
        (ValueError, lambda: D.SylvesterFactorization(I2, -I2, I3, -I3, tol=-1.0)),
        (TypeError, lambda: D.h2_norm(I2, -I2, Bm, Cm, alg=D.FactoredSign())),
        (TypeError, lambda: D.h2_norm(I2, -I2, "B", Cm)),
        (ValueError, lambda: D.h2_norm(I2, -I3, Bm, Cm)),
        (ValueError, lambda: D.h2_norm(I2, -I2, Bm, np.ones((1, 3)))),
        (TypeError, lambda: D.h2_inner((I2, -I2, Bm), (I2, -I2, Bm, Cm))),
        (ValueError, lambda: D.h2_inner((I2, -I2, Bm, Cm), (I2, -I2, np.ones((2, 2)), Cm))),
        (TypeError, lambda: D.h2_error(I2, -I2, Bm, Cm, object())),
        (TypeError, lambda: D.h2_error(I2, -I2, Bm, Cm, rom, alg=D.Doubling())),
        (ValueError, lambda: D.h2_error(I2, -I2, np.ones((2, 2)), Cm, rom)),
        (ValueError, lambda: rom.h2_error(I2, -I2, Bm, np.ones((2, 2)))),
    ]
    for i, (exc, call) in enumerate(bad_calls):
        with pytest.raises(exc, match="nothing was run on the device"):
            call()
    assert D.GSYLEProblem(None, I2, None, I3, C23).E is None
    assert D.ReducedModel.h2_error is D.LQGReducedModel.h2_error and callable(D.SylvesterFactorization.solve)


def test_version_and_symbols():
    lib = D._lib.load()
    assert lib.dre_version() >= 119
    for name in ("dre_dense_sylvester_solve", "dre_dense_sylvester_residual", "dre_sylvester_create", "dre_sylvester_solve", "dre_sylvester_iters",
                 "dre_sylvester_destroy"):
        assert getattr(lib, name).argtypes is not None, name
