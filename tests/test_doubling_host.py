"""Host checks of the discrete-time dense solvers (no GPU): the NumPy model tests/_doubling_model.py against SciPy and against its record
tests/golden/doubling_model.json, the decision rule csrc/doubling_decide.hpp compiled with g++ into a stand-alone program, the failure cases on
the model, and the Python argument checks, which raise before a context is needed."""
import os
import subprocess

import numpy as np
import pytest

import dre_amd as D
import _doubling_model as dm
from conftest import ROOT

EPS = np.finfo(float).eps
CSRC = os.path.join(ROOT, "differentialriccatiequations.jl_amd", "csrc")
REC = dm.recorded()
SIZES = list(dm.DARE_SIZES)


def _same_size(live, rec, n, keys):
    for key in keys:
        assert live[key] <= 3 * rec[key] + n * EPS and rec[key] <= 3 * live[key] + n * EPS, (key, live[key], rec[key])


@pytest.mark.parametrize("n", SIZES)
def test_dare_model_against_scipy_and_the_record(n):
    E, A, B, C = dm.dare_system(n)
    m, q, _ = dm.DARE_SIZES[n]
    assert B.shape == (n, m) and C.shape == (q, n) and (m != q or n == 1)
    live, rec = dm.record_dare(n), REC["dare"][str(n)]
    target = dm.refine_target(n)
    print(n, live)
    # the model's residuals, in double and in extended precision, hold the solver's own target; SciPy's standard form agrees
    for key in ("res_x", "res_y", "res_x_ext", "res_y_ext"):
        assert live[key] <= target, key
    assert live["x_err"] <= 1e3 * n * EPS and live["y_err"] <= 1e3 * n * EPS
    assert live["closed_loop"] < 1.0 < live["open_loop"]
    assert 4 <= live["iters"] <= 10
    # ... and the record is this run's
    for key in ("m", "q", "iters", "refinements_x", "refinements_y"):
        assert live[key] == rec[key], key
    _same_size(live, rec, n, ("res_x", "res_y", "res_x_ext", "res_y_ext", "x_err", "y_err"))
    for key in ("open_loop", "closed_loop"):
        assert live[key] == pytest.approx(rec[key], rel=1e-9), key
    # Y is the X of the transposed problem, and both are symmetric positive semidefinite
    X, Y, _ = dm.model_pair(n)
    Xt, _, _ = dm.dare_pair(E.T, A.T, C.T, B.T)
    assert dm.rel(Y, Xt) <= 1e3 * n * EPS
    for M in (X, Y):
        assert np.array_equal(M, M.T) and np.linalg.eigvalsh(M).min() >= -n * EPS * np.linalg.norm(M, 2)


@pytest.mark.parametrize("n", SIZES)
def test_stein_model_against_scipy_and_the_record(n):
    live, rec = dm.record_stein(n), REC["stein"][str(n)]
    print(n, live)
    assert live["rho"] < 1.0
    assert live["res"] <= dm.refine_target(n) and live["res_dual"] <= dm.refine_target(n)
    assert live["x_err"] <= 100 * n * EPS and live["y_err"] <= 100 * n * EPS
    assert (live["iters"], live["iters_dual"]) == (rec["iters"], rec["iters_dual"]) and live["rho"] == pytest.approx(rec["rho"], rel=1e-9)
    _same_size(live, rec, n, ("res", "res_dual", "x_err", "y_err"))


@pytest.mark.parametrize("n", dm.TUSTIN_SIZES)
def test_tustin_identity_on_the_model(n):
    """the Stein solve of (E - theta A, E + theta A, 2 theta Q) is the continuous Lyapunov solve of (E, A, Q)"""
    live, rec = dm.record_tustin(n), REC["tustin"][str(n)]
    print(n, live)
    assert live["rho"] < 1.0 and live["x_err"] <= 1e4 * n * EPS
    assert (live["theta"], live["iters"]) == (rec["theta"], rec["iters"]) and live["rho"] == pytest.approx(rec["rho"], rel=1e-9)
    _same_size(live, rec, n, ("x_err",))


def test_a_loose_tolerance_is_repaired_by_the_refinement_on_the_model():
    live, rec = dm.record_loose(), REC["loose"]
    print(live)
    target = dm.refine_target(live["n"])
    for side in ("x", "y"):
        assert live["res0_" + side] > target >= live["res_" + side]
        assert 1 <= live["refinements_" + side] <= 2 and live["refinements_" + side] == rec["refinements_" + side]
        assert live[side + "_err"] < live[side + "_err0"]
    assert live["iters"] == rec["iters"] < REC["dare"][str(live["n"])]["iters"]
    _same_size(live, rec, live["n"], ("res0_x", "res0_y", "res_x", "res_y", "x_err0", "y_err0", "x_err", "y_err"))


def test_failure_cases_on_the_model():
    cases = dm.failure_cases()
    for name, (_, _, _, done, iters) in cases.items():
        got = dm.run_failure(name)
        print(name, got)
        assert got[0] == done and (iters is None or got[1] == iters) and list(got) == REC["failures"][name], name
    assert dm.run_failure("stein_unit_circle") == (dm.OUT_OF_ITERS, 50)
    # E = I, A = diag(1, .5, .3, -.2), Q = I: H_11 doubles in every iteration, so the step stays 0.5
    with pytest.raises(dm.NotStable, match="relative step 0.5"):
        dm.stein(*cases["stein_unit_circle"][1])
    with pytest.raises(dm.Singular):
        dm.stein(np.zeros((2, 2)), np.eye(2), np.eye(2))
    # Q = 0: X = 0 on a stable pencil, no convergence on an unstable one
    assert np.array_equal(dm.stein(np.eye(3), 0.5 * np.eye(3), np.zeros((3, 3)))[0], np.zeros((3, 3)))
    with pytest.raises(dm.NotStable):
        dm.stein(np.eye(3), 1.5 * np.eye(3), np.zeros((3, 3)))


DECIDE_SRC = r"""
#include <cstdio>
#include <limits>
#include "doubling_decide.hpp"

using namespace dre;
static long bad = 0;
static void expect(const char* what, bool ok) { if (!ok) { ++bad; std::printf("FAILED: %s\n", what); } }

// E = I, diagonal A, Q = I (Stein) run through the rule: returns done, *iters the iteration (1-based) it was decided at
static int stein_diag(const double* a, int n, int maxiters, int* iters, double* step) {
    double m[8], h[8];
    for (int i = 0; i < n; ++i) { m[i] = a[i]; h[i] = 1.0; }
    const double tol = doubling_default_tol(n, 0.0);
    for (int k = 0; k < maxiters; ++k) {
        double dh2 = 0, h2 = 0, a2 = 0;
        for (int i = 0; i < n; ++i) {
            const double d = m[i] * h[i] * m[i];
            h[i] += d; m[i] *= m[i];
            dh2 += d * d; h2 += h[i] * h[i]; a2 += m[i] * m[i];
        }
        const DoublingDecision dec = doubling_decide(dh2, h2, a2, 0.0, 0.0, tol);
        *iters = k + 1; *step = dec.step;
        if (dec.done) return dec.done;
    }
    return DOUBLING_OUT_OF_ITERS;
}

// the SDA on E = I, A = diag(a1, a2), B = e2, C = e1': everything stays diagonal
static int dare_diag(double a1, double a2, int maxiters, int* iters) {
    double a[2] = {a1, a2}, g[2] = {0.0, 1.0}, h[2] = {1.0, 0.0};
    const double tol = doubling_default_tol(2, 0.0);
    for (int k = 0; k < maxiters; ++k) {
        double dh2 = 0, h2 = 0, A2 = 0, dg2 = 0, g2 = 0;
        for (int i = 0; i < 2; ++i) {
            const double wi = 1.0 / (1.0 + g[i] * h[i]), t1 = wi * a[i], t2 = wi * g[i];
            const double an = a[i] * t1, dg = a[i] * t2 * a[i], dh = a[i] * h[i] * t1;
            g[i] += dg; h[i] += dh; a[i] = an;
            dh2 += dh * dh; h2 += h[i] * h[i]; A2 += an * an; dg2 += dg * dg; g2 += g[i] * g[i];
        }
        const DoublingDecision dec = doubling_decide(dh2, h2, A2, dg2, g2, tol);
        *iters = k + 1;
        if (dec.done) return dec.done;
    }
    return DOUBLING_OUT_OF_ITERS;
}

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double tol = 1e-13;
    // dH = 0: converged only with ||A|| < 1
    expect("dH = 0 with ||A|| >= 1 is not converged", doubling_decide(0.0, 0.0, 1.0, 0.0, 0.0, tol).done == DOUBLING_RUNNING);
    expect("dH = 0 with ||A|| = 1.5 is not converged", doubling_decide(0.0, 4.0, 2.25, 0.0, 0.0, tol).done == DOUBLING_RUNNING);
    expect("dH = 0 with ||A|| < 1 is converged", doubling_decide(0.0, 0.0, 0.25, 0.0, 0.0, tol).done == DOUBLING_CONVERGED);
    expect("dH = 0 gives step 0", doubling_decide(0.0, 0.0, 0.25, 0.0, 0.0, tol).step == 0.0);
    expect("normA is the root of the sum", doubling_decide(0.0, 0.0, 0.25, 0.0, 0.0, tol).normA == 0.5);
    // the step and its tolerance, for H and for G
    expect("step = ||dH|| / ||H||", doubling_decide(1.0, 4.0, 0.0, 0.0, 0.0, tol).step == 0.5);
    expect("a step above tol runs on", doubling_decide(1.0, 4.0, 0.0, 0.0, 0.0, tol).done == DOUBLING_RUNNING);
    expect("a step at tol converges", doubling_decide(1e-26, 1.0, 0.0, 0.0, 0.0, tol).done == DOUBLING_CONVERGED);
    expect("the G sequence must have converged too", doubling_decide(1e-26, 1.0, 0.0, 1.0, 4.0, tol).done == DOUBLING_RUNNING);
    expect("the larger step is reported", doubling_decide(1e-26, 1.0, 0.0, 1.0, 4.0, tol).step == 0.5);
    expect("small step but ||A|| >= 1 runs on", doubling_decide(1e-26, 1.0, 1.0, 0.0, 0.0, tol).done == DOUBLING_RUNNING);
    // non-finite sums, in every position
    for (int pos = 0; pos < 5; ++pos)
        for (int which = 0; which < 2; ++which) {
            double s[5] = {1.0, 4.0, 0.25, 1.0, 4.0};
            s[pos] = which ? nan : inf;
            expect("a non-finite sum ends the iteration", doubling_decide(s[0], s[1], s[2], s[3], s[4], tol).done == DOUBLING_NON_FINITE);
        }
    expect("tol <= 0 means 10 n eps", doubling_default_tol(33, 0.0) == 10.0 * 33 * std::numeric_limits<double>::epsilon() && doubling_default_tol(33, -1.0) == doubling_default_tol(33, 0.0));
    expect("a positive tol is kept", doubling_default_tol(33, 1e-3) == 1e-3);
    expect("the refinement target is 100 n eps", doubling_refine_target(70) == 100.0 * 70 * std::numeric_limits<double>::epsilon());
    // the iterations of the failure cases
    int it = 0; double step = 0;
    const double a_circle[4] = {1.0, 0.5, 0.3, -0.2}, a_out[4] = {1.3, 0.5, 0.3, -0.2}, a_in[4] = {0.9, 0.5, 0.3, -0.2};
    int done = stein_diag(a_circle, 4, 50, &it, &step);
    std::printf("stein_unit_circle %d %d %.17g\n", done, it, step);
    expect("an eigenvalue on the unit circle runs out of iterations with the step at 0.5", done == DOUBLING_OUT_OF_ITERS && it == 50 && step > 0.49 && step < 0.51);
    done = stein_diag(a_out, 4, 50, &it, &step);
    std::printf("stein_unstable %d %d\n", done, it);
    expect("an unstable Stein pencil ends non-finite", done == DOUBLING_NON_FINITE);
    done = stein_diag(a_in, 4, 50, &it, &step);
    std::printf("stein_stable %d %d\n", done, it);
    expect("a stable Stein pencil converges", done == DOUBLING_CONVERGED && it <= 10);
    done = dare_diag(1.0, 0.5, 50, &it);
    std::printf("dare_unit_circle %d %d\n", done, it);
    expect("an uncontrollable mode on the unit circle runs out of iterations", done == DOUBLING_OUT_OF_ITERS && it == 50);
    done = dare_diag(1.5, 0.5, 50, &it);
    std::printf("dare_uncontrollable %d %d\n", done, it);
    expect("an uncontrollable unstable mode ends non-finite", done == DOUBLING_NON_FINITE);
    done = dare_diag(0.9, 0.5, 50, &it);
    expect("a stable plant converges", done == DOUBLING_CONVERGED && it <= 10);
    std::printf("%ld failures\n", bad);
    return bad ? 1 : 0;
}
"""


def test_decision_header_stand_alone(tmp_path):
    """csrc/doubling_decide.hpp without HIP, every row of the rule pinned; the failure cases' iteration counts are the model's"""
    cpp = tmp_path / "decide.cpp"
    cpp.write_text(DECIDE_SRC)
    exe = tmp_path / "decide"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, str(cpp), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failures"), r.stdout
    got = {ln.split()[0]: [int(v) for v in ln.split()[1:3]] for ln in r.stdout.splitlines() if ln.split()[0] in dm.failure_cases()}
    assert got == {k: list(dm.run_failure(k)) for k in dm.failure_cases()}, r.stdout
    # the model's rule is the header's on the same sums
    for sums in ((0.0, 0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 0.25, 0.0, 0.0), (1.0, 4.0, 0.0, 0.0, 0.0), (1e-26, 1.0, 0.0, 1.0, 4.0), (np.inf, 1.0, 0.0, 0.0, 0.0),
                 (1.0, np.nan, 0.0, 0.0, 0.0)):
        done = dm.decide(*sums, 1e-13)[0]
        want = dm.NON_FINITE if not np.isfinite(sums).all() else (dm.CONVERGED if sums[0] == 0 and sums[3] == 0 and sums[2] < 1 else dm.RUNNING)
        assert done == want, sums


def test_python_argument_checks_raise_before_a_context_is_needed():
    I2, B, Cm = np.eye(2), np.ones((2, 1)), np.ones((1, 2))
    good = D.GDAREProblem(I2, 0.5 * I2, D.lowrank(B), D.lowrank(np.ascontiguousarray(Cm.T)))
    bad_calls = [
        (TypeError, lambda: D.solve(D.GDALEProblem(I2, I2, I2), D.MatrixSign())),
        (TypeError, lambda: D.solve(good, D.MatrixSign())),
        (TypeError, lambda: D.solve_gdare_pair(I2, I2, B, Cm, D.MatrixSign())),
        (TypeError, lambda: D.solve_gdale_dense(good, D.Doubling())),
        (TypeError, lambda: D.solve_gdare_dense(D.GDALEProblem(I2, I2, I2), D.Doubling())),
        (ValueError, lambda: D.solve(D.GDALEProblem(I2, np.eye(3), I2), D.Doubling())),
        (ValueError, lambda: D.solve(D.GDALEProblem(I2, I2, np.eye(3)), D.Doubling())),
        (ValueError, lambda: D.solve(D.GDALEProblem(np.ones((2, 3)), I2, I2), D.Doubling())),
        (ValueError, lambda: D.solve(D.GDALEProblem(I2, I2, I2), D.Doubling(maxiters=0))),
        (ValueError, lambda: D.solve(D.GDALEProblem(I2, I2, I2), D.Doubling(tol=-1.0))),
        (ValueError, lambda: D.solve(good, D.Doubling(max_refine=-1))),
        (ValueError, lambda: D.solve(D.GDAREProblem(I2, I2, D.lowrank(np.ones((3, 1))), D.lowrank(np.ones((2, 1)))), D.Doubling())),
        (ValueError, lambda: D.solve(D.GDAREProblem(I2, I2, D.lowrank(B), D.lowrank(np.ones((3, 1)))), D.Doubling())),
        (ValueError, lambda: D.solve_gdare_pair(I2, I2, B, np.ones((1, 3)))),
        (ValueError, lambda: D.solve_gdare_pair(I2, I2, B, Cm, Rinv=np.eye(2))),
        (ValueError, lambda: D.solve_gdare_pair(I2, I2, B, Cm, S=np.eye(2))),
        (ValueError, lambda: D.gdale_residual_dense(D.GDALEProblem(I2, I2, I2), np.eye(3))),
        (ValueError, lambda: D.gdare_residual_dense(good, np.eye(3))),
    ]
    for i, (exc, call) in enumerate(bad_calls):
        with pytest.raises(exc, match="nothing was run on the device"):
            call()
    with pytest.raises(TypeError, match="unsupported problem type"):
        D.solve(object(), D.Doubling())
    assert D.Doubling() == D.Doubling(maxiters=50, tol=None, max_refine=2)


def test_version_and_symbols():
    lib = D._lib.load()
    assert lib.dre_version() >= 118
    for name in ("dre_dense_stein_solve", "dre_dense_stein_residual", "dre_dense_dare_solve", "dre_dense_dare_solve_pair", "dre_dense_dare_residual"):
        assert getattr(lib, name).argtypes is not None, name
