// The decision rule of the doubling iterations (dense_doubling.hip: squared Smith for the Stein equation, SDA for the DARE) as plain
// arithmetic, free of HIP: the device's decision kernel, the host driver and the stand-alone program of tests/test_doubling_host.py share this
// one statement of it.  The NumPy model tests/_doubling_model.py (decide) repeats it line by line.
//
//   step      = ||dH||_F / ||H_{k+1}||_F, 0 when dH = 0; for the DARE the larger of that and ||dG||_F / ||G_{k+1}||_F (G_inf is returned as Y)
//   converged   iff step <= tol AND ||A_{k+1}||_F < 1   (Q = 0 with an unstable pencil has dH = 0 from the first iteration on: the second
//               condition keeps it from "converging" to X = 0)
//   non-finite  any sum that is not finite ends the iteration at once
// Running out of maxiters is decided on the host (DOUBLING_OUT_OF_ITERS).
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define DRE_DOUBLING_FN __host__ __device__ inline
#else
#define DRE_DOUBLING_FN inline
#endif

namespace dre {

enum : int {
    DOUBLING_RUNNING = 0,
    DOUBLING_CONVERGED = 1,
    DOUBLING_NON_FINITE = 3,       // (the numbering of the sign family's done words: 2, stagnation, has no rule here)
    DOUBLING_SINGULAR = 4,         // set by the decision kernel from the inversion's control word, not by doubling_decide
    DOUBLING_OUT_OF_ITERS = 5,     // host only
};

struct DoublingDecision {
    int done;
    double step;       // the relative step
    double normA;      // ||A_{k+1}||_F
};

// one relative step from two sums of squares: ||d||_F / ||x||_F, 0 when d = 0 (also when x = 0 then)
DRE_DOUBLING_FN double doubling_rel_step(double d2, double x2) { return d2 == 0.0 ? 0.0 : std::sqrt(d2 / x2); }

// sums of squares: dh2 = ||dH||^2, h2 = ||H_{k+1}||^2, a2 = ||A_{k+1}||^2, dg2 = ||dG||^2, g2 = ||G_{k+1}||^2 (Stein: dg2 = g2 = 0)
DRE_DOUBLING_FN DoublingDecision doubling_decide(double dh2, double h2, double a2, double dg2, double g2, double tol) {
    DoublingDecision d;
    d.done = DOUBLING_RUNNING;
    d.step = 0.0;
    d.normA = std::sqrt(a2);
    if (!(std::isfinite(dh2) && std::isfinite(h2) && std::isfinite(a2) && std::isfinite(dg2) && std::isfinite(g2))) {
        d.done = DOUBLING_NON_FINITE;
        d.step = INFINITY;
        return d;
    }
    const double sh = doubling_rel_step(dh2, h2), sg = doubling_rel_step(dg2, g2);
    d.step = sh > sg ? sh : sg;
    if (!std::isfinite(d.step)) { d.done = DOUBLING_NON_FINITE; return d; }       // (0 < d2 with x2 = 0 cannot happen for a sum; kept for safety)
    if (d.step <= tol && d.normA < 1.0) d.done = DOUBLING_CONVERGED;
    return d;
}

// tol <= 0: 10 n eps
DRE_DOUBLING_FN double doubling_default_tol(int n, double tol) { return tol > 0.0 ? tol : 10.0 * n * 2.220446049250313e-16; }

// the refinement rule of refine() in dense_are.hip: steps continue while the scaled residual exceeds 100 n eps ...
DRE_DOUBLING_FN double doubling_refine_target(int n) { return 100.0 * n * 2.220446049250313e-16; }

}  // namespace dre
