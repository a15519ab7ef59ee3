// The decision rule of the coupled sign iteration for the generalized Sylvester equation A X F + E X B = -C (dense_sylvester.hip) as plain
// arithmetic, free of HIP: the device's decision kernel, the host driver and the stand-alone program of tests/test_sylvester_host.py share
// this one statement of it.  The NumPy model tests/_sylvester_model.py (decide) repeats it line by line.
//
//   e_A = ||A_{k+1} + E||_F / ||E||_F,  e_B = ||B_{k+1} + F||_F / ||F||_F     the two distances
//   d_A = ||A_{k+1} - A_k||_F / ||A_{k+1}||_F,  d_B likewise,  d_C = ||C_{k+1} - C_k||_F / ||C_{k+1}||_F (0 when C did not move)   the steps
//   singular    an inversion's control word reports a zero pivot: ends the iteration, names the side
//   non-finite  a distance or a step that is not finite ends the iteration at once; the side is the pencil whose figures are not finite, or
//               the right-hand side when only the step of C is not finite (a C with non-finite entries on two sound pencils)
//   converged   iff BOTH distances are <= tol; the step of C is reported, it does not decide
//   stagnated   per side, the rule of the Lyapunov solver (sign_decision of dense_sign_body.hpp): d <= STAG_STEP while e > STAG_DIST; the left
//               pencil is named when both stagnate
// Running out of maxiters is decided on the host (SYLV_OUT_OF_ITERS).  The numbering of `done` is SignCtl::done's.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define DRE_SYLV_FN __host__ __device__ inline
#else
#define DRE_SYLV_FN inline
#endif

namespace dre {

enum : int {
    SYLV_RUNNING = 0,
    SYLV_CONVERGED = 1,
    SYLV_STAGNATED = 2,
    SYLV_NON_FINITE = 3,
    SYLV_SINGULAR = 4,
    SYLV_OUT_OF_ITERS = 5,      // host only
};

// the pencil at fault
enum : int {
    SYLV_SIDE_NONE = 0,
    SYLV_SIDE_LEFT = 1,         // (A, E)
    SYLV_SIDE_RIGHT = 2,        // (B, F)
    SYLV_SIDE_RHS = 3,          // neither: the right-hand side C
};

// dense_sign_body.hpp's STAG_STEP and STAG_DIST (that header needs HIP; dense_sylvester.hip asserts that the values agree)
constexpr double SYLV_STAG_STEP = 1e-8;
constexpr double SYLV_STAG_DIST = 1e-4;

struct SylvDecision {
    int done;
    int side;
};

// one relative step from two sums of squares: ||d||_F / ||x||_F, 0 when d = 0 (also when x = 0 then)
DRE_SYLV_FN double sylvester_rel_step(double d2, double x2) { return d2 == 0.0 ? 0.0 : std::sqrt(d2 / x2); }

DRE_SYLV_FN SylvDecision sylvester_decide(double eA, double eB, double dA, double dB, double dC, int singular_left, int singular_right, double tol) {
    SylvDecision d;
    d.done = SYLV_RUNNING;
    d.side = SYLV_SIDE_NONE;
    if (singular_left || singular_right) {
        d.done = SYLV_SINGULAR;
        d.side = singular_left ? SYLV_SIDE_LEFT : SYLV_SIDE_RIGHT;
    } else if (!(std::isfinite(eA) && std::isfinite(dA))) {
        d.done = SYLV_NON_FINITE;
        d.side = SYLV_SIDE_LEFT;
    } else if (!(std::isfinite(eB) && std::isfinite(dB))) {
        d.done = SYLV_NON_FINITE;
        d.side = SYLV_SIDE_RIGHT;
    } else if (!std::isfinite(dC)) {
        d.done = SYLV_NON_FINITE;
        d.side = SYLV_SIDE_RHS;
    } else if (eA <= tol && eB <= tol) {
        d.done = SYLV_CONVERGED;
    } else if (dA <= SYLV_STAG_STEP && eA > SYLV_STAG_DIST) {
        d.done = SYLV_STAGNATED;
        d.side = SYLV_SIDE_LEFT;
    } else if (dB <= SYLV_STAG_STEP && eB > SYLV_STAG_DIST) {
        d.done = SYLV_STAGNATED;
        d.side = SYLV_SIDE_RIGHT;
    }
    return d;
}

// tol <= 0: 10 max(n, m) eps
DRE_SYLV_FN double sylvester_default_tol(int n, int m, double tol) { return tol > 0.0 ? tol : 10.0 * (n > m ? n : m) * 2.220446049250313e-16; }

// the refinement rule of SignLyap::solve_impl: steps continue while the relative residual exceeds 100 max(n, m) eps
DRE_SYLV_FN double sylvester_refine_target(int n, int m) { return 100.0 * (n > m ? n : m) * 2.220446049250313e-16; }

}  // namespace dre
