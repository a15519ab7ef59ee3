// Discrete-time dense solvers by doubling (GDALEProblem / GDAREProblem + Doubling), device resident (dense_doubling.hip): the squared Smith
// iteration for the generalized Stein equation and the structure-preserving doubling algorithm (SDA) for the generalized discrete-time
// algebraic Riccati equation, with Newton (Hewer) refinement on the Stein solver.  See DESIGN.md §9.14; host model tests/_doubling_model.py.
#pragma once
#include "dense_sign.hpp"
#include "doubling_decide.hpp"

namespace dre {

// Device-side control words of a doubling iteration, the inversion's in front (read back once per iteration by the host).
struct DoublingCtl {
    GjCtl gj;           // of the last inverted matrix (E, or W_k = I + G_k H_k)
    int done;           // doubling_decide.hpp: 0 running, 1 converged, 3 non-finite, 4 singular W_k
    double step;        // the relative step of doubling_decide
    double normA;       // ||A_{k+1}||_F
};

struct DenseSteinResult {
    Mat X;              // n x n symmetric
    long iters = 0;     // doubling iterations
    double step = 0.0;  // the last relative step
};

// A'XA - E'XE = -Q (dual: A Y A' - E Y E' = -Q) for a symmetric Q (its symmetric part is taken); E, A, Q n x n (ld n), n <= DENSE_MAX_N.
// M = E^-1 A (dual: A E^-1), H_0 = sym(Q), H_{k+1} = H_k + sym(M_k' H_k M_k) (dual: M_k H_k M_k'), M_{k+1} = M_k^2, X = sym(E^-T H E^-1) (dual:
// sym(E^-1 H E^-T)).  Throws Error(ERR_NOT_STABLE) when the iteration produces non-finite values or runs out of maxiters (E^-1 A has
// eigenvalues on or outside the unit circle), Error(ERR_SINGULAR) for a singular E, Error(ERR_ALLOC) from the up-front memory check of
// 7 n^2 doubles.  tol <= 0: 10 n eps on the relative step.
DenseSteinResult dense_stein_solve(Ctx* ctx, const Mat& E, const Mat& A, const Mat& Q, bool dual, int maxiters, double tol);

// Res = sym(Q + A'XA - E'XE) (dual: Q + A X A' - E X E') as a new n x n matrix; *fro = ||Res||_F, *scaled = ||Res||_F / (||Q||_F + ||A'XA||_F +
// ||E'XE||_F) (either may be null; synchronising).  4 n^2 doubles.
Mat dense_stein_residual(Ctx* ctx, const Mat& E, const Mat& A, const Mat& Q, const Mat& X, bool dual, double* fro, double* scaled);

struct DenseDareResult {
    Mat X;                           // the stabilizing solution, n x n symmetric
    long iters = 0, refinements = 0; // SDA iterations, Newton steps
    double res0 = 0.0, res = 0.0;    // scaled residual after the doubling, final
};

// Q + A'X(I + GX)^-1 A - E'XE = 0 with G = B Rinv B', Q = Ct S Ct' (Rinv, S null: identity).  E, A n x n (ld n), B n x m, Ct n x q, n <= DENSE_MAX_N.
// Throws Error(ERR_NOT_STABLE) when the SDA produces non-finite values or runs out of maxiters (symplectic pencil with eigenvalues on or near
// the unit circle, or not d-stabilizable) and when a refinement's closed loop is not d-stable; Error(ERR_SINGULAR) for a singular E or
// W_k = I + G_k H_k; Error(ERR_ALLOC) from the up-front memory check (17 n^2 doubles).  tol <= 0: 10 n eps.
DenseDareResult dense_dare_solve(Ctx* ctx, const Mat& E, const Mat& A, const Mat& B, const Mat* Rinv, const Mat& Ct, const Mat* S, int maxiters,
                                 double tol, int max_refine);

// Both solutions from ONE doubling: X as dense_dare_solve returns it, bit for bit, and the filter's Y = G_inf, the stabilizing solution of
//   G + A Y (I + QY)^-1 A' - E Y E' = 0,
// which needs no back-transformation.  Y.iters is the shared count; refinements, res0 and res are the filter's own.  18 n^2 doubles.
struct DenseDarePair { DenseDareResult X, Y; };
DenseDarePair dense_dare_solve_pair(Ctx* ctx, const Mat& E, const Mat& A, const Mat& B, const Mat* Rinv, const Mat& Ct, const Mat* S, int maxiters,
                                    double tol, int max_refine);

// R(X) = sym(Q + A'X(I + GX)^-1 A - E'XE) as a new n x n matrix; *fro = ||R||_F, *scaled = ||R||_F / (||Q||_F + ||A'X(I + GX)^-1 A||_F + ||E'XE||_F)
// (either may be null; synchronising).  Error(ERR_SINGULAR) for a singular I + GX.  8 n^2 doubles.
Mat dense_dare_residual(Ctx* ctx, const Mat& E, const Mat& A, const Mat& B, const Mat* Rinv, const Mat& Ct, const Mat* S, const Mat& X, double* fro,
                        double* scaled);

}  // namespace dre
