// Dense GARE solver (GAREProblem + MatrixSign): the matrix sign function of the Hamiltonian pencil, extraction of the stabilizing solution
// and Newton-Kleinman refinement, device resident (dense_are.hip).  See DESIGN.md, "Dense path", GARE.
#pragma once
#include "dense_sign.hpp"

namespace dre {

struct DenseGareResult {
    Mat X;                           // the stabilizing solution, n x n symmetric
    long iters = 0, refinements = 0; // sign iterations, Newton-Kleinman steps
    double res0 = 0.0, res = 0.0;    // scaled residual after extraction, final
};

// Q + A'XE + E'XA - E'XGXE = 0 with G = B Rinv B', Q = Ct S Ct' (Rinv, S null: identity).  E, A n x n (ld n), B n x m, Ct n x q, 2n <= DENSE_MAX_N.
// Throws Error(ERR_NOT_STABLE) when the sign iteration stagnates, produces non-finite values or runs out of maxiters (Hamiltonian eigenvalues on
// or near the imaginary axis) and when the refinement's closed loop is not c-stable; Error(ERR_SINGULAR) for a singular E, Z_k or extraction
// factor; Error(ERR_ALLOC) from the up-front memory check.  tol <= 0: 10 (2n) eps on the relative step of the sign iteration.
DenseGareResult dense_gare_solve(Ctx* ctx, const Mat& E, const Mat& A, const Mat& B, const Mat* Rinv, const Mat& Ct, const Mat* S, int maxiters,
                                 double tol, int max_refine);

// What went wrong in a Hamiltonian sign iteration that ended with done = 2 (stagnated), 3 (non-finite), 4 (singular Z_k) or 5 (out of maxiters),
// shared by the single and the batched solver, which put "dense GARE: " or "batched dense GARE, member b: " in front.  k: the iteration of the
// singular Z_k; step: the last relative step.
std::string gare_sign_failure(int done, int k, double step, int maxiters);

// Both Riccati solutions of LQG design from ONE Hamiltonian sign iteration: X as dense_gare_solve returns it, bit for bit, and the
// filter solution Y of  G + A Y E' + E Y A' - E Y Q Y E' = 0,  extracted from the transposed blocks of the same Z_inf (the filter's pencil is
// (H', K')) and refined on the dual closed loop A - E Y Q with SignLyap::solve_t.  Y.iters is the shared iteration count; refinements, res0 and res
// are the filter's own, the scaled residual being ||R_f||_F / (||G||_F + 2 ||A Y E'||_F + ||E Y Q Y E'||_F).  Checks and errors of dense_gare_solve;
// a failure that concerns one solution only names it ("regulator", "filter") in the message.  Memory: 25 n^2 instead of 24 n^2.
struct DenseGarePair { DenseGareResult X, Y; };
DenseGarePair dense_gare_solve_pair(Ctx* ctx, const Mat& E, const Mat& A, const Mat& B, const Mat* Rinv, const Mat& Ct, const Mat* S, int maxiters,
                                    double tol, int max_refine);

// R(X) = Q + A'XE + E'XA - E'XGXE (symmetrised) as a new n x n matrix; *fro = ||R(X)||_F (synchronising)
Mat dense_gare_residual(Ctx* ctx, const Mat& E, const Mat& A, const Mat& B, const Mat* Rinv, const Mat& Ct, const Mat* S, const Mat& X, double* fro);

}  // namespace dre
