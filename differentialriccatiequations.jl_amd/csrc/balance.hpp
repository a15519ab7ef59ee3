// Square-root balanced truncation of a descriptor system  E x' = A x + B u,  y = C x  from its Gramians in factored form (balance.hip).
// See DESIGN.md §9.8; the host restatement is tests/_svd_jacobi_model.py (balance).
#pragma once
#include "dense.hpp"
#include "dense_batch.hpp"

namespace dre {

struct BalanceResult {
    Mat hsv;           // k x 1: the Hankel singular values, k = min(r_o, r_c)
    Mat T, W;          // n x r: right and left projection, W'E T = I
    Mat Ar, Br, Cr;    // W'A T (r x r), W'B (r x m), C T (q x r)
    int order = 0;     // r
    long rank = 0;     // numerical rank of Z_o'E Z_c
    int r_c = 0, r_o = 0;   // columns of Z_c and Z_o
    long dropped = 0;       // non-positive entries of D_c and D_o, left out
    long sweeps = 0;        // block sweeps of the SVD
    double eye_err = 0.0;   // ||W'E T - I||_F
    double bound = 0.0;     // 2 sum_{i > r} sigma_i
    double neg_max = 0.0;   // largest |d| among the dropped entries
};

// P = Lc Dc Lc' from A P E' + E P A' = -B B' and Q = Lo Do Lo' from A'Q E + E'Q A = -C'C, in the form dre_sign_solve_lr_t / dre_sign_solve_lr
// return them; Dc, Do: a diagonal matrix (its diagonal is read) or a vector.  order > 0: that order (above the numerical rank: DRE_ERR_INVALID);
// order = 0: the smallest r with 2 sum_{i > r} sigma_i <= tol sigma_1, at most the numerical rank.  Shape errors are DRE_ERR_INVALID before any
// launch.
BalanceResult balance_lr(Ctx* ctx, const Mat& E, const Mat& A, const Mat& B, const Mat& C, const Mat& Lc, const Mat& Dc, const Mat& Lo, const Mat& Do,
                         int order, double tol);

// LQG balanced truncation (host restatement tests/_lqg_model.py): X and Y are the dense stabilising solutions of the regulator
// and the filter Riccati equations (dense_gare_solve_pair).  Both are factored by the Householder + QL eigensolver (non-positive eigenvalues are
// left out) and balance_lr's steps run with (Lo, Do) from X and (Lc, Dc) from Y: bal.hsv holds the LQG characteristic values mu, and W'E T = I.
// order = 0: the smallest r with 2 sum_{i > r} nu_i <= tol, nu_i = mu_i / sqrt(1 + mu_i^2) (absolute); bal.bound is that sum, the bound on the
// error of the normalised right coprime factors.  The reduced-order controller x_c' = Ac x_c + Lr y, u = -Kr x_c comes with it:
// Kr = Br' Sigma_r (m x r), Lr = Sigma_r Cr' (r x q), Ac = Ar - Br Kr - Lr Cr.  Shape errors are DRE_ERR_INVALID before any launch; n <= 8192.
struct LqgBalanceResult {
    BalanceResult bal;
    Mat Kr, Lr, Ac;
};
LqgBalanceResult lqg_balance(Ctx* ctx, const Mat& E, const Mat& A, const Mat& B, const Mat& C, const Mat& X, const Mat& Y, int order, double tol);

// Ensemble form: the members share (n, m, q); each has its own E, A, B, C and factored Gramians, whose ranks may differ.  Every
// M_b = Z_o'(E Z_c) is written into a zero-filled stack of the common shape (max_b r_o) x (max_b r_c) and ONE svd_jacobi_batch diagonalises the
// stack; the order rule, the projections and the reduced matrices then run per member with balance_lr's steps, the member's own r_o and r_c
// bounding its numerical rank.
//
// Contract: a member's result is a bitwise function of its own data and of the padded shape only; it depends on the other members only
// through that shape.  (Zero rows add nothing to a Gram matrix and zero columns are never rotated, so a member's non-zero singular triplets are
// those of its own M_b up to rounding, and the padding's singular values are zeros at the tail.)  A batch of one member, whose padded shape is
// its own, is bitwise balance_lr.
//
// Shape errors, batch < 1 and a D that matches no factor are the call's DRE_ERR_INVALID before any launch.  A member's own failure (an order
// above its numerical rank, a non-finite Gramian factor, an SVD that does not converge) is recorded in status[b]; the others go on.
struct BalanceBatch {
    std::vector<BalanceResult> res;              // per member (empty for a failed member)
    std::vector<BatchMemberStatus> status;
    int padded_rows = 0, padded_cols = 0;        // the stack's shape: max_b r_o, max_b r_c
};
struct BalanceMember { const Mat *E, *A, *B, *C, *Lc, *Dc, *Lo, *Do; };
BalanceBatch balance_lr_batch(Ctx* ctx, const std::vector<BalanceMember>& mem, int order, double tol, const char* who = "balance_lr_batch");

}  // namespace dre
