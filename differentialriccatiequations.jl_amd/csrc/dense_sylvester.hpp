// Dense generalized Sylvester solver by the coupled sign iteration (GSYLEProblem + MatrixSign), device resident (dense_sylvester.hip):
//   A X F + E X B = -C        (A, E n x n;  B, F m x m;  C, X n x m;  both pencils c-stable)
// and its transposed equation A'Y F' + E'Y B' = -C from the same kept sequence.  See DESIGN.md §9.15; host model tests/_sylvester_model.py.
//
// Memory, checked once before any kernel (doubles; the partial sums and the pivots not counted):
//   maxiters (n^2 + m^2)   the kept sequence L_k = E A_k^-1 (n x n) and R_k = B_k^-1 F (m x m)
//   5 (n^2 + m^2)          E^-1, A, A_k, A_k^-1, L_k E   and   F^-1, B, B_k, B_k^-1, F R_k
//   7 n m                  the recursion's W, the two products of a step, the residual's two terms, the residual, a refinement's increment
// dense_sylvester_solve adds n m for X (and n^2, m^2 for an identity E or F); dense_sylvester_residual holds 5 n m.
#pragma once
#include <vector>

#include "dense_sign.hpp"
#include "sylvester_decide.hpp"

namespace dre {

// Device-side control words of the coupled iteration, the two inversions' in front (read back once per iteration by the host).
struct SylvCtl {
    GjCtl gjA, gjB;     // of the last inverted A_k (or E) and B_k (or F)
    double c;           // the joint scaling factor of the running iteration (k_sylv_scale)
    int done, side;     // sylvester_decide.hpp
    double distA, distB, stepA, stepB;
    double stepC;       // ||C_{k+1} - C_k||_F / ||C_{k+1}||_F of the last update of a right-hand side
    double res;         // relative residual ||Res||_F / ||C||_F of the last residual evaluation (||Res||_F for C = 0)
    double scaled;      // ||Res||_F / (||C||_F + ||A X F||_F + ||E X B||_F)
    double resnorm;     // ||Res||_F
};

struct SylvStats {
    long iters = 0, refinements = 0;
    double res0 = 0.0, res = 0.0;   // relative residual after the first replay, final
    double step = 0.0;              // C's last relative step
};

// Two pencils with E and F fixed: the coupled sign iteration of (A, E) and (B, F) keeps (L_k, R_k, c_k), so that every right-hand side, in
// either direction, costs only the recursion of C (replay), and a solve is refined by replaying its residual (the rule of SignLyap::solve_impl
// with the target 100 max(n, m) eps).  Everything runs on the context's stream.
class SignSylvester {
  public:
    // Throws Error(ERR_INVALID) on shapes, orders above DENSE_MAX_N, maxiters outside 1 .. 1000 and max_refine < 0 before any device work,
    // Error(ERR_ALLOC) from the memory check (the count above plus `extra` doubles of the caller's), Error(ERR_SINGULAR) for a singular E or F.
    // tol <= 0: 10 max(n, m) eps.
    SignSylvester(Ctx* ctx, const Mat& E, const Mat& F, int maxiters, double tol, int max_refine, size_t extra = 0);
    // the coupled iteration: throws Error(ERR_NOT_STABLE) naming the pencil that is not c-stable, Error(ERR_SINGULAR) naming the singular A_k or B_k
    void factor(const Mat& A, const Mat& B) { factor_impl(A, B, nullptr); }
    // factor(A, B) with C riding along in the iteration, then the refinement of solve(): X is bit for bit what factor() and solve() return
    SylvStats factor_solve(const Mat& A, const Mat& B, const Mat& C, Mat& X);
    // A X F + E X B = -C with the kept sequence; C, X n x m (ld n).  Error(ERR_INVALID) for a C with non-finite entries.
    SylvStats solve(const Mat& C, Mat& X) { return solve_impl(false, C, X, false); }
    // A'Y F' + E'Y B' = -C from the same sequence: V_0 = E^-T C F^-T, V_{k+1} = V_k / (2 c_k) + (c_k / 2) L_k' V_k R_k', Y = V_inf / 2
    SylvStats solve_t(const Mat& C, Mat& Y) { return solve_impl(true, C, Y, false); }
    int iters() const { return iters_; }
    int n() const { return n_; }
    int m() const { return m_; }
    void set_max_refine(int max_refine) { max_refine_ = max_refine; }

  private:
    void factor_impl(const Mat& A, const Mat& B, const Mat* C);
    void c_step(bool transposed, const Mat& L, const Mat& R, double c, bool c_on_device);
    void replay(bool transposed, const Mat& C, Mat& X);
    void exit_transform(Mat& X);
    SylvCtl residual(bool transposed, const Mat& C, const Mat& X);
    SylvStats solve_impl(bool transposed, const Mat& C, Mat& X, bool have_x);
    Ctx* c_;
    int n_, m_, maxiters_, max_refine_, iters_ = 0;
    double tol_, logdetEF_ = 0.0;
    Mat E_, F_, Einv_, Finv_, A_, B_, Ak_, Ai_, Bk_, Bi_, YA_, YB_, Lstore_, Rstore_;
    Mat W_, T_, U_, G1_, G2_, Res_, dX_;
    std::vector<double> cs_;
    DevArr<int> piv_;
    DevArr<SylvCtl> ctl_;
    DevArr<double> part_, nrm_;
};

struct DenseSylvesterResult {
    Mat X;
    SylvStats st;
};

// One solve: E or F null is the identity.  transposed: A'X F' + E'X B' = -C.  Errors as SignSylvester's.
DenseSylvesterResult dense_sylvester_solve(Ctx* ctx, const Mat* E, const Mat& A, const Mat* F, const Mat& B, const Mat& C, bool transposed, int maxiters,
                                           double tol, int max_refine);

// Res = C + A X F + E X B (transposed: C + A'X F' + E'X B') as a new n x m matrix; *fro = ||Res||_F, *scaled = ||Res||_F / (||C||_F + ||A X F||_F +
// ||E X B||_F) (either may be null; synchronising).
Mat dense_sylvester_residual(Ctx* ctx, const Mat* E, const Mat& A, const Mat* F, const Mat& B, const Mat& C, const Mat& X, bool transposed, double* fro,
                             double* scaled);

}  // namespace dre
