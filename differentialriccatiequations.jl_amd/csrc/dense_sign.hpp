// Dense path (GDREProblem{<:Matrix}): in-place Gauss-Jordan inversion with partial pivoting, the generalized matrix-sign-function
// Lyapunov solver built on it, and the dense Rosenbrock drivers Ros1..Ros4 (dense_sign.hip).  See DESIGN.md, "Dense path".
#pragma once
#include "common.hpp"

namespace dre {

enum : int { ERR_NOT_STABLE = -7 };    // = DRE_ERR_NOT_STABLE of include/dre_hip.h

// Order limits of the dense path.  DENSE_MAX_N is the index limit: every device kernel the dense path launches (dense_sign.hip, the element-wise
// copies and norms of dense.hip, the GEMM family of gemm.hip) forms element offsets inside an n x n operand either in size_t or as an int
// row / column index below n, and every int product it forms (row + col * ld of the n x n, n x nb and nb x n operands, the
// k * n column offset of a stored P_k) stays below 2^31 - 1 while n <= 46340 = floor(sqrt(2^31 - 1)).  Below that limit the device memory
// decides (require_memory).  GJ_REGISTER_MAX_N is the limit of the register panel, which keeps ceil(n / 512) rows per thread in registers
// (dense_gj_panel = 1 refuses larger n; the default 0 switches to the tournament panel above it).
#define DENSE_MAX_N 46340
#define GJ_REGISTER_MAX_N 4096

// Device-side control words of the inversion and of one sign iteration (read back once per step by the host).
struct SignCtl {
    double logdet;      // log |det| of the last inverted matrix (sum of log |pivot|)
    int singular;       // the inversion met an exactly zero (or non-finite) pivot column
    int done;           // sign iteration: 0 running, 1 converged, 2 stagnated away from -E (not c-stable), 3 non-finite
    double dist;        // ||Z_{k+1} + E||_F / ||E||_F
    double step;        // ||Z_{k+1} - Z_k||_F / ||Z_{k+1}||_F
    double res;         // relative residual ||R + F'XE + E'XF||_F / ||R||_F of the last residual evaluation
    double pad[3];
};

// A <- inv(A) in place (n x n, n <= DENSE_MAX_N); ctl->logdet = log|det A|, ctl->singular set on a zero pivot; piv[0..n) the row interchanges
// (LAPACK style: row j was swapped with row piv[j] >= j).  The panel follows ctx->dense_gj_panel (0 auto, 1 register, 2 tournament) and
// (the tournament panel's width is 32).  No synchronisation.
void gj_invert(Ctx* ctx, Mat& A, int* piv_dev, SignCtl* ctl_dev);

// DRE_ERR_ALLOC unless `doubles` doubles fit in the free device memory plus the pool's released buffers (no allocation, no kernel)
void require_memory(Ctx* ctx, size_t doubles);

struct SignStats { long iters = 0, refinements = 0; double res0 = 0.0, res = 0.0; };
struct SignLrStats;      // dense_sign_lr.hpp

// One pencil E (fixed) with a stage matrix F: the sign iteration keeps its (P_k, c_k) sequence so that further right-hand sides
// on the same pencil cost only the W recursion (replay).
class SignLyap {
  public:
    // lazy_dense: the n x n work matrices W, T, Res of solve() are allocated by the first solve() instead of here (a solver that is only used
    // through solve_lr never needs them)
    SignLyap(Ctx* ctx, const Mat& E, int maxiters, double tol, int max_refine, size_t extra_n2 = 0, bool lazy_dense = false);
    // sign iteration on (F, E): throws Error(ERR_NOT_STABLE) / Error(ERR_SINGULAR)
    void factor(const Mat& F);
    // F'XE + E'XF = -R (R symmetric) with the kept sequence, refined by replay; X is n x n
    SignStats solve(const Mat& R, Mat& X);
    int iters() const { return iters_; }
    int n() const { return n_; }
    void set_max_refine(int max_refine) { max_refine_ = max_refine; }      // refinement steps of the following solve() calls
    // Factored replay (dense_sign_lr.hip): F'XE + E'XF = -G S G' (G n x r, S r x r symmetric, indefinite allowed) with the kept sequence applied
    // to the factor; X = L D L' with D diagonal (r = 0: L is n x 0).  Throws Error(ERR_INVALID) on rtol outside (0, 1) or max_width < max(r, 1).
    SignLrStats solve_lr(const Mat& G, const Mat& S, double rtol, int max_width, int max_refine, Mat& L, Mat& D);

  private:
    void ensure_dense_work();
    void replay(const Mat& R, Mat& X);
    double residual(const Mat& R, const Mat& X);
    void read_ctl(SignCtl* h);
    Ctx* c_;
    int n_, maxiters_, max_refine_, iters_ = 0;
    double tol_, logdetE_ = 0.0;
    Mat E_, Einv_, F_, Z_, Zi_, Y_, W_, T_, Res_, Pstore_;
    std::vector<double> cs_;
    DevArr<int> piv_;
    DevArr<SignCtl> ctl_;
    DevArr<double> part_, nrm_;
};

struct DenseGdreResult {
    std::vector<double> t;
    std::vector<Mat> Kt;         // K(t_i)' as n x m
    std::vector<Mat> X;          // X(t_i): first and last, or all under save_state
    std::vector<SignStats> solves;
};
DenseGdreResult dense_gdre_solve(Ctx* ctx, const Mat& E, const Mat& A, const Mat& B, const Mat& C, const Mat& X0, double t0, double tf, double dt,
                                 int order, bool save_state, int maxiters, double tol, int max_refine);

}  // namespace dre
