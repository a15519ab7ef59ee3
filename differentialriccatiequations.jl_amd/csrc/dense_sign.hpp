// Dense path (GDREProblem{<:Matrix}): the generalized matrix-sign-function Lyapunov solver on the Gauss-Jordan inversion of dense_gj.hip, and
// the dense Rosenbrock drivers Ros1..Ros4 (dense_sign.hip; the factored replay solve_lr: dense_sign_lr.hip).  See DESIGN.md, "Dense path".
#pragma once
#include "dense_gj.hpp"

namespace dre {

enum : int { ERR_NOT_STABLE = -7 };    // = DRE_ERR_NOT_STABLE of include/dre_hip.h

// Device-side control words of one sign iteration, the inversion's in front (read back once per step by the host).
struct SignCtl {
    GjCtl gj;           // of the last inverted matrix
    int done;           // sign iteration: 0 running, 1 converged, 2 stagnated away from -E (not c-stable), 3 non-finite
    double dist;        // ||Z_{k+1} + E||_F / ||E||_F
    double step;        // ||Z_{k+1} - Z_k||_F / ||Z_{k+1}||_F
    double res;         // relative residual ||R + F'XE + E'XF||_F / ||R||_F of the last residual evaluation
};

// out = sym?(a0 M0 + a1 M1 + a2 M2) for n x n matrices (M1, M2 may be null; M0 with any leading dimension, the others and out with ld n; under
// sym out must not alias an input).  tag and words: the profiler's class and the 8-byte words it counts per element (0: one per matrix).
void comb(Ctx* ctx, Mat& out, double a0, const Mat& M0, double a1 = 0.0, const Mat* M1 = nullptr, double a2 = 0.0, const Mat* M2 = nullptr,
          bool sym = false, const char* tag = "dense_comb", int words = 0);

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
    // The dual equation of the same pencil, F Y E' + E Y F' = -R, from the same kept sequence: the sign iteration of (F', E') has the iterates
    // Z_k' and the same c_k, and with V = E^-1 W E^-T its W recursion reads V <- sym(V/(2c) + (c/2) P_k V P_k'), V_0 = E^-1 R E^-T, Y = V/2.
    // Same refinement rule as solve(); the kept state is not changed.  DESIGN.md §9.7.
    SignStats solve_t(const Mat& R, Mat& Y);
    // Factored dual replay: F Y E' + E Y F' = -G S G', L_0 = E^-1 G, L_{k+1} = [L_k, P_k L_k]; arguments, cap, compression and refinement as solve_lr
    SignLrStats solve_lr_t(const Mat& G, const Mat& S, double rtol, int max_width, int max_refine, Mat& L, Mat& D);

  private:
    void ensure_dense_work();
    void replay(const Mat& R, Mat& X);
    double residual(const Mat& R, const Mat& X);
    void replay_t(const Mat& R, Mat& Y);
    double residual_t(const Mat& R, const Mat& Y);
    SignStats solve_impl(bool dual, const Mat& R, Mat& X);          // solve() / solve_t(): one refinement loop on replay[_t], residual[_t]
    SignLrStats solve_lr_impl(bool dual, const Mat& G, const Mat& S, double rtol, int max_width, int max_refine, Mat& L, Mat& D);
    Ctx* c_;
    int n_, maxiters_, max_refine_, iters_ = 0;
    double tol_, logdetE_ = 0.0;
    Mat E_, Einv_, F_, Z_, Zi_, Y_, W_, T_, Res_, Pstore_;
    std::vector<double> cs_;
    DevArr<int> piv_;
    DevArr<SignCtl> ctl_;
    DevArr<double> part_, nrm_;
};

// What went wrong in a sign iteration that ended with done = 2 (stagnated away from -E), 3 (non-finite), 4 (singular Z_k) or 5 (out of
// maxiters), shared by SignLyap and BatchedSignLyap, which put "dense path: " or "batched dense path, member b: " in front.  k: the iteration
// of the singular Z_k; dist: the last ||Z + E|| / ||E||.
std::string sign_failure(int done, int k, double dist, int maxiters);

// The single-problem back end of the stage program dense_ros.hpp, for dense_gdre_solve and dense_gdre_solve_adaptive: gemm with the tag
// "dense_ros", comb, copy_mat and lyap's factor / solve; the statistics of every solve are appended to solves.
struct DenseRosOps {
    using M = Mat;
    Ctx* ctx;
    SignLyap& lyap;
    std::vector<SignStats>& solves;
    void gemm(bool tA, bool tB, double alpha, const Mat& A, const Mat& B, double beta, Mat& C);
    void comb(Mat& out, double a0, const Mat& M0, double a1, const Mat* M1, double a2, const Mat* M2, bool sym);
    void copy(const Mat& src, Mat& dst);
    void factor(const Mat& F) { lyap.factor(F); }
    void solve(const Mat& R, Mat& X) { solves.push_back(lyap.solve(R, X)); }
};

// The argument checks the dense drivers share, each in front of any device work: the order, the operands' shapes (who: "dense path",
// "adaptive dense path"), and the fixed grid t0, t0 + dt, .. of floor((tf - t0) / dt) steps (dt finite, nonzero and pointing from t0 to tf).
void dense_check_order(int order);
void dense_check_shapes(const char* who, const Mat& E, const Mat& A, const Mat& B, const Mat& C, const Mat& X0);
std::vector<double> dense_time_grid(double t0, double tf, double dt);

struct DenseGdreResult {
    std::vector<double> t;
    std::vector<Mat> Kt;         // K(t_i)' as n x m
    std::vector<Mat> X;          // X(t_i): first and last, or all under save_state
    std::vector<SignStats> solves;
};
DenseGdreResult dense_gdre_solve(Ctx* ctx, const Mat& E, const Mat& A, const Mat& B, const Mat& C, const Mat& X0, double t0, double tf, double dt,
                                 int order, bool save_state, int maxiters, double tol, int max_refine);

}  // namespace dre
