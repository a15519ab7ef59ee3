// Batched dense path (dense_batch.hip): B independent problems of one order n side by side on one device, member b on a grid axis of every
// launch.  Stacks: member b of a rows x cols stack lies at base + (size_t)b * rows * cols (a Mat of rows x cols*B with ld = rows; member b is
// colsview(b * cols, cols)).  A member's result depends on that member's data only: no atomics, per-member grids that do not depend on B,
// per-member masks.  See DESIGN.md §9.3.
#pragma once
#include <string>
#include <vector>

#include "dense_sign.hpp"

namespace dre {

// Control block of one member (device resident, all B read back in one copy).  The sign iteration's decisions are taken on the device, so
// that a member that is finished or has failed drops out of the following launches without a host round trip per member.
struct BatchCtl {
    SignCtl s;          // the single path's words: inversion (logdet, singular), done, dist, step, res
    double logdetE;     // log|det E| of the member
    double res0;        // relative residual of the current solve before refinement
    int fail;           // 0, or the DRE error code that dropped the member from every later launch
    int iters;          // sign iterations of the member's current factorisation
    int scale;          // determinantal scaling still on
    int refine;         // the last residual asks for another refinement step
    int nref;           // refinement steps of the current solve
    int pad;
};

// Which members a launch leaves out (always: the failed ones).
enum : int {
    BM_LIVE = 0,
    BM_GJ = 1,          // ... and those whose running inversion met a zero pivot
    BM_FACTOR = 2,      // ... and those whose sign iteration has ended (or whose inversion met a zero pivot)
    BM_REPLAY = 4,      // ... and those whose factorisation has no iteration k
    BM_REFINE = 8,      // ... and those that need no further refinement step
};
struct BatchMask { const BatchCtl* ctl = nullptr; int mode = BM_LIVE; int k = 0; };      // ctl null: every member takes part

#if defined(__HIPCC__)
__device__ __forceinline__ bool batch_off(const BatchMask& m, int b) {
    if (!m.ctl) return false;
    const BatchCtl& c = m.ctl[b];
    if (c.fail) return true;
    if ((m.mode & (BM_GJ | BM_FACTOR)) && c.s.gj.singular) return true;
    if ((m.mode & BM_FACTOR) && c.s.done) return true;
    if ((m.mode & BM_REPLAY) && m.k >= c.iters) return true;
    if ((m.mode & BM_REFINE) && !c.refine) return true;
    return false;
}
#endif

// C_b = alpha op(A_b) op(B_b) + beta C_b for b < batch (gemm.hip, on gemm_tile): 64 x 64 tiles over the whole K, blockIdx.z = member, no
// split-K, no atomics; the tiling of one member does not depend on batch.  sA, sB, sC: member strides in doubles.  coef (optional): member b
// takes alpha = coef[b * coef_stride], beta = coef[b * coef_stride + 1] from device memory instead of the arguments.
void gemm_strided(Ctx* ctx, int batch, bool tA, bool tB, int M, int N, int K, double alpha, const double* A, int lda, size_t sA, const double* B,
                  int ldb, size_t sB, double beta, double* C, int ldc, size_t sC, BatchMask mask, const char* tag = "batch_gemm",
                  const double* coef = nullptr, size_t coef_stride = 0);

// Stack of n x n inverses in place with the register panel (n <= GJ_REGISTER_MAX_N): member b's interchanges in piv + b n, its log|det| and
// singular flag in ctl[b].s.gj.  Pn (n x nb per member) and W (nb x n per member) are work stacks of batch * n * gj_batch_nb(n) doubles each.
int gj_batch_nb(int n);
void gj_invert_batched(Ctx* ctx, int batch, int n, double* A, int* piv, BatchCtl* ctl, int mode, double* Pn, double* W);

// out_b = sym?(a0 M0_b + a1 M1_b + a2 M2_b) for stacks of rows x cols members (sym: square members, out must not alias an input)
void comb_batched(Ctx* ctx, int batch, int rows, int cols, double* out, double a0, const double* M0, double a1, const double* M1, double a2,
                  const double* M2, bool sym, BatchMask mask, const char* tag = "batch_comb");

struct BatchMemberStatus { int code = 0; std::string msg; };

// SignLyap for a stack of pencils (E_b fixed, F_b per factorisation).  No member's failure throws: it is recorded in status(), the member is
// dropped from every later launch and the others go on.
class BatchedSignLyap {
  public:
    // E: n x n*B stack (kept by reference).  DRE_ERR_ALLOC unless doubles_needed() doubles fit, before any kernel.
    BatchedSignLyap(Ctx* ctx, int batch, const Mat& E, int maxiters, double tol, int max_refine, size_t extra_n2 = 0);
    void factor(const Mat& F);                      // sign iteration on every live (F_b, E_b)
    // F_b' X_b E_b + E_b' X_b F_b = -R_b on the kept sequences, refined per member; stats[b] is written for live members
    void solve(const Mat& R, Mat& X, std::vector<SignStats>& stats);
    const std::vector<BatchMemberStatus>& status() const { return status_; }
    bool alive(int b) const { return status_[(size_t)b].code == 0; }
    int n() const { return n_; }
    int batch() const { return B_; }
    BatchMask live() const { return BatchMask{ctl_.p, BM_LIVE, 0}; }
    // B times the single path's (maxiters + 10 + extra_n2) n^2, plus the panel's work stacks Pn and W
    static size_t doubles_needed(int batch, int n, int maxiters, size_t extra_n2) {
        return (size_t)batch * (((size_t)maxiters + 10 + extra_n2) * n * n + (size_t)2 * n * gj_batch_nb(n));
    }

  private:
    void fetch();                                   // all B control blocks in one copy
    void replay(const Mat& R, Mat& X, int extra_mode);
    void residual(const Mat& R, const Mat& X, int extra_mode, int phase);
    Ctx* c_;
    int B_, n_, maxiters_, max_refine_, max_iters_live_ = 0;
    double tol_;
    size_t nn_;
    Mat E_, Einv_, F_, Z_, Zi_, Y_, W_, T_, Res_, dX_, Pstore_, Pn_, Wp_;
    DevArr<int> piv_;
    DevArr<BatchCtl> ctl_;
    DevArr<double> part_, nrm_, coef_;
    std::vector<BatchCtl> h_;
    std::vector<BatchMemberStatus> status_;
};

// Batched Ros1 / Ros2 (dense_gdre_solve's equations, operands and order of operations on stacks).  E, A, X0: n x n*B; Bm: n x m*B; C: q x n*B.
// out[b]: member b's result, cut after its last completed step when status[b].code != 0.
void dense_gdre_solve_batched(Ctx* ctx, int batch, const Mat& E, const Mat& A, const Mat& Bm, const Mat& C, const Mat& X0, int m, int q, double t0,
                              double tf, double dt, int order, bool save_state, int maxiters, double tol, int max_refine,
                              std::vector<DenseGdreResult>& out, std::vector<BatchMemberStatus>& status);
// device memory of that call in doubles (the formula of DESIGN.md §9.3)
size_t dense_gdre_batched_doubles(int batch, int n, int m, int q, int nsteps, int order, bool save_state, int maxiters);

}  // namespace dre
