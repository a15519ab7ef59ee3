// Dense generalized Sylvester solver (GSYLEProblem + MatrixSign); DESIGN.md §9.15, host model tests/_sylvester_model.py.
//
//   A X F + E X B = -C        (A, E n x n;  B, F m x m;  C, X n x m;  both pencils c-stable)
// by the coupled sign iteration of Benner, Quintana-Orti and Quintana-Orti: with A_0 = A, B_0 = B, C_0 = C
//   L_k = E A_k^-1,  R_k = B_k^-1 F                          two gj_invert, two GEMMs
//   A_{k+1} = A_k / (2c) + (c/2) L_k E                       one GEMM, sign_update_body (||A + E||^2, ||dA||^2, ||A||^2)
//   B_{k+1} = B_k / (2c) + (c/2) F R_k                       the same at order m
//   C_{k+1} = C_k / (2c) + (c/2) L_k C_k R_k                 two GEMMs, the rectangular update (||dC||^2, ||C||^2)
// A_k -> -E, B_k -> -F, X = E^-1 C_inf F^-1 / 2.  c is ONE factor for both sides, the determinant scaling of the block matrix
//   c_k = exp((log|det A_k| + log|det B_k| - log|det E| - log|det F|) / (n + m)),
// formed on the device from the two inversions' control words (k_sylv_scale) and switched off, c = 1, once both distances are below SCALE_OFF:
// separate factors per side would break the recursion of C, whose two factors L_k and R_k must belong to the same scaled step.
// The decision rule is sylvester_decide.hpp's; the host reads the control struct back once per iteration and keeps c_k with L_k and R_k.
//
// The kept sequence (L_k, R_k, c_k) serves every further right-hand side (replay: the recursion of C alone), the refinement (the residual is
// replayed and added, the rule of SignLyap::solve_impl) and the transposed equation A'Y F' + E'Y B' = -C:
//   V_0 = E^-T C F^-T,  V_{k+1} = V_k / (2c) + (c/2) L_k' V_k R_k',  Y = V_inf / 2          (no back-transformation)
// A right-hand side that rides along in factor_solve passes through the same launches as a replay, so both give the same bits.
// Everything runs on the context's stream; nothing is allocated inside a loop.  The memory count: dense_sylvester.hpp.
#include "dense_sylvester.hpp"

#include <cmath>

#include "dense.hpp"
#include "dense_sign_body.hpp"
#include "profiling.hpp"

namespace dre {

static_assert(SYLV_STAG_STEP == STAG_STEP && SYLV_STAG_DIST == STAG_DIST, "sylvester_decide.hpp repeats the constants of dense_sign_body.hpp");

// the partial sums of one iteration: [0, 3) the left pencil's, [3, 6) the right pencil's, [6, 8) the right-hand side's (NORM_PARTS each); a
// residual evaluation uses [0, 4)
static constexpr int PART_A = 0, PART_B = 3, PART_C = 6, PART_SETS = 8;

__global__ void k_sylv_ctl_init(SylvCtl* c) {
    c->gjA.logdet = 0.0; c->gjA.singular = 0;
    c->gjB.logdet = 0.0; c->gjB.singular = 0;
    c->c = 1.0; c->done = 0; c->side = 0;
    c->distA = 0.0; c->distB = 0.0; c->stepA = 0.0; c->stepB = 0.0; c->stepC = 0.0;
    c->res = 0.0; c->scaled = 0.0; c->resnorm = 0.0;
}

// the joint scaling factor of the iteration whose two inversions have just run (logdetEF = log|det E| + log|det F|, order = n + m)
__global__ void k_sylv_scale(SylvCtl* c, int scale, double logdetEF, int order) {
    c->c = scale ? exp((c->gjA.logdet + c->gjB.logdet - logdetEF) / order) : 1.0;
}

// one side's update Z <- Z / (2c) + (c/2) Y with c from the control struct: the body is the Lyapunov solver's
__global__ __launch_bounds__(256) void k_sylv_side_update(int n, double* __restrict__ Z, double* __restrict__ Zi, const double* __restrict__ Y,
                                                          const double* __restrict__ E, const SylvCtl* ctl, double* __restrict__ part) {
    sign_update_body(KERNEL_GRID_STRIDE, n, Z, Zi, Y, E, ctl->c, part);
}

// the rectangular update W <- W / (2c) + (c/2) U over tot = n m elements, with the partial sums of ||dW||^2 and ||W||^2; c from the control
// struct (ctl non-null: the running iteration) or the kept value (replay)
__global__ __launch_bounds__(256) void k_sylv_rect_update(size_t tot, double* __restrict__ W, const double* __restrict__ U, const SylvCtl* ctl, double c,
                                                          double* __restrict__ part) {
    const GridStride g = KERNEL_GRID_STRIDE;
    const double cf = ctl ? ctl->c : c;
    double s0 = 0.0, s1 = 0.0;
    for (size_t idx = g.first; idx < tot; idx += g.step) {
        const double w = W[idx], wn = w / (2.0 * cf) + (0.5 * cf) * U[idx];
        const double d = wn - w;
        s0 += d * d; s1 += wn * wn;
        W[idx] = wn;
    }
    store_partials(part, s0, s1);
}

// the decision of one coupled iteration: one workgroup adds the three sets of partial sums in a fixed order and applies sylvester_decide
__global__ __launch_bounds__(256) void k_sylv_decide(int nparts, const double* __restrict__ part, const double* __restrict__ nEF2, double tol, SylvCtl* c) {
    double s[PART_SETS];
    load_partials(nparts, part, s);
    if (threadIdx.x != 0) return;
    const double eA = sqrt(s[PART_A] / nEF2[0]), dA = sqrt(s[PART_A + 1] / s[PART_A + 2]);
    const double eB = sqrt(s[PART_B] / nEF2[1]), dB = sqrt(s[PART_B + 1] / s[PART_B + 2]);
    const double dC = sylvester_rel_step(s[PART_C], s[PART_C + 1]);
    const SylvDecision d = sylvester_decide(eA, eB, dA, dB, dC, c->gjA.singular, c->gjB.singular, tol);
    c->distA = eA; c->distB = eB; c->stepA = dA; c->stepB = dB; c->stepC = dC;
    c->done = d.done; c->side = d.side;
}

// Res = C + G1 + G2 (G1 = A X F, G2 = E X B, or the transposed products) over tot = n m elements and the partial sums of ||Res||^2, ||C||^2,
// ||G1||^2, ||G2||^2 in one pass
__global__ __launch_bounds__(256) void k_sylv_residual(size_t tot, const double* __restrict__ Cm, const double* __restrict__ G1, const double* __restrict__ G2,
                                                       double* __restrict__ Res, double* __restrict__ part) {
    const GridStride g = KERNEL_GRID_STRIDE;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (size_t idx = g.first; idx < tot; idx += g.step) {
        const double cv = Cm[idx], g1 = G1[idx], g2 = G2[idx], v = cv + g1 + g2;
        Res[idx] = v;
        s0 += v * v; s1 += cv * cv; s2 += g1 * g1; s3 += g2 * g2;
    }
    store_partials(part, s0, s1, s2, s3);
}

// the residual's norms, and the step of the right-hand side's last update from its own set of partial sums (stepc: null when there is none)
__global__ __launch_bounds__(256) void k_sylv_residual_finish(int nparts, const double* __restrict__ part, const double* __restrict__ stepc, SylvCtl* c) {
    double s[4], sc[2] = {0.0, 0.0};
    load_partials(nparts, part, s);
    if (stepc) load_partials(nparts, stepc, sc);
    if (threadIdx.x != 0) return;
    const double r = sqrt(s[0]), den = sqrt(s[1]) + sqrt(s[2]) + sqrt(s[3]);
    c->resnorm = r;
    c->res = relative_residual(s[0], s[1]);
    c->scaled = den > 0.0 ? r / den : r;
    if (stepc) c->stepC = sylvester_rel_step(sc[0], sc[1]);
}

// X += D over tot elements
__global__ __launch_bounds__(256) void k_sylv_add(size_t tot, double* __restrict__ X, const double* __restrict__ D) {
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < tot; idx += (size_t)gridDim.x * blockDim.x) X[idx] += D[idx];
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
namespace {

const char* side_name(int side) { return side == SYLV_SIDE_LEFT ? "left pencil (A, E)" : "right pencil (B, F)"; }

// the "what" of a coupled iteration that ended with done > 1, behind "dense Sylvester: "
std::string sylvester_failure(const SylvCtl& h, int done, int k, int maxiters) {
    const bool left = h.side == SYLV_SIDE_LEFT;
    const std::string dist = std::string(left ? "||A_k + E|| / ||E|| = " : "||B_k + F|| / ||F|| = ") + std::to_string(left ? h.distA : h.distB);
    if (done == SYLV_SINGULAR) return std::string("singular ") + (left ? "A_" : "B_") + std::to_string(k) + " in the sign iteration (" + (left ? "A" : "B") +
                                      " singular?)";
    if (done == SYLV_STAGNATED) return std::string("the ") + side_name(h.side) + " is not c-stable (sign iteration stagnated at " + dist + ")";
    if (done == SYLV_NON_FINITE) return std::string("the sign iteration produced non-finite values on the ") + side_name(h.side) + " (pencil not c-stable?)";
    return std::string("the sign iteration did not reach (-E, -F) in ") + std::to_string(maxiters) + " iterations (" + dist + "); the " + side_name(h.side) +
           " is not c-stable";
}

const char* RHS_NON_FINITE = "dense Sylvester: the right-hand side C has non-finite entries";

// the shapes of one problem, before any device work (E, F null: the identity)
void check_shapes(Ctx* ctx, const char* who, const Mat* E, const Mat& A, const Mat* F, const Mat& B, const Mat& C, const Mat* X) {
    const int n = A.rows, m = B.rows;
    const std::string w(who);
    DRE_REQUIRE(n >= 1 && n <= DENSE_MAX_N && m >= 1 && m <= DENSE_MAX_N, w + ": A and B must be square of orders 1 .. " + std::to_string(DENSE_MAX_N) +
                                                                              " (the device's 32-bit index limit)");
    DRE_REQUIRE(A.cols == n && B.cols == m, w + ": A must be n x n and B m x m");
    DRE_REQUIRE((!E || (E->rows == n && E->cols == n)) && (!F || (F->rows == m && F->cols == m)), w + ": E must be n x n and F m x m");
    DRE_REQUIRE(A.ld == n && B.ld == m && (!E || E->ld == n) && (!F || F->ld == m), w + ": E, A, F and B must be stored with leading dimensions n and m");
    DRE_REQUIRE(C.rows == n && C.cols == m && C.ld == n, w + ": C must be n x m with leading dimension n");
    DRE_REQUIRE(!X || (X->rows == n && X->cols == m && X->ld == n), w + ": X must be n x m with leading dimension n");
    gj_check_order(ctx, n, who);
    gj_check_order(ctx, m, who);
}

Mat identity(Ctx* ctx, int n) {
    Mat I(ctx, n, n);
    set_identity(ctx, I);
    return I;
}

// Res = C + A X F + E X B (transposed: C + A'X F' + E'X B') through the products T = X F, G1 = A T, T = X B, G2 = E T, and its norms into ctl
// (stepc: k_sylv_residual_finish's); no synchronisation
void residual_launch(Ctx* ctx, bool tr, const Mat& E, const Mat& A, const Mat& F, const Mat& B, const Mat& C, const Mat& X, Mat& T, Mat& G1, Mat& G2,
                     Mat& Res, double* part, const double* stepc, SylvCtl* ctl) {
    const size_t tot = (size_t)C.rows * C.cols;
    gemm(ctx, false, tr, 1.0, X, F, 0.0, T, nullptr, "sylv_gemm");           // X F       (transposed: X F')
    gemm(ctx, tr, false, 1.0, A, T, 0.0, G1, nullptr, "sylv_gemm");          // A X F     (A'X F')
    gemm(ctx, false, tr, 1.0, X, B, 0.0, T, nullptr, "sylv_gemm");           // X B       (X B')
    gemm(ctx, tr, false, 1.0, E, T, 0.0, G2, nullptr, "sylv_gemm");          // E X B     (E'X B')
    TimedScope ts(ctx, "sylv_residual", 40.0 * tot, 0.0);
    hipLaunchKernelGGL(k_sylv_residual, dim3(NORM_PARTS), dim3(256), 0, ctx->stream, tot, (const double*)C.p, (const double*)G1.p, (const double*)G2.p, Res.p,
                       part);
    hipLaunchKernelGGL(k_sylv_residual_finish, dim3(1), dim3(256), 0, ctx->stream, NORM_PARTS, (const double*)part, stepc, ctl);
}

}  // namespace

// ---- SignSylvester ------------------------------------------------------------------------------------------------------------------
SignSylvester::SignSylvester(Ctx* ctx, const Mat& E, const Mat& F, int maxiters, double tol, int max_refine, size_t extra)
    : c_(ctx), n_(E.rows), m_(F.rows), maxiters_(maxiters), max_refine_(max_refine), tol_(tol) {
    const int n = n_, m = m_;
    const char* who = "dense Sylvester";
    DRE_REQUIRE(n >= 1 && n <= DENSE_MAX_N && m >= 1 && m <= DENSE_MAX_N && E.cols == n && F.cols == m,
                std::string(who) + ": E and F must be square of orders 1 .. " + std::to_string(DENSE_MAX_N) + " (the device's 32-bit index limit)");
    DRE_REQUIRE(E.ld == n && F.ld == m, std::string(who) + ": E and F must be stored with leading dimensions n and m");
    gj_check_order(ctx, n, who);
    gj_check_order(ctx, m, who);
    DRE_REQUIRE(maxiters >= 1 && maxiters <= 1000, std::string(who) + ": maxiters must be in 1 .. 1000");
    DRE_REQUIRE(max_refine >= 0, std::string(who) + ": max_refine must be >= 0");
    tol_ = sylvester_default_tol(n, m, tol);
    const size_t n2 = (size_t)n * n, m2 = (size_t)m * m, nm = (size_t)n * m;
    require_memory(ctx, ((size_t)maxiters + 5) * (n2 + m2) + 7 * nm + extra);       // (the count: dense_sylvester.hpp)
    Lstore_ = Mat(ctx, n, n * maxiters);
    Rstore_ = Mat(ctx, m, m * maxiters);
    E_ = E; F_ = F;
    Einv_ = Mat(ctx, n, n); A_ = Mat(ctx, n, n); Ak_ = Mat(ctx, n, n); Ai_ = Mat(ctx, n, n); YA_ = Mat(ctx, n, n);
    Finv_ = Mat(ctx, m, m); B_ = Mat(ctx, m, m); Bk_ = Mat(ctx, m, m); Bi_ = Mat(ctx, m, m); YB_ = Mat(ctx, m, m);
    W_ = Mat(ctx, n, m); T_ = Mat(ctx, n, m); U_ = Mat(ctx, n, m); G1_ = Mat(ctx, n, m); G2_ = Mat(ctx, n, m); Res_ = Mat(ctx, n, m); dX_ = Mat(ctx, n, m);
    piv_ = DevArr<int>(ctx, (size_t)std::max(n, m));
    ctl_ = DevArr<SylvCtl>(ctx, 1);
    part_ = DevArr<double>(ctx, (size_t)PART_SETS * NORM_PARTS);
    nrm_ = DevArr<double>(ctx, 2);
    hipLaunchKernelGGL(k_sylv_ctl_init, dim3(1), dim3(1), 0, ctx->stream, ctl_.p);
    // E^-1, F^-1, their log-determinants and norms once
    copy_mat(ctx, E, Einv_);
    gj_invert(ctx, Einv_, piv_.p, &ctl_.p->gjA);
    copy_mat(ctx, F, Finv_);
    gj_invert(ctx, Finv_, piv_.p, &ctl_.p->gjB);
    frob2_device(ctx, E, nrm_.p);
    frob2_device(ctx, F, nrm_.p + 1);
    const SylvCtl h = read_back(ctx, ctl_.p);
    if (h.gjA.singular) throw Error(ERR_SINGULAR, std::string(who) + ": E is singular (zero pivot in the Gauss-Jordan inversion)");
    if (h.gjB.singular) throw Error(ERR_SINGULAR, std::string(who) + ": F is singular (zero pivot in the Gauss-Jordan inversion)");
    logdetEF_ = h.gjA.logdet + h.gjB.logdet;
}

// one step of the right-hand side's recursion on W_: W <- W / (2c) + (c/2) L W R (transposed: L'W R'), c from the control struct or the kept value
void SignSylvester::c_step(bool tr, const Mat& L, const Mat& R, double c, bool c_on_device) {
    const size_t tot = (size_t)n_ * m_;
    gemm(c_, tr, false, 1.0, L, W_, 0.0, T_, nullptr, "sylv_gemm");          // L W       (L'W)
    gemm(c_, false, tr, 1.0, T_, R, 0.0, U_, nullptr, "sylv_gemm");          // L W R     (L'W R')
    TimedScope ts(c_, "sylv_rect_update", 24.0 * tot, 0.0);
    hipLaunchKernelGGL(k_sylv_rect_update, dim3(NORM_PARTS), dim3(256), 0, c_->stream, tot, W_.p, (const double*)U_.p,
                       (const SylvCtl*)(c_on_device ? ctl_.p : nullptr), c, part_.p + (size_t)PART_C * NORM_PARTS);
}

void SignSylvester::factor_impl(const Mat& A, const Mat& B, const Mat* C) {
    const int n = n_, m = m_;
    DRE_REQUIRE(A.rows == n && A.cols == n && B.rows == m && B.cols == m, "dense Sylvester: A must be n x n and B m x m");
    copy_mat(c_, A, A_); copy_mat(c_, A, Ak_); copy_mat(c_, A, Ai_);
    copy_mat(c_, B, B_); copy_mat(c_, B, Bk_); copy_mat(c_, B, Bi_);
    if (C) copy_mat(c_, *C, W_);
    DRE_HIP(hipMemsetAsync(part_.p, 0, (size_t)PART_SETS * NORM_PARTS * sizeof(double), c_->stream));      // (no C: its sums stay 0, its step 0)
    cs_.clear();
    iters_ = 0;
    bool scale = true;
    SylvCtl h{};
    for (int k = 0; k < maxiters_; ++k) {
        gj_invert(c_, Ai_, piv_.p, &ctl_.p->gjA);
        gj_invert(c_, Bi_, piv_.p, &ctl_.p->gjB);
        hipLaunchKernelGGL(k_sylv_scale, dim3(1), dim3(1), 0, c_->stream, ctl_.p, scale ? 1 : 0, logdetEF_, n + m);
        Mat L = Lstore_.colsview(k * n, n), R = Rstore_.colsview(k * m, m);
        gemm(c_, false, false, 1.0, E_, Ai_, 0.0, L, nullptr, "sylv_gemm");          // L_k = E A_k^-1
        gemm(c_, false, false, 1.0, L, E_, 0.0, YA_, nullptr, "sylv_gemm");          // L_k E
        gemm(c_, false, false, 1.0, Bi_, F_, 0.0, R, nullptr, "sylv_gemm_b");          // R_k = B_k^-1 F
        gemm(c_, false, false, 1.0, F_, R, 0.0, YB_, nullptr, "sylv_gemm_b");          // F R_k
        if (C) c_step(false, L, R, 0.0, true);
        {
            TimedScope ts(c_, "sylv_update", 40.0 * ((double)n * n + (double)m * m), 0.0);
            hipLaunchKernelGGL(k_sylv_side_update, dim3(NORM_PARTS), dim3(256), 0, c_->stream, n, Ak_.p, Ai_.p, (const double*)YA_.p, (const double*)E_.p,
                               (const SylvCtl*)ctl_.p, part_.p + (size_t)PART_A * NORM_PARTS);
            hipLaunchKernelGGL(k_sylv_side_update, dim3(NORM_PARTS), dim3(256), 0, c_->stream, m, Bk_.p, Bi_.p, (const double*)YB_.p, (const double*)F_.p,
                               (const SylvCtl*)ctl_.p, part_.p + (size_t)PART_B * NORM_PARTS);
            hipLaunchKernelGGL(k_sylv_decide, dim3(1), dim3(256), 0, c_->stream, NORM_PARTS, (const double*)part_.p, (const double*)nrm_.p, tol_, ctl_.p);
        }
        h = read_back(c_, ctl_.p);
        if (h.done == SYLV_SINGULAR) { iters_ = 0; throw Error(ERR_SINGULAR, "dense Sylvester: " + sylvester_failure(h, h.done, k, maxiters_)); }
        cs_.push_back(h.c);
        iters_ = k + 1;
        if (h.done == SYLV_CONVERGED) return;
        if (h.done == SYLV_NON_FINITE && h.side == SYLV_SIDE_RHS) { iters_ = 0; throw Error(ERR_INVALID, RHS_NON_FINITE); }
        if (h.done) { iters_ = 0; throw Error(ERR_NOT_STABLE, "dense Sylvester: " + sylvester_failure(h, h.done, k, maxiters_)); }
        if (h.distA < SCALE_OFF && h.distB < SCALE_OFF) scale = false;
    }
    iters_ = 0;
    h.side = h.distA > tol_ ? SYLV_SIDE_LEFT : SYLV_SIDE_RIGHT;
    throw Error(ERR_NOT_STABLE, "dense Sylvester: " + sylvester_failure(h, SYLV_OUT_OF_ITERS, maxiters_, maxiters_));
}

// X = E^-1 W F^-1 / 2 from the recursion's limit in W_
void SignSylvester::exit_transform(Mat& X) {
    gemm(c_, false, false, 1.0, Einv_, W_, 0.0, T_, nullptr, "sylv_gemm");
    gemm(c_, false, false, 0.5, T_, Finv_, 0.0, X, nullptr, "sylv_gemm");
}

void SignSylvester::replay(bool tr, const Mat& C, Mat& X) {
    const int n = n_, m = m_;
    if (tr) {
        gemm(c_, true, false, 1.0, Einv_, C, 0.0, T_, nullptr, "sylv_gemm");         // E^-T C
        gemm(c_, false, true, 1.0, T_, Finv_, 0.0, W_, nullptr, "sylv_gemm");        // E^-T C F^-T
    } else {
        copy_mat(c_, C, W_);
    }
    for (int k = 0; k < iters_; ++k) c_step(tr, Lstore_.colsview(k * n, n), Rstore_.colsview(k * m, m), cs_[(size_t)k], false);
    if (tr) copy_mat(c_, W_, X, 0.5);
    else exit_transform(X);
}

SylvCtl SignSylvester::residual(bool tr, const Mat& C, const Mat& X) {
    residual_launch(c_, tr, E_, A_, F_, B_, C, X, T_, G1_, G2_, Res_, part_.p, part_.p + (size_t)PART_C * NORM_PARTS, ctl_.p);
    return read_back(c_, ctl_.p);
}

// solve(), solve_t() and the tail of factor_solve() (have_x: X already holds the ride-along's solution): SignLyap::solve_impl's refinement loop
SylvStats SignSylvester::solve_impl(bool tr, const Mat& C, Mat& X, bool have_x) {
    const int n = n_, m = m_;
    DRE_REQUIRE(C.rows == n && C.cols == m && C.ld == n && X.rows == n && X.cols == m && X.ld == n, "dense Sylvester: C and X must be n x m");
    DRE_REQUIRE(iters_ > 0, "dense Sylvester: factor() first");
    const size_t tot = (size_t)n * m;
    SylvStats s;
    s.iters = iters_;
    if (!have_x) replay(tr, C, X);
    SylvCtl h = residual(tr, C, X);
    s.step = h.stepC;
    s.res0 = s.res = h.res;
    const double target = sylvester_refine_target(n, m);
    while (s.res > target && s.refinements < max_refine_) {
        replay(tr, Res_, dX_);
        {
            TimedScope ts(c_, "sylv_add", 24.0 * tot, 0.0);
            hipLaunchKernelGGL(k_sylv_add, dim3(grid_for(tot)), dim3(256), 0, c_->stream, tot, X.p, (const double*)dX_.p);
        }
        s.res = residual(tr, C, X).res;
        ++s.refinements;
    }
    if (!std::isfinite(s.res)) throw Error(ERR_INVALID, RHS_NON_FINITE);
    return s;
}

SylvStats SignSylvester::factor_solve(const Mat& A, const Mat& B, const Mat& C, Mat& X) {
    DRE_REQUIRE(C.rows == n_ && C.cols == m_ && C.ld == n_ && X.rows == n_ && X.cols == m_ && X.ld == n_, "dense Sylvester: C and X must be n x m");
    factor_impl(A, B, &C);
    exit_transform(X);
    return solve_impl(false, C, X, true);
}

// ---- the one-shot entry points -------------------------------------------------------------------------------------------------------------
DenseSylvesterResult dense_sylvester_solve(Ctx* ctx, const Mat* E, const Mat& A, const Mat* F, const Mat& B, const Mat& C, bool transposed, int maxiters,
                                           double tol, int max_refine) {
    const char* who = "dense Sylvester";
    check_shapes(ctx, who, E, A, F, B, C, nullptr);
    DRE_REQUIRE(maxiters >= 1 && maxiters <= 1000, std::string(who) + ": maxiters must be in 1 .. 1000");
    DRE_REQUIRE(max_refine >= 0, std::string(who) + ": max_refine must be >= 0");
    const int n = A.rows, m = B.rows;
    const size_t extra = (size_t)n * m + (E ? 0 : (size_t)n * n) + (F ? 0 : (size_t)m * m);         // X and the identities
    SignSylvester s(ctx, E ? *E : identity(ctx, n), F ? *F : identity(ctx, m), maxiters, tol, max_refine, extra);
    DenseSylvesterResult out;
    out.X = Mat(ctx, n, m);
    if (transposed) {
        s.factor(A, B);
        out.st = s.solve_t(C, out.X);
    } else {
        out.st = s.factor_solve(A, B, C, out.X);
    }
    ctx->sync();
    return out;
}

Mat dense_sylvester_residual(Ctx* ctx, const Mat* E, const Mat& A, const Mat* F, const Mat& B, const Mat& C, const Mat& X, bool transposed, double* fro,
                             double* scaled) {
    const char* who = "dense Sylvester residual";
    check_shapes(ctx, who, E, A, F, B, C, &X);
    const int n = A.rows, m = B.rows;
    require_memory(ctx, 5 * (size_t)n * m + (E ? 0 : (size_t)n * n) + (F ? 0 : (size_t)m * m));
    const Mat Em = E ? *E : identity(ctx, n), Fm = F ? *F : identity(ctx, m);
    Mat T(ctx, n, m), G1(ctx, n, m), G2(ctx, n, m), Res(ctx, n, m);
    DevArr<double> part(ctx, (size_t)4 * NORM_PARTS);
    DevArr<SylvCtl> ctl(ctx, 1);
    hipLaunchKernelGGL(k_sylv_ctl_init, dim3(1), dim3(1), 0, ctx->stream, ctl.p);
    residual_launch(ctx, transposed, Em, A, Fm, B, C, X, T, G1, G2, Res, part.p, nullptr, ctl.p);
    const SylvCtl h = read_back(ctx, ctl.p);
    if (fro) *fro = h.resnorm;
    if (scaled) *scaled = h.scaled;
    return Res;
}

}  // namespace dre
