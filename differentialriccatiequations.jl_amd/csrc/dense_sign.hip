// Dense path (GDREProblem{<:Matrix}, src/riccati/dense_ros{1,2,3,4}.jl of the reference):
//   SignLyap         generalized matrix-sign-function solver of F'XE + E'XF = -R (Benner & Quintana-Orti 1999) on the Gauss-Jordan
//                    inversion of dense_gj.hip, with the (P_k, c_k) sequence kept for further right-hand sides and for iterative
//                    refinement by replay;
//   dense_gdre_solve the fixed-grid Rosenbrock driver Ros1..Ros4, device resident (the stage program itself: dense_ros.hpp).
// The host model of exactly this iteration is tests/_sign_model.py.
#include "dense_sign.hpp"

#include <cmath>

#include "dense.hpp"
#include "dense_ros.hpp"
#include "dense_sign_body.hpp"
#include "profiling.hpp"

namespace dre {

// ---- element-wise kernels with fused partial norms: the bodies are dense_sign_body.hpp's, shared with dense_batch.hip --------------------
__global__ __launch_bounds__(256) void k_sign_update(int n, double* __restrict__ Z, double* __restrict__ Zi, const double* __restrict__ Y,
                                                     const double* __restrict__ E, double c, double* __restrict__ part) {
    sign_update_body(KERNEL_GRID_STRIDE, n, Z, Zi, Y, E, c, part);
}

// the stopping norm and the decision of the sign iteration
__global__ __launch_bounds__(256) void k_sign_decide(int nparts, const double* __restrict__ part, const double* __restrict__ nE2, double tol,
                                                     SignCtl* ctl) {
    double s[3];
    load_partials(nparts, part, s);
    if (threadIdx.x == 0) {
        const double e = sqrt(s[0] / nE2[0]), d = sqrt(s[1] / s[2]);
        ctl->dist = e; ctl->step = d;
        ctl->done = sign_decision(e, d, tol);
    }
}

__global__ __launch_bounds__(256) void k_res_sym(int n, const double* __restrict__ Rm, const double* __restrict__ G, double* __restrict__ Res,
                                                 double* __restrict__ part) {
    res_sym_body(KERNEL_GRID_STRIDE, n, Rm, G, Res, part);
}

__global__ __launch_bounds__(256) void k_res_finish(int nparts, const double* __restrict__ part, const double* __restrict__ nR2, SignCtl* ctl) {
    double s[1];
    load_partials(nparts, part, s);
    if (threadIdx.x == 0) ctl->res = relative_residual(s[0], nR2[0]);
}

// out = sym?(a0 M0 + a1 M1 + a2 M2), n x n column-major, M0 with ld ld0, the others with ld n (M1, M2 may be null); out may alias an input unless sym
__global__ __launch_bounds__(256) void k_comb(int n, double a0, const double* M0, int ld0, double a1, const double* M1, double a2,
                                              const double* M2, double* out, int sym) {
    const size_t tot = (size_t)n * n;
    const bool ij = sym || ld0 != n;                // (uniform) the row and column of an element are needed
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < tot; idx += (size_t)gridDim.x * blockDim.x) {
        const int i = ij ? idx % n : 0, j = ij ? idx / n : 0;
        double v = a0 * M0[ij ? i + (size_t)j * ld0 : idx] + (M1 ? a1 * M1[idx] : 0.0) + (M2 ? a2 * M2[idx] : 0.0);
        if (sym) {
            const size_t t = j + (size_t)i * n;
            v = 0.5 * (v + a0 * M0[j + (size_t)i * ld0] + (M1 ? a1 * M1[t] : 0.0) + (M2 ? a2 * M2[t] : 0.0));
        }
        out[idx] = v;
    }
}

void comb(Ctx* ctx, Mat& out, double a0, const Mat& M0, double a1, const Mat* M1, double a2, const Mat* M2, bool sym, const char* tag, int words) {
    const int n = out.rows;
    if (words == 0) words = 2 + (M1 != nullptr) + (M2 != nullptr);
    TimedScope ts(ctx, tag, 8.0 * words * n * n, 0.0);
    hipLaunchKernelGGL(k_comb, dim3(grid_for((size_t)n * n)), dim3(256), 0, ctx->stream, n, a0, (const double*)M0.p, M0.ld, a1,
                       (const double*)(M1 ? M1->p : nullptr), a2, (const double*)(M2 ? M2->p : nullptr), out.p, sym ? 1 : 0);
}

// ---- SignLyap --------------------------------------------------------------------------------------------------------------------
static Mat square(Ctx* ctx, int n) { return Mat(ctx, n, n); }

SignLyap::SignLyap(Ctx* ctx, const Mat& E, int maxiters, double tol, int max_refine, size_t extra_n2, bool lazy_dense)
    : c_(ctx), n_(E.rows), maxiters_(maxiters), max_refine_(max_refine), tol_(tol) {
    const int n = n_;
    DRE_REQUIRE(E.cols == n && n >= 1 && n <= DENSE_MAX_N, "dense path: E must be square of order 1 .. " + std::to_string(DENSE_MAX_N) +
                                                            " (the device's 32-bit index limit)");
    gj_check_order(ctx, n, "dense path");
    DRE_REQUIRE(E.ld == n, "dense path: E must be stored with leading dimension n");     // (the element-wise kernels index n x n operands densely)
    DRE_REQUIRE(maxiters >= 1 && maxiters <= 1000, "dense path: maxiters must be in 1 .. 1000");
    DRE_REQUIRE(max_refine >= 0, "dense path: max_refine must be >= 0");
    if (!(tol_ > 0.0)) tol_ = 10.0 * n * DBL_EPS;
    require_memory(ctx, ((size_t)maxiters + (lazy_dense ? 7 : 10) + extra_n2) * n * n);
    Pstore_ = Mat(ctx, n, n * maxiters);
    E_ = E;
    Einv_ = square(ctx, n); F_ = square(ctx, n); Z_ = square(ctx, n); Zi_ = square(ctx, n); Y_ = square(ctx, n);
    if (!lazy_dense) { W_ = square(ctx, n); T_ = square(ctx, n); Res_ = square(ctx, n); }
    piv_ = DevArr<int>(ctx, n);
    ctl_ = DevArr<SignCtl>(ctx, 1);
    part_ = DevArr<double>(ctx, 3 * NORM_PARTS);
    nrm_ = DevArr<double>(ctx, 2);
    DRE_HIP(hipMemsetAsync(ctl_.p, 0, sizeof(SignCtl), ctx->stream));
    // E^-1 and log|det E| once per solve
    copy_mat(ctx, E, Einv_);
    gj_invert(ctx, Einv_, piv_.p, &ctl_.p->gj);
    frob2_device(ctx, E, nrm_.p);
    const GjCtl h = read_back(ctx, ctl_.p).gj;
    if (h.singular) throw Error(ERR_SINGULAR, "dense path: E is singular (zero pivot in the Gauss-Jordan inversion)");
    logdetE_ = h.logdet;
}

void SignLyap::ensure_dense_work() {
    if (W_.p) return;
    require_memory(c_, (size_t)3 * n_ * n_);
    W_ = square(c_, n_); T_ = square(c_, n_); Res_ = square(c_, n_);
}

std::string sign_failure(int done, int k, double dist, int maxiters) {
    if (done == 4) return "singular Z_" + std::to_string(k) + " in the sign iteration (F singular?)";
    if (done == 2) return "the pencil is not c-stable (sign iteration stagnated at ||Z + E|| / ||E|| = " + std::to_string(dist) + ")";
    if (done == 3) return "the sign iteration produced non-finite values (pencil not c-stable?)";
    return "the sign iteration did not reach -E in " + std::to_string(maxiters) + " iterations (||Z + E|| / ||E|| = " + std::to_string(dist) +
           "); the pencil is not c-stable";
}

void SignLyap::factor(const Mat& F) {
    const int n = n_;
    DRE_REQUIRE(F.rows == n && F.cols == n, "dense path: F must be n x n");
    copy_mat(c_, F, F_);
    copy_mat(c_, F, Z_);
    copy_mat(c_, F, Zi_);
    cs_.clear();
    iters_ = 0;
    bool scale = true;
    SignCtl h;
    for (int k = 0; k < maxiters_; ++k) {
        gj_invert(c_, Zi_, piv_.p, &ctl_.p->gj);
        h = read_back(c_, ctl_.p);
        if (h.gj.singular) throw Error(ERR_SINGULAR, "dense path: " + sign_failure(4, k, 0.0, maxiters_));
        const double cfac = scale ? std::exp((h.gj.logdet - logdetE_) / n) : 1.0;
        Mat P = Pstore_.colsview(k * n, n);
        gemm(c_, false, false, 1.0, Zi_, E_, 0.0, P, nullptr, "sign_gemm");            // P_k = Z_k^-1 E
        gemm(c_, false, false, 1.0, E_, P, 0.0, Y_, nullptr, "sign_gemm");             // E P_k
        {
            TimedScope ts(c_, "sign_update", 40.0 * n * n, 0.0);
            hipLaunchKernelGGL(k_sign_update, dim3(NORM_PARTS), dim3(256), 0, c_->stream, n, Z_.p, Zi_.p, (const double*)Y_.p, (const double*)E_.p, cfac,
                               part_.p);
            hipLaunchKernelGGL(k_sign_decide, dim3(1), dim3(256), 0, c_->stream, NORM_PARTS, (const double*)part_.p, (const double*)nrm_.p, tol_, ctl_.p);
        }
        cs_.push_back(cfac);
        iters_ = k + 1;
        h = read_back(c_, ctl_.p);
        if (h.done == 1) return;
        if (h.done) throw Error(ERR_NOT_STABLE, "dense path: " + sign_failure(h.done, k, h.dist, maxiters_));
        if (h.dist < SCALE_OFF) scale = false;
    }
    throw Error(ERR_NOT_STABLE, "dense path: " + sign_failure(5, maxiters_, h.dist, maxiters_));
}

void SignLyap::replay(const Mat& R, Mat& X) {
    const int n = n_;
    copy_mat(c_, R, W_);
    for (int k = 0; k < iters_; ++k) {
        const Mat P = Pstore_.colsview(k * n, n);
        const double cf = cs_[(size_t)k];
        gemm(c_, false, false, 1.0, W_, P, 0.0, T_, nullptr, "sign_gemm");                     // W P
        gemm(c_, true, false, 0.5 * cf, P, T_, 1.0 / (2.0 * cf), W_, nullptr, "sign_gemm");    // W/(2c) + (c/2) P' W P
        comb(c_, Y_, 1.0, W_, 0.0, nullptr, 0.0, nullptr, true);
        std::swap(W_, Y_);
    }
    gemm(c_, false, false, 1.0, W_, Einv_, 0.0, T_, nullptr, "sign_gemm");                     // X = E^-T (W/2) E^-1
    gemm(c_, true, false, 0.5, Einv_, T_, 0.0, Y_, nullptr, "sign_gemm");
    comb(c_, X, 1.0, Y_, 0.0, nullptr, 0.0, nullptr, true);
}

double SignLyap::residual(const Mat& R, const Mat& X) {
    const int n = n_;
    gemm(c_, false, false, 1.0, X, E_, 0.0, T_, nullptr, "sign_gemm");       // X E
    gemm(c_, true, false, 1.0, F_, T_, 0.0, Y_, nullptr, "sign_gemm");       // F' X E
    TimedScope ts(c_, "sign_residual", 24.0 * n * n, 0.0);
    hipLaunchKernelGGL(k_res_sym, dim3(NORM_PARTS), dim3(256), 0, c_->stream, n, (const double*)R.p, (const double*)Y_.p, Res_.p, part_.p);
    hipLaunchKernelGGL(k_res_finish, dim3(1), dim3(256), 0, c_->stream, NORM_PARTS, (const double*)part_.p, (const double*)(nrm_.p + 1), ctl_.p);
    return read_back(c_, ctl_.p).res;
}

// solve() and solve_t() (the dual equation, below): the two directions differ in their replay and residual; the primal's residual wants
// ||R||_F^2 beforehand, the dual's takes it from its own pass
SignStats SignLyap::solve_impl(bool dual, const Mat& R, Mat& X) {
    const int n = n_;
    DRE_REQUIRE(R.rows == n && R.cols == n && R.ld == n && X.rows == n && X.cols == n && X.ld == n,
                dual ? "dense path: R and Y must be n x n" : "dense path: R and X must be n x n");
    DRE_REQUIRE(iters_ > 0, "dense path: factor() first");
    ensure_dense_work();
    if (!dual) frob2_device(c_, R, nrm_.p + 1);
    auto rep = [&](const Mat& rhs, Mat& out) { if (dual) replay_t(rhs, out); else replay(rhs, out); };
    auto res = [&] { return dual ? residual_t(R, X) : residual(R, X); };
    SignStats s;
    s.iters = iters_;
    rep(R, X);
    s.res0 = s.res = res();
    const double target = 100.0 * n * DBL_EPS;
    Mat dX = square(c_, n);
    while (s.res > target && s.refinements < max_refine_) {
        rep(Res_, dX);
        comb(c_, X, 1.0, X, 1.0, &dX);
        s.res = res();
        ++s.refinements;
    }
    return s;
}

SignStats SignLyap::solve(const Mat& R, Mat& X) { return solve_impl(false, R, X); }

// ---- the dual equation F Y E' + E Y F' = -R on the same kept sequence (host model: tests/_sign_dual_model.py) ------------------
// Res = R + G + G' (G = F Y E'), with the partial sums of squares of Res AND of R from the same pass: the dual solve needs no norm launch of its
// own for the right-hand side, and a refinement step re-reads R anyway
__global__ __launch_bounds__(256) void k_res_sym_norms(int n, const double* __restrict__ Rm, const double* __restrict__ G, double* __restrict__ Res,
                                                       double* __restrict__ part) {
    double s = 0.0, sr = 0.0;
    const size_t tot = (size_t)n * n;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < tot; idx += (size_t)gridDim.x * blockDim.x) {
        const int i = idx % n, j = idx / n;
        const double r = Rm[idx], v = r + G[idx] + G[j + (size_t)i * n];
        Res[idx] = v;
        s += v * v; sr += r * r;
    }
    store_partials(part, s, sr);
}

__global__ __launch_bounds__(256) void k_res_norms_finish(int nparts, const double* __restrict__ part, SignCtl* ctl) {
    double s[2];
    load_partials(nparts, part, s);
    if (threadIdx.x == 0) ctl->res = s[1] > 0.0 ? sqrt(s[0] / s[1]) : sqrt(s[0]);
}

// V_0 = sym(E^-1 R E^-T), V_{k+1} = sym(V_k / (2 c_k) + (c_k / 2) P_k V_k P_k'), Y = V_inf / 2: two GEMMs and one combiner pass per iteration as in
// replay(); the entry transform takes the place of replay()'s exit transform, and the last combiner pass carries the factor 1/2 and writes Y
void SignLyap::replay_t(const Mat& R, Mat& Y) {
    const int n = n_;
    gemm(c_, false, false, 1.0, Einv_, R, 0.0, T_, nullptr, "sign_gemm");                      // E^-1 R
    gemm(c_, false, true, 1.0, T_, Einv_, 0.0, Y_, nullptr, "sign_gemm");                      // E^-1 R E^-T
    comb(c_, W_, 1.0, Y_, 0.0, nullptr, 0.0, nullptr, true);
    for (int k = 0; k < iters_; ++k) {
        const Mat P = Pstore_.colsview(k * n, n);
        const double cf = cs_[(size_t)k];
        gemm(c_, false, false, 1.0, P, W_, 0.0, T_, nullptr, "sign_gemm");                     // P V
        gemm(c_, false, true, 0.5 * cf, T_, P, 1.0 / (2.0 * cf), W_, nullptr, "sign_gemm");    // V/(2c) + (c/2) P V P'
        if (k + 1 == iters_) comb(c_, Y, 0.5, W_, 0.0, nullptr, 0.0, nullptr, true);
        else {
            comb(c_, Y_, 1.0, W_, 0.0, nullptr, 0.0, nullptr, true);
            std::swap(W_, Y_);
        }
    }
}

double SignLyap::residual_t(const Mat& R, const Mat& Y) {
    const int n = n_;
    gemm(c_, false, true, 1.0, Y, E_, 0.0, T_, nullptr, "sign_gemm");        // Y E'
    gemm(c_, false, false, 1.0, F_, T_, 0.0, Y_, nullptr, "sign_gemm");      // F Y E'
    TimedScope ts(c_, "sign_residual", 24.0 * n * n, 0.0);
    hipLaunchKernelGGL(k_res_sym_norms, dim3(NORM_PARTS), dim3(256), 0, c_->stream, n, (const double*)R.p, (const double*)Y_.p, Res_.p, part_.p);
    hipLaunchKernelGGL(k_res_norms_finish, dim3(1), dim3(256), 0, c_->stream, NORM_PARTS, (const double*)part_.p, ctl_.p);
    return read_back(c_, ctl_.p).res;
}

SignStats SignLyap::solve_t(const Mat& R, Mat& Y) { return solve_impl(true, R, Y); }

// ---- Rosenbrock drivers (dense_ros{1,2,3,4}.jl of the reference): the stage program is dense_ros.hpp's ------------------------------
void DenseRosOps::gemm(bool tA, bool tB, double alpha, const Mat& A, const Mat& B, double beta, Mat& C) {
    dre::gemm(ctx, tA, tB, alpha, A, B, beta, C, nullptr, "dense_ros");
}
void DenseRosOps::comb(Mat& out, double a0, const Mat& M0, double a1, const Mat* M1, double a2, const Mat* M2, bool sym) {
    dre::comb(ctx, out, a0, M0, a1, M1, a2, M2, sym);
}
void DenseRosOps::copy(const Mat& src, Mat& dst) { copy_mat(ctx, src, dst); }

void dense_check_order(int order) { DRE_REQUIRE(order >= 1 && order <= 4, "dense path: order must be 1 .. 4"); }

void dense_check_shapes(const char* who, const Mat& E, const Mat& A, const Mat& B, const Mat& C, const Mat& X0) {
    const int n = E.rows;
    DRE_REQUIRE(E.cols == n && A.rows == n && A.cols == n && B.rows == n && C.cols == n && X0.rows == n && X0.cols == n,
                std::string(who) + ": E, A, X0 must be n x n, B n x m, C q x n");
}

std::vector<double> dense_time_grid(double t0, double tf, double dt) {
    DRE_REQUIRE(dt != 0.0 && std::isfinite(dt), "dense path: dt must be finite and nonzero");
    const int nsteps = (int)std::floor((tf - t0) / dt + 1e-9);
    DRE_REQUIRE(nsteps >= 0, "tspan and dt point in opposite directions");
    std::vector<double> t;
    for (int i = 0; i <= nsteps; ++i) t.push_back(t0 + i * dt);
    return t;
}

DenseGdreResult dense_gdre_solve(Ctx* ctx, const Mat& E, const Mat& A, const Mat& B, const Mat& C, const Mat& X0, double t0, double tf, double dt,
                                 int order, bool save_state, int maxiters, double tol, int max_refine) {
    const int n = E.rows, m = B.cols;
    dense_check_order(order);
    dense_check_shapes("dense path", E, A, B, C, X0);
    DenseGdreResult out;
    out.t = dense_time_grid(t0, tf, dt);
    const int nsteps = (int)out.t.size() - 1;
    // the sign solver's own (maxiters + 10) n^2, the driver's matrices (16 n^2 for Ros4) and the saved states
    SignLyap lyap(ctx, E, maxiters, tol, max_refine, 16 + (save_state ? (size_t)nsteps : 1));
    DenseRosOps ops{ctx, lyap, out.solves};
    auto sq = [&] { return Mat(ctx, n, n); };
    Mat X = sq(), CtC = sq();
    RosWork<Mat> w{sq(), sq(), sq(), sq(), sq(), sq(), sq(), sq(), sq(), sq(), Mat(ctx, n, m), Mat(ctx, n, m), Mat(ctx, n, m)};
    const RosOperands<Mat> p{E, A, B, CtC};
    copy_mat(ctx, X0, X);
    ops.gemm(true, false, 1.0, C, C, 0.0, CtC);
    // Kt = (B'XE)' = E'XB
    auto feedback = [&](const Mat& Xs) {
        Mat Kt(ctx, n, m);
        ros_EtKB(ops, p, w, Xs, Kt);
        return Kt;
    };
    auto save = [&](const Mat& Xs) { Mat c = sq(); copy_mat(ctx, Xs, c); out.X.push_back(c); };
    save(X);
    Mat Kt = feedback(X);
    out.Kt.push_back(Kt);
    for (int i = 1; i <= nsteps; ++i) {
        const double tau = out.t[(size_t)i - 1] - out.t[(size_t)i];
        ros_stages(ops, order, tau, p, X, Kt, w);
        ros_combine(ops, order, tau, X, w);
        if (save_state) save(X);
        Kt = feedback(X);
        out.Kt.push_back(Kt);
    }
    if (!save_state && nsteps > 0) save(X);         // (no step: X0 is the only state, as t and K have one entry)
    ctx->sync();
    return out;
}

}  // namespace dre
