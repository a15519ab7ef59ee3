// Square-root balanced truncation from factored Gramians (host restatement: tests/_svd_jacobi_model.py, balance).
//
//   Z_c = L_c sqrt(d_c), Z_o = L_o sqrt(d_o) over the positive entries;  M = Z_o'(E Z_c) = U Sigma V' (svd_jacobi);
//   W = Z_o U_r Sigma_r^{-1/2},  T = Z_c V_r Sigma_r^{-1/2};  A_r = W'A T, B_r = W'B, C_r = C T;  W'E T = I by construction.
// Every product goes through gemm(); the two kernels here scale columns.
#include "balance.hpp"

#include <cmath>

#include "dense_gj.hpp"
#include "profiling.hpp"
#include "svd_jacobi.hpp"

namespace dre {

namespace {

// Z(:, j) = L(:, idx[j]) * sqrt(d[idx[j] * stride])
__global__ __launch_bounds__(256) void k_bal_sqrt_cols(int n, int cols, const double* __restrict__ L, size_t ldl, const double* __restrict__ d, size_t stride,
                                                       const int* __restrict__ idx, double* __restrict__ Z, size_t ldz) {
    const size_t tot = (size_t)n * (size_t)cols;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(e % (size_t)n), j = (int)(e / (size_t)n);
        const size_t src = (size_t)idx[j];
        Z[(size_t)i + (size_t)j * ldz] = L[(size_t)i + src * ldl] * sqrt(d[src * stride]);
    }
}

// X(:, j) <- X(:, j) / sqrt(s[j])
__global__ __launch_bounds__(256) void k_bal_scale_cols(int n, int cols, double* __restrict__ X, size_t ldx, const double* __restrict__ s) {
    const size_t tot = (size_t)n * (size_t)cols;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < tot; e += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(e % (size_t)n), j = (int)(e / (size_t)n);
        X[(size_t)i + (size_t)j * ldx] /= sqrt(s[j]);
    }
}

// element stride of the r entries of D: a diagonal matrix, a column or a row; -1: neither
long diag_stride(const Mat& D, int r) {
    if (D.rows == r && D.cols == r) return (long)D.ld + 1;
    if (D.rows == r && D.cols == 1) return 1;
    if (D.rows == 1 && D.cols == r) return D.ld;
    return -1;
}

struct SqrtFactor { Mat Z; long dropped = 0; double neg_max = 0.0; };

SqrtFactor sqrt_factor(Ctx* ctx, const Mat& L, const Mat& D) {
    SqrtFactor f;
    const int n = L.rows, r = L.cols;
    const size_t stride = (size_t)diag_stride(D, r);
    std::vector<double> d(r);
    if (r) {
        DRE_HIP(hipMemcpy2DAsync(d.data(), sizeof(double), D.p, stride * sizeof(double), sizeof(double), r, hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
    }
    std::vector<int> idx;
    for (int j = 0; j < r; ++j) {
        if (d[j] > 0.0) idx.push_back(j);
        else { ++f.dropped; f.neg_max = std::isnan(d[j]) ? d[j] : std::max(f.neg_max, std::fabs(d[j])); }
    }
    DRE_REQUIRE(!std::isnan(f.neg_max), "balance_lr: a Gramian factor has a non-finite diagonal entry");
    const int cols = (int)idx.size();
    f.Z = Mat(ctx, n, cols);
    if (cols && n) {
        DevArr<int> didx(ctx, idx.size());
        didx.upload(ctx, idx);
        TimedScope ts(ctx, "bal_scale", 16.0 * n * cols, 0.0);
        hipLaunchKernelGGL(k_bal_sqrt_cols, dim3(grid_for((size_t)n * cols)), dim3(256), 0, ctx->stream, n, cols, (const double*)L.p, (size_t)L.ld, (const double*)D.p,
                           stride, (const int*)didx.p, f.Z.p, (size_t)f.Z.ld);
        ctx->sync();          // (didx is released on return)
    }
    return f;
}

void scale_cols(Ctx* ctx, Mat& X, const double* s_dev) {
    if (X.empty()) return;
    TimedScope ts(ctx, "bal_scale", 16.0 * X.rows * X.cols, 0.0);
    hipLaunchKernelGGL(k_bal_scale_cols, dim3(grid_for((size_t)X.rows * X.cols)), dim3(256), 0, ctx->stream, X.rows, X.cols, X.p, (size_t)X.ld, s_dev);
}

}  // namespace

BalanceResult balance_lr(Ctx* ctx, const Mat& E, const Mat& A, const Mat& B, const Mat& C, const Mat& Lc, const Mat& Dc, const Mat& Lo, const Mat& Do,
                         int order, double tol) {
    const int n = E.rows;
    DRE_REQUIRE(n >= 1 && E.cols == n && A.rows == n && A.cols == n, "balance_lr: E and A must be n x n");
    DRE_REQUIRE(n <= DENSE_MAX_N, "balance_lr: order beyond the device's 32-bit index limit");
    DRE_REQUIRE(B.rows == n && C.cols == n, "balance_lr: B must have n rows and C n columns");
    DRE_REQUIRE(Lc.rows == n && Lo.rows == n, "balance_lr: the Gramian factors must have n rows");
    DRE_REQUIRE(diag_stride(Dc, Lc.cols) > 0 && diag_stride(Do, Lo.cols) > 0, "balance_lr: D must be a diagonal matrix or a vector matching its factor's columns");
    DRE_REQUIRE(order >= 0, "balance_lr: negative order");
    DRE_REQUIRE(order > 0 || (tol >= 0.0 && std::isfinite(tol)), "balance_lr: tol must be finite and non-negative");
    DRE_REQUIRE(std::min(Lc.cols, Lo.cols) <= SVJ_MAX_W, "balance_lr: more than 4096 columns in both Gramian factors");
    const size_t rc0 = Lc.cols, ro0 = Lo.cols, mb = B.cols, qc = C.rows;
    // Z_c, Z_o, E Z_c, M and its SVD (svd_jacobi checks its own share again), the projections with their products, the reduced matrices
    require_memory(ctx, (size_t)n * (2 * rc0 + ro0) + 6 * ro0 * rc0 + 4 * (size_t)n * std::min(rc0, ro0) + (mb + qc + std::min(rc0, ro0)) * std::min(rc0, ro0));

    BalanceResult out;
    SqrtFactor fc = sqrt_factor(ctx, Lc, Dc), fo = sqrt_factor(ctx, Lo, Do);
    const Mat &Zc = fc.Z, &Zo = fo.Z;
    out.r_c = Zc.cols; out.r_o = Zo.cols;
    out.dropped = fc.dropped + fo.dropped;
    out.neg_max = std::max(fc.neg_max, fo.neg_max);
    const int k = std::min(out.r_c, out.r_o);
    if (k == 0) {
        DRE_REQUIRE(order == 0, "balance_lr: the requested order is above the numerical rank 0");
        out.hsv = Mat(ctx, 0, 1);
        out.T = Mat(ctx, n, 0); out.W = Mat(ctx, n, 0);
        out.Ar = Mat(ctx, 0, 0); out.Br = Mat(ctx, 0, B.cols); out.Cr = Mat(ctx, C.rows, 0);
        return out;
    }

    Mat EZ(ctx, n, out.r_c), M(ctx, out.r_o, out.r_c);
    gemm(ctx, false, false, 1.0, E, Zc, 0.0, EZ, nullptr, "bal_gemm");
    gemm(ctx, true, false, 1.0, Zo, EZ, 0.0, M, nullptr, "bal_gemm");
    SvjStats st;
    SvdResult sv = svd_jacobi(ctx, M, 0.0, &st);
    out.hsv = sv.S;
    out.rank = st.rank; out.sweeps = st.sweeps;

    int r = order;
    if (order > 0) {
        if (order > st.rank)
            throw Error(ERR_INVALID, "balance_lr: the requested order " + std::to_string(order) + " is above the numerical rank " + std::to_string(st.rank));
    } else {
        // the smallest r with 2 sum_{i > r} sigma_i <= tol sigma_1, the tail summed from the smallest sigma upward
        r = k;
        double tail = 0.0;
        while (r > 0 && 2.0 * (tail + sv.s[r - 1]) <= tol * sv.s[0]) { tail += sv.s[r - 1]; --r; }
        r = (int)std::min<long>(r, st.rank);
    }
    out.order = r;
    { double tail = 0.0; for (int i = k - 1; i >= r; --i) tail += sv.s[i]; out.bound = 2.0 * tail; }

    out.W = Mat(ctx, n, r); out.T = Mat(ctx, n, r);
    out.Ar = Mat(ctx, r, r); out.Br = Mat(ctx, r, B.cols); out.Cr = Mat(ctx, C.rows, r);
    if (r == 0) return out;
    const Mat Ur = sv.U.colsview(0, r), Vr = sv.V.colsview(0, r);
    gemm(ctx, false, false, 1.0, Zo, Ur, 0.0, out.W, nullptr, "bal_gemm");
    gemm(ctx, false, false, 1.0, Zc, Vr, 0.0, out.T, nullptr, "bal_gemm");
    scale_cols(ctx, out.W, sv.S.p);
    scale_cols(ctx, out.T, sv.S.p);
    Mat XT(ctx, n, r), I(ctx, r, r);
    gemm(ctx, false, false, 1.0, A, out.T, 0.0, XT, nullptr, "bal_gemm");
    gemm(ctx, true, false, 1.0, out.W, XT, 0.0, out.Ar, nullptr, "bal_gemm");
    if (B.cols) gemm(ctx, true, false, 1.0, out.W, B, 0.0, out.Br, nullptr, "bal_gemm");
    if (C.rows) gemm(ctx, false, false, 1.0, C, out.T, 0.0, out.Cr, nullptr, "bal_gemm");
    gemm(ctx, false, false, 1.0, E, out.T, 0.0, XT, nullptr, "bal_gemm");
    set_identity(ctx, I, 1.0);
    gemm(ctx, true, false, 1.0, out.W, XT, -1.0, I, nullptr, "bal_gemm");
    out.eye_err = frob_norm_host(ctx, I);
    return out;
}

}  // namespace dre
