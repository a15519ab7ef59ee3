// Square-root balanced truncation from factored Gramians (host restatement: tests/_svd_jacobi_model.py, balance).
//
//   Z_c = L_c sqrt(d_c), Z_o = L_o sqrt(d_o) over the positive entries;  M = Z_o'(E Z_c) = U Sigma V' (svd_jacobi);
//   W = Z_o U_r Sigma_r^{-1/2},  T = Z_c V_r Sigma_r^{-1/2};  A_r = W'A T, B_r = W'B, C_r = C T;  W'E T = I by construction.
// Every product goes through gemm(); the two kernels here scale columns.
#include "balance.hpp"

#include <cmath>

#include "dense_gj.hpp"
#include "jacobi_batch.hpp"
#include "profiling.hpp"
#include "svd_jacobi.hpp"

namespace dre {

namespace {

enum OrderRule { ORDER_HANKEL, ORDER_LQG };      // order = 0: 2 sum_{i > r} sigma_i <= tol sigma_1 (balance_lr), 2 sum_{i > r} nu_i <= tol (lqg_balance)

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

// steps (4)-(7) for one system after the SVD: U, V are the factors of M (r_o x k' and r_c x k'; in a batch the member's blocks of the padded
// factors), s the singular values on the host (the first k = min(r_o, r_c) count), S_dev the same on the device
void balance_member_finish(Ctx* ctx, const Mat& E, const Mat& A, const Mat& B, const Mat& C, const Mat& Zc, const Mat& Zo, const Mat& U, const Mat& V,
                           const std::vector<double>& s, const double* S_dev, long rank, int order, double tol, BalanceResult& out,
                           OrderRule rule = ORDER_HANKEL) {
    const int n = E.rows, k = std::min(out.r_c, out.r_o);
    int r = order;
    auto nu = [&](int i) { return s[i] / std::sqrt(1.0 + s[i] * s[i]); };
    if (order > 0) {
        if (order > rank)
            throw Error(ERR_INVALID, "balance_lr: the requested order " + std::to_string(order) + " is above the numerical rank " + std::to_string(rank));
    } else if (rule == ORDER_LQG) {
        // the smallest r with 2 sum_{i > r} nu_i <= tol, nu_i = mu_i / sqrt(1 + mu_i^2): absolute, the normalised coprime factors have norm 1
        r = k;
        double tail = 0.0;
        while (r > 0 && 2.0 * (tail + nu(r - 1)) <= tol) { tail += nu(r - 1); --r; }
        r = (int)std::min<long>(r, rank);
    } else {
        // the smallest r with 2 sum_{i > r} sigma_i <= tol sigma_1, the tail summed from the smallest sigma upward
        r = k;
        double tail = 0.0;
        while (r > 0 && 2.0 * (tail + s[r - 1]) <= tol * s[0]) { tail += s[r - 1]; --r; }
        r = (int)std::min<long>(r, rank);
    }
    out.order = r;
    { double tail = 0.0; for (int i = k - 1; i >= r; --i) tail += rule == ORDER_LQG ? nu(i) : s[i]; out.bound = 2.0 * tail; }

    out.W = Mat(ctx, n, r); out.T = Mat(ctx, n, r);
    out.Ar = Mat(ctx, r, r); out.Br = Mat(ctx, r, B.cols); out.Cr = Mat(ctx, C.rows, r);
    if (r == 0) return;
    const Mat Ur = U.colsview(0, r), Vr = V.colsview(0, r);
    gemm(ctx, false, false, 1.0, Zo, Ur, 0.0, out.W, nullptr, "bal_gemm");
    gemm(ctx, false, false, 1.0, Zc, Vr, 0.0, out.T, nullptr, "bal_gemm");
    scale_cols(ctx, out.W, S_dev);
    scale_cols(ctx, out.T, S_dev);
    Mat XT(ctx, n, r), I(ctx, r, r);
    gemm(ctx, false, false, 1.0, A, out.T, 0.0, XT, nullptr, "bal_gemm");
    gemm(ctx, true, false, 1.0, out.W, XT, 0.0, out.Ar, nullptr, "bal_gemm");
    if (B.cols) gemm(ctx, true, false, 1.0, out.W, B, 0.0, out.Br, nullptr, "bal_gemm");
    if (C.rows) gemm(ctx, false, false, 1.0, C, out.T, 0.0, out.Cr, nullptr, "bal_gemm");
    gemm(ctx, false, false, 1.0, E, out.T, 0.0, XT, nullptr, "bal_gemm");
    set_identity(ctx, I, 1.0);
    gemm(ctx, true, false, 1.0, out.W, XT, -1.0, I, nullptr, "bal_gemm");
    out.eye_err = frob_norm_host(ctx, I);
}

// the argument checks of balance_lr and the size of its work space in doubles: Z_c, Z_o, E Z_c, M and its SVD (svd_jacobi checks its own share
// again), the projections with their products, the reduced matrices
size_t balance_check(const Mat& E, const Mat& A, const Mat& B, const Mat& C, const Mat& Lc, const Mat& Dc, const Mat& Lo, const Mat& Do, int order,
                     double tol) {
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
    return (size_t)n * (2 * rc0 + ro0) + 6 * ro0 * rc0 + 4 * (size_t)n * std::min(rc0, ro0) + (mb + qc + std::min(rc0, ro0)) * std::min(rc0, ro0);
}

// steps (1)-(7) of balance_lr after its checks; rule: how order = 0 chooses r and what `bound` sums
BalanceResult balance_core(Ctx* ctx, const Mat& E, const Mat& A, const Mat& B, const Mat& C, const Mat& Lc, const Mat& Dc, const Mat& Lo, const Mat& Do,
                           int order, double tol, OrderRule rule) {
    const int n = E.rows;
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
    balance_member_finish(ctx, E, A, B, C, Zc, Zo, sv.U, sv.V, sv.s, sv.S.p, st.rank, order, tol, out, rule);
    return out;
}

}  // namespace

BalanceResult balance_lr(Ctx* ctx, const Mat& E, const Mat& A, const Mat& B, const Mat& C, const Mat& Lc, const Mat& Dc, const Mat& Lo, const Mat& Do,
                         int order, double tol) {
    require_memory(ctx, balance_check(E, A, B, C, Lc, Dc, Lo, Do, order, tol));
    return balance_core(ctx, E, A, B, C, Lc, Dc, Lo, Do, order, tol, ORDER_HANKEL);
}

// ---- LQG balanced truncation -----------------------------------------------------------------------------------------------
namespace {

// S = L diag(d) L' by the Householder + QL solver, in the form dre_sym_eig returns it: d ascending (j x 1), L n x j (j < n after the early
// termination on a low-rank S)
void eig_factor(Ctx* ctx, const Mat& S, Mat& L, Mat& D) {
    Mat W(ctx, S.rows, S.cols);
    copy_mat(ctx, S, W);
    struct Method0 { Ctx* c; int was; ~Method0() { c->sym_eig_method = was; } } method0{ctx, ctx->sym_eig_method};
    ctx->sym_eig_method = 0;
    SymEig e = sym_eig(ctx, W, 4.0);
    std::vector<int> ids((size_t)e.j);
    for (int i = 0; i < e.j; ++i) ids[(size_t)i] = i;
    std::sort(ids.begin(), ids.end(), [&](int a, int b) { return e.w[(size_t)a] < e.w[(size_t)b]; });
    std::vector<double> w((size_t)e.j);
    for (int i = 0; i < e.j; ++i) w[(size_t)i] = e.w[(size_t)ids[(size_t)i]];
    L = sym_eig_backtransform(ctx, e, ids);
    D = Mat(ctx, e.j, 1);
    if (e.j) {
        DRE_HIP(hipMemcpyAsync(D.p, w.data(), (size_t)e.j * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        ctx->sync();          // (w is released on return)
    }
}

}  // namespace

LqgBalanceResult lqg_balance(Ctx* ctx, const Mat& E, const Mat& A, const Mat& B, const Mat& C, const Mat& X, const Mat& Y, int order, double tol) {
    const int n = E.rows;
    DRE_REQUIRE(n >= 1 && E.cols == n && A.rows == n && A.cols == n, "lqg_balance: E and A must be n x n");
    DRE_REQUIRE(n <= 8192, "lqg_balance: order above 8192 (the eigensolver that factors X and Y)");
    DRE_REQUIRE(B.rows == n && C.cols == n && B.cols >= 1 && C.rows >= 1, "lqg_balance: B must be n x m and C q x n with m, q >= 1");
    DRE_REQUIRE(X.rows == n && X.cols == n && Y.rows == n && Y.cols == n, "lqg_balance: X and Y must be n x n");
    DRE_REQUIRE(order >= 0, "lqg_balance: negative order");
    DRE_REQUIRE(order > 0 || (tol >= 0.0 && std::isfinite(tol)), "lqg_balance: tol must be finite and non-negative");
    const size_t nn = (size_t)n * n, mb = B.cols, qc = C.rows;
    // the two eigen-factors (2 n^2 + 2 n), one eigensolver's work at a time (copy, reflectors, tridiagonal vectors, back-transform: 4 n^2),
    // balance_lr's work space at full rank, and the controller's matrices
    require_memory(ctx, 6 * nn + 2 * (size_t)n + (3 * nn + 6 * nn + 4 * nn + (mb + qc + n) * n) + (2 * (mb + qc) + 2 * (size_t)n) * n);

    Mat Lo, Do, Lc, Dc;
    eig_factor(ctx, X, Lo, Do);
    eig_factor(ctx, Y, Lc, Dc);
    LqgBalanceResult out;
    try {
        balance_check(E, A, B, C, Lc, Dc, Lo, Do, order, tol);
        out.bal = balance_core(ctx, E, A, B, C, Lc, Dc, Lo, Do, order, tol, ORDER_LQG);
    } catch (const Error& e) {
        std::string msg = e.what();
        if (msg.rfind("balance_lr: ", 0) == 0) msg = "lqg_balance: " + msg.substr(12);
        throw Error(e.code, msg);
    }
    // the reduced-order LQG controller x_c' = Ac x_c + Lr y, u = -Kr x_c:  Kr = Br' Sigma_r, Lr = Sigma_r Cr', Ac = Ar - Br Kr - Lr Cr
    const int r = out.bal.order, m = B.cols, q = C.rows;
    out.Kr = Mat(ctx, m, r); out.Lr = Mat(ctx, r, q); out.Ac = Mat(ctx, r, r);
    if (r > 0) {
        Mat Sig(ctx, r, r);
        std::vector<double> mu((size_t)r), hs((size_t)r * Sig.ld, 0.0);          // Sigma_r, built on the host (r is small)
        DRE_HIP(hipMemcpyAsync(mu.data(), out.bal.hsv.p, (size_t)r * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        for (int i = 0; i < r; ++i) hs[(size_t)i * ((size_t)Sig.ld + 1)] = mu[(size_t)i];
        DRE_HIP(hipMemcpyAsync(Sig.p, hs.data(), hs.size() * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
        ctx->sync();
        gemm(ctx, true, false, 1.0, out.bal.Br, Sig, 0.0, out.Kr, nullptr, "bal_gemm");
        gemm(ctx, false, true, 1.0, Sig, out.bal.Cr, 0.0, out.Lr, nullptr, "bal_gemm");
        copy_mat(ctx, out.bal.Ar, out.Ac);
        gemm(ctx, false, false, -1.0, out.bal.Br, out.Kr, 1.0, out.Ac, nullptr, "bal_gemm");
        gemm(ctx, false, false, -1.0, out.Lr, out.bal.Cr, 1.0, out.Ac, nullptr, "bal_gemm");
    }
    ctx->sync();
    return out;
}

// ---- ensemble form ---------------------------------------------------------------------------------------------------------------------------
BalanceBatch balance_lr_batch(Ctx* ctx, const std::vector<BalanceMember>& mem, int order, double tol, const char* who) {
    const std::string w_ = std::string(who) + ": ";
    DRE_REQUIRE(!mem.empty() && mem.size() <= (size_t)JACOBI_BATCH_MAX, w_ + "batch must be in 1 .. 65535");
    const int nb = (int)mem.size();
    const int n = mem[0].E->rows, mB = mem[0].B->cols, qC = mem[0].C->rows;
    DRE_REQUIRE(n >= 1 && n <= DENSE_MAX_N, w_ + "order beyond the device's 32-bit index limit, or empty");
    DRE_REQUIRE(order >= 0, w_ + "negative order");
    DRE_REQUIRE(order > 0 || (tol >= 0.0 && std::isfinite(tol)), w_ + "tol must be finite and non-negative");
    size_t need = 0, ro_cap = 0, rc_cap = 0;
    for (int b = 0; b < nb; ++b) {
        const BalanceMember& m = mem[(size_t)b];
        const std::string mb_ = w_ + "member " + std::to_string(b) + ": ";
        DRE_REQUIRE(m.E->rows == n && m.E->cols == n && m.A->rows == n && m.A->cols == n, mb_ + "E and A must be n x n with the n of member 0");
        DRE_REQUIRE(m.B->rows == n && m.B->cols == mB && m.C->cols == n && m.C->rows == qC, mb_ + "B must be n x m and C q x n with the (n, m, q) of member 0");
        DRE_REQUIRE(m.Lc->rows == n && m.Lo->rows == n, mb_ + "the Gramian factors must have n rows");
        DRE_REQUIRE(diag_stride(*m.Dc, m.Lc->cols) > 0 && diag_stride(*m.Do, m.Lo->cols) > 0, mb_ + "D must be a diagonal matrix or a vector matching its factor's columns");
        const size_t rc0 = m.Lc->cols, ro0 = m.Lo->cols, k0 = std::min(rc0, ro0);
        need += (size_t)n * (2 * rc0 + ro0) + 4 * (size_t)n * k0 + ((size_t)mB + qC + k0) * k0;
        ro_cap = std::max(ro_cap, ro0); rc_cap = std::max(rc_cap, rc0);
    }
    DRE_REQUIRE(std::min(ro_cap, rc_cap) <= (size_t)SVJ_MAX_W, w_ + "more than 4096 columns in both Gramian factors");
    // the members' factors, projections and reduced matrices, the stack of M and its SVD (svd_jacobi_batch checks its own share again)
    require_memory(ctx, need + (size_t)nb * 6 * ro_cap * rc_cap);

    BalanceBatch out;
    out.res.resize((size_t)nb); out.status.resize((size_t)nb);
    auto fail = [&](int b, const Error& e) {
        std::string msg = e.what();
        if (msg.rfind("balance_lr: ", 0) == 0) msg = msg.substr(12);
        out.status[(size_t)b] = {e.code, std::string(who) + ", member " + std::to_string(b) + ": " + msg};
        out.res[(size_t)b] = BalanceResult{};
    };
    std::vector<SqrtFactor> fc((size_t)nb), fo((size_t)nb);
    int ro_max = 0, rc_max = 0;
    for (int b = 0; b < nb; ++b) {
        try {
            fc[(size_t)b] = sqrt_factor(ctx, *mem[(size_t)b].Lc, *mem[(size_t)b].Dc);
            fo[(size_t)b] = sqrt_factor(ctx, *mem[(size_t)b].Lo, *mem[(size_t)b].Do);
        } catch (const Error& e) {
            if (e.code != ERR_INVALID) throw;
            fail(b, e);
            continue;
        }
        BalanceResult& r = out.res[(size_t)b];
        r.r_c = fc[(size_t)b].Z.cols; r.r_o = fo[(size_t)b].Z.cols;
        r.dropped = fc[(size_t)b].dropped + fo[(size_t)b].dropped;
        r.neg_max = std::max(fc[(size_t)b].neg_max, fo[(size_t)b].neg_max);
        ro_max = std::max(ro_max, r.r_o); rc_max = std::max(rc_max, r.r_c);
    }
    out.padded_rows = ro_max; out.padded_cols = rc_max;

    // the members that reach the SVD: M_b into the top left corner of its zero-filled slot
    std::vector<int> ids;
    std::vector<Mat> Ms;
    Mat stack;
    const size_t slot = (size_t)ro_max * rc_max;
    for (int b = 0; b < nb; ++b) {
        if (out.status[(size_t)b].code) continue;
        BalanceResult& r = out.res[(size_t)b];
        if (std::min(r.r_c, r.r_o) == 0) {
            if (order != 0) { fail(b, Error(ERR_INVALID, "the requested order is above the numerical rank 0")); continue; }
            r.hsv = Mat(ctx, 0, 1);
            r.T = Mat(ctx, n, 0); r.W = Mat(ctx, n, 0);
            r.Ar = Mat(ctx, 0, 0); r.Br = Mat(ctx, 0, mB); r.Cr = Mat(ctx, qC, 0);
            continue;
        }
        ids.push_back(b);
    }
    if (!ids.empty()) {
        DevArr<double> st(ctx, slot * ids.size());
        DRE_HIP(hipMemsetAsync(st.p, 0, slot * ids.size() * sizeof(double), ctx->stream));
        for (size_t i = 0; i < ids.size(); ++i) {
            const int b = ids[i];
            const BalanceResult& r = out.res[(size_t)b];
            Mat slotm;
            slotm.buf = st.buf; slotm.p = st.p + i * slot; slotm.rows = ro_max; slotm.cols = rc_max; slotm.ld = ro_max;
            Mat EZ(ctx, n, r.r_c), M = slotm.view(0, 0, r.r_o, r.r_c);
            gemm(ctx, false, false, 1.0, *mem[(size_t)b].E, fc[(size_t)b].Z, 0.0, EZ, nullptr, "bal_gemm");
            gemm(ctx, true, false, 1.0, fo[(size_t)b].Z, EZ, 0.0, M, nullptr, "bal_gemm");
            Ms.push_back(slotm);
        }
        SvdBatch sv = svd_jacobi_run(ctx, Ms, 0.0, who, false);
        for (size_t i = 0; i < ids.size(); ++i) {
            const int b = ids[i];
            BalanceResult& r = out.res[(size_t)b];
            if (sv.status[i].code) { fail(b, Error(sv.status[i].code, sv.status[i].msg)); continue; }
            const int k = std::min(r.r_c, r.r_o);
            const SvdResult& s = sv.svd[i];
            r.hsv = s.S.view(0, 0, k, 1);
            r.rank = std::min<long>(sv.stats[i].rank, k); r.sweeps = sv.stats[i].sweeps;
            try {
                const BalanceMember& mb = mem[(size_t)b];
                balance_member_finish(ctx, *mb.E, *mb.A, *mb.B, *mb.C, fc[(size_t)b].Z, fo[(size_t)b].Z, s.U.view(0, 0, r.r_o, s.U.cols),
                                      s.V.view(0, 0, r.r_c, s.V.cols), s.s, s.S.p, r.rank, order, tol, r);
            } catch (const Error& e) {
                if (e.code != ERR_INVALID) throw;
                fail(b, e);
            }
        }
    }
    ctx->sync();
    return out;
}

}  // namespace dre
