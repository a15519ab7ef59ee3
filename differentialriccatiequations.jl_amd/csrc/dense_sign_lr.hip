// Factored replay of the sign iteration (Benner & Quintana-Orti 1999, section 4; Baur & Benner 2006): with W_k = L_k D_k L_k',
//     L_{k+1} = [L_k, P_k' L_k],   D_{k+1} = blkdiag(D_k / (2 c_k), (c_k / 2) D_k),   X = (E^-T L) (D / 2) (E^-T L)'
// on the (P_k, c_k) that SignLyap::factor() kept, with a rank-revealing compression (Householder QR, R D R', symmetric eigensolver,
// |lambda| > rtol max|lambda|) whenever the width passes the cap and once at the end.  The products, the QR and the eigensolver are the
// library's existing ones (gemm.hip, qr_band.hip); this file adds the three small kernels that assemble the block matrices.
// solve_lr (this equation) and solve_lr_t (the dual one) are two directions of one body, solve_lr_impl.
// NumPy restatement: tests/_factored_sign_model.py, tests/_sign_dual_model.py.   DESIGN.md §9.2.
#include "dense_sign_lr.hpp"

#include <algorithm>
#include <cmath>

#include "dense.hpp"
#include "profiling.hpp"

namespace dre {

// Every kernel below indexes matrices of order <= 2 SIGN_LR_MAX_WIDTH + DENSE_MAX_N columns through size_t offsets; the int row / column
// indices stay below 2^31 by the DENSE_MAX_N argument of dense_gj.hpp.

// Out ((wa + wb) x (wa + wb)) = blkdiag(a A, b B); A and B may be the same matrix (the D recursion: both scalings in one pass)
__global__ __launch_bounds__(256) void k_lr_blkdiag(int wa, const double* __restrict__ A, int lda, double a, int wb, const double* __restrict__ B, int ldb,
                                                    double b, double* __restrict__ Out, int ldo) {
    const int w = wa + wb;
    const size_t tot = (size_t)w * w;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < tot; idx += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(idx % w), j = (int)(idx / w);
        double v = 0.0;
        if (i < wa && j < wa) v = a * A[i + (size_t)j * lda];
        else if (i >= wa && j >= wa) v = b * B[(i - wa) + (size_t)(j - wa) * ldb];
        Out[i + (size_t)j * ldo] = v;
    }
}

// D (r x r) = scale diag(vals)
__global__ __launch_bounds__(256) void k_lr_diag(int r, const double* __restrict__ vals, double scale, double* __restrict__ D, int ld) {
    const size_t tot = (size_t)r * r;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < tot; idx += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(idx % r), j = (int)(idx / r);
        D[i + (size_t)j * ld] = i == j ? scale * vals[i] : 0.0;
    }
}

// T ((r + 2 p) x (r + 2 p)) = blkdiag(S, [[0, D], [D, 0]]): the middle matrix of the residual factor [G, F'L, E'L]
__global__ __launch_bounds__(256) void k_lr_res_t(int r, const double* __restrict__ S, int lds_, int p, const double* __restrict__ D, int ldd,
                                                  double* __restrict__ T, int ldt) {
    const int w = r + 2 * p;
    const size_t tot = (size_t)w * w;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < tot; idx += (size_t)gridDim.x * blockDim.x) {
        const int i = (int)(idx % w), j = (int)(idx / w);
        double v = 0.0;
        if (i < r && j < r) v = S[i + (size_t)j * lds_];
        else if (i >= r && j >= r) {
            const int a = i - r, b = j - r;
            if (a < p && b >= p) v = D[a + (size_t)(b - p) * ldd];
            else if (a >= p && b < p) v = D[(a - p) + (size_t)b * ldd];
        }
        T[i + (size_t)j * ldt] = v;
    }
}

namespace {

void blkdiag(Ctx* c, const Mat& A, double a, const Mat& B, double b, Mat& Out) {
    const int w = A.rows + B.rows;
    TimedScope ts(c, "signlr_small", 16.0 * w * w, 0.0);
    hipLaunchKernelGGL(k_lr_blkdiag, dim3(grid_for((size_t)w * w)), dim3(256), 0, c->stream, A.rows, (const double*)A.p, A.ld, a, B.rows,
                       (const double*)B.p, B.ld, b, Out.p, Out.ld);
}

// D = scale diag(vals) as a device matrix (the values travel as r doubles)
Mat diag_mat(Ctx* c, const std::vector<double>& vals, double scale) {
    const int r = (int)vals.size();
    Mat D(c, r, r);
    if (r == 0) return D;
    DevArr<double> dv(c, (size_t)r);
    dv.upload(c, vals);
    TimedScope ts(c, "signlr_small", 8.0 * r * r, 0.0);
    hipLaunchKernelGGL(k_lr_diag, dim3(grid_for((size_t)r * r)), dim3(256), 0, c->stream, r, (const double*)dv.p, scale, D.p, D.ld);
    c->sync();              // (dv dies with this scope)
    return D;
}

// Rank-revealing compression of L D L' in two steps, so that the residual's norm is known before its eigenvalues are asked for:
// form(): the small symmetric matrix of L D L' on an orthonormal basis of range(L) (S = R D R' from the Householder QR of a copy of L; when L has at least as many
// columns as rows the basis is the identity and S = L D L' itself, which is then no larger than R D R' would be);
// norm(): ||L D L'||_F = ||S||_F;  finish(): eigenvalues of S, |lambda| > rtol max|lambda| kept (ascending), dst[:, 0:rank] <- basis * V_kept.
struct Compressor {
    Ctx* c;
    Mat S;
    QRFact qr;
    bool wide = false;
    int n = 0, q = 0;
    DevArr<double> nrm;
    explicit Compressor(Ctx* ctx) : c(ctx), nrm(ctx, 1) {}

    void form(const Mat& Lv, const Mat& D) {
        n = Lv.rows;
        const int w = Lv.cols;
        DRE_REQUIRE(D.rows == w && D.cols == w && w >= 1, "solve_lr: factor and middle matrix do not match");
        wide = w >= n;
        if (wide) {
            q = n;
            Mat LD(c, n, w);
            gemm(c, false, false, 1.0, Lv, D, 0.0, LD, nullptr, "signlr_gemm_small");
            S = Mat(c, n, n);
            gemm(c, false, true, 1.0, LD, Lv, 0.0, S, nullptr, "signlr_gemm_small");
        } else {
            Mat A(c, n, w);
            copy_mat(c, Lv, A);
            qr = qr_factor(c, A);
            q = qr.kq;
            Mat RD(c, q, w);
            gemm(c, false, false, 1.0, qr.R, D, 0.0, RD, nullptr, "signlr_gemm_small");
            S = Mat(c, q, q);
            gemm(c, false, true, 1.0, RD, qr.R, 0.0, S, nullptr, "signlr_gemm_small");
        }
        symmetrize(c, S);
    }

    double norm() {
        frob2_device(c, S, nrm.p);
        return std::sqrt(read_back(c, nrm.p));
    }

    std::vector<double> finish(Mat& dst, double rtol) {
        // the tridiagonalisation may stop early once the remainder is below tolfac eps ||S||_F: keep that below the truncation threshold
        const double tolfac = std::max(0.25, std::min(4.0, rtol / (8.0 * DBL_EPS)));
        SymEig e = sym_eig(c, S, tolfac, true);
        double wmax = 0.0;
        for (double v : e.w) wmax = std::max(wmax, std::fabs(v));
        std::vector<int> ids;
        for (int i = 0; i < e.j; ++i)
            if (std::fabs(e.w[(size_t)i]) > rtol * wmax) ids.push_back(i);
        std::sort(ids.begin(), ids.end(), [&](int a, int b) { return e.w[(size_t)a] < e.w[(size_t)b]; });
        const int r = (int)ids.size();
        std::vector<double> vals((size_t)r);
        for (int i = 0; i < r; ++i) vals[(size_t)i] = e.w[(size_t)ids[(size_t)i]];
        if (r == 0) return vals;
        DRE_REQUIRE(dst.rows == n && dst.cols >= r, "solve_lr: compression target too narrow");
        Mat B = sym_eig_backtransform(c, e, ids);          // q x r
        Mat Lnew = dst.view(0, 0, n, r);
        if (wide) copy_mat(c, B, Lnew);
        else {
            fill_mat(c, Lnew, 0.0);
            Mat top = Lnew.view(0, 0, q, r);
            copy_mat(c, B, top);
            qr_apply_q(c, qr, Lnew, false);
        }
        return vals;
    }
};

}  // namespace

// One body for both directions (tests/_factored_sign_model.py, tests/_sign_dual_model.py).  The primal equation
// F'XE + E'XF = -G S G' replays  L_0 = G,  L_{k+1} = [L_k, P_k' L_k]  and leaves through  X = (E^-T L) (D / 2) (E^-T L)';  the dual equation
// F Y E' + E Y F' = -G S G' replays  L_0 = E^-1 G,  L_{k+1} = [L_k, P_k L_k]  and  Y = L_inf (D_inf / 2) L_inf'.  `dual` therefore selects: the
// transform with E^-1 at the entry instead of the exit, no transposed operand (P_k, and F and E in the residual factor [G, F L, E L]), the
// memory of the entry and residual blocks on top of sign_lr_doubles, and the name in the messages.  Cap, compression, regrowth, refinement
// and the statistics are common.
SignLrStats SignLyap::solve_lr_impl(bool dual, const Mat& G, const Mat& S, double rtol, int max_width, int max_refine, Mat& L, Mat& D) {
    Ctx* c = c_;
    const int n = n_, r = G.cols;
    const std::string who = dual ? "solve_lr_t: " : "solve_lr: ";
    const bool tr = !dual;          // the primal's products with P_k, F and E are transposed
    DRE_REQUIRE(iters_ > 0, who + "factor() first");
    DRE_REQUIRE(G.rows == n && S.rows == r && S.cols == r, who + "G must be n x r and S r x r");
    DRE_REQUIRE(rtol > 0.0 && rtol < 1.0, who + "rtol must lie in (0, 1)");
    DRE_REQUIRE(max_width >= 1 && max_width >= r && max_width <= SIGN_LR_MAX_WIDTH,
                who + "max_width must be at least the width of G (and 1) and at most " + std::to_string(SIGN_LR_MAX_WIDTH));
    DRE_REQUIRE(max_refine >= 0, who + "max_refine must be >= 0");
    SignLrStats st;
    st.iters = iters_;
    if (r == 0) { L = Mat(c, n, 0); D = Mat(c, 0, 0); return st; }
    auto doubles = [&](int w) { return dual ? sign_lr_t_doubles(n, r, w) : sign_lr_doubles(n, w); };
    require_memory(c, doubles(max_width));

    // (L0, D0) -> (L_inf or E^-T L_inf, D_inf / 2) with D diagonal; the factor lives in the left columns of one buffer (the dual writes
    // E^-1 L0 straight into them) and its product with P_k is written into the columns to its right
    auto replay_lr = [&](const Mat& L0, const Mat& D0, Mat& LX, Mat& DX) {
        int w = L0.cols;
        const int cap = std::max(max_width, w);
        if (cap > max_width) require_memory(c, doubles(cap));
        Mat buf(c, n, 2 * cap);
        Mat left0 = buf.colsview(0, w);
        if (dual) gemm(c, false, false, 1.0, Einv_, L0, 0.0, left0, nullptr, "signlr_gemm");           // E^-1 L0
        else copy_mat(c, L0, left0);
        Mat Dk = D0;
        Compressor comp(c);
        auto compress = [&]() -> std::vector<double> {
            Mat Lv = buf.colsview(0, w);
            comp.form(Lv, Dk);
            std::vector<double> vals = comp.finish(buf, rtol);
            ++st.compressions;
            w = (int)vals.size();
            return vals;
        };
        std::vector<double> vals;
        bool fresh = false;          // Dk == diag(vals) of a compression that nothing has touched since
        for (int k = 0; k < iters_ && w > 0; ++k) {
            if (2 * w > buf.cols) {         // a rank above the cap survived the compression: the buffer follows it
                require_memory(c, doubles(w));
                Mat nb(c, n, 2 * w);
                Mat dstv = nb.colsview(0, w), srcv = buf.colsview(0, w);
                copy_mat(c, srcv, dstv);
                buf = nb;
            }
            const Mat P = Pstore_.colsview(k * n, n);
            const double cf = cs_[(size_t)k];
            Mat left = buf.colsview(0, w), right = buf.colsview(w, w);
            gemm(c, tr, false, 1.0, P, left, 0.0, right, nullptr, "signlr_gemm");            // P_k' L_k (dual: P_k L_k)
            Mat Dn(c, 2 * w, 2 * w);
            blkdiag(c, Dk, 1.0 / (2.0 * cf), Dk, 0.5 * cf, Dn);
            Dk = Dn;
            w *= 2;
            fresh = false;
            st.peak_width = std::max<long>(st.peak_width, w);
            if (w > max_width) { vals = compress(); Dk = diag_mat(c, vals, 1.0); fresh = true; }
        }
        if (!fresh && w > 0) vals = compress();
        LX = Mat(c, n, w);
        if (w > 0) {
            Mat Lv = buf.colsview(0, w);
            if (dual) copy_mat(c, Lv, LX);
            else gemm(c, true, false, 1.0, Einv_, Lv, 0.0, LX, nullptr, "signlr_gemm");      // E^-T L
        }
        DX = diag_mat(c, vals, 0.5);
    };

    Compressor comp(c);
    comp.form(G, S);
    const double normR = comp.norm();
    st.peak_width = r;
    Mat LX, DX;
    replay_lr(G, S, LX, DX);

    // factored residual [G, F'L, E'L] blkdiag(S, [[0, D], [D, 0]]) [..]' (dual: [G, F L, E L]): its norm through the small matrix on the QR's
    // basis
    const double target = 100.0 * n * DBL_EPS + 10.0 * rtol;
    Mat Rf, T;
    auto residual = [&]() -> double {
        const int p = LX.cols, w = r + 2 * p;
        Rf = Mat(c, n, w);
        Mat g = Rf.colsview(0, r);
        copy_mat(c, G, g);
        if (p > 0) {
            Mat fl = Rf.colsview(r, p), el = Rf.colsview(r + p, p);
            gemm(c, tr, false, 1.0, F_, LX, 0.0, fl, nullptr, "signlr_gemm");
            gemm(c, tr, false, 1.0, E_, LX, 0.0, el, nullptr, "signlr_gemm");
        }
        T = Mat(c, w, w);
        {
            TimedScope ts(c, "signlr_small", 8.0 * w * w, 0.0);
            hipLaunchKernelGGL(k_lr_res_t, dim3(grid_for((size_t)w * w)), dim3(256), 0, c->stream, r, (const double*)S.p, S.ld, p, (const double*)DX.p,
                               DX.ld, T.p, T.ld);
        }
        comp.form(Rf, T);
        const double nr = comp.norm();
        return normR > 0.0 ? nr / normR : nr;
    };
    st.res0 = st.res = residual();
    while (st.res > target && st.refinements < max_refine && std::isfinite(st.res)) {
        std::vector<double> rv = comp.finish(Rf, rtol);          // the compressed residual factor, in the left columns of Rf
        ++st.compressions;
        const int pr = (int)rv.size();
        if (pr == 0) break;
        Mat Lr = Rf.colsview(0, pr), Dr = diag_mat(c, rv, 1.0), LdX, DdX;
        replay_lr(Lr, Dr, LdX, DdX);
        // X <- X + dX: append and compress
        const int p = LX.cols, pd = LdX.cols, w = p + pd;
        if (pd == 0) break;
        Mat cat(c, n, w), Dc(c, w, w);
        Mat a = cat.colsview(0, p), b = cat.colsview(p, pd);
        copy_mat(c, LX, a);
        copy_mat(c, LdX, b);
        blkdiag(c, DX, 1.0, DdX, 1.0, Dc);
        st.peak_width = std::max<long>(st.peak_width, w);
        Compressor cx(c);
        cx.form(cat, Dc);
        std::vector<double> xv = cx.finish(cat, rtol);
        ++st.compressions;
        const int px = (int)xv.size();
        LX = Mat(c, n, px);
        if (px > 0) { Mat src = cat.colsview(0, px); copy_mat(c, src, LX); }
        DX = diag_mat(c, xv, 1.0);
        ++st.refinements;
        st.res = residual();
    }
    DRE_HIP(hipGetLastError());
    st.rank = LX.cols;
    L = LX;
    D = DX;
    return st;
}

SignLrStats SignLyap::solve_lr(const Mat& G, const Mat& S, double rtol, int max_width, int max_refine, Mat& L, Mat& D) {
    return solve_lr_impl(false, G, S, rtol, max_width, max_refine, L, D);
}
SignLrStats SignLyap::solve_lr_t(const Mat& G, const Mat& S, double rtol, int max_width, int max_refine, Mat& L, Mat& D) {
    return solve_lr_impl(true, G, S, rtol, max_width, max_refine, L, D);
}

}  // namespace dre
