// Transfer function of dense descriptor systems at complex points, batched by point (transfer_eval.hpp).
#include "transfer_eval.hpp"

#include "dense_cgj.hpp"
#include "freq_sweep.hpp"

namespace dre {

static_assert(sizeof(BatchCtl) <= 16 * sizeof(double), "fr_member_doubles_c counts 16 doubles for a member's control block (and 6 coefficients)");

// The planes Zr = sigma E - A, Zi = omega E (n x n each, ld = n, Zi behind Zr) for the members of one system: blockIdx.z = member, one thread
// per (i, j) (threadIdx.x runs along i: coalesced reads and writes), each of E and A read once.  Every offset is size_t.
__global__ __launch_bounds__(256) void k_tf_assemble(int n, const double* __restrict__ E, int lde, const double* __restrict__ A, int lda,
                                                     const double* __restrict__ sre, const double* __restrict__ sim, double* __restrict__ Z) {
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y;
    if (i >= n || j >= n) return;
    const size_t b = blockIdx.z, nn = (size_t)n * n;
    const double e = E[(size_t)i + (size_t)j * lde];
    double* Zb = Z + b * 2 * nn;
    const size_t o = (size_t)i + (size_t)j * n;
    Zb[o] = sre[b] * e - A[(size_t)i + (size_t)j * lda];
    Zb[o + nn] = sim[b] * e;
}

// start of a member's residual in the top half of its block form Rt (2n x 2m, ld = 2n): [Rr | Ri] = [B | 0], and the coefficients
// (alpha, beta) of its three products with E: coef[6 b .. 6 b + 5] = (-sigma, 1, omega, 1, -omega, 1).  blockIdx.z = member of one system,
// one thread per element of [Rr | Ri].
__global__ __launch_bounds__(256) void k_tf_rhs(int n, int m, const double* __restrict__ B, int ldb, const double* __restrict__ sre,
                                                const double* __restrict__ sim, double* __restrict__ Rt, double* __restrict__ coef) {
    const size_t b = blockIdx.z, N = (size_t)2 * n, tot = (size_t)n * 2 * m;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx == 0) {
        const double sg = sre[b], w = sim[b];
        double* c = coef + 6 * b;
        c[0] = -sg; c[1] = 1.0; c[2] = w; c[3] = 1.0; c[4] = -w; c[5] = 1.0;
    }
    if (idx >= tot) return;
    const size_t i = idx % n, j = idx / n;
    Rt[b * N * 2 * m + i + j * N] = j < (size_t)m ? B[i + j * (size_t)ldb] : 0.0;
}

// bottom half of the block form: Rt[n + i, j] = -Ri[i, j], Rt[n + i, m + j] = Rr[i, j]; blockIdx.z = member, one thread per element
__global__ __launch_bounds__(256) void k_tf_block(int n, int m, double* __restrict__ Rt, BatchMask mask) {
    const int b = blockIdx.z;
    if (batch_off(mask, b)) return;
    const size_t N = (size_t)2 * n, tot = (size_t)n * m;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= tot) return;
    const size_t i = idx % n, j = idx / n;
    double* R = Rt + (size_t)b * N * 2 * m;
    R[n + i + j * N] = -R[i + (m + j) * N];
    R[n + i + (m + j) * N] = R[i + j * N];
}

// freq_sweep.hpp's description of this method: the points are s = sigma + i omega, a member is the two planes of s E - A
struct TfMethod {
    static constexpr const char *name = "transfer_eval", *noun = "point", *nouns = "points", *sym = "s", *pencil = "s E - A";
    static constexpr const char *points_msg = "at least one point is needed (K >= 1), with a real and an imaginary part each", *panel_fn = "cgj_batch_nb";
    const std::vector<double>&s_re, &s_im;
    int n = 0, m = 0, q = 0, nb = 0;
    size_t qm = 0, nn = 0;
    DevArr<double> sr, si, coef;
    Mat Z, Pt, Wt, Y, Rt;
    DevArr<int> piv;

    size_t points() const { return s_re.size() == s_im.size() ? s_re.size() : 0; }
    bool finite(size_t k) const { return std::isfinite(s_re[k]) && std::isfinite(s_im[k]); }
    std::string point_text(size_t k) const {
        char stxt[96];
        std::snprintf(stxt, sizeof(stxt), "%.17g%+.17gi", s_re[k], s_im[k]);
        return stxt;
    }
    std::string order_msg(int n_) const {
        if (n_ <= GJ_REGISTER_MAX_N) return "";
        return "s E - A goes through the complex register panel: n <= " + std::to_string(GJ_REGISTER_MAX_N) + ", n = " + std::to_string(n_);
    }
    bool panel_ok(int n_) const { return cgj_batch_nb(n_) == fr_panel_nb_c(n_); }
    size_t member_doubles(int n_, int m_, int q_) const { return fr_member_doubles_c(n_, m_, q_); }
    size_t fixed_doubles(int K) const { return (size_t)2 * K + 512; }

    void allocate(Ctx* ctx, int n_, int m_, int q_, int cs) {
        n = n_; m = m_; q = q_; nb = cgj_batch_nb(n);
        qm = (size_t)q * m; nn = (size_t)n * n;
        sr = DevArr<double>(ctx, s_re.size()); si = DevArr<double>(ctx, s_im.size());
        sr.upload(ctx, s_re);
        si.upload(ctx, s_im);
        Z = Mat(ctx, n, 2 * n * cs); Pt = Mat(ctx, n, 2 * nb * cs); Wt = Mat(ctx, 2 * nb, 2 * n * cs); Y = Mat(ctx, n, 2 * m * cs); Rt = Mat(ctx, 2 * n, 2 * m * cs);
        coef = DevArr<double>(ctx, (size_t)6 * cs);
        piv = DevArr<int>(ctx, (size_t)n * cs);
    }
    void assemble(Ctx* ctx, const FreqSystem& f, int b0, int cnt, int k0) {
        TimedScope ts(ctx, "tf_assemble", 8.0 * cnt * (2.0 * n * n + 2.0 * n * n), 2.0 * cnt * n * n);
        hipLaunchKernelGGL(k_tf_assemble, dim3(ceil_div(n, 64), ceil_div(n, 4), cnt), dim3(64, 4), 0, ctx->stream, n, (const double*)f.E.p, f.E.ld,
                           (const double*)f.A.p, f.A.ld, (const double*)(sr.p + k0), (const double*)(si.p + k0), Z.p + (size_t)b0 * 2 * nn);
    }
    void invert(Ctx* ctx, int len, BatchCtl* ctl) { cgj_invert_batched(ctx, len, n, Z.p, piv.p, ctl, BM_GJ, Pt.p, Wt.p); }
    void solve(Ctx* ctx, const FreqSystem& f, int b0, int cnt, int k0, BatchCtl* ctl, double* Hre, double* Him) {
        const BatchMask mask{ctl + b0, BM_GJ, 0};
        const size_t sZ = 2 * nn, sY = (size_t)n * 2 * m, sR = (size_t)4 * n * m, nm = (size_t)n * m;
        double* Yb = Y.p + (size_t)b0 * sY;              // [Yr | Yi], ld n
        double* Rb = Rt.p + (size_t)b0 * sR;             // [[Rr, Ri], [-Ri, Rr]], ld 2n
        double* Xb = Z.p + (size_t)b0 * sZ;              // [Xr | Xi], ld n
        const double* cf = coef.p + (size_t)6 * b0;
        // Y = X B, plane by plane
        gemm_strided(ctx, cnt, false, false, n, m, n, 1.0, Xb, n, sZ, f.B.p, f.B.ld, 0, 0.0, Yb, n, sY, mask, "tf_gemm");
        gemm_strided(ctx, cnt, false, false, n, m, n, 1.0, Xb + nn, n, sZ, f.B.p, f.B.ld, 0, 0.0, Yb + nm, n, sY, mask, "tf_gemm");
        // one refinement step, the residual from E and A (s E - A is gone):  R = B - (s E - A) Y,  Y += X R
        {
            TimedScope ts(ctx, "tf_rhs", 8.0 * cnt * sY, 0.0);
            hipLaunchKernelGGL(k_tf_rhs, dim3((unsigned)((sY + 255) / 256), 1, cnt), dim3(256), 0, ctx->stream, n, m, (const double*)f.B.p, f.B.ld,
                               (const double*)(sr.p + k0), (const double*)(si.p + k0), Rb, coef.p + (size_t)6 * b0);
        }
        gemm_strided(ctx, cnt, false, false, n, 2 * m, n, 1.0, f.A.p, f.A.ld, 0, Yb, n, sY, 1.0, Rb, 2 * n, sR, mask, "tf_gemm");                 // + A [Yr | Yi]
        gemm_strided(ctx, cnt, false, false, n, 2 * m, n, 0.0, f.E.p, f.E.ld, 0, Yb, n, sY, 0.0, Rb, 2 * n, sR, mask, "tf_gemm", cf, 6);          // - sigma E [Yr | Yi]
        gemm_strided(ctx, cnt, false, false, n, m, n, 0.0, f.E.p, f.E.ld, 0, Yb + nm, n, sY, 0.0, Rb, 2 * n, sR, mask, "tf_gemm", cf + 2, 6);     // Rr += omega E Yi
        gemm_strided(ctx, cnt, false, false, n, m, n, 0.0, f.E.p, f.E.ld, 0, Yb, n, sY, 0.0, Rb + (size_t)2 * n * m, 2 * n, sR, mask, "tf_gemm", cf + 4, 6);   // Ri -= omega E Yr
        {
            TimedScope ts(ctx, "tf_rhs", 32.0 * cnt * nm, 0.0);
            hipLaunchKernelGGL(k_tf_block, dim3((unsigned)((nm + 255) / 256), 1, cnt), dim3(256), 0, ctx->stream, n, m, Rb, mask);
        }
        gemm_strided(ctx, cnt, false, false, n, 2 * m, 2 * n, 1.0, Xb, n, sZ, Rb, 2 * n, sR, 1.0, Yb, n, sY, mask, "tf_gemm");
        // Re H = C Yr, Im H = C Yi
        gemm_strided(ctx, cnt, false, false, q, m, n, 1.0, f.C.p, f.C.ld, 0, Yb, n, sY, 0.0, Hre + (size_t)b0 * qm, q, qm, mask, "tf_gemm");
        gemm_strided(ctx, cnt, false, false, q, m, n, 1.0, f.C.p, f.C.ld, 0, Yb + nm, n, sY, 0.0, Him + (size_t)b0 * qm, q, qm, mask, "tf_gemm");
    }
};

FreqResponse transfer_eval(Ctx* ctx, const std::vector<FreqSystem>& sys, const std::vector<double>& s_re, const std::vector<double>& s_im, int chunk) {
    TfMethod md{s_re, s_im};
    return freq_sweep(ctx, sys, chunk, md);
}

}  // namespace dre
