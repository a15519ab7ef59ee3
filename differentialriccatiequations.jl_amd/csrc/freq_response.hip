// Frequency response of dense descriptor systems, batched by frequency (freq_response.hpp).
#include "freq_response.hpp"

#include "dense_gj.hpp"
#include "freq_sweep.hpp"

namespace dre {

static_assert(sizeof(BatchCtl) <= 16 * sizeof(double), "fr_member_doubles counts 16 doubles for a member's control block (and 4 coefficients)");

// M = [[-A, -w E], [w E, -A]] (2n x 2n, ld = 2n) for the members of one system: blockIdx.z = member, w = omega[member], one thread per
// (i, j) of the n x n operands (threadIdx.x runs along i: coalesced reads and writes), each of E and A read once and written to its two
// blocks.  Every offset is size_t.
__global__ __launch_bounds__(256) void k_fr_assemble(int n, const double* __restrict__ E, int lde, const double* __restrict__ A, int lda,
                                                     const double* __restrict__ omega, double* __restrict__ M) {
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y;
    if (i >= n || j >= n) return;
    const size_t b = blockIdx.z, N = (size_t)2 * n;
    const double w = omega[b];
    const double a = -A[(size_t)i + (size_t)j * lda], e = w * E[(size_t)i + (size_t)j * lde];
    double* Mb = M + b * N * N;
    const size_t tl = (size_t)i + (size_t)j * N;         // top left block
    Mb[tl] = a;
    Mb[tl + n] = e;                                      // bottom left:  w E
    Mb[tl + (size_t)n * N] = -e;                         // top right:   -w E
    Mb[tl + (size_t)n * N + n] = a;                      // bottom right
}

// start of a member's residual: R = [B; 0] (2n x m, ld = 2n), and the coefficients (alpha, beta) of its two products with E:
// coef[4 b .. 4 b + 3] = (w, 1, -w, 1).  blockIdx.z = member of one system, one thread per element of R.
__global__ __launch_bounds__(256) void k_fr_rhs(int n, int m, const double* __restrict__ B, int ldb, const double* __restrict__ omega,
                                                double* __restrict__ R, double* __restrict__ coef) {
    const size_t b = blockIdx.z, N = (size_t)2 * n, tot = N * m;
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx == 0) {
        const double w = omega[b];
        double* c = coef + 4 * b;
        c[0] = w; c[1] = 1.0; c[2] = -w; c[3] = 1.0;
    }
    if (idx >= tot) return;
    const size_t i = idx % N, j = idx / N;
    R[b * tot + idx] = i < (size_t)n ? B[i + j * (size_t)ldb] : 0.0;
}

// freq_sweep.hpp's description of this method: the points are the frequencies, a member is the real form of order N = 2n
struct FrMethod {
    static constexpr const char *name = "freq_response", *noun = "frequency", *nouns = "frequencies", *sym = "omega", *pencil = "i omega E - A";
    static constexpr const char *points_msg = "at least one frequency is needed (K >= 1)", *panel_fn = "gj_batch_nb";
    const std::vector<double>& omega;
    int n = 0, m = 0, q = 0, N = 0, nb = 0;
    size_t qm = 0, NN = 0;
    DevArr<double> w, coef;
    Mat M, Pn, W, Y, R;
    DevArr<int> piv;

    size_t points() const { return omega.size(); }
    bool finite(size_t k) const { return std::isfinite(omega[k]); }
    std::string point_text(size_t k) const {
        char wtxt[40];
        std::snprintf(wtxt, sizeof(wtxt), "%.17g", omega[k]);
        return wtxt;
    }
    std::string order_msg(int n_) const {
        if (2 * (long long)n_ <= GJ_REGISTER_MAX_N) return "";
        return "the real form of i w E - A has order 2n and goes through the register panel: 2n <= " + std::to_string(GJ_REGISTER_MAX_N) +
               ", n = " + std::to_string(n_);
    }
    bool panel_ok(int n_) const { return gj_batch_nb(2 * n_) == fr_panel_nb(2 * n_); }
    size_t member_doubles(int n_, int m_, int q_) const { return fr_member_doubles(n_, m_, q_); }
    size_t fixed_doubles(int K) const { return (size_t)K + 512; }

    void allocate(Ctx* ctx, int n_, int m_, int q_, int cs) {
        n = n_; m = m_; q = q_; N = 2 * n; nb = gj_batch_nb(N);
        qm = (size_t)q * m; NN = (size_t)N * N;
        w = DevArr<double>(ctx, omega.size());
        w.upload(ctx, omega);
        M = Mat(ctx, N, N * cs); Pn = Mat(ctx, N, nb * cs); W = Mat(ctx, nb, N * cs); Y = Mat(ctx, N, m * cs); R = Mat(ctx, N, m * cs);
        coef = DevArr<double>(ctx, (size_t)4 * cs);
        piv = DevArr<int>(ctx, (size_t)N * cs);
    }
    void assemble(Ctx* ctx, const FreqSystem& f, int b0, int cnt, int k0) {
        TimedScope ts(ctx, "fr_assemble", 8.0 * cnt * (2.0 * n * n + 4.0 * n * n), 1.0 * cnt * n * n);
        hipLaunchKernelGGL(k_fr_assemble, dim3(ceil_div(n, 64), ceil_div(n, 4), cnt), dim3(64, 4), 0, ctx->stream, n, (const double*)f.E.p, f.E.ld,
                           (const double*)f.A.p, f.A.ld, (const double*)(w.p + k0), M.p + (size_t)b0 * NN);
    }
    void invert(Ctx* ctx, int len, BatchCtl* ctl) { gj_invert_batched(ctx, len, N, M.p, piv.p, ctl, BM_GJ, Pn.p, W.p); }
    void solve(Ctx* ctx, const FreqSystem& f, int b0, int cnt, int k0, BatchCtl* ctl, double* Hre, double* Him) {
        const BatchMask mask{ctl + b0, BM_GJ, 0};
        const size_t sY = (size_t)N * m;
        double* Yb = Y.p + (size_t)b0 * sY;
        double* Rb = R.p + (size_t)b0 * sY;
        double* Xb = M.p + (size_t)b0 * NN;
        const double* cf = coef.p + (size_t)4 * b0;
        // Y = M^-1[:, 0:n] B
        gemm_strided(ctx, cnt, false, false, N, m, n, 1.0, Xb, N, NN, f.B.p, f.B.ld, 0, 0.0, Yb, N, sY, mask, "fr_gemm");
        // one refinement step, the residual from E and A (M is gone):  R = [B; 0] - M Y = [B + A Yr + w E Yi; A Yi - w E Yr],  Y += M^-1 R.
        // The blocked inversion is accurate norm-wise only; where H is small beside |C| |M^-1| |B| (a response that has decayed) this
        // step restores its relative accuracy.
        {
            TimedScope ts(ctx, "fr_rhs", 8.0 * cnt * sY, 0.0);
            hipLaunchKernelGGL(k_fr_rhs, dim3((unsigned)((sY + 255) / 256), 1, cnt), dim3(256), 0, ctx->stream, n, m, (const double*)f.B.p, f.B.ld,
                               (const double*)(w.p + k0), Rb, coef.p + (size_t)4 * b0);
        }
        gemm_strided(ctx, cnt, false, false, n, m, n, 1.0, f.A.p, f.A.ld, 0, Yb, N, sY, 1.0, Rb, N, sY, mask, "fr_gemm");
        gemm_strided(ctx, cnt, false, false, n, m, n, 0.0, f.E.p, f.E.ld, 0, Yb + n, N, sY, 0.0, Rb, N, sY, mask, "fr_gemm", cf, 4);
        gemm_strided(ctx, cnt, false, false, n, m, n, 1.0, f.A.p, f.A.ld, 0, Yb + n, N, sY, 1.0, Rb + n, N, sY, mask, "fr_gemm");
        gemm_strided(ctx, cnt, false, false, n, m, n, 0.0, f.E.p, f.E.ld, 0, Yb, N, sY, 0.0, Rb + n, N, sY, mask, "fr_gemm", cf + 2, 4);
        gemm_strided(ctx, cnt, false, false, N, m, N, 1.0, Xb, N, NN, Rb, N, sY, 1.0, Yb, N, sY, mask, "fr_gemm");
        // Re H = C Y[0:n], Im H = C Y[n:2n]
        gemm_strided(ctx, cnt, false, false, q, m, n, 1.0, f.C.p, f.C.ld, 0, Yb, N, (size_t)N * m, 0.0, Hre + (size_t)b0 * qm, q, qm, mask, "fr_gemm");
        gemm_strided(ctx, cnt, false, false, q, m, n, 1.0, f.C.p, f.C.ld, 0, Yb + n, N, (size_t)N * m, 0.0, Him + (size_t)b0 * qm, q, qm, mask, "fr_gemm");
    }
};

FreqResponse freq_response(Ctx* ctx, const std::vector<FreqSystem>& sys, const std::vector<double>& omega, int chunk) {
    FrMethod md{omega};
    return freq_sweep(ctx, sys, chunk, md);
}

}  // namespace dre
