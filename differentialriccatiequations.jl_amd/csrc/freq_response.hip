// Frequency response of dense descriptor systems, batched by frequency (freq_response.hpp).
#include "freq_response.hpp"

#include <cmath>

#include "dense_gj.hpp"
#include "profiling.hpp"

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

static size_t free_doubles(Ctx* ctx) {                   // what require_memory compares with
    size_t fr = 0, total = 0;
    DRE_HIP(hipMemGetInfo(&fr, &total));
    return (fr + ctx->pool.cached_bytes()) / sizeof(double);
}

FreqResponse freq_response(Ctx* ctx, const std::vector<FreqSystem>& sys, const std::vector<double>& omega, int chunk) {
    const char* who = "freq_response: ";
    DRE_REQUIRE(!sys.empty(), std::string(who) + "no systems");
    DRE_REQUIRE(!omega.empty(), std::string(who) + "at least one frequency is needed (K >= 1)");
    DRE_REQUIRE(omega.size() <= 2147483647u, std::string(who) + "too many frequencies");
    for (size_t k = 0; k < omega.size(); ++k)
        DRE_REQUIRE(std::isfinite(omega[k]), std::string(who) + "frequency " + std::to_string(k) + " is not finite");
    const int n = sys[0].E.rows, m = sys[0].B.cols, q = sys[0].C.rows;
    DRE_REQUIRE(n >= 1 && m >= 1 && q >= 1, std::string(who) + "n, m and q must be at least 1");
    for (size_t s = 0; s < sys.size(); ++s) {
        const FreqSystem& f = sys[s];
        DRE_REQUIRE(f.E.rows == n && f.E.cols == n && f.A.rows == n && f.A.cols == n && f.B.rows == n && f.B.cols == m && f.C.rows == q && f.C.cols == n,
                    std::string(who) + "system " + std::to_string(s) + ": E and A must be " + std::to_string(n) + " x " + std::to_string(n) + ", B " +
                        std::to_string(n) + " x " + std::to_string(m) + " and C " + std::to_string(q) + " x " + std::to_string(n));
    }
    DRE_REQUIRE(2 * (long long)n <= GJ_REGISTER_MAX_N, std::string(who) + "the real form of i w E - A has order 2n and goes through the register panel: 2n <= " +
                                                           std::to_string(GJ_REGISTER_MAX_N) + ", n = " + std::to_string(n));
    DRE_REQUIRE(chunk >= 0 && chunk <= FR_MAX_CHUNK, std::string(who) + "chunk must be in 0 .. 65535 (0: as many members as fit)");
    const int N = 2 * n, K = (int)omega.size(), nb = gj_batch_nb(N);
    DRE_REQUIRE(nb == fr_panel_nb(N), std::string(who) + "panel width table out of step with gj_batch_nb");
    const long long members = (long long)sys.size() * K;
    const size_t qm = (size_t)q * m, NN = (size_t)N * N;
    DRE_REQUIRE((unsigned long long)members * qm <= (1ull << 40), std::string(who) + "result too large");

    // the plan, and the memory of a whole chunk (and the frequencies) before the first kernel
    const size_t avail = free_doubles(ctx), fixed = (size_t)K + 512;
    const FrChunkPlan plan = fr_chunk_plan(avail > fixed ? avail - fixed : 0, n, m, q, members, chunk);
    if (plan.err == FR_PLAN_MEMORY)
        throw Error(ERR_ALLOC, std::string(who) + (chunk > 0 ? "a chunk of " + std::to_string(std::min<long long>(chunk, members)) + " members" : std::string("one member")) +
                                   " needs " + std::to_string(((size_t)std::max<long long>(1, std::min<long long>(chunk, members)) * fr_member_doubles(n, m, q) * 8) >> 20) +
                                   " MiB of device memory, " + std::to_string((avail * 8) >> 20) + " MiB available");
    DRE_REQUIRE(plan.err == FR_PLAN_OK, std::string(who) + "invalid chunk plan");
    DRE_REQUIRE(plan.chunks <= 2147483647LL, std::string(who) + "too many chunks");
    const int cs = plan.chunk;
    require_memory(ctx, (size_t)cs * fr_member_doubles(n, m, q) + fixed);

    FreqResponse out;
    out.chunk = cs; out.chunks = (int)plan.chunks;
    out.re.assign((size_t)members * qm, 0.0);
    out.im.assign((size_t)members * qm, 0.0);
    out.status.assign((size_t)members, BatchMemberStatus{});

    DevArr<double> w(ctx, (size_t)K);
    w.upload(ctx, omega);
    Mat M(ctx, N, N * cs), Pn(ctx, N, nb * cs), W(ctx, nb, N * cs), Y(ctx, N, m * cs), R(ctx, N, m * cs);
    DevArr<double> H(ctx, 2 * qm * cs), coef(ctx, (size_t)4 * cs);
    DevArr<int> piv(ctx, (size_t)N * cs);
    DevArr<BatchCtl> ctl(ctx, (size_t)cs);
    std::vector<BatchCtl> hctl((size_t)cs);
    std::vector<double> hH(2 * qm * cs);
    const double nan = std::nan("");

    for (long long g0 = 0; g0 < members; g0 += cs) {
        const int len = (int)std::min<long long>(cs, members - g0);
        double* Hre = H.p;
        double* Him = H.p + (size_t)len * qm;
        DRE_HIP(hipMemsetAsync(ctl.p, 0, sizeof(BatchCtl) * (size_t)len, ctx->stream));
        // the members of one system that fall into this chunk share that system's operands: [b0, b1) of the chunk, frequencies k0 ..
        auto segments = [&](auto&& f) {
            for (int b0 = 0; b0 < len;) {
                const long long g = g0 + b0;
                const int s = (int)(g / K), k0 = (int)(g % K), b1 = (int)std::min<long long>(len, b0 + (K - k0));
                f(sys[(size_t)s], b0, b1 - b0, k0);
                b0 = b1;
            }
        };
        segments([&](const FreqSystem& f, int b0, int cnt, int k0) {
            TimedScope ts(ctx, "fr_assemble", 8.0 * cnt * (2.0 * n * n + 4.0 * n * n), 1.0 * cnt * n * n);
            hipLaunchKernelGGL(k_fr_assemble, dim3(ceil_div(n, 64), ceil_div(n, 4), cnt), dim3(64, 4), 0, ctx->stream, n, (const double*)f.E.p, f.E.ld,
                               (const double*)f.A.p, f.A.ld, (const double*)(w.p + k0), M.p + (size_t)b0 * NN);
        });
        DRE_HIP(hipGetLastError());
        gj_invert_batched(ctx, len, N, M.p, piv.p, ctl.p, BM_GJ, Pn.p, W.p);
        segments([&](const FreqSystem& f, int b0, int cnt, int k0) {
            const BatchMask mask{ctl.p + b0, BM_GJ, 0};
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
        });
        // one copy of the chunk's Re H and Im H, one of its control blocks
        DRE_HIP(hipMemcpyAsync(hH.data(), H.p, sizeof(double) * 2 * qm * (size_t)len, hipMemcpyDeviceToHost, ctx->stream));
        DRE_HIP(hipMemcpyAsync(hctl.data(), ctl.p, sizeof(BatchCtl) * (size_t)len, hipMemcpyDeviceToHost, ctx->stream));
        ctx->sync();
        for (int b = 0; b < len; ++b) {
            const size_t g = (size_t)(g0 + b);
            double* re = out.re.data() + g * qm;
            double* im = out.im.data() + g * qm;
            if (hctl[(size_t)b].s.gj.singular) {
                BatchMemberStatus& st = out.status[g];
                st.code = ERR_SINGULAR;
                char wtxt[40];
                std::snprintf(wtxt, sizeof(wtxt), "%.17g", omega[g % (size_t)K]);
                st.msg = "freq_response, system " + std::to_string(g / (size_t)K) + ", frequency " + std::to_string(g % (size_t)K) + " (omega = " + wtxt +
                         "): i omega E - A is singular (exactly zero or non-finite pivot: omega on a pole, or a non-finite entry)";
                for (size_t t = 0; t < qm; ++t) { re[t] = nan; im[t] = nan; }
                continue;
            }
            std::memcpy(re, hH.data() + (size_t)b * qm, sizeof(double) * qm);
            std::memcpy(im, hH.data() + ((size_t)len + b) * qm, sizeof(double) * qm);
        }
    }
    return out;
}

}  // namespace dre
