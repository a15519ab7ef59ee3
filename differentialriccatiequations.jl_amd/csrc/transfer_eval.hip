// Transfer function of dense descriptor systems at complex points, batched by point (transfer_eval.hpp).
#include "transfer_eval.hpp"

#include <cmath>

#include "dense_cgj.hpp"
#include "profiling.hpp"

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

static size_t free_doubles(Ctx* ctx) {                   // what require_memory compares with
    size_t fr = 0, total = 0;
    DRE_HIP(hipMemGetInfo(&fr, &total));
    return (fr + ctx->pool.cached_bytes()) / sizeof(double);
}

FreqResponse transfer_eval(Ctx* ctx, const std::vector<FreqSystem>& sys, const std::vector<double>& s_re, const std::vector<double>& s_im, int chunk) {
    const char* who = "transfer_eval: ";
    DRE_REQUIRE(!sys.empty(), std::string(who) + "no systems");
    DRE_REQUIRE(!s_re.empty() && s_re.size() == s_im.size(), std::string(who) + "at least one point is needed (K >= 1), with a real and an imaginary part each");
    DRE_REQUIRE(s_re.size() <= 2147483647u, std::string(who) + "too many points");
    for (size_t k = 0; k < s_re.size(); ++k)
        DRE_REQUIRE(std::isfinite(s_re[k]) && std::isfinite(s_im[k]), std::string(who) + "point " + std::to_string(k) + " is not finite");
    const int n = sys[0].E.rows, m = sys[0].B.cols, q = sys[0].C.rows;
    DRE_REQUIRE(n >= 1 && m >= 1 && q >= 1, std::string(who) + "n, m and q must be at least 1");
    for (size_t s = 0; s < sys.size(); ++s) {
        const FreqSystem& f = sys[s];
        DRE_REQUIRE(f.E.rows == n && f.E.cols == n && f.A.rows == n && f.A.cols == n && f.B.rows == n && f.B.cols == m && f.C.rows == q && f.C.cols == n,
                    std::string(who) + "system " + std::to_string(s) + ": E and A must be " + std::to_string(n) + " x " + std::to_string(n) + ", B " +
                        std::to_string(n) + " x " + std::to_string(m) + " and C " + std::to_string(q) + " x " + std::to_string(n));
    }
    DRE_REQUIRE(n <= GJ_REGISTER_MAX_N, std::string(who) + "s E - A goes through the complex register panel: n <= " + std::to_string(GJ_REGISTER_MAX_N) +
                                            ", n = " + std::to_string(n));
    DRE_REQUIRE(chunk >= 0 && chunk <= FR_MAX_CHUNK, std::string(who) + "chunk must be in 0 .. 65535 (0: as many members as fit)");
    const int K = (int)s_re.size(), nb = cgj_batch_nb(n);
    DRE_REQUIRE(nb == fr_panel_nb_c(n), std::string(who) + "panel width table out of step with cgj_batch_nb");
    const long long members = (long long)sys.size() * K;
    const size_t qm = (size_t)q * m, nn = (size_t)n * n;
    DRE_REQUIRE((unsigned long long)members * qm <= (1ull << 40), std::string(who) + "result too large");

    // the plan, and the memory of a whole chunk (and the points) before the first kernel
    const size_t avail = free_doubles(ctx), fixed = (size_t)2 * K + 512;
    const FrChunkPlan plan = fr_chunk_plan_c(avail > fixed ? avail - fixed : 0, n, m, q, members, chunk);
    if (plan.err == FR_PLAN_MEMORY)
        throw Error(ERR_ALLOC, std::string(who) + (chunk > 0 ? "a chunk of " + std::to_string(std::min<long long>(chunk, members)) + " members" : std::string("one member")) +
                                   " needs " + std::to_string(((size_t)std::max<long long>(1, std::min<long long>(chunk, members)) * fr_member_doubles_c(n, m, q) * 8) >> 20) +
                                   " MiB of device memory, " + std::to_string((avail * 8) >> 20) + " MiB available");
    DRE_REQUIRE(plan.err == FR_PLAN_OK, std::string(who) + "invalid chunk plan");
    DRE_REQUIRE(plan.chunks <= 2147483647LL, std::string(who) + "too many chunks");
    const int cs = plan.chunk;
    require_memory(ctx, (size_t)cs * fr_member_doubles_c(n, m, q) + fixed);

    FreqResponse out;
    out.chunk = cs; out.chunks = (int)plan.chunks;
    out.re.assign((size_t)members * qm, 0.0);
    out.im.assign((size_t)members * qm, 0.0);
    out.status.assign((size_t)members, BatchMemberStatus{});

    DevArr<double> sr(ctx, (size_t)K), si(ctx, (size_t)K);
    sr.upload(ctx, s_re);
    si.upload(ctx, s_im);
    Mat Z(ctx, n, 2 * n * cs), Pt(ctx, n, 2 * nb * cs), Wt(ctx, 2 * nb, 2 * n * cs), Y(ctx, n, 2 * m * cs), Rt(ctx, 2 * n, 2 * m * cs);
    DevArr<double> H(ctx, 2 * qm * cs), coef(ctx, (size_t)6 * cs);
    DevArr<int> piv(ctx, (size_t)n * cs);
    DevArr<BatchCtl> ctl(ctx, (size_t)cs);
    std::vector<BatchCtl> hctl((size_t)cs);
    std::vector<double> hH(2 * qm * cs);
    const double nan = std::nan("");

    for (long long g0 = 0; g0 < members; g0 += cs) {
        const int len = (int)std::min<long long>(cs, members - g0);
        double* Hre = H.p;
        double* Him = H.p + (size_t)len * qm;
        DRE_HIP(hipMemsetAsync(ctl.p, 0, sizeof(BatchCtl) * (size_t)len, ctx->stream));
        // the members of one system that fall into this chunk share that system's operands: [b0, b1) of the chunk, points k0 ..
        auto segments = [&](auto&& f) {
            for (int b0 = 0; b0 < len;) {
                const long long g = g0 + b0;
                const int s = (int)(g / K), k0 = (int)(g % K), b1 = (int)std::min<long long>(len, b0 + (K - k0));
                f(sys[(size_t)s], b0, b1 - b0, k0);
                b0 = b1;
            }
        };
        segments([&](const FreqSystem& f, int b0, int cnt, int k0) {
            TimedScope ts(ctx, "tf_assemble", 8.0 * cnt * (2.0 * n * n + 2.0 * n * n), 2.0 * cnt * n * n);
            hipLaunchKernelGGL(k_tf_assemble, dim3(ceil_div(n, 64), ceil_div(n, 4), cnt), dim3(64, 4), 0, ctx->stream, n, (const double*)f.E.p, f.E.ld,
                               (const double*)f.A.p, f.A.ld, (const double*)(sr.p + k0), (const double*)(si.p + k0), Z.p + (size_t)b0 * 2 * nn);
        });
        DRE_HIP(hipGetLastError());
        cgj_invert_batched(ctx, len, n, Z.p, piv.p, ctl.p, BM_GJ, Pt.p, Wt.p);
        segments([&](const FreqSystem& f, int b0, int cnt, int k0) {
            const BatchMask mask{ctl.p + b0, BM_GJ, 0};
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
        });
        DRE_HIP(hipGetLastError());
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
                char stxt[96];
                std::snprintf(stxt, sizeof(stxt), "%.17g%+.17gi", s_re[g % (size_t)K], s_im[g % (size_t)K]);
                st.msg = "transfer_eval, system " + std::to_string(g / (size_t)K) + ", point " + std::to_string(g % (size_t)K) + " (s = " + stxt +
                         "): s E - A is singular (exactly zero or non-finite pivot: s on a pole, or a non-finite entry)";
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
