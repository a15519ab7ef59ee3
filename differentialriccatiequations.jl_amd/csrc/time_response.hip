// Time response of dense descriptor systems: step, impulse, simulate (time_response.hpp).
#include "time_response.hpp"

#include <climits>

#include "dense.hpp"
#include "dense_gj.hpp"
#include "profiling.hpp"

namespace dre {

#define TR_SCAN_T 64        // time steps per chunk of the prefix sum
#define TR_CONV_HS 2048     // LDS doubles of k_tr_conv for a chunk of h
#define TR_CONV_WS 4096     // ... and for the window of w
#define TR_CONV_JC 64       // at most this many j per chunk

// P = E - theta A (n x n, ld n) in one pass: one thread per (i, j), threadIdx.x along i.  Every offset is size_t.
__global__ __launch_bounds__(256) void k_tr_pencil(int n, const double* __restrict__ E, int lde, const double* __restrict__ A, int lda, double theta,
                                                   double* __restrict__ P) {
    const int i = blockIdx.x * 64 + threadIdx.x, j = blockIdx.y * 4 + threadIdx.y;
    if (i >= n || j >= n) return;
    P[(size_t)i + (size_t)j * n] = E[(size_t)i + (size_t)j * lde] - theta * A[(size_t)i + (size_t)j * lda];
}

// The three phases of the exclusive prefix sum  y_k = beta sum_{j < k} h_j  of the q m channels.  H holds h_k[i, c] at k q + i + c R (the thin
// GEMM's output, R its leading dimension); a channel is ch = c q + i, a chunk is TR_SCAN_T consecutive k, thread g = chunk * q m + ch
// (neighbouring threads read neighbouring i).  Within a chunk and across the chunk sums the order is ascending k: it follows from K alone.
// phase 1: bs[g] = sum of the chunk's h_k, k <= K
__global__ __launch_bounds__(256) void k_tr_scan_sums(int K, int q, int m, int nch, const double* __restrict__ H, size_t R, double* __restrict__ bs) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x, qm = (size_t)q * m;
    if (g >= (size_t)nch * qm) return;
    const size_t t = g / qm, ch = g - t * qm, c = ch / q, i = ch - c * q;
    const size_t kb = t * TR_SCAN_T, ke = kb + TR_SCAN_T < (size_t)K + 1 ? kb + TR_SCAN_T : (size_t)K + 1;
    const double* h = H + i + c * R;
    double s = 0.0;
    for (size_t k = kb; k < ke; ++k) s += h[k * q];
    bs[g] = s;
}
// phase 2: the chunk sums of one channel -> their exclusive prefix sums, one thread per channel
__global__ __launch_bounds__(256) void k_tr_scan_blocks(int qm, int nch, double* __restrict__ bs) {
    const int ch = blockIdx.x * 256 + threadIdx.x;
    if (ch >= qm) return;
    double run = 0.0;
    for (int t = 0; t < nch; ++t) {
        const size_t g = (size_t)t * qm + ch;
        const double v = bs[g];
        bs[g] = run;
        run += v;
    }
}
// phase 3: Y[k q m + ch] = beta (chunk offset + the chunk's own running sum), k <= K
__global__ __launch_bounds__(256) void k_tr_scan_add(int K, int q, int m, int nch, const double* __restrict__ H, size_t R, const double* __restrict__ bs,
                                                     double beta, double* __restrict__ Y) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x, qm = (size_t)q * m;
    if (g >= (size_t)nch * qm) return;
    const size_t t = g / qm, ch = g - t * qm, c = ch / q, i = ch - c * q;
    const size_t kb = t * TR_SCAN_T, ke = kb + TR_SCAN_T < (size_t)K + 1 ? kb + TR_SCAN_T : (size_t)K + 1;
    const double* h = H + i + c * R;
    double run = bs[g];
    for (size_t k = kb; k < ke; ++k) {
        Y[k * qm + ch] = beta * run;
        run += h[k * q];
    }
}

// impulse: Y[k q m + c q + i] = H[k q + i + c R], k <= K (the thin GEMM's layout -> the samples' layout)
__global__ __launch_bounds__(256) void k_tr_layout(int K, int q, int m, const double* __restrict__ H, size_t R, double* __restrict__ Y) {
    const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x, qm = (size_t)q * m;
    if (g >= ((size_t)K + 1) * qm) return;
    const size_t k = g / qm, ch = g - k * qm, c = ch / q, i = ch - c * q;
    Y[g] = H[k * q + i + c * R];
}

// simulate: the causal convolution  y_k = sum_{j < k} h_j w_{k-1-j} + G_k x_0  of scenario s = blockIdx.y for the TK samples k0 .. k0 + TK - 1
// of tile blockIdx.x; thread (kl, i) = (tid / q, tid % q) owns output i of sample k0 + kl (TK q <= 256) and accumulates it alone, j ascending,
// the input channel c innermost.  Per chunk of JC values of j the workgroup stages h_j[:, :] (JC q m <= TR_CONV_HS doubles; per channel the
// JC q rows are contiguous in H) and the window w_t, t = k0 - j0 - JC .. k0 + TK - 2 - j0 ((JC + TK - 1) m <= TR_CONV_WS doubles), formed from
// u on the fly: w_t = u_t + u_{t+1} (tustin) or u_{t+1} (backward Euler), zero outside 0 <= t < K.  U: u_k[c] of scenario s at
// s (K+1) m + k m + c.  GX (may be null): (G_k x_0^s)[i] at k q + i + s R.  Y: s (K+1) q + k q + i.
__global__ __launch_bounds__(256) void k_tr_conv(int K, int q, int m, int JC, int TK, int method, const double* __restrict__ H, size_t R,
                                                 const double* __restrict__ U, const double* __restrict__ GX, double* __restrict__ Y) {
    __shared__ double hs[TR_CONV_HS];
    __shared__ double ws[TR_CONV_WS];
    const int tid = threadIdx.x;
    const int k0 = blockIdx.x * TK;
    const size_t s = blockIdx.y;
    const int kl = tid / q, i = tid - kl * q;
    const int k = k0 + kl;
    const bool active = kl < TK && k <= K;
    const int kmax = min(k0 + TK - 1, K);                   // the tile's last sample: j < kmax is all it needs
    const double* Us = U + s * ((size_t)K + 1) * m;
    const int hrows = JC * q, wlen = (JC + TK - 1) * m;
    double acc = 0.0;
    for (int j0 = 0; j0 < kmax; j0 += JC) {
        const int tlo = k0 - j0 - JC;                       // the time of the window's first row (may be negative)
        for (int e = tid; e < hrows * m; e += 256) {
            const int c = e / hrows, rho = e - c * hrows;
            const int jj = rho / q, ii = rho - jj * q;
            const int j = j0 + jj;
            hs[(jj * m + c) * q + ii] = j < kmax ? H[(size_t)j * q + ii + (size_t)c * R] : 0.0;
        }
        for (int e = tid; e < wlen; e += 256) {
            const int tt = e / m, c = e - tt * m;
            const int t = tlo + tt;
            double w = 0.0;
            if (t >= 0 && t < K) {
                const double u1 = Us[(size_t)(t + 1) * m + c];
                w = method == TR_TUSTIN ? Us[(size_t)t * m + c] + u1 : u1;
            }
            ws[e] = w;
        }
        __syncthreads();
        if (active) {
            const int jend = min(JC, k - j0);               // j < k
            for (int jj = 0; jj < jend; ++jj) {
                const double* hp = hs + jj * m * q + i;
                const double* wp = ws + (kl + JC - 1 - jj) * m;      // w_{k-1-j}
                for (int c = 0; c < m; ++c) acc += hp[c * q] * wp[c];
            }
        }
        __syncthreads();
    }
    if (active) Y[(s * ((size_t)K + 1) + k) * q + i] = acc + (GX ? GX[(size_t)k * q + i + s * R] : 0.0);
}

static int pow2_at_least(long long v) {
    int p = 1;
    while (p < v) p *= 2;
    return p;
}

int tr_default_block(int q, int K, int n) {
    // the marching GEMM (L q x n)(n x n) has ceil(L q / 64) ceil(n / 64) output tiles of 64 x 64: L fills the device once ...
    const long long coltiles = (n + 63) / 64, K1 = (long long)K + 1;
    long long L = 1;
    while (((L * q + 63) / 64) * coltiles < TR_FILL_TILES) L *= 2;
    L = std::min<long long>(L, pow2_at_least(K1));
    // ... unless the stack, rounded up to whole blocks, would then hold a quarter more rows than samples
    while (L > 1 && (K1 + L - 1) / L * L * 4 > K1 * 5) L /= 2;
    return (int)L;
}

TimeResponse time_response(Ctx* ctx, const Mat& E, const Mat& A, const Mat& B, const Mat& C, int method, double dt, int K, int kind,
                           const double* U, int S, const double* X0, int block) {
    const char* who = "time_response";
    DRE_REQUIRE(method == TR_TUSTIN || method == TR_BACKWARD_EULER, std::string(who) + ": unknown method (0 tustin, 1 backward Euler)");
    DRE_REQUIRE(kind == TR_STEP || kind == TR_IMPULSE || kind == TR_SIMULATE, std::string(who) + ": unknown kind (0 step, 1 impulse, 2 simulate)");
    DRE_REQUIRE(K >= 1 && K < INT_MAX - 1, std::string(who) + ": at least one time step is needed (K >= 1)");
    DRE_REQUIRE(std::isfinite(dt) && dt > 0.0, std::string(who) + ": dt must be finite and positive");
    const int n = E.rows, m = B.cols, q = C.rows;
    DRE_REQUIRE(n >= 1 && n <= DENSE_MAX_N && E.cols == n && A.rows == n && A.cols == n && B.rows == n && m >= 1 && C.cols == n && q >= 1,
                std::string(who) + ": E and A must be n x n, B n x m and C q x n (n, m, q >= 1, n <= " + std::to_string(DENSE_MAX_N) + ")");
    DRE_REQUIRE(block >= 0 && (block & (block - 1)) == 0, std::string(who) + ": block must be 0 (default) or a power of two");
    if (kind == TR_SIMULATE) {
        DRE_REQUIRE(U && S >= 1 && S <= 65535, std::string(who) + ": simulate needs the input signals U and 1 <= S <= 65535 scenarios");
        DRE_REQUIRE(q <= TR_CONV_MAX_Q && (long long)q * m <= TR_CONV_MAX_QM, std::string(who) + ": simulate takes q <= " + std::to_string(TR_CONV_MAX_Q) +
                                                                                  " outputs and q m <= " + std::to_string(TR_CONV_MAX_QM));
    } else {
        DRE_REQUIRE(!U && !X0, std::string(who) + ": U and X0 go with kind 2 (simulate) only");
        S = 0;
    }
    gj_check_order(ctx, n, who);
    const int Lcap = pow2_at_least((long long)K + 1);
    const int L = block ? std::min(block, Lcap) : tr_default_block(q, K, n);
    const long long nblocks = ((long long)K + 1 + L - 1) / L;
    const long long Rll = nblocks * L * q;
    const int wide = std::max(std::max(m, S), 1);
    DRE_REQUIRE(Rll * n <= INT_MAX && Rll * wide <= INT_MAX && ((long long)K + 1) * q * std::max(m, 1) <= INT_MAX,
                std::string(who) + ": the stack of (K + 1 rounded up to the block) q rows does not fit an int index; fewer steps or a smaller block");
    const int R = (int)Rll;
    const size_t qm = (size_t)q * m, nout = kind == TR_SIMULATE ? (size_t)S * ((size_t)K + 1) * q : ((size_t)K + 1) * qm;
    const int nch = (int)(((size_t)K + 1 + TR_SCAN_T - 1) / TR_SCAN_T);
    // the stack, P / M / two powers of M (E^-1 borrows one), N and E^-1 B, h, G x_0, X_0, U, Y, the chunk sums; the split-K slabs of the GEMMs
    require_memory(ctx, (size_t)R * n + (size_t)4 * n * n + (size_t)2 * n * m + (size_t)R * m + (size_t)(R + n) * S + (size_t)S * ((size_t)K + 1) * m +
                            nout + (size_t)nch * qm + (size_t)2 * n * n);

    TimeResponse out;
    out.block = L;
    out.blocks = (int)nblocks;
    const double theta = method == TR_TUSTIN ? 0.5 * dt : dt;
    Mat P(ctx, n, n), Mm(ctx, n, n), T1(ctx, n, n), Nm(ctx, n, m), O(ctx, R, n), H(ctx, R, m);
    DevArr<int> piv(ctx, n);
    DevArr<GjCtl> ctl(ctx, 1);
    DevArr<double> Yd(ctx, nout);
    auto invert = [&](Mat& X, const char* what) {
        DRE_HIP(hipMemsetAsync(ctl.p, 0, sizeof(GjCtl), ctx->stream));
        gj_invert(ctx, X, piv.p, ctl.p);
        ++out.launches;
        if (read_back(ctx, ctl.p).singular)
            throw Error(ERR_SINGULAR, std::string(who) + ": " + what + " is singular (exactly zero or non-finite pivot)");
    };
    auto mul = [&](int Mr, int Nc, int Kc, double alpha, const double* Ap, int lda, const double* Bp, int ldb, double beta, double* Cp, int ldc,
                   const char* tag) {
        gemm(ctx, false, false, Mr, Nc, Kc, alpha, Ap, lda, Bp, ldb, beta, Cp, ldc, nullptr, tag);
        ++out.launches;
    };
    // 1. P = E - theta A, inverted in place
    {
        TimedScope ts(ctx, "tr_pencil", 24.0 * n * n, 2.0 * n * n);
        hipLaunchKernelGGL(k_tr_pencil, dim3(ceil_div(n, 64), ceil_div(n, 4)), dim3(64, 4), 0, ctx->stream, n, (const double*)E.p, E.ld, (const double*)A.p,
                           A.ld, theta, P.p);
        DRE_HIP(hipGetLastError());
        ++out.launches;
    }
    invert(P, method == TR_TUSTIN ? "E - (dt/2) A" : "E - dt A");
    // 2. M = 2 P^-1 E - I (tustin: beta = -1 on C = I) or P^-1 E;  N = theta P^-1 B
    if (method == TR_TUSTIN) {
        set_identity(ctx, Mm);
        ++out.launches;
        mul(n, n, n, 2.0, P.p, n, E.p, E.ld, -1.0, Mm.p, n, "tr_gemm_setup");
    } else {
        mul(n, n, n, 1.0, P.p, n, E.p, E.ld, 0.0, Mm.p, n, "tr_gemm_setup");
    }
    mul(n, m, n, theta, P.p, n, B.p, B.ld, 0.0, Nm.p, n, "tr_gemm_setup");
    // the right-hand operand of the thin product:  N, or E^-1 B for the impulse response (E^-1 in T1, which the squarings reuse)
    Mat Wm = Nm;
    if (kind == TR_IMPULSE) {
        copy_mat(ctx, E, T1);
        ++out.launches;
        invert(T1, "E (the impulse response starts from x(0+) = E^-1 B)");
        Wm = Mat(ctx, n, m);
        mul(n, m, n, 1.0, T1.p, n, B.p, B.ld, 0.0, Wm.p, n, "tr_gemm_setup");
    }
    // 3. doubling: rows [J q, 2 J q) = rows [0, J q) M^J;  the powers alternate between T1 and P (P^-1 is no longer needed)
    {
        Mat G0 = O.view(0, 0, q, n);
        copy_mat(ctx, C, G0);
        ++out.launches;
    }
    const double* Mp = Mm.p;       // M^J
    double* spare[2] = {T1.p, P.p};
    int flip = 0;
    for (int J = 1; J < L; J *= 2) {
        mul(J * q, n, n, 1.0, O.p, R, Mp, n, 0.0, O.p + (size_t)J * q, R, "tr_gemm_double");
        if (2 * J < L || nblocks > 1) {
            double* next = spare[flip];
            mul(n, n, n, 1.0, Mp, n, Mp, n, 0.0, next, n, "tr_gemm_square");
            ++out.squarings;
            Mp = next;
            flip ^= 1;
        }
    }
    // 4. block marching: block b + 1 = block b M^L
    for (long long b = 0; b + 1 < nblocks; ++b)
        mul(L * q, n, n, 1.0, O.p + (size_t)b * L * q, R, Mp, n, 0.0, O.p + (size_t)(b + 1) * L * q, R, "tr_gemm_march");
    // 5. h = O N (or O E^-1 B)
    mul(R, m, n, 1.0, O.p, R, Wm.p, n, 0.0, H.p, R, "tr_gemm_thin");
    // 6. the outputs
    if (kind == TR_STEP) {
        DevArr<double> bs(ctx, (size_t)nch * qm);
        const unsigned grid = (unsigned)(((size_t)nch * qm + 255) / 256);
        TimedScope ts(ctx, "tr_scan", 8.0 * (2.0 * (K + 1.0) * qm + nout), 2.0 * (K + 1.0) * qm, 3);
        hipLaunchKernelGGL(k_tr_scan_sums, dim3(grid), dim3(256), 0, ctx->stream, K, q, m, nch, (const double*)H.p, (size_t)R, bs.p);
        hipLaunchKernelGGL(k_tr_scan_blocks, dim3((unsigned)((qm + 255) / 256)), dim3(256), 0, ctx->stream, (int)qm, nch, bs.p);
        hipLaunchKernelGGL(k_tr_scan_add, dim3(grid), dim3(256), 0, ctx->stream, K, q, m, nch, (const double*)H.p, (size_t)R, (const double*)bs.p,
                           method == TR_TUSTIN ? 2.0 : 1.0, Yd.p);
        DRE_HIP(hipGetLastError());
        out.launches += 3;
    } else if (kind == TR_IMPULSE) {
        TimedScope ts(ctx, "tr_layout", 16.0 * nout, 0.0);
        hipLaunchKernelGGL(k_tr_layout, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, ctx->stream, K, q, m, (const double*)H.p, (size_t)R, Yd.p);
        DRE_HIP(hipGetLastError());
        ++out.launches;
    } else {
        DevArr<double> Ud(ctx, (size_t)S * ((size_t)K + 1) * m);
        Ud.upload(ctx, U, Ud.n);
        Mat GX;
        if (X0) {
            Mat Xd(ctx, n, S);
            DRE_HIP(hipMemcpyAsync(Xd.p, X0, (size_t)n * S * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
            ctx->sync();
            GX = Mat(ctx, R, S);
            mul(R, S, n, 1.0, O.p, R, Xd.p, n, 0.0, GX.p, R, "tr_gemm_thin");
        }
        const int JC = std::max(1, std::min(TR_CONV_JC, (int)(TR_CONV_HS / qm)));
        const int TK = std::max(1, std::min(256 / q, 1024 / m));
        DRE_REQUIRE((size_t)JC * qm <= TR_CONV_HS && (size_t)(JC + TK - 1) * m <= TR_CONV_WS && TK * q <= 256, "time_response: internal: the staging of k_tr_conv");
        const int tiles = (int)(((long long)K + 1 + TK - 1) / TK);
        TimedScope ts(ctx, "tr_conv", 8.0 * S * ((K + 1.0) * (m + q) + 1.0 * tiles * (K + 1.0) * qm / 2), 1.0 * S * K * (K + 1.0) * qm);
        hipLaunchKernelGGL(k_tr_conv, dim3(tiles, S), dim3(256), 0, ctx->stream, K, q, m, JC, TK, method, (const double*)H.p, (size_t)R, (const double*)Ud.p,
                           (const double*)GX.p, Yd.p);
        DRE_HIP(hipGetLastError());
        ++out.launches;
    }
    out.Y.resize(nout);
    DRE_HIP(hipMemcpyAsync(out.Y.data(), Yd.p, nout * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    return out;
}

}  // namespace dre
