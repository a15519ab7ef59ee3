// Whole-device symmetric eigensolver: two-sided cyclic block Jacobi (host model: tests/_block_jacobi_model.py).
//
// The q x q matrix is padded with zero rows and columns to Q = 16 p (p >= 2) and cut into p x p blocks of 16 x 16.  A sweep is the p - 1 (p even)
// or p (p odd: one block sits out per round) rounds of the round-robin tournament of the blocks; the floor(p / 2) block pairs of a round are
// disjoint, so their 32 x 32 pivot blocks are diagonalised independently (k_bj_pivot, one workgroup each, J_P to global memory, A untouched) and
// the whole similarity transformation of the round, A <- J' A J and V <- V J with J = blockdiag(J_P), is one launch (k_bj_update: one workgroup
// per 32 x 32 super-block, both products on v_mfma_f64_16x16x4_f64, every super-block read and written once).  Kernel boundaries are the only
// synchronisation between workgroups.  After every sweep off(A)^2 and ||A||_F^2 are summed in two launches (store_partials / load_partials) into
// the control block, which the host reads once per sweep.
//
// Index arithmetic: block, row and column indices are ints below the padded order Q <= DENSE_MAX_N; every element offset is formed in size_t.
#include "sym_jacobi.hpp"

#include <cmath>

#include "dense_device.hpp"
#include "dense_gj.hpp"
#include "profiling.hpp"

namespace dre {

namespace {

constexpr int PB = 2 * BJ_BLOCK;      // order of a pivot block
constexpr int LDP = PB + 1;           // leading dimension of a 32 x 32 block in LDS (odd: rows and columns both walk over all banks)

// pair k (0 <= k < players / 2) of round `step` (0 <= step < players - 1) of the round-robin tournament of an even number of players
__host__ __device__ inline void rr_pair(int players, int step, int k, int& a, int& b) {
    const int m = players - 1;
    if (k == 0) { a = m; b = step; }
    else { a = (step + k) % m; b = (step - k + m) % m; }
}

// ---- pivot blocks ------------------------------------------------------------------------------------------------------------------------
// One workgroup per block pair (bi, bj) of the round: gathers the 32 x 32 pivot block [A_ii A_ij; A_ji A_jj] into LDS, diagonalises it by
// cyclic Jacobi (16 disjoint rotations per step, 31 steps per sweep, round-robin order) and leaves J (column-major, 32 x 32) in Jbuf and
// "a rotation was done" in rotated.  A rotation (r, c) is done when |a_rc| > (tol / Q) ||A||_F; a skipped rotation is the exact identity,
// so a zero padding row stays a unit row of J.
__global__ __launch_bounds__(256) void k_bj_pivot(int Q, const double* __restrict__ A, const int* __restrict__ pairs, const BjCtl* __restrict__ ctl,
                                                  double tol, double* __restrict__ Jbuf, int* __restrict__ rotated) {
    __shared__ double G[PB * LDP], J[PB * LDP], cs[2 * BJ_BLOCK];
    __shared__ int flag;
    const int tid = threadIdx.x;
    const int bi = pairs[2 * blockIdx.x], bj = pairs[2 * blockIdx.x + 1];
    const double thr = tol / (double)Q * ctl->norm;
    for (int e = tid; e < PB * PB; e += 256) {
        const int i = e & (PB - 1), j = e >> 5;
        const int gi = (i < BJ_BLOCK ? bi : bj) * BJ_BLOCK + (i & (BJ_BLOCK - 1)), gj = (j < BJ_BLOCK ? bi : bj) * BJ_BLOCK + (j & (BJ_BLOCK - 1));
        G[i + LDP * j] = A[(size_t)gi + (size_t)gj * (size_t)Q];
        J[i + LDP * j] = i == j ? 1.0 : 0.0;
    }
    if (tid == 0) flag = 0;
    __syncthreads();
    int any = 0;
    for (int sw = 0; sw < BJ_INNER_MAX; ++sw) {
        for (int step = 0; step < PB - 1; ++step) {
            if (tid < BJ_BLOCK) {
                int a, b;
                rr_pair(PB, step, tid, a, b);
                const int p = a < b ? a : b, q = a < b ? b : a;
                const double app = G[p + LDP * p], aqq = G[q + LDP * q], apq = G[p + LDP * q];
                double c = 1.0, s = 0.0;
                if (fabs(apq) > thr) {
                    const double tau = (aqq - app) / (2.0 * apq);
                    const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                    c = 1.0 / sqrt(1.0 + t * t);
                    s = t * c;
                    flag = 1;
                }
                cs[2 * tid] = c; cs[2 * tid + 1] = s;
            }
            __syncthreads();
            // columns of G and of J: (G or J, pair k, row i)
            for (int e = tid; e < 2 * BJ_BLOCK * PB; e += 256) {
                const int i = e & (PB - 1), k = (e >> 5) & (BJ_BLOCK - 1);
                double* M = e >= BJ_BLOCK * PB ? J : G;
                const double c = cs[2 * k], s = cs[2 * k + 1];
                if (s != 0.0) {
                    int a, b;
                    rr_pair(PB, step, k, a, b);
                    const int p = a < b ? a : b, q = a < b ? b : a;
                    const double x = M[i + LDP * p], y = M[i + LDP * q];
                    M[i + LDP * p] = c * x - s * y;
                    M[i + LDP * q] = s * x + c * y;
                }
            }
            __syncthreads();
            // rows of G: (pair k, column j); the annihilated entries are set to zero exactly
            for (int e = tid; e < BJ_BLOCK * PB; e += 256) {
                const int j = e & (PB - 1), k = e >> 5;
                const double c = cs[2 * k], s = cs[2 * k + 1];
                if (s != 0.0) {
                    int a, b;
                    rr_pair(PB, step, k, a, b);
                    const int p = a < b ? a : b, q = a < b ? b : a;
                    const double x = G[p + LDP * j], y = G[q + LDP * j];
                    G[p + LDP * j] = j == q ? 0.0 : c * x - s * y;
                    G[q + LDP * j] = j == p ? 0.0 : s * x + c * y;
                }
            }
            __syncthreads();
        }
        const int f = flag;          // (uniform: every write of this sweep is behind a barrier)
        __syncthreads();
        if (tid == 0) flag = 0;
        __syncthreads();
        if (!f) break;
        any = 1;
    }
    double* Jo = Jbuf + (size_t)blockIdx.x * (PB * PB);
    for (int e = tid; e < PB * PB; e += 256) Jo[e] = J[(e & (PB - 1)) + LDP * (e >> 5)];
    if (tid == 0) rotated[blockIdx.x] = any;
}

// ---- the similarity transformation of a round ---------------------------------------------------------------------------------------------
// One workgroup per 32 x 32 super-block X of A or V:  X <- L' X R  with L, R one of the round's J_P or the identity.  m block pairs, `sit` the
// block that sits out (-1: none), p blocks.  Workgroups, in order:
//   m * m          A_PQ <- J_P' A_PQ J_Q                     (P, Q block pairs)
//   2 m if sit     A_sQ <- A_sQ J_Q,  A_Ps <- J_P' A_Ps      (16 x 32 and 32 x 16: the absent half is zero in LDS and not written)
//   ceil(p/2) * m  V_tQ <- V_tQ J_Q                          (t: two block rows of V)
// A pair whose pivot block needed no rotation has J = I exactly: its factor is skipped, and a super-block with both factors skipped is left alone.
// Four waves, wave (wr, wc) owns the 16 x 16 tile (wr, wc) of the super-block in both products.
__global__ __launch_bounds__(256) void k_bj_update(int Q, int p, int m, int sit, const int* __restrict__ pairs, const double* __restrict__ Jbuf,
                                                   const int* __restrict__ rotated, double* __restrict__ A, double* __restrict__ V) {
    __shared__ double Xs[PB * LDP], Ts[PB * LDP], JL[PB * LDP], JR[PB * LDP];
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    int rb0, rb1, cb0, cb1, L = -1, R = -1;
    double* M = A;
    if (b < m * m) {
        L = b / m; R = b % m;
        rb0 = pairs[2 * L]; rb1 = pairs[2 * L + 1]; cb0 = pairs[2 * R]; cb1 = pairs[2 * R + 1];
    } else {
        b -= m * m;
        if (sit >= 0 && b < 2 * m) {
            if (b < m) { R = b; rb0 = sit; rb1 = -1; cb0 = pairs[2 * R]; cb1 = pairs[2 * R + 1]; }
            else { L = b - m; rb0 = pairs[2 * L]; rb1 = pairs[2 * L + 1]; cb0 = sit; cb1 = -1; }
        } else {
            if (sit >= 0) b -= 2 * m;
            const int t = b / m;
            R = b % m; M = V;
            rb0 = 2 * t; rb1 = 2 * t + 1 < p ? 2 * t + 1 : -1; cb0 = pairs[2 * R]; cb1 = pairs[2 * R + 1];
        }
    }
    if (L >= 0 && !rotated[L]) L = -1;
    if (R >= 0 && !rotated[R]) R = -1;
    if (L < 0 && R < 0) return;          // (uniform in the workgroup)
    for (int e = tid; e < PB * PB; e += 256) {
        const int i = e & (PB - 1), j = e >> 5;
        const int br = (i >> 4) ? rb1 : rb0, bc = (j >> 4) ? cb1 : cb0;
        double x = 0.0;
        if (br >= 0 && bc >= 0) x = M[(size_t)(br * BJ_BLOCK + (i & 15)) + (size_t)(bc * BJ_BLOCK + (j & 15)) * (size_t)Q];
        Xs[i + LDP * j] = x;
        if (L >= 0) JL[i + LDP * j] = Jbuf[(size_t)L * (PB * PB) + e];
        if (R >= 0) JR[i + LDP * j] = Jbuf[(size_t)R * (PB * PB) + e];
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63, wr = wave >> 1, wc = wave & 1;
    const int lr = lane & 15, lk = lane >> 4;
    // T = L' X  (MFMA operand maps: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15]; D: column lane & 15, row (lane >> 4) + 4 reg)
    if (L >= 0) {
        v4d acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k0 = 0; k0 < PB; k0 += 4)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(JL[(k0 + lk) + LDP * (wr * 16 + lr)], Xs[(k0 + lk) + LDP * (wc * 16 + lr)], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) Ts[(wr * 16 + lk + 4 * r) + LDP * (wc * 16 + lr)] = acc[r];
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) Ts[(wr * 16 + lk + 4 * r) + LDP * (wc * 16 + lr)] = Xs[(wr * 16 + lk + 4 * r) + LDP * (wc * 16 + lr)];
    }
    __syncthreads();          // (T complete; every read of Xs is done, so the result may go there)
    if (R >= 0) {
        v4d acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k0 = 0; k0 < PB; k0 += 4)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Ts[(wr * 16 + lr) + LDP * (k0 + lk)], JR[(k0 + lk) + LDP * (wc * 16 + lr)], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) Xs[(wr * 16 + lk + 4 * r) + LDP * (wc * 16 + lr)] = acc[r];
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) Xs[(wr * 16 + lk + 4 * r) + LDP * (wc * 16 + lr)] = Ts[(wr * 16 + lk + 4 * r) + LDP * (wc * 16 + lr)];
    }
    __syncthreads();
    for (int e = tid; e < PB * PB; e += 256) {
        const int i = e & (PB - 1), j = e >> 5;
        const int br = (i >> 4) ? rb1 : rb0, bc = (j >> 4) ? cb1 : cb0;
        if (br >= 0 && bc >= 0) M[(size_t)(br * BJ_BLOCK + (i & 15)) + (size_t)(bc * BJ_BLOCK + (j & 15)) * (size_t)Q] = Xs[i + LDP * j];
    }
}

// ---- norms and the decision -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_bj_norms(int Q, const double* __restrict__ A, double* __restrict__ part) {
    double s_off = 0.0, s_diag = 0.0;
    const size_t tot = (size_t)Q * (size_t)Q;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < tot; idx += (size_t)gridDim.x * blockDim.x) {
        const double x = A[idx];
        if (idx % (size_t)Q == idx / (size_t)Q) s_diag += x * x; else s_off += x * x;
    }
    store_partials(part, s_off, s_diag);
}

__global__ __launch_bounds__(256) void k_bj_decide(int nparts, const double* __restrict__ part, double tol, int count, BjCtl* ctl) {
    double s[2];
    load_partials(nparts, part, s);
    if (threadIdx.x == 0) {
        const double off = sqrt(s[0]), norm = sqrt(s[0] + s[1]);
        ctl->off = off; ctl->norm = norm;
        ctl->nonfinite = isfinite(norm) ? 0 : 1;
        ctl->done = isfinite(norm) && off <= tol * norm ? 1 : 0;
        ctl->sweeps += count;
    }
}

__global__ void k_bj_diag(int q, int Q, const double* __restrict__ A, double* __restrict__ w) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < q) w[i] = A[(size_t)i + (size_t)i * (size_t)Q];
}

}  // namespace

void sym_eig_dump_input(Ctx* ctx, const Mat& S) {
    const char* dir = std::getenv("DRE_SYM_EIG_DUMP");
    if (!dir || !*dir || S.rows == 0 || S.rows != S.cols) return;
    static std::atomic<long> count{0};
    const int q = S.rows;
    std::vector<double> h((size_t)q * q);
    DRE_HIP(hipMemcpy2DAsync(h.data(), (size_t)q * sizeof(double), S.p, (size_t)S.ld * sizeof(double), (size_t)q * sizeof(double), q, hipMemcpyDeviceToHost,
                             ctx->stream));
    ctx->sync();
    const std::string path = std::string(dir) + "/S_" + std::to_string(count++) + "_" + std::to_string(q) + ".f64";
    if (FILE* f = std::fopen(path.c_str(), "wb")) { (void)std::fwrite(h.data(), sizeof(double), h.size(), f); std::fclose(f); }
}

SymEig sym_eig_jacobi(Ctx* ctx, const Mat& S, double tol, BjStats* stats) {
    DRE_REQUIRE(S.rows == S.cols, "sym_eig_jacobi: square matrix expected");
    SymEig out;
    const int q = S.rows;
    out.q = q;
    if (stats) *stats = BjStats{};
    if (q == 0) return out;
    DRE_REQUIRE(q <= DENSE_MAX_N - 2 * BJ_BLOCK, "sym_eig_jacobi: order beyond the device's 32-bit index limit");
    if (!(tol > 0.0)) tol = q * DBL_EPS;
    const int Q = bj_padded_order(q), p = Q / BJ_BLOCK, players = p + (p & 1), nrounds = players - 1, m = p / 2;
    require_memory(ctx, (size_t)2 * Q * Q + (size_t)q * q);

    // the schedule: per round the m block pairs (i < j), then the block that sits out
    std::vector<int> tab((size_t)nrounds * (2 * m + 1));
    for (int r = 0; r < nrounds; ++r) {
        int* t = tab.data() + (size_t)r * (2 * m + 1);
        int np_ = 0, sit = -1;
        for (int k = 0; k < players / 2; ++k) {
            int a, b;
            rr_pair(players, r, k, a, b);
            if (a >= p) sit = b;
            else if (b >= p) sit = a;
            else { t[2 * np_] = std::min(a, b); t[2 * np_ + 1] = std::max(a, b); ++np_; }
        }
        t[2 * m] = sit;
    }
    DevArr<int> dtab(ctx, tab.size());
    dtab.upload(ctx, tab);

    Mat A(ctx, Q, Q), V(ctx, Q, Q);
    if (Q != q) fill_mat(ctx, A, 0.0);
    { Mat top = A.view(0, 0, q, q); copy_mat(ctx, S, top); }
    set_identity(ctx, V, 1.0);
    DevArr<double> Jbuf(ctx, (size_t)m * PB * PB), part(ctx, 2 * NORM_PARTS);
    DevArr<int> rotated(ctx, m);
    DevArr<BjCtl> ctl(ctx, 1);
    DRE_HIP(hipMemsetAsync(ctl.p, 0, sizeof(BjCtl), ctx->stream));

    auto measure = [&](int count) {
        TimedScope ts(ctx, "bj_norm", 8.0 * Q * Q, 0.0, 2);
        hipLaunchKernelGGL(k_bj_norms, dim3(NORM_PARTS), dim3(256), 0, ctx->stream, Q, (const double*)A.p, part.p);
        hipLaunchKernelGGL(k_bj_decide, dim3(1), dim3(256), 0, ctx->stream, NORM_PARTS, (const double*)part.p, tol, count, ctl.p);
        return read_back(ctx, ctl.p);
    };
    BjCtl h = measure(0);
    if (h.nonfinite) throw Error(ERR_INVALID, "sym_eig_jacobi: the matrix has non-finite entries");
    long rounds = 0;
    const unsigned vjobs = (unsigned)((p + 1) / 2) * (unsigned)m;
    while (!h.done) {
        if (h.sweeps >= BJ_MAX_SWEEPS)
            throw Error(ERR_INTERNAL, "sym_eig_jacobi: no convergence in " + std::to_string(h.sweeps) + " sweeps (off / norm = " + std::to_string(h.off / h.norm) + ")");
        for (int r = 0; r < nrounds; ++r) {
            const int* t = dtab.p + (size_t)r * (2 * m + 1);
            const int sit = tab[(size_t)r * (2 * m + 1) + 2 * m];
            {
                TimedScope ts(ctx, "bj_pivot", 16.0 * m * PB * PB, 0.0);
                hipLaunchKernelGGL(k_bj_pivot, dim3(m), dim3(256), 0, ctx->stream, Q, (const double*)A.p, t, (const BjCtl*)ctl.p, tol, Jbuf.p, rotated.p);
            }
            {
                const unsigned grid = (unsigned)m * (unsigned)m + (sit >= 0 ? 2u * (unsigned)m : 0u) + vjobs;
                TimedScope ts(ctx, "bj_update", 32.0 * Q * Q, 8.0 * PB * (double)Q * Q * 1.5);
                hipLaunchKernelGGL(k_bj_update, dim3(grid), dim3(256), 0, ctx->stream, Q, p, m, sit, t, (const double*)Jbuf.p, (const int*)rotated.p, A.p, V.p);
            }
            ++rounds;
        }
        h = measure(1);
        if (h.nonfinite) throw Error(ERR_INVALID, "sym_eig_jacobi: non-finite values in sweep " + std::to_string(h.sweeps));
    }
    DRE_HIP(hipGetLastError());
    if (env_trace("compress")) std::fprintf(stderr, "[sym_eig_jacobi] q=%d: %d sweeps, %ld rounds, off / norm = %.2e\n", q, h.sweeps, rounds, h.norm > 0 ? h.off / h.norm : 0.0);
    if (stats) { stats->sweeps = h.sweeps; stats->rounds = rounds; }
    out.j = q; out.nref = 0; out.snorm = h.norm;
    out.Z = Mat(ctx, q, q);
    { Mat top = V.view(0, 0, q, q); copy_mat(ctx, top, out.Z); }
    DevArr<double> dw(ctx, q);
    hipLaunchKernelGGL(k_bj_diag, dim3(ceil_div(q, 256)), dim3(256), 0, ctx->stream, q, Q, (const double*)A.p, dw.p);
    out.w.resize(q);
    DRE_HIP(hipMemcpyAsync(out.w.data(), dw.p, q * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    return out;
}

}  // namespace dre
