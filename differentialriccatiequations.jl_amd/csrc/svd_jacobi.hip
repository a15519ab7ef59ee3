// Device SVD: one-sided (Hestenes) cyclic block Jacobi (host model: tests/_svd_jacobi_model.py).
//
// The m x w matrix (m >= w; a wide input is transposed once at the entry, U and V are swapped at the exit) is padded with zero columns to
// W = 16 p (p >= 2) and cut into p column blocks of 16: the working copy G (m x W), V = I (W x W).  A sweep is the p - 1 (p even) or p (p odd:
// one block sits out per round) rounds of the round-robin tournament of the blocks.  ONE launch per round (k_svj_round): one workgroup of 256
// per block pair (i, j) forms H = [G_i G_j]'[G_i G_j] (32 x 32, v_mfma_f64_16x16x4_f64, row slabs of 64 through LDS), diagonalises it by cyclic
// Jacobi in LDS (J accumulated) and, if anything was rotated, applies [G_i G_j] <- [G_i G_j] J and [V_i V_j] <- [V_i V_j] J on MFMA.  The pairs
// of a round own disjoint columns, so G and V are updated in place; kernel boundaries are the only synchronisation between workgroups.  After
// every sweep a one-workgroup kernel folds the `rotated` flags into the control block, which the host reads once per sweep; a sweep without a
// rotation ends the iteration.
//
// Index arithmetic: row and column indices are ints below max(m, W) <= DENSE_MAX_N; every element offset is formed in size_t.
#include "svd_jacobi.hpp"

#include <algorithm>
#include <cmath>
#include <numeric>

#include "dense_device.hpp"
#include "dense_gj.hpp"
#include "profiling.hpp"

namespace dre {

namespace {

constexpr int SB = 16;                // column block
constexpr int PB = 2 * SB;            // columns of a block pair, order of its Gram matrix
constexpr int LDP = PB + 1;           // leading dimension of a 32 x 32 block in LDS (odd: rows and columns both walk over all banks)
constexpr int LDX = SVJ_SLAB + 1;     // leading dimension of a 64 x 32 row slab in LDS
constexpr int SVJ_INNER_MAX = 10;     // cyclic sweeps of a Gram block at most (ended by the first sweep without a rotation)

// pair k (0 <= k < players / 2) of round `step` (0 <= step < players - 1) of the round-robin tournament of an even number of players
// (the tournament of sym_jacobi.hip)
__host__ __device__ inline void rr_pair(int players, int step, int k, int& a, int& b) {
    const int m = players - 1;
    if (k == 0) { a = m; b = step; }
    else { a = (step + k) % m; b = (step - k + m) % m; }
}

// rows [r0, r0 + 64) of the column blocks c0 and c1 (first columns) of M (rows x ., leading dimension ld) into Xs; rows beyond `rows` are zero
__device__ inline void svj_load_slab(const double* __restrict__ M, int rows, size_t ld, int c0, int c1, int r0, double* Xs) {
    for (int e = threadIdx.x; e < SVJ_SLAB * PB; e += 256) {
        const int i = e & (SVJ_SLAB - 1), j = e >> 6;
        const int row = r0 + i, col = (j < SB ? c0 : c1) + (j & (SB - 1));
        Xs[i + LDX * j] = row < rows ? M[(size_t)row + (size_t)col * ld] : 0.0;
    }
}

// [M_c0 M_c1] <- [M_c0 M_c1] J, slab by slab: wave w owns the rows 16 w .. 16 w + 15 of the slab in both column tiles
__device__ inline void svj_apply(double* __restrict__ M, int rows, size_t ld, int c0, int c1, const double* J, double* Xs) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
    for (int r0 = 0; r0 < rows; r0 += SVJ_SLAB) {
        svj_load_slab(M, rows, ld, c0, c1, r0, Xs);
        __syncthreads();
        // MFMA operand maps: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15]; D: column lane & 15, row (lane >> 4) + 4 reg
        v4d acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k0 = 0; k0 < PB; k0 += 4) {
            const double a = Xs[(wave * 16 + lr) + LDX * (k0 + lk)];
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, J[(k0 + lk) + LDP * lr], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, J[(k0 + lk) + LDP * (16 + lr)], acc1, 0, 0, 0);
        }
        // (a wave reads and writes its own 16 rows of the slab only)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            Xs[(wave * 16 + lk + 4 * r) + LDX * lr] = acc0[r];
            Xs[(wave * 16 + lk + 4 * r) + LDX * (16 + lr)] = acc1[r];
        }
        __syncthreads();
        for (int e = tid; e < SVJ_SLAB * PB; e += 256) {
            const int i = e & (SVJ_SLAB - 1), j = e >> 6;
            const int row = r0 + i, col = (j < SB ? c0 : c1) + (j & (SB - 1));
            if (row < rows) M[(size_t)row + (size_t)col * ld] = Xs[i + LDX * j];
        }
        __syncthreads();
    }
}

// ---- one round -------------------------------------------------------------------------------------------------------------------------------
// G: m x W (leading dimension ldg), V: W x W (leading dimension W); pairs: the round's block pairs (bi < bj); rotated: one flag per pair.
// A rotation (r, c) is done when h_rc != 0, h_rr h_cc > 0, |h_rc| > tol sqrt(h_rr h_cc) and sqrt(h_rr h_cc) > (tol ||A||_F)^2; a skipped rotation is
// the exact identity, so a zero padding column stays a zero column of G and a unit column of V.
__global__ __launch_bounds__(256) void k_svj_round(int m, int W, double* __restrict__ G, size_t ldg, double* __restrict__ V, const int* __restrict__ pairs,
                                                   const SvjCtl* __restrict__ ctl, double tol, int* __restrict__ rotated) {
    __shared__ double Xs[LDX * PB], H[PB * LDP], J[PB * LDP], cs[2 * SB];
    __shared__ int flag;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, wr = wave >> 1, wc = wave & 1, lr = lane & 15, lk = lane >> 4;
    const int c0 = pairs[2 * blockIdx.x] * SB, c1 = pairs[2 * blockIdx.x + 1] * SB;
    const double floor_ = (tol * ctl->norm) * (tol * ctl->norm);

    // 1. H = X'X, X = [G_i G_j]: wave (wr, wc) owns the tile (wr, wc); both operands come from the same slab
    v4d acc = {0.0, 0.0, 0.0, 0.0};
    for (int r0 = 0; r0 < m; r0 += SVJ_SLAB) {
        svj_load_slab(G, m, ldg, c0, c1, r0, Xs);
        __syncthreads();
#pragma unroll
        for (int k0 = 0; k0 < SVJ_SLAB; k0 += 4)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Xs[(k0 + lk) + LDX * (wr * 16 + lr)], Xs[(k0 + lk) + LDX * (wc * 16 + lr)], acc, 0, 0, 0);
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) H[(wr * 16 + lk + 4 * r) + LDP * (wc * 16 + lr)] = acc[r];
    for (int e = tid; e < PB * PB; e += 256) J[(e & (PB - 1)) + LDP * (e >> 5)] = (e & (PB - 1)) == (e >> 5) ? 1.0 : 0.0;
    if (tid == 0) flag = 0;
    __syncthreads();

    // 2. cyclic Jacobi on H (16 disjoint rotations per step, 31 steps per sweep, round-robin order), J accumulated
    int any = 0;
    for (int sw = 0; sw < SVJ_INNER_MAX; ++sw) {
        for (int step = 0; step < PB - 1; ++step) {
            if (tid < SB) {
                int a, b;
                rr_pair(PB, step, tid, a, b);
                const int p = a < b ? a : b, q = a < b ? b : a;
                const double app = H[p + LDP * p], aqq = H[q + LDP * q], apq = H[p + LDP * q];
                const double prod = app * aqq;
                double c = 1.0, s = 0.0;
                if (apq != 0.0 && prod > 0.0) {
                    const double g = sqrt(prod);
                    if (fabs(apq) > tol * g && g > floor_) {
                        const double tau = (aqq - app) / (2.0 * apq);
                        const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                        c = 1.0 / sqrt(1.0 + t * t);
                        s = t * c;
                        flag = 1;
                    }
                }
                cs[2 * tid] = c; cs[2 * tid + 1] = s;
            }
            __syncthreads();
            // columns of H and of J: (H or J, pair k, row i)
            for (int e = tid; e < 2 * SB * PB; e += 256) {
                const int i = e & (PB - 1), k = (e >> 5) & (SB - 1);
                double* M = e >= SB * PB ? J : H;
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
            // rows of H: (pair k, column j); the annihilated entries are set to zero exactly
            for (int e = tid; e < SB * PB; e += 256) {
                const int j = e & (PB - 1), k = e >> 5;
                const double c = cs[2 * k], s = cs[2 * k + 1];
                if (s != 0.0) {
                    int a, b;
                    rr_pair(PB, step, k, a, b);
                    const int p = a < b ? a : b, q = a < b ? b : a;
                    const double x = H[p + LDP * j], y = H[q + LDP * j];
                    H[p + LDP * j] = j == q ? 0.0 : c * x - s * y;
                    H[q + LDP * j] = j == p ? 0.0 : s * x + c * y;
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
    if (tid == 0) rotated[blockIdx.x] = any;
    if (!any) return;                // (uniform in the workgroup)

    // 3. [G_i G_j] <- [G_i G_j] J,  [V_i V_j] <- [V_i V_j] J
    svj_apply(G, m, ldg, c0, c1, J, Xs);
    svj_apply(V, W, (size_t)W, c0, c1, J, Xs);
}

// ---- control -------------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_svj_sumsq(int rows, int cols, const double* __restrict__ A, size_t ld, double* __restrict__ part) {
    double s = 0.0;
    const size_t tot = (size_t)rows * (size_t)cols;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < tot; idx += (size_t)gridDim.x * blockDim.x) {
        const double x = A[idx % (size_t)rows + (idx / (size_t)rows) * ld];
        s += x * x;
    }
    store_partials(part, s);
}

__global__ __launch_bounds__(256) void k_svj_init(int nparts, const double* __restrict__ part, SvjCtl* ctl) {
    double s[1];
    load_partials(nparts, part, s);
    if (threadIdx.x == 0) {
        const double norm = sqrt(s[0]);
        ctl->norm = norm; ctl->pad0_ = 0.0;
        ctl->sweeps = 0; ctl->done = 0; ctl->pad_ = 0;
        ctl->nonfinite = isfinite(norm) ? 0 : 1;
    }
}

__global__ __launch_bounds__(256) void k_svj_fold(int n, const int* __restrict__ rotated, SvjCtl* ctl) {
    int any = 0;
    for (int i = threadIdx.x; i < n; i += 256) any |= rotated[i];
    any = __syncthreads_or(any);
    if (threadIdx.x == 0) { ctl->sweeps += 1; ctl->done = any ? 0 : 1; }
}

// ---- exit ----------------------------------------------------------------------------------------------------------------------------------
// one workgroup per column: sig[c] = ||G(:, c)||
__global__ __launch_bounds__(256) void k_svj_colnorm(int m, const double* __restrict__ G, size_t ldg, double* __restrict__ sig) {
    __shared__ double red[17];
    const double* g = G + (size_t)blockIdx.x * ldg;
    double s = 0.0;
    for (int i = threadIdx.x; i < m; i += 256) s += g[i] * g[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) sig[blockIdx.x] = sqrt(s);
}

// U(:, j) = G(:, perm[j]) / sig[j] where sig[j] > thr, a zero column otherwise;  Vout(:, j) = V(0 .. w, perm[j])
__global__ __launch_bounds__(256) void k_svj_gather(int m, int w, int k, const double* __restrict__ G, size_t ldg, const double* __restrict__ V, size_t ldv,
                                                    const int* __restrict__ perm, const double* __restrict__ sig, double thr, double* __restrict__ U,
                                                    size_t ldu, double* __restrict__ Vout, size_t ldvo) {
    const size_t h = (size_t)m + (size_t)w, tot = h * (size_t)k;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < tot; idx += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(idx / h), i = (int)(idx % h);
        const size_t src = (size_t)perm[j];
        if (i < m) U[(size_t)i + (size_t)j * ldu] = sig[j] > thr ? G[(size_t)i + src * ldg] / sig[j] : 0.0;
        else Vout[(size_t)(i - m) + (size_t)j * ldvo] = V[(size_t)(i - m) + src * ldv];
    }
}

// the tall case: A is m x w with m >= w >= 1
SvdResult svd_tall(Ctx* ctx, const Mat& A, double tol, SvjStats* stats) {
    const int m = A.rows, w = A.cols;
    const int p = std::max(2, ceil_div(w, SB)), W = p * SB, players = p + (p & 1), nrounds = players - 1, np = p / 2;
    SvdResult out;

    // the schedule: per round the np block pairs (i < j)
    std::vector<int> tab((size_t)nrounds * 2 * np);
    for (int r = 0; r < nrounds; ++r) {
        int* t = tab.data() + (size_t)r * 2 * np;
        int cnt = 0;
        for (int k = 0; k < players / 2; ++k) {
            int a, b;
            rr_pair(players, r, k, a, b);
            if (a >= p || b >= p) continue;          // (the pair of the block that sits out)
            t[2 * cnt] = std::min(a, b); t[2 * cnt + 1] = std::max(a, b); ++cnt;
        }
    }
    DevArr<int> dtab(ctx, tab.size());
    dtab.upload(ctx, tab);

    Mat G(ctx, m, W), V(ctx, W, W);
    if (W != w) fill_mat(ctx, G, 0.0);
    { Mat left = G.view(0, 0, m, w); copy_mat(ctx, A, left); }
    set_identity(ctx, V, 1.0);
    DevArr<double> part(ctx, NORM_PARTS), dsig(ctx, w);
    DevArr<int> rotated(ctx, (size_t)nrounds * np), dperm(ctx, w);
    DevArr<SvjCtl> ctl(ctx, 1);
    {
        TimedScope ts(ctx, "svj_norm", 8.0 * m * w, 0.0, 2);
        hipLaunchKernelGGL(k_svj_sumsq, dim3(NORM_PARTS), dim3(256), 0, ctx->stream, m, w, (const double*)A.p, (size_t)A.ld, part.p);
        hipLaunchKernelGGL(k_svj_init, dim3(1), dim3(256), 0, ctx->stream, NORM_PARTS, (const double*)part.p, ctl.p);
    }
    SvjCtl h = read_back(ctx, ctl.p);
    if (h.nonfinite) throw Error(ERR_INVALID, "svd_jacobi: the matrix has non-finite entries");
    if (!(tol > 0.0)) tol = std::sqrt((double)m) * DBL_EPS;

    long rounds = 0;
    while (!h.done) {
        if (h.sweeps >= SVJ_MAX_SWEEPS) throw Error(ERR_INTERNAL, "svd_jacobi: no convergence in " + std::to_string(h.sweeps) + " sweeps");
        {
            TimedScope ts(ctx, "svj_round", 16.0 * nrounds * ((double)m + W) * W, 2.0 * nrounds * np * (3.0 * m + 2.0 * W) * PB * PB, nrounds);
            for (int r = 0; r < nrounds; ++r)
                hipLaunchKernelGGL(k_svj_round, dim3(np), dim3(256), 0, ctx->stream, m, W, G.p, (size_t)G.ld, V.p, (const int*)(dtab.p + (size_t)r * 2 * np),
                                   (const SvjCtl*)ctl.p, tol, rotated.p + (size_t)r * np);
        }
        rounds += nrounds;
        hipLaunchKernelGGL(k_svj_fold, dim3(1), dim3(256), 0, ctx->stream, nrounds * np, (const int*)rotated.p, ctl.p);
        h = read_back(ctx, ctl.p);
    }
    DRE_HIP(hipGetLastError());

    // sigma = column norms, sorted on the host (stable, descending)
    hipLaunchKernelGGL(k_svj_colnorm, dim3(w), dim3(256), 0, ctx->stream, m, (const double*)G.p, (size_t)G.ld, dsig.p);
    std::vector<double> sig(w);
    DRE_HIP(hipMemcpyAsync(sig.data(), dsig.p, (size_t)w * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    std::vector<int> perm(w);
    std::iota(perm.begin(), perm.end(), 0);
    std::stable_sort(perm.begin(), perm.end(), [&](int a, int b) { return sig[a] > sig[b]; });
    out.s.resize(w);
    for (int j = 0; j < w; ++j) out.s[j] = sig[perm[j]];
    const double thr = tol * h.norm;
    long rank = 0;
    for (int j = 0; j < w; ++j) rank += out.s[j] > thr ? 1 : 0;
    dperm.upload(ctx, perm);
    out.S = Mat(ctx, w, 1);
    DRE_HIP(hipMemcpyAsync(out.S.p, out.s.data(), (size_t)w * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    ctx->sync();
    out.U = Mat(ctx, m, w);
    out.V = Mat(ctx, w, w);
    hipLaunchKernelGGL(k_svj_gather, dim3(grid_for(((size_t)m + w) * w)), dim3(256), 0, ctx->stream, m, w, w, (const double*)G.p, (size_t)G.ld,
                       (const double*)V.p, (size_t)V.ld, (const int*)dperm.p, (const double*)out.S.p, thr, out.U.p, (size_t)out.U.ld, out.V.p,
                       (size_t)out.V.ld);
    DRE_HIP(hipGetLastError());
    ctx->sync();
    out.norm = h.norm;
    if (env_trace("compress")) std::fprintf(stderr, "[svd_jacobi] %d x %d: %d sweeps, %ld rounds, rank %ld\n", m, w, h.sweeps, rounds, rank);
    if (stats) { stats->sweeps = h.sweeps; stats->rounds = rounds; stats->rank = rank; }
    return out;
}

}  // namespace

SvdResult svd_jacobi(Ctx* ctx, const Mat& A, double tol, SvjStats* stats) {
    if (stats) *stats = SvjStats{};
    const int m = std::max(A.rows, A.cols), w = std::min(A.rows, A.cols);
    DRE_REQUIRE(A.rows >= 0 && A.cols >= 0, "svd_jacobi: negative shape");
    DRE_REQUIRE(w <= SVJ_MAX_W, "svd_jacobi: the shorter dimension is limited to 4096");
    DRE_REQUIRE(m <= DENSE_MAX_N, "svd_jacobi: the longer dimension is beyond the device's 32-bit index limit");
    DRE_REQUIRE(std::isfinite(tol), "svd_jacobi: tol is not finite");
    if (w == 0) {
        SvdResult out;
        out.U = Mat(ctx, A.rows, 0); out.S = Mat(ctx, 0, 1); out.V = Mat(ctx, A.cols, 0);
        return out;
    }
    const size_t W = (size_t)std::max(2, ceil_div(w, SB)) * SB;
    // G, V, the outputs U and V, the transposed copy of a wide input, partial sums and the small arrays
    require_memory(ctx, (size_t)m * W + W * W + 2 * (size_t)m * w + (size_t)w * w + NORM_PARTS + 4 * W + (W / SB) * (W / SB));
    if (A.rows >= A.cols) return svd_tall(ctx, A, tol, stats);
    Mat At(ctx, A.cols, A.rows);
    transpose_mat(ctx, A, At);
    SvdResult out = svd_tall(ctx, At, tol, stats);
    std::swap(out.U, out.V);
    return out;
}

}  // namespace dre
