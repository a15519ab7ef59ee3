// Member-indexed block Jacobi: the two iterations of sym_jacobi.hip and svd_jacobi.hip with member b = blockIdx.y on every
// launch.  The kernels are those files' kernels with a member offset on every pointer and a return at entry for a member that is finished or
// dropped; the arithmetic of a workgroup on its member, and its order, are the single solvers', so a member's outputs are bitwise the single
// call's.  Every member has its own control block, `rotated` flags, partial sums and (eigensolver) J buffer; nothing is summed across members and
// there are no atomics, so a member's result does not depend on the others.  ctl[b] is written by the one-workgroup-per-member kernels only;
// kernel boundaries on the context's stream are the only ordering.  The host reads the B control blocks in one copy per sweep.
//
// Index arithmetic: block, row and column indices are ints below DENSE_MAX_N; every element offset and every member stride is a size_t.
#include "jacobi_batch.hpp"

#include <algorithm>
#include <cmath>
#include <numeric>

#include "dense_device.hpp"
#include "dense_gj.hpp"
#include "profiling.hpp"

namespace dre {

namespace {

constexpr int SB = 16;                // block (BJ_BLOCK of the eigensolver, the column block of the SVD)
constexpr int PB = 2 * SB;            // order of a pivot block / a Gram block
constexpr int LDP = PB + 1;           // leading dimension of a 32 x 32 block in LDS (odd: rows and columns both walk over all banks)
constexpr int LDX = SVJ_SLAB + 1;     // leading dimension of a 64 x 32 row slab in LDS
constexpr int SVJ_INNER_MAX = 10;     // cyclic sweeps of a Gram block at most (svd_jacobi.hip)
static_assert(SB == BJ_BLOCK, "one block size for both iterations");

// pair k (0 <= k < players / 2) of round `step` (0 <= step < players - 1) of the round-robin tournament of an even number of players
// (the tournament of sym_jacobi.hip)
__host__ __device__ inline void rr_pair(int players, int step, int k, int& a, int& b) {
    const int m = players - 1;
    if (k == 0) { a = m; b = step; }
    else { a = (step + k) % m; b = (step - k + m) % m; }
}

template <class Ctl>
__device__ inline bool member_off(const Ctl& c) { return c.done | c.nonfinite | c.failed; }

// M_b = I for every member of a stack of n x n matrices
__global__ __launch_bounds__(256) void k_jb_eye(int n, double* __restrict__ M, size_t stride) {
    double* Mb = M + (size_t)blockIdx.y * stride;
    const size_t tot = (size_t)n * (size_t)n;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < tot; idx += (size_t)gridDim.x * blockDim.x)
        Mb[idx] = idx % (size_t)n == idx / (size_t)n ? 1.0 : 0.0;
}

// =================================================================================================================================================
// Symmetric eigensolver (k_bj_* of sym_jacobi.hip)
// =================================================================================================================================================
// grid (m pairs, B); Jbuf and rotated: m slices per member
__global__ __launch_bounds__(256) void k_bjb_pivot(int Q, const double* __restrict__ As, size_t stride, const int* __restrict__ pairs,
                                                   const BjbCtl* __restrict__ ctls, double tol, double* __restrict__ Jbufs, int* __restrict__ rotateds) {
    __shared__ double G[PB * LDP], J[PB * LDP], cs[2 * SB];
    __shared__ int flag;
    const BjbCtl* ctl = ctls + blockIdx.y;
    if (member_off(*ctl)) return;          // (uniform in the workgroup)
    const double* A = As + (size_t)blockIdx.y * stride;
    double* Jbuf = Jbufs + (size_t)blockIdx.y * (size_t)gridDim.x * (PB * PB);
    int* rotated = rotateds + (size_t)blockIdx.y * gridDim.x;
    const int tid = threadIdx.x;
    const int bi = pairs[2 * blockIdx.x], bj = pairs[2 * blockIdx.x + 1];
    const double thr = tol / (double)Q * ctl->norm;
    for (int e = tid; e < PB * PB; e += 256) {
        const int i = e & (PB - 1), j = e >> 5;
        const int gi = (i < SB ? bi : bj) * SB + (i & (SB - 1)), gj = (j < SB ? bi : bj) * SB + (j & (SB - 1));
        G[i + LDP * j] = A[(size_t)gi + (size_t)gj * (size_t)Q];
        J[i + LDP * j] = i == j ? 1.0 : 0.0;
    }
    if (tid == 0) flag = 0;
    __syncthreads();
    int any = 0;
    for (int sw = 0; sw < BJ_INNER_MAX; ++sw) {
        for (int step = 0; step < PB - 1; ++step) {
            if (tid < SB) {
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
            for (int e = tid; e < 2 * SB * PB; e += 256) {
                const int i = e & (PB - 1), k = (e >> 5) & (SB - 1);
                double* M = e >= SB * PB ? J : G;
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
            for (int e = tid; e < SB * PB; e += 256) {
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

// grid (super-blocks of k_bj_update, B)
__global__ __launch_bounds__(256) void k_bjb_update(int Q, int p, int m, int sit, const int* __restrict__ pairs, const double* __restrict__ Jbufs,
                                                    const int* __restrict__ rotateds, double* __restrict__ As, double* __restrict__ Vs, size_t stride,
                                                    const BjbCtl* __restrict__ ctls) {
    __shared__ double Xs[PB * LDP], Ts[PB * LDP], JL[PB * LDP], JR[PB * LDP];
    if (member_off(ctls[blockIdx.y])) return;          // (uniform in the workgroup)
    const double* Jbuf = Jbufs + (size_t)blockIdx.y * (size_t)m * (PB * PB);
    const int* rotated = rotateds + (size_t)blockIdx.y * m;
    double* A = As + (size_t)blockIdx.y * stride;
    double* V = Vs + (size_t)blockIdx.y * stride;
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
        if (br >= 0 && bc >= 0) x = M[(size_t)(br * SB + (i & 15)) + (size_t)(bc * SB + (j & 15)) * (size_t)Q];
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
        if (br >= 0 && bc >= 0) M[(size_t)(br * SB + (i & 15)) + (size_t)(bc * SB + (j & 15)) * (size_t)Q] = Xs[i + LDP * j];
    }
}

// grid (NORM_PARTS, B): the partition of k_bj_norms per member, the partial sums of member b in part + 2 NORM_PARTS b
__global__ __launch_bounds__(256) void k_bjb_norms(int Q, const double* __restrict__ As, size_t stride, double* __restrict__ parts,
                                                   const BjbCtl* __restrict__ ctls) {
    if (member_off(ctls[blockIdx.y])) return;          // (uniform in the workgroup)
    const double* A = As + (size_t)blockIdx.y * stride;
    double s_off = 0.0, s_diag = 0.0;
    const size_t tot = (size_t)Q * (size_t)Q;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < tot; idx += (size_t)gridDim.x * blockDim.x) {
        const double x = A[idx];
        if (idx % (size_t)Q == idx / (size_t)Q) s_diag += x * x; else s_off += x * x;
    }
    store_partials(parts + (size_t)blockIdx.y * (2 * gridDim.x), s_off, s_diag);
}

// grid (B): the decision of k_bj_decide per member; a member still rotating after BJ_MAX_SWEEPS sweeps is dropped here
__global__ __launch_bounds__(256) void k_bjb_decide(int nparts, const double* __restrict__ parts, double tol, int count, BjbCtl* ctls) {
    BjbCtl* ctl = ctls + blockIdx.x;
    if (member_off(*ctl)) return;          // (uniform in the workgroup)
    double s[2];
    load_partials(nparts, parts + (size_t)blockIdx.x * (2 * nparts), s);
    if (threadIdx.x == 0) {
        const double off = sqrt(s[0]), norm = sqrt(s[0] + s[1]);
        ctl->off = off; ctl->norm = norm;
        ctl->nonfinite = isfinite(norm) ? 0 : 1;
        ctl->done = isfinite(norm) && off <= tol * norm ? 1 : 0;
        ctl->sweeps += count;
        ctl->failed = isfinite(norm) && !ctl->done && ctl->sweeps >= BJ_MAX_SWEEPS ? 1 : 0;
    }
}

// grid (ceil(q / 256), B): w[b q + i] = A_b(i, i)
__global__ void k_bjb_diag(int q, int Q, const double* __restrict__ As, size_t stride, double* __restrict__ w) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < q) w[(size_t)blockIdx.y * q + i] = As[(size_t)blockIdx.y * stride + (size_t)i + (size_t)i * (size_t)Q];
}

// =================================================================================================================================================
// SVD (k_svj_* of svd_jacobi.hip)
// =================================================================================================================================================
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

// grid (np pairs of the round, B).  Gs: m x W per member (leading dimension ldg, member stride sg), Vs: W x W per member (stride sv);
// rotateds: this round's np flags of member b at rotateds + b * rstride
__global__ __launch_bounds__(256) void k_svjb_round(int m, int W, double* __restrict__ Gs, size_t ldg, size_t sg, double* __restrict__ Vs, size_t sv,
                                                    const int* __restrict__ pairs, const SvjbCtl* __restrict__ ctls, double tol,
                                                    int* __restrict__ rotateds, size_t rstride) {
    __shared__ double Xs[LDX * PB], H[PB * LDP], J[PB * LDP], cs[2 * SB];
    __shared__ int flag;
    const SvjbCtl* ctl = ctls + blockIdx.y;
    if (member_off(*ctl)) return;          // (uniform in the workgroup)
    double* G = Gs + (size_t)blockIdx.y * sg;
    double* V = Vs + (size_t)blockIdx.y * sv;
    int* rotated = rotateds + (size_t)blockIdx.y * rstride;
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

// grid (NORM_PARTS, B): the partition of k_svj_sumsq per member, the partial sums of member b in parts + NORM_PARTS b
__global__ __launch_bounds__(256) void k_svjb_sumsq(int rows, int cols, const double* __restrict__ As, size_t ld, size_t stride, double* __restrict__ parts) {
    const double* A = As + (size_t)blockIdx.y * stride;
    double s = 0.0;
    const size_t tot = (size_t)rows * (size_t)cols;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < tot; idx += (size_t)gridDim.x * blockDim.x) {
        const double x = A[idx % (size_t)rows + (idx / (size_t)rows) * ld];
        s += x * x;
    }
    store_partials(parts + (size_t)blockIdx.y * gridDim.x, s);
}

// grid (B)
__global__ __launch_bounds__(256) void k_svjb_init(int nparts, const double* __restrict__ parts, SvjbCtl* ctls) {
    SvjbCtl* ctl = ctls + blockIdx.x;
    double s[1];
    load_partials(nparts, parts + (size_t)blockIdx.x * nparts, s);
    if (threadIdx.x == 0) {
        const double norm = sqrt(s[0]);
        ctl->norm = norm; ctl->pad0_ = 0.0;
        ctl->sweeps = 0; ctl->done = 0; ctl->failed = 0;
        ctl->nonfinite = isfinite(norm) ? 0 : 1;
    }
}

// grid (B): n flags per member at rotateds + b * n; a member still rotating after SVJ_MAX_SWEEPS sweeps is dropped here
__global__ __launch_bounds__(256) void k_svjb_fold(int n, const int* __restrict__ rotateds, SvjbCtl* ctls) {
    SvjbCtl* ctl = ctls + blockIdx.x;
    if (member_off(*ctl)) return;          // (uniform in the workgroup)
    const int* rotated = rotateds + (size_t)blockIdx.x * n;
    int any = 0;
    for (int i = threadIdx.x; i < n; i += 256) any |= rotated[i];
    any = __syncthreads_or(any);
    if (threadIdx.x == 0) {
        ctl->sweeps += 1; ctl->done = any ? 0 : 1;
        ctl->failed = any && ctl->sweeps >= SVJ_MAX_SWEEPS ? 1 : 0;
    }
}

// grid (w, B): sig[b w + c] = ||G_b(:, c)||
__global__ __launch_bounds__(256) void k_svjb_colnorm(int m, const double* __restrict__ Gs, size_t ldg, size_t sg, double* __restrict__ sig) {
    __shared__ double red[17];
    const double* g = Gs + (size_t)blockIdx.y * sg + (size_t)blockIdx.x * ldg;
    double s = 0.0;
    for (int i = threadIdx.x; i < m; i += 256) s += g[i] * g[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) sig[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = sqrt(s);
}

// grid (., B): k_svj_gather per member; perm and sig are w per member, U m x w, Vout w x w per member (contiguous); thr = tol ||A_b||_F
__global__ __launch_bounds__(256) void k_svjb_gather(int m, int w, const double* __restrict__ Gs, size_t ldg, size_t sg, const double* __restrict__ Vs, size_t ldv,
                                                     size_t sv, const int* __restrict__ perms, const double* __restrict__ sigs, double tol,
                                                     const SvjbCtl* __restrict__ ctls, double* __restrict__ Us, double* __restrict__ Vouts) {
    const SvjbCtl* ctl = ctls + blockIdx.y;
    if (ctl->nonfinite | ctl->failed) return;
    const double thr = tol * ctl->norm;
    const double* G = Gs + (size_t)blockIdx.y * sg;
    const double* V = Vs + (size_t)blockIdx.y * sv;
    const int* perm = perms + (size_t)blockIdx.y * w;
    const double* sig = sigs + (size_t)blockIdx.y * w;
    double* U = Us + (size_t)blockIdx.y * (size_t)m * (size_t)w;
    double* Vout = Vouts + (size_t)blockIdx.y * (size_t)w * (size_t)w;
    const size_t ldu = (size_t)m, ldvo = (size_t)w;
    const size_t h = (size_t)m + (size_t)w, tot = h * (size_t)w;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < tot; idx += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(idx / h), i = (int)(idx % h);
        const size_t src = (size_t)perm[j];
        if (i < m) U[(size_t)i + (size_t)j * ldu] = sig[j] > thr ? G[(size_t)i + src * ldg] / sig[j] : 0.0;
        else Vout[(size_t)(i - m) + (size_t)j * ldvo] = V[(size_t)(i - m) + src * ldv];
    }
}

// a rows x cols view (contiguous columns) at `off` doubles into a stack
Mat stack_view(const DevArr<double>& st, size_t off, int rows, int cols) {
    Mat m;
    m.buf = st.buf; m.p = st.p + off; m.rows = rows; m.cols = cols; m.ld = rows > 0 ? rows : 1;
    return m;
}

template <class Ctl>
void fetch_ctl(Ctx* ctx, const DevArr<Ctl>& d, std::vector<Ctl>& h) {
    DRE_HIP(hipMemcpyAsync(h.data(), d.p, h.size() * sizeof(Ctl), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
}

std::string member_msg(const char* who, int b, const std::string& what) { return std::string(who) + ", member " + std::to_string(b) + ": " + what; }

void check_batch(const std::vector<Mat>& A, const char* who) {
    DRE_REQUIRE(!A.empty() && A.size() <= (size_t)JACOBI_BATCH_MAX, std::string(who) + ": batch must be in 1 .. 65535");
    for (size_t b = 0; b < A.size(); ++b)
        DRE_REQUIRE(A[b].rows == A[0].rows && A[b].cols == A[0].cols,
                    std::string(who) + ": member " + std::to_string(b) + " is " + std::to_string(A[b].rows) + " x " + std::to_string(A[b].cols) + ", member 0 is " +
                        std::to_string(A[0].rows) + " x " + std::to_string(A[0].cols) + ": the members of a batch share one shape");
}

}  // namespace

// =================================================================================================================================================
SymEigBatch sym_eig_jacobi_batch(Ctx* ctx, const std::vector<Mat>& S, double tol, const char* who) {
    check_batch(S, who);
    const int B = (int)S.size(), q = S[0].rows;
    DRE_REQUIRE(S[0].rows == S[0].cols, std::string(who) + ": square matrices expected");
    DRE_REQUIRE(q <= DENSE_MAX_N - 2 * BJ_BLOCK, std::string(who) + ": order beyond the device's 32-bit index limit");
    DRE_REQUIRE(std::isfinite(tol), std::string(who) + ": tol is not finite");
    SymEigBatch out;
    out.eig.resize((size_t)B); out.stats.resize((size_t)B); out.status.resize((size_t)B);
    for (auto& e : out.eig) e.q = q;
    if (q == 0) return out;
    if (!(tol > 0.0)) tol = q * DBL_EPS;
    const int Q = bj_padded_order(q), p = Q / BJ_BLOCK, players = p + (p & 1), nrounds = players - 1, m = p / 2;
    const size_t QQ = (size_t)Q * Q;
    // per member: A, V, the result's Z, the J buffer, the partial sums, the eigenvalues
    require_memory(ctx, (size_t)B * (2 * QQ + (size_t)q * q + (size_t)m * PB * PB + 2 * NORM_PARTS + q));

    // the schedule: per round the m block pairs (i < j), then the block that sits out (one table for all members)
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

    DevArr<double> A(ctx, (size_t)B * QQ), V(ctx, (size_t)B * QQ), Jbuf(ctx, (size_t)B * m * PB * PB), part(ctx, (size_t)B * 2 * NORM_PARTS);
    DevArr<int> rotated(ctx, (size_t)B * m);
    DevArr<BjbCtl> ctl(ctx, (size_t)B);
    if (Q != q) DRE_HIP(hipMemsetAsync(A.p, 0, (size_t)B * QQ * sizeof(double), ctx->stream));
    {
        std::vector<CopyDesc> cp((size_t)B);
        for (int b = 0; b < B; ++b) cp[(size_t)b] = CopyDesc{S[(size_t)b].p, A.p + (size_t)b * QQ, q, q, S[(size_t)b].ld, Q};
        copy_batched(ctx, cp);
    }
    hipLaunchKernelGGL(k_jb_eye, dim3(grid_for(QQ), B), dim3(256), 0, ctx->stream, Q, V.p, QQ);
    DRE_HIP(hipMemsetAsync(ctl.p, 0, sizeof(BjbCtl) * (size_t)B, ctx->stream));

    std::vector<BjbCtl> h((size_t)B);
    auto measure = [&](int count) {
        TimedScope ts(ctx, "bjb_norm", 8.0 * B * Q * Q, 0.0, 2);
        hipLaunchKernelGGL(k_bjb_norms, dim3(NORM_PARTS, B), dim3(256), 0, ctx->stream, Q, (const double*)A.p, QQ, part.p, (const BjbCtl*)ctl.p);
        hipLaunchKernelGGL(k_bjb_decide, dim3(B), dim3(256), 0, ctx->stream, NORM_PARTS, (const double*)part.p, tol, count, ctl.p);
        fetch_ctl(ctx, ctl, h);
    };
    auto off = [&](int b) { return h[(size_t)b].done || out.status[(size_t)b].code != 0; };
    // the outcomes of the last measurement: a dropped member's code and message
    auto judge = [&](bool entry) {
        bool live = false;
        for (int b = 0; b < B; ++b) {
            if (off(b)) continue;
            const BjbCtl& c = h[(size_t)b];
            if (c.nonfinite)
                out.status[(size_t)b] = {ERR_INVALID, member_msg(who, b, entry ? "the matrix has non-finite entries" : "non-finite values in sweep " + std::to_string(c.sweeps))};
            else if (c.failed)
                out.status[(size_t)b] = {ERR_INTERNAL, member_msg(who, b, "no convergence in " + std::to_string(c.sweeps) + " sweeps (off / norm = " + std::to_string(c.off / c.norm) + ")")};
            else live = true;
        }
        return live;
    };
    measure(0);
    bool live = judge(true);
    const unsigned vjobs = (unsigned)((p + 1) / 2) * (unsigned)m;
    while (live) {
        for (int r = 0; r < nrounds; ++r) {
            const int* t = dtab.p + (size_t)r * (2 * m + 1);
            const int sit = tab[(size_t)r * (2 * m + 1) + 2 * m];
            {
                TimedScope ts(ctx, "bjb_pivot", 16.0 * B * m * PB * PB, 0.0);
                hipLaunchKernelGGL(k_bjb_pivot, dim3(m, B), dim3(256), 0, ctx->stream, Q, (const double*)A.p, QQ, t, (const BjbCtl*)ctl.p, tol, Jbuf.p, rotated.p);
            }
            {
                const unsigned grid = (unsigned)m * (unsigned)m + (sit >= 0 ? 2u * (unsigned)m : 0u) + vjobs;
                TimedScope ts(ctx, "bjb_update", 32.0 * B * Q * Q, 8.0 * PB * (double)B * Q * Q * 1.5);
                hipLaunchKernelGGL(k_bjb_update, dim3(grid, B), dim3(256), 0, ctx->stream, Q, p, m, sit, t, (const double*)Jbuf.p, (const int*)rotated.p, A.p, V.p,
                                   QQ, (const BjbCtl*)ctl.p);
            }
        }
        measure(1);
        live = judge(false);
    }
    DRE_HIP(hipGetLastError());

    DevArr<double> dw(ctx, (size_t)B * q);
    hipLaunchKernelGGL(k_bjb_diag, dim3(ceil_div(q, 256), B), dim3(256), 0, ctx->stream, q, Q, (const double*)A.p, QQ, dw.p);
    std::vector<double> w((size_t)B * q);
    DRE_HIP(hipMemcpyAsync(w.data(), dw.p, w.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    std::vector<CopyDesc> cp;
    for (int b = 0; b < B; ++b) {
        if (out.status[(size_t)b].code) continue;
        SymEig& e = out.eig[(size_t)b];
        e.j = q; e.nref = 0; e.snorm = h[(size_t)b].norm;
        e.Z = Mat(ctx, q, q);
        cp.push_back(CopyDesc{V.p + (size_t)b * QQ, e.Z.p, q, q, Q, e.Z.ld});
        out.stats[(size_t)b].sweeps = h[(size_t)b].sweeps;
        out.stats[(size_t)b].rounds = (long)nrounds * h[(size_t)b].sweeps;
    }
    copy_batched(ctx, cp);
    ctx->sync();
    for (int b = 0; b < B; ++b)
        if (!out.status[(size_t)b].code) out.eig[(size_t)b].w.assign(w.begin() + (size_t)b * q, w.begin() + (size_t)(b + 1) * q);
    if (env_trace("compress")) {
        for (int b = 0; b < B; ++b)
            std::fprintf(stderr, "[sym_eig_jacobi_batch] member %d, q=%d: %d sweeps, status %d\n", b, q, h[(size_t)b].sweeps, out.status[(size_t)b].code);
    }
    return out;
}

// =================================================================================================================================================
SvdBatch svd_jacobi_batch(Ctx* ctx, const std::vector<Mat>& A, double tol, const char* who) {
    check_batch(A, who);
    const int B = (int)A.size(), rows = A[0].rows, cols = A[0].cols;
    const int m = std::max(rows, cols), w = std::min(rows, cols);
    const bool wide = rows < cols;
    DRE_REQUIRE(rows >= 0 && cols >= 0, std::string(who) + ": negative shape");
    DRE_REQUIRE(w <= SVJ_MAX_W, std::string(who) + ": the shorter dimension is limited to 4096");
    DRE_REQUIRE(m <= DENSE_MAX_N, std::string(who) + ": the longer dimension is beyond the device's 32-bit index limit");
    DRE_REQUIRE(std::isfinite(tol), std::string(who) + ": tol is not finite");
    SvdBatch out;
    out.svd.resize((size_t)B); out.stats.resize((size_t)B); out.status.resize((size_t)B);
    if (w == 0) {
        for (auto& r : out.svd) { r.U = Mat(ctx, rows, 0); r.S = Mat(ctx, 0, 1); r.V = Mat(ctx, cols, 0); }
        return out;
    }
    const int p = std::max(2, ceil_div(w, SB)), W = p * SB, players = p + (p & 1), nrounds = players - 1, np = p / 2;
    const size_t sg = (size_t)m * W, sv = (size_t)W * W, ldg = (size_t)m, nrot = (size_t)nrounds * np;
    // B times the single call's count (G, V, the outputs, partial sums and the small arrays)
    require_memory(ctx, (size_t)B * (sg + sv + 2 * (size_t)m * w + (size_t)w * w + NORM_PARTS + 4 * (size_t)W + (size_t)(W / SB) * (W / SB)));

    // the schedule: per round the np block pairs (i < j), one table for all members
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

    // G_b = [A_b 0] (m x W; a wide member is transposed on the way in), V_b = I
    DevArr<double> G(ctx, (size_t)B * sg), V(ctx, (size_t)B * sv), part(ctx, (size_t)B * NORM_PARTS), dsig(ctx, (size_t)B * w);
    DevArr<int> rotated(ctx, (size_t)B * nrot), dperm(ctx, (size_t)B * w);
    DevArr<SvjbCtl> ctl(ctx, (size_t)B);
    if (W != w) DRE_HIP(hipMemsetAsync(G.p, 0, (size_t)B * sg * sizeof(double), ctx->stream));
    if (wide) {
        for (int b = 0; b < B; ++b) { Mat left = stack_view(G, (size_t)b * sg, m, w); transpose_mat(ctx, A[(size_t)b], left); }
    } else {
        std::vector<CopyDesc> cp((size_t)B);
        for (int b = 0; b < B; ++b) cp[(size_t)b] = CopyDesc{A[(size_t)b].p, G.p + (size_t)b * sg, m, w, A[(size_t)b].ld, m};
        copy_batched(ctx, cp);
    }
    hipLaunchKernelGGL(k_jb_eye, dim3(grid_for(sv), B), dim3(256), 0, ctx->stream, W, V.p, sv);
    {
        TimedScope ts(ctx, "svjb_norm", 8.0 * B * m * w, 0.0, 2);
        hipLaunchKernelGGL(k_svjb_sumsq, dim3(NORM_PARTS, B), dim3(256), 0, ctx->stream, m, w, (const double*)G.p, ldg, sg, part.p);
        hipLaunchKernelGGL(k_svjb_init, dim3(B), dim3(256), 0, ctx->stream, NORM_PARTS, (const double*)part.p, ctl.p);
    }
    std::vector<SvjbCtl> h((size_t)B);
    fetch_ctl(ctx, ctl, h);
    if (!(tol > 0.0)) tol = std::sqrt((double)m) * DBL_EPS;
    auto judge = [&] {
        bool live = false;
        for (int b = 0; b < B; ++b) {
            if (h[(size_t)b].done || out.status[(size_t)b].code) continue;
            if (h[(size_t)b].nonfinite) out.status[(size_t)b] = {ERR_INVALID, member_msg(who, b, "the matrix has non-finite entries")};
            else if (h[(size_t)b].failed) out.status[(size_t)b] = {ERR_INTERNAL, member_msg(who, b, "no convergence in " + std::to_string(h[(size_t)b].sweeps) + " sweeps")};
            else live = true;
        }
        return live;
    };
    bool live = judge();
    while (live) {
        {
            TimedScope ts(ctx, "svjb_round", 16.0 * B * nrounds * ((double)m + W) * W, 2.0 * B * nrounds * np * (3.0 * m + 2.0 * W) * PB * PB, nrounds);
            for (int r = 0; r < nrounds; ++r)
                hipLaunchKernelGGL(k_svjb_round, dim3(np, B), dim3(256), 0, ctx->stream, m, W, G.p, ldg, sg, V.p, sv, (const int*)(dtab.p + (size_t)r * 2 * np),
                                   (const SvjbCtl*)ctl.p, tol, rotated.p + (size_t)r * np, nrot);
        }
        hipLaunchKernelGGL(k_svjb_fold, dim3(B), dim3(256), 0, ctx->stream, (int)nrot, (const int*)rotated.p, ctl.p);
        fetch_ctl(ctx, ctl, h);
        live = judge();
    }
    DRE_HIP(hipGetLastError());

    // sigma = column norms of every member in one copy, sorted per member on the host (stable, descending); the permutations in one upload
    hipLaunchKernelGGL(k_svjb_colnorm, dim3(w, B), dim3(256), 0, ctx->stream, m, (const double*)G.p, ldg, sg, dsig.p);
    std::vector<double> sig((size_t)B * w), ssort((size_t)B * w);
    DRE_HIP(hipMemcpyAsync(sig.data(), dsig.p, sig.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    std::vector<int> perm((size_t)B * w);
    for (int b = 0; b < B; ++b) {
        int* pb = perm.data() + (size_t)b * w;
        const double* sb = sig.data() + (size_t)b * w;
        std::iota(pb, pb + w, 0);
        if (out.status[(size_t)b].code) continue;          // (a dropped member's columns are not looked at)
        std::stable_sort(pb, pb + w, [&](int a, int c) { return sb[a] > sb[c]; });
        SvdResult& r = out.svd[(size_t)b];
        r.s.resize((size_t)w);
        for (int j = 0; j < w; ++j) r.s[(size_t)j] = ssort[(size_t)b * w + j] = sb[pb[j]];
        const double thr = tol * h[(size_t)b].norm;
        long rank = 0;
        for (int j = 0; j < w; ++j) rank += r.s[(size_t)j] > thr ? 1 : 0;
        r.norm = h[(size_t)b].norm;
        out.stats[(size_t)b].sweeps = h[(size_t)b].sweeps;
        out.stats[(size_t)b].rounds = (long)nrounds * h[(size_t)b].sweeps;
        out.stats[(size_t)b].rank = rank;
    }
    dperm.upload(ctx, perm);
    DevArr<double> Ss(ctx, (size_t)B * w), Us(ctx, (size_t)B * m * w), Vo(ctx, (size_t)B * w * w);
    Ss.upload(ctx, ssort);
    hipLaunchKernelGGL(k_svjb_gather, dim3(grid_for(((size_t)m + w) * w), B), dim3(256), 0, ctx->stream, m, w, (const double*)G.p, ldg, sg, (const double*)V.p,
                       (size_t)W, sv, (const int*)dperm.p, (const double*)Ss.p, tol, (const SvjbCtl*)ctl.p, Us.p, Vo.p);
    DRE_HIP(hipGetLastError());
    ctx->sync();
    for (int b = 0; b < B; ++b) {
        if (out.status[(size_t)b].code) continue;
        SvdResult& r = out.svd[(size_t)b];
        r.S = stack_view(Ss, (size_t)b * w, w, 1);
        r.U = stack_view(Us, (size_t)b * m * w, m, w);
        r.V = stack_view(Vo, (size_t)b * w * w, w, w);
        if (wide) std::swap(r.U, r.V);
        if (env_trace("compress"))
            std::fprintf(stderr, "[svd_jacobi_batch] member %d, %d x %d: %ld sweeps, rank %ld\n", b, rows, cols, out.stats[(size_t)b].sweeps, out.stats[(size_t)b].rank);
    }
    return out;
}

}  // namespace dre
