// What the block Jacobi eigensolver (sym_jacobi.hip) and the block Jacobi SVD (svd_jacobi.hip) share: the block sizes, the round-robin
// tournament and its schedule table, the cyclic Jacobi iteration on a 32 x 32 block in LDS, and the member bookkeeping of their drivers.
// Internal to those two files.  See DESIGN.md §9.6, §9.8 and §9.9.
//
// Every kernel of the two files takes the member b on blockIdx.y (blockIdx.x where it runs one workgroup per member), size_t member strides and
// one control block per member, and the kernels of a sweep return before their first global write for a member that is done, non-finite or
// out of sweeps.  A single call is a batch of one.
#pragma once
#include <algorithm>
#include <string>
#include <vector>

#include "dense_device.hpp"
#include "jacobi_batch.hpp"

namespace dre {

namespace {

constexpr int SB = BJ_BLOCK;          // block: 16 rows and columns of the eigensolver, 16 columns of the SVD
constexpr int PB = 2 * SB;            // order of a pivot block / of the Gram matrix of a block pair
constexpr int LDP = PB + 1;           // leading dimension of a 32 x 32 block in LDS (odd: rows and columns both walk over all banks)
constexpr int INNER_MAX = 10;         // cyclic sweeps of a 32 x 32 block at most (ended by the first sweep without a rotation)

// pair k (0 <= k < players / 2) of round `step` (0 <= step < players - 1) of the round-robin tournament of an even number of players
__host__ __device__ inline void rr_pair(int players, int step, int k, int& a, int& b) {
    const int m = players - 1;
    if (k == 0) { a = m; b = step; }
    else { a = (step + k) % m; b = (step - k + m) % m; }
}

// The schedule of a sweep over p blocks, one table for all members: p - 1 (p even) or p (p odd: one block sits out per round) rounds, per round
// the p / 2 block pairs (i < j) and, with_sit, the block that sits out (-1: none) behind them.
inline std::vector<int> rr_schedule(int p, bool with_sit) {
    const int players = p + (p & 1), nrounds = players - 1, np = p / 2, per_round = 2 * np + (with_sit ? 1 : 0);
    std::vector<int> tab((size_t)nrounds * per_round);
    for (int r = 0; r < nrounds; ++r) {
        int* t = tab.data() + (size_t)r * per_round;
        int cnt = 0, sit = -1;
        for (int k = 0; k < players / 2; ++k) {
            int a, b;
            rr_pair(players, r, k, a, b);
            if (a >= p) sit = b;
            else if (b >= p) sit = a;
            else { t[2 * cnt] = std::min(a, b); t[2 * cnt + 1] = std::max(a, b); ++cnt; }
        }
        if (with_sit) t[2 * np] = sit;
    }
    return tab;
}

// Cyclic Jacobi on the symmetric 32 x 32 block G in LDS (leading dimension LDP) with the rotations accumulated in J: sweeps of 31 steps of 16
// disjoint rotations in round-robin order, until a sweep rotates nothing or max_sweeps are done.  rotate(g_pp, g_qq, g_pq) says whether the pair
// (p, q) is rotated; a skipped rotation is the exact identity.  For all 256 threads of the workgroup, with G, J and *flag = 0 written and a
// barrier behind them; cs (2 SB doubles) and flag are in LDS.  Returns, uniform in the workgroup, whether anything was rotated.
template <class Rotate>
__device__ __forceinline__ int cyclic_jacobi_32(double* G, double* J, double* cs, int* flag, int max_sweeps, Rotate rotate) {
    const int tid = threadIdx.x;
    int any = 0;
    for (int sw = 0; sw < max_sweeps; ++sw) {
        for (int step = 0; step < PB - 1; ++step) {
            if (tid < SB) {
                int a, b;
                rr_pair(PB, step, tid, a, b);
                const int p = a < b ? a : b, q = a < b ? b : a;
                const double app = G[p + LDP * p], aqq = G[q + LDP * q], apq = G[p + LDP * q];
                double c = 1.0, s = 0.0;
                if (rotate(app, aqq, apq)) {
                    const double tau = (aqq - app) / (2.0 * apq);
                    const double t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                    c = 1.0 / sqrt(1.0 + t * t);
                    s = t * c;
                    *flag = 1;
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
        const int f = *flag;          // (uniform: every write of this sweep is behind a barrier)
        __syncthreads();
        if (tid == 0) *flag = 0;
        __syncthreads();
        if (!f) break;
        any = 1;
    }
    return any;
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

// the control blocks of all members in one copy (synchronising)
template <class Ctl>
void fetch_ctl(Ctx* ctx, const DevArr<Ctl>& d, std::vector<Ctl>& h) {
    DRE_HIP(hipMemcpyAsync(h.data(), d.p, h.size() * sizeof(Ctl), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
}

// A driver records only the "what" of a member's failure; its callers put "who: " (a single call) or "who, member b: " in front.
inline std::string member_msg(const char* who, int b, const std::string& what) { return std::string(who) + ", member " + std::to_string(b) + ": " + what; }
inline void name_members(std::vector<BatchMemberStatus>& status, const char* who) {
    for (size_t b = 0; b < status.size(); ++b)
        if (status[b].code) status[b].msg = member_msg(who, (int)b, status[b].msg);
}

inline void check_batch(const std::vector<Mat>& A, const char* who) {
    DRE_REQUIRE(!A.empty() && A.size() <= (size_t)JACOBI_BATCH_MAX, std::string(who) + ": batch must be in 1 .. 65535");
    for (size_t b = 0; b < A.size(); ++b)
        DRE_REQUIRE(A[b].rows == A[0].rows && A[b].cols == A[0].cols,
                    std::string(who) + ": member " + std::to_string(b) + " is " + std::to_string(A[b].rows) + " x " + std::to_string(A[b].cols) + ", member 0 is " +
                        std::to_string(A[0].rows) + " x " + std::to_string(A[0].cols) + ": the members of a batch share one shape");
}

}  // namespace

}  // namespace dre
