// Dense path (GDREProblem{<:Matrix}, src/riccati/dense_ros{1,2,3,4}.jl of the reference):
//   gj_invert        in-place blocked Gauss-Jordan inversion with row pivoting: a register-resident panel kernel (pivot search, row
//                    interchanges, elimination inside the panel, log|det|; n <= 4096) or the multi-workgroup tournament panel (any n),
//                    and rank-nb updates on the MFMA GEMM;
//   SignLyap         generalized matrix-sign-function solver of F'XE + E'XF = -R (Benner & Quintana-Orti 1999) with the
//                    (P_k, c_k) sequence kept for further right-hand sides and for iterative refinement by replay;
//   dense_gdre_solve the Rosenbrock drivers Ros1..Ros4, device resident.
// The host model of exactly this iteration is tests/_sign_model.py, of the tournament panel tests/_tslu_model.py.
#include "dense_sign.hpp"

#include <algorithm>
#include <cmath>

#include "dense.hpp"
#include "dense_device.hpp"
#include "profiling.hpp"

namespace dre {

static constexpr int GJ_THREADS = 512;
// the tournament panel's width: 64 columns do not fit the selection round's registers at one row per thread (604 bytes of scratch), so the
// trailing update runs at K = 32 as the register panel's does for n <= 1536
static constexpr int GJ_TSLU_NB = 32;
static constexpr int SIGN_PARTS = 256;           // workgroups of the fused element-wise + partial-norm kernels
static constexpr double SCALE_OFF = 1e-2;        // tests/_sign_model.py: SCALE_OFF, STAG_STEP, STAG_DIST
static constexpr double STAG_STEP = 1e-8;
static constexpr double STAG_DIST = 1e-4;

// ---- Gauss-Jordan inversion ------------------------------------------------------------------------------------------------------
// Panel kernel: columns k .. k+kb-1 of A, all n rows, in registers (thread t owns rows t, t + 512, ...).  Step jj: pivot search over rows
// >= j = k + jj, interchange of rows j and p (through LDS), scaling of the pivot row, elimination of column j from every other row.  On exit
// the panel columns hold the columns of the accumulated transform M, and Pn (n x kb) = M - I on the panel's rows: the trailing update of
// every other column c is A(:, c) += Pn W(:, c) with W = A(k:k+kb, :) after the interchanges.
template <int NB, int R>
__global__ __launch_bounds__(GJ_THREADS) void k_gj_panel(int n, int k, int kb, double* __restrict__ A, int lda, double* __restrict__ Pn,
                                                         int* __restrict__ piv, SignCtl* ctl) {
    if (ctl->singular) return;
    __shared__ double prow[2][NB], jrow[2][NB];
    __shared__ double redv[GJ_THREADS / 64];
    __shared__ int redi[GJ_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double a[R][NB];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = tid + r * GJ_THREADS;
#pragma unroll
        for (int c = 0; c < NB; ++c) a[r][c] = (i < n && c < kb) ? A[i + (size_t)(k + c) * lda] : 0.0;
    }
    double ldacc = 0.0;
    // fully unrolled, so that a[r][jj] has a compile-time column index and the panel stays in registers: the tail panel (kb < NB) is
    // handled by predicating the body on the uniform jj < kb, not by leaving the loop (a loop exit keeps it rolled and moves a[][] to scratch)
#pragma clang loop unroll(full)
    for (int jj = 0; jj < NB; ++jj) {
        if (jj < kb) {
        const int j = k + jj, buf = jj & 1;
        double best = -1.0;
        int bi = n;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = tid + r * GJ_THREADS;
            const double v = fabs(a[r][jj]);
            if (i >= j && i < n && v > best) { best = v; bi = i; }      // (rows ascend with r: ties keep the smaller index; NaN never wins)
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(best, off);
            const int oi = __shfl_xor(bi, off);
            if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
        }
        if (lane == 0) { redv[wave] = best; redi[wave] = bi; }
        __syncthreads();
        best = redv[0]; bi = redi[0];
#pragma unroll
        for (int w = 1; w < GJ_THREADS / 64; ++w)
            if (redv[w] > best || (redv[w] == best && redi[w] < bi)) { best = redv[w]; bi = redi[w]; }
        const int p = bi;
        if (!(best > 0.0) || p >= n || !isfinite(best)) {        // an exactly zero (or non-finite) pivot column
            if (tid == 0) ctl->singular = 1;
            return;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = tid + r * GJ_THREADS;
            if (i == p) {
#pragma unroll
                for (int c = 0; c < NB; ++c) prow[buf][c] = a[r][c];
            }
            if (i == j) {
#pragma unroll
                for (int c = 0; c < NB; ++c) jrow[buf][c] = a[r][c];
            }
        }
        __syncthreads();
        const double dinv = 1.0 / prow[buf][jj];
        if (tid == 0) { ldacc += log(fabs(prow[buf][jj])); piv[j] = p; }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = tid + r * GJ_THREADS;
            if (i >= n) continue;
            if (i == p && p != j) {
#pragma unroll
                for (int c = 0; c < NB; ++c) a[r][c] = jrow[buf][c];
            }
            if (i == j) {
#pragma unroll
                for (int c = 0; c < NB; ++c) a[r][c] = (c == jj) ? dinv : prow[buf][c] * dinv;
            } else {
                const double f = a[r][jj];
#pragma unroll
                for (int c = 0; c < NB; ++c) a[r][c] = (c == jj) ? -f * dinv : a[r][c] - f * (prow[buf][c] * dinv);
            }
        }
        }
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = tid + r * GJ_THREADS;
        if (i >= n) continue;
#pragma unroll
        for (int c = 0; c < NB; ++c) {
            if (c < kb) {
                A[i + (size_t)(k + c) * lda] = a[r][c];
                Pn[i + (size_t)c * n] = a[r][c] - (i == k + c ? 1.0 : 0.0);
            }
        }
    }
    if (tid == 0) ctl->logdet += ldacc;
}

// Tournament panel, one selection round (TSLU / CALU pivoting, Grigori, Demmel & Xiang 2011): the steps of k_gj_panel on a set of candidate
// rows.  Workgroup g takes the entries [g 512R, (g + 1) 512R) of a list of candidate rows (rows k .. n-1 when cand_in is null) with the local
// position jj as the diagonal of step jj.  A round of several workgroups writes each one's kb pivot rows (original indices, in pivot order) to
// cand_out and leaves A alone; a workgroup whose column has no usable pivot keeps the row in place and goes on (the final round decides).
// The final round (one workgroup) sets ctl->singular on an exactly zero or non-finite pivot, or else writes the inverse of the winning kb x kb
// block P to Pinv (ld NB), adds log|det P| to ctl->logdet and turns the winners into the interchanges piv[k .. k+kb) (LAPACK style, piv[j] >= j).
// A pivot-row entry equal to the pivot scales to exactly 1, so that a column equal to an earlier one of the panel eliminates to exact zeros
// and the exactly singular panel is flagged.
template <int NB, int R>
__global__ __launch_bounds__(GJ_THREADS) void k_gj_tslu(int k, int kb, const double* __restrict__ A, int lda, int* __restrict__ piv, SignCtl* ctl,
                                                        const int* __restrict__ cand_in, int ncand, int* __restrict__ cand_out,
                                                        double* __restrict__ Pinv) {
    if (ctl->singular) return;
    __shared__ double prow[2][NB], jrow[2][NB];
    __shared__ double redv[2][GJ_THREADS / 64];
    __shared__ int redi[2][GJ_THREADS / 64];
    __shared__ int porg[2], jorg[2], win[NB];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int base = (int)blockIdx.x * (GJ_THREADS * R);                   // this workgroup's first entry of the candidate list
    const int m = min(GJ_THREADS * R, ncand - base);                       // its local rows
    const bool fin = gridDim.x == 1;                                       // this workgroup decides the pivots
    double a[R][NB];
    int org[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = tid + r * GJ_THREADS;
        const int row = i < m ? (cand_in ? cand_in[base + i] : k + base + i) : 0;
        org[r] = row;
#pragma unroll
        for (int c = 0; c < NB; ++c) a[r][c] = (i < m && c < kb) ? A[row + (size_t)(k + c) * lda] : 0.0;
    }
    double ldacc = 0.0;
    // fully unrolled, so that a[r][jj] has a compile-time column index and the panel stays in registers: the tail panel (kb < NB) is
    // handled by predicating the body on the uniform jj < kb, not by leaving the loop (a loop exit keeps it rolled and moves a[][] to scratch)
#pragma clang loop unroll(full)
    for (int jj = 0; jj < NB; ++jj) {
        if (jj < kb) {
        const int j = jj, buf = jj & 1;
        double best = -1.0;
        int bi = m;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = tid + r * GJ_THREADS;
            const double v = fabs(a[r][jj]);
            if (i >= j && i < m && v > best) { best = v; bi = i; }      // (rows ascend with r: ties keep the smaller index; NaN never wins)
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(best, off);
            const int oi = __shfl_xor(bi, off);
            if (ov > best || (ov == best && oi < bi)) { best = ov; bi = oi; }
        }
        if (lane == 0) { redv[buf][wave] = best; redi[buf][wave] = bi; }
        __syncthreads();
        best = redv[buf][0]; bi = redi[buf][0];
#pragma unroll
        for (int w = 1; w < GJ_THREADS / 64; ++w)
            if (redv[buf][w] > best || (redv[buf][w] == best && redi[buf][w] < bi)) { best = redv[buf][w]; bi = redi[buf][w]; }
        const int p = bi;
        const bool bad = !(best > 0.0) || p >= m || !isfinite(best);     // an exactly zero (or non-finite) pivot column
        if (bad && fin) {
            if (tid == 0) ctl->singular = 1;
            return;
        }
        if (!bad) {          // (a local round without a usable pivot keeps row j where it is; redv is double-buffered for that skipped barrier)
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = tid + r * GJ_THREADS;
            if (i == p) {
#pragma unroll
                for (int c = 0; c < NB; ++c) prow[buf][c] = a[r][c];
                porg[buf] = org[r];
            }
            if (i == j) {
#pragma unroll
                for (int c = 0; c < NB; ++c) jrow[buf][c] = a[r][c];
                jorg[buf] = org[r];
            }
        }
        __syncthreads();
        const double pv = prow[buf][jj], dinv = 1.0 / pv;
        if (tid == 0 && fin) ldacc += log(fabs(pv));
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = tid + r * GJ_THREADS;
            if (i >= m) continue;
            if (i == p && p != j) {
#pragma unroll
                for (int c = 0; c < NB; ++c) a[r][c] = jrow[buf][c];
                org[r] = jorg[buf];
            }
            if (i == j) {
#pragma unroll
                for (int c = 0; c < NB; ++c) a[r][c] = (c == jj) ? dinv : (prow[buf][c] == pv ? 1.0 : prow[buf][c] * dinv);
                org[r] = porg[buf];
            } else {
                const double f = a[r][jj];
#pragma unroll
                for (int c = 0; c < NB; ++c)
                    a[r][c] = (c == jj) ? -f * dinv : a[r][c] - f * (prow[buf][c] == pv ? 1.0 : prow[buf][c] * dinv);
            }
        }
        }
        }
    }
    if (!fin) {              // kb candidates of this workgroup (fewer when it has fewer rows: only the last one), in pivot order
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = tid + r * GJ_THREADS;
            if (i < kb && i < m) cand_out[blockIdx.x * kb + i] = org[r];
        }
        return;
    }
    // final round: local rows 0 .. kb-1 are the winners; their panel entries are P^-1 (the in-place Gauss-Jordan transform of [P; O])
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = tid + r * GJ_THREADS;
        if (i < kb) {
            win[i] = org[r];
#pragma unroll
            for (int c = 0; c < NB; ++c)
                if (c < kb) Pinv[i + c * NB] = a[r][c];
        }
    }
    if (tid == 0) ctl->logdet += ldacc;
    __syncthreads();
    // Winners -> ordered swaps by wave 0.  The table holds the positions a swap can touch (the panel rows k .. k+kb-1 and the winners
    // below them), one entry per lane and slot, with the original row each one holds now; step jj swaps position k + jj with the
    // current position of winner jj.
    if (wave == 0) {
        constexpr int S = (2 * NB + 63) / 64;
        int pos[S], occ[S];
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const int e = lane + 64 * s;
            pos[s] = occ[s] = -1;
            if (e < kb) pos[s] = occ[s] = k + e;
            else if (e >= NB && e - NB < kb && win[e - NB] >= k + kb) pos[s] = occ[s] = win[e - NB];
        }
        for (int jj = 0; jj < kb; ++jj) {
            const int tgt = win[jj], d = k + jj;
            int p = d, y = d;
#pragma unroll
            for (int s = 0; s < S; ++s) {
                const unsigned long long b = __ballot(occ[s] == tgt);
                if (b) p = __shfl(pos[s], __ffsll((unsigned long long)b) - 1);
                const int v = __shfl(occ[s], jj & 63);
                if ((jj >> 6) == s) y = v;
            }
#pragma unroll
            for (int s = 0; s < S; ++s) {
                if (occ[s] == tgt && pos[s] != d) occ[s] = y;
                if (lane + 64 * s == jj) occ[s] = tgt;
            }
            if (lane == 0) piv[d] = p;
        }
    }
}

// the panel's row interchanges applied to every column outside it (with_panel: to the panel's columns too), and W(:, c) = A(k:k+kb, c) (ld nb)
// for the trailing update
__global__ __launch_bounds__(256) void k_gj_swap(int n, int k, int kb, int nb, double* __restrict__ A, int lda, const int* __restrict__ piv,
                                                 double* __restrict__ W, const SignCtl* ctl, int with_panel) {
    if (ctl->singular) return;
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= n || (!with_panel && col >= k && col < k + kb)) return;
    double* Ac = A + (size_t)col * lda;
    for (int jj = 0; jj < kb; ++jj) {
        const int j = k + jj, p = piv[j];
        if (p != j && p > j && p < n) { const double t = Ac[j]; Ac[j] = Ac[p]; Ac[p] = t; }
    }
    for (int c = 0; c < kb; ++c) W[c + (size_t)col * nb] = Ac[k + c];
}

// Tournament panel, after the interchanges: A(k:k+kb, J) <- P^-1 and A(i, J) <- -A(i, J) P^-1 for every other row i (the columns J of the
// Gauss-Jordan transform M), Pn = M - I on the panel's rows.  64 rows per workgroup, a quarter of the kb output columns per wave.
template <int NB>
__global__ __launch_bounds__(256) void k_gj_apply(int n, int k, int kb, double* __restrict__ A, int lda, double* __restrict__ Pn,
                                                  const double* __restrict__ Pinv, const SignCtl* ctl) {
    if (ctl->singular) return;
    __shared__ double Ps[NB][NB];
    const int tid = threadIdx.x, q = tid >> 6, i = blockIdx.x * 64 + (tid & 63);
    for (int e = tid; e < NB * NB; e += 256) {
        const int t = e % NB, c = e / NB;
        Ps[t][c] = (t < kb && c < kb) ? Pinv[t + c * NB] : 0.0;
    }
    double a[NB];
#pragma unroll
    for (int t = 0; t < NB; ++t) a[t] = (i < n && t < kb) ? A[i + (size_t)(k + t) * lda] : 0.0;
    __syncthreads();         // (the row's four threads read all of it before any of them writes)
    if (i >= n) return;
    const bool prow = i >= k && i < k + kb;
#pragma unroll
    for (int cc = 0; cc < NB / 4; ++cc) {
        const int c = q * (NB / 4) + cc;
        if (c < kb) {
            double v;
            if (prow) {
                v = Ps[i - k][c];
            } else {
                double s = 0.0;
#pragma unroll
                for (int t = 0; t < NB; ++t) s += a[t] * Ps[t][c];
                v = -s;
            }
            A[i + (size_t)(k + c) * lda] = v;
            Pn[i + (size_t)c * n] = v - (prow && i - k == c ? 1.0 : 0.0);
        }
    }
}

// inv(A) = M P_{n-1} ... P_0: the column interchanges in reverse order, one row per thread
__global__ __launch_bounds__(256) void k_gj_unpivot(int n, double* __restrict__ A, int lda, const int* __restrict__ piv, const SignCtl* ctl) {
    if (ctl->singular) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int j = n - 1; j >= 0; --j) {
        const int p = piv[j];
        if (p != j && p > j && p < n) {
            const double t = A[i + (size_t)j * lda];
            A[i + (size_t)j * lda] = A[i + (size_t)p * lda];
            A[i + (size_t)p * lda] = t;
        }
    }
}

__global__ void k_ctl_reset(SignCtl* ctl) { ctl->logdet = 0.0; ctl->singular = 0; }

template <int NB, int R>
static void launch_panel(Ctx* ctx, int n, int k, int kb, double* A, int lda, double* Pn, int* piv, SignCtl* ctl) {
    hipLaunchKernelGGL((k_gj_panel<NB, R>), dim3(1), dim3(GJ_THREADS), 0, ctx->stream, n, k, kb, A, lda, Pn, piv, ctl);
}

// the register panel: one workgroup per panel, nb shrinking with n (n <= GJ_REGISTER_MAX_N)
static void gj_invert_register(Ctx* ctx, Mat& A, int* piv, SignCtl* ctl) {
    const int n = A.rows;
    const int R = ceil_div(n, GJ_THREADS);
    const int nb = R <= 3 ? 32 : (R <= 5 ? 16 : 8);     // the panel's registers: R x nb doubles per thread (no scratch in any instantiation)
    Mat Pn(ctx, n, nb), W(ctx, nb, n);
    for (int k = 0; k < n; k += nb) {
        const int kb = std::min(nb, n - k);
        {
            TimedScope ts(ctx, "gj_panel", 16.0 * n * kb, 2.0 * n * kb * kb);
            switch (R) {
                case 1: launch_panel<32, 1>(ctx, n, k, kb, A.p, A.ld, Pn.p, piv, ctl); break;
                case 2: launch_panel<32, 2>(ctx, n, k, kb, A.p, A.ld, Pn.p, piv, ctl); break;
                case 3: launch_panel<32, 3>(ctx, n, k, kb, A.p, A.ld, Pn.p, piv, ctl); break;
                case 4: launch_panel<16, 4>(ctx, n, k, kb, A.p, A.ld, Pn.p, piv, ctl); break;
                case 5: launch_panel<16, 5>(ctx, n, k, kb, A.p, A.ld, Pn.p, piv, ctl); break;
                case 6: launch_panel<8, 6>(ctx, n, k, kb, A.p, A.ld, Pn.p, piv, ctl); break;
                case 7: launch_panel<8, 7>(ctx, n, k, kb, A.p, A.ld, Pn.p, piv, ctl); break;
                default: launch_panel<8, 8>(ctx, n, k, kb, A.p, A.ld, Pn.p, piv, ctl); break;
            }
            hipLaunchKernelGGL(k_gj_swap, dim3(ceil_div(n, 256)), dim3(256), 0, ctx->stream, n, k, kb, nb, A.p, A.ld, (const int*)piv, W.p,
                               (const SignCtl*)ctl, 0);
        }
        // rank-kb updates of the columns left and right of the panel
        gemm(ctx, false, false, n, k, kb, 1.0, Pn.p, n, W.p, nb, 1.0, A.p, A.ld, nullptr, "gj_update");
        const int c1 = k + kb;
        gemm(ctx, false, false, n, n - c1, kb, 1.0, Pn.p, n, W.p + (size_t)c1 * nb, nb, 1.0, A.p + (size_t)c1 * A.ld, A.ld, nullptr, "gj_update");
    }
}

// the tournament panel (any n <= DENSE_MAX_N): per panel the selection rounds (slabs of 512 rows, then the candidates in groups of 512, until
// one workgroup holds them all), the interchanges of all columns, the apply kernel and the same rank-kb updates.  No wait between workgroups anywhere.
template <int NB>
static void gj_invert_tournament(Ctx* ctx, Mat& A, int* piv, SignCtl* ctl) {
    const int n = A.rows;
    Mat Pn(ctx, n, NB), W(ctx, NB, n);
    DevArr<int> cand0(ctx, n), cand1(ctx, n);
    DevArr<double> Pinv(ctx, NB * NB);
    for (int k = 0; k < n; k += NB) {
        const int kb = std::min(NB, n - k);
        {
            TimedScope ts(ctx, "gj_tslu", 8.0 * (n - k) * kb, 2.0 * (n - k) * kb * kb);
            int cnt = n - k;
            const int* in = nullptr;
            int* out = cand0.p;
            for (;;) {
                const int G = ceil_div(cnt, GJ_THREADS);
                hipLaunchKernelGGL((k_gj_tslu<NB, 1>), dim3(G), dim3(GJ_THREADS), 0, ctx->stream, k, kb, (const double*)A.p, A.ld, piv, ctl, in, cnt,
                                   out, Pinv.p);
                if (G == 1) break;
                cnt = (G - 1) * kb + std::min(kb, cnt - (G - 1) * GJ_THREADS);
                in = out;
                out = out == cand0.p ? cand1.p : cand0.p;
            }
        }
        {
            TimedScope ts(ctx, "gj_swap", 16.0 * kb * n, 0.0);
            hipLaunchKernelGGL(k_gj_swap, dim3(ceil_div(n, 256)), dim3(256), 0, ctx->stream, n, k, kb, NB, A.p, A.ld, (const int*)piv, W.p,
                               (const SignCtl*)ctl, 1);
        }
        {
            TimedScope ts(ctx, "gj_apply", 24.0 * n * kb, 2.0 * n * kb * kb);
            hipLaunchKernelGGL((k_gj_apply<NB>), dim3(ceil_div(n, 64)), dim3(256), 0, ctx->stream, n, k, kb, A.p, A.ld, Pn.p, (const double*)Pinv.p,
                               (const SignCtl*)ctl);
        }
        gemm(ctx, false, false, n, k, kb, 1.0, Pn.p, n, W.p, NB, 1.0, A.p, A.ld, nullptr, "gj_update");
        const int c1 = k + kb;
        gemm(ctx, false, false, n, n - c1, kb, 1.0, Pn.p, n, W.p + (size_t)c1 * NB, NB, 1.0, A.p + (size_t)c1 * A.ld, A.ld, nullptr, "gj_update");
    }
}

void gj_invert(Ctx* ctx, Mat& A, int* piv, SignCtl* ctl) {
    const int n = A.rows;
    DRE_REQUIRE(A.cols == n && n >= 1 && n <= DENSE_MAX_N, "gj_invert: square matrix of order 1 .. " + std::to_string(DENSE_MAX_N) + " expected");
    const int mode = ctx->dense_gj_panel;
    DRE_REQUIRE(mode >= 0 && mode <= 2, "dense_gj_panel must be 0, 1 or 2");
    DRE_REQUIRE(mode != 1 || n <= GJ_REGISTER_MAX_N, "dense path: the register panel (dense_gj_panel = 1) takes n <= " +
                                                         std::to_string(GJ_REGISTER_MAX_N) + ", n = " + std::to_string(n));
    hipLaunchKernelGGL(k_ctl_reset, dim3(1), dim3(1), 0, ctx->stream, ctl);
    if (mode == 2 || (mode == 0 && n > GJ_REGISTER_MAX_N)) {
        gj_invert_tournament<GJ_TSLU_NB>(ctx, A, piv, ctl);
    } else {
        gj_invert_register(ctx, A, piv, ctl);
    }
    {
        TimedScope ts(ctx, "gj_unpivot", 16.0 * n * n, 0.0);
        hipLaunchKernelGGL(k_gj_unpivot, dim3(ceil_div(n, 256)), dim3(256), 0, ctx->stream, n, A.p, A.ld, (const int*)piv, (const SignCtl*)ctl);
    }
    DRE_HIP(hipGetLastError());
}

// ---- element-wise kernels with fused partial norms ----------------------------------------------------------------------------------
// Z_{k+1} = Z_k / (2c) + (c/2) Y  (Y = E P_k), written to Z and to Zi (the next inversion's operand); partial sums of ||Z_{k+1} + E||^2,
// ||Z_{k+1} - Z_k||^2 and ||Z_{k+1}||^2 per workgroup
__global__ __launch_bounds__(256) void k_sign_update(int n, double* __restrict__ Z, double* __restrict__ Zi, const double* __restrict__ Y,
                                                     const double* __restrict__ E, double c, double* __restrict__ part) {
    __shared__ double red[17];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    const size_t tot = (size_t)n * n;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < tot; idx += (size_t)gridDim.x * blockDim.x) {
        const double z = Z[idx], zn = z / (2.0 * c) + (0.5 * c) * Y[idx];
        const double a = zn + E[idx], b = zn - z;
        s0 += a * a; s1 += b * b; s2 += zn * zn;
        Z[idx] = zn; Zi[idx] = zn;
    }
    s0 = block_sum(s0, red);
    s1 = block_sum(s1, red);
    s2 = block_sum(s2, red);
    if (threadIdx.x == 0) { part[blockIdx.x] = s0; part[gridDim.x + blockIdx.x] = s1; part[2 * gridDim.x + blockIdx.x] = s2; }
}

// the stopping norm and the decision of the sign iteration (tests/_sign_model.py)
__global__ __launch_bounds__(256) void k_sign_decide(int nparts, const double* __restrict__ part, const double* __restrict__ nE2, double tol,
                                                     SignCtl* ctl) {
    __shared__ double red[17];
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) { s0 += part[i]; s1 += part[nparts + i]; s2 += part[2 * nparts + i]; }
    s0 = block_sum(s0, red);
    s1 = block_sum(s1, red);
    s2 = block_sum(s2, red);
    if (threadIdx.x == 0) {
        const double e = sqrt(s0 / nE2[0]), d = sqrt(s1 / s2);
        ctl->dist = e; ctl->step = d;
        ctl->done = !isfinite(e) || !isfinite(d) ? 3 : (e <= tol ? 1 : ((d <= STAG_STEP && e > STAG_DIST) ? 2 : 0));
    }
}

// Res = R + G + G' (G = F'XE) and its partial sums of squares
__global__ __launch_bounds__(256) void k_res_sym(int n, const double* __restrict__ Rm, const double* __restrict__ G, double* __restrict__ Res,
                                                 double* __restrict__ part) {
    __shared__ double red[17];
    double s = 0.0;
    const size_t tot = (size_t)n * n;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < tot; idx += (size_t)gridDim.x * blockDim.x) {
        const int i = idx % n, j = idx / n;
        const double v = Rm[idx] + G[idx] + G[j + (size_t)i * n];
        Res[idx] = v;
        s += v * v;
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void k_res_finish(int nparts, const double* __restrict__ part, const double* __restrict__ nR2, SignCtl* ctl) {
    __shared__ double red[17];
    double s = 0.0;
    for (int i = threadIdx.x; i < nparts; i += blockDim.x) s += part[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) ctl->res = nR2[0] > 0.0 ? sqrt(s / nR2[0]) : sqrt(s);
}

// out = sym?(a0 M0 + a1 M1 + a2 M2) for n x n column-major matrices with ld n (M1, M2 may be null); out must not alias an input when sym
__global__ __launch_bounds__(256) void k_comb(int n, double a0, const double* __restrict__ M0, double a1, const double* M1, double a2,
                                              const double* M2, double* out, int sym) {
    const size_t tot = (size_t)n * n;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < tot; idx += (size_t)gridDim.x * blockDim.x) {
        double v = a0 * M0[idx] + (M1 ? a1 * M1[idx] : 0.0) + (M2 ? a2 * M2[idx] : 0.0);
        if (sym) {
            const int i = idx % n, j = idx / n;
            const size_t t = j + (size_t)i * n;
            v = 0.5 * (v + a0 * M0[t] + (M1 ? a1 * M1[t] : 0.0) + (M2 ? a2 * M2[t] : 0.0));
        }
        out[idx] = v;
    }
}

static unsigned grid_for(size_t tot) { return (unsigned)std::max<size_t>(1, std::min<size_t>(1024, (tot + 255) / 256)); }

static void comb(Ctx* ctx, Mat& out, double a0, const Mat& M0, double a1 = 0.0, const Mat* M1 = nullptr, double a2 = 0.0, const Mat* M2 = nullptr,
                 bool sym = false) {
    const int n = out.rows;
    TimedScope ts(ctx, "dense_comb", 8.0 * (2 + (M1 != nullptr) + (M2 != nullptr)) * n * n, 0.0);
    hipLaunchKernelGGL(k_comb, dim3(grid_for((size_t)n * n)), dim3(256), 0, ctx->stream, n, a0, (const double*)M0.p, a1,
                       (const double*)(M1 ? M1->p : nullptr), a2, (const double*)(M2 ? M2->p : nullptr), out.p, sym ? 1 : 0);
}

// ---- SignLyap --------------------------------------------------------------------------------------------------------------------
static Mat square(Ctx* ctx, int n) { return Mat(ctx, n, n); }

void require_memory(Ctx* ctx, size_t doubles) {
    size_t fr = 0, total = 0;
    DRE_HIP(hipMemGetInfo(&fr, &total));
    const size_t need = doubles * sizeof(double);
    const size_t avail = fr + ctx->pool.cached_bytes();       // free device memory + the pool's released (reusable) buffers, not its live ones
    if (need > avail)
        throw Error(ERR_ALLOC, "dense path: " + std::to_string(need >> 20) + " MiB of device memory needed, " + std::to_string(avail >> 20) +
                                   " MiB available");
}

SignLyap::SignLyap(Ctx* ctx, const Mat& E, int maxiters, double tol, int max_refine, size_t extra_n2, bool lazy_dense)
    : c_(ctx), n_(E.rows), maxiters_(maxiters), max_refine_(max_refine), tol_(tol) {
    const int n = n_;
    DRE_REQUIRE(E.cols == n && n >= 1 && n <= DENSE_MAX_N, "dense path: E must be square of order 1 .. " + std::to_string(DENSE_MAX_N) +
                                                            " (the device's 32-bit index limit)");
    DRE_REQUIRE(ctx->dense_gj_panel != 1 || n <= GJ_REGISTER_MAX_N, "dense path: the register panel (dense_gj_panel = 1) takes n <= " +
                                                                         std::to_string(GJ_REGISTER_MAX_N) + ", n = " + std::to_string(n));
    DRE_REQUIRE(E.ld == n, "dense path: E must be stored with leading dimension n");     // (the element-wise kernels index n x n operands densely)
    DRE_REQUIRE(maxiters >= 1 && maxiters <= 1000, "dense path: maxiters must be in 1 .. 1000");
    DRE_REQUIRE(max_refine >= 0, "dense path: max_refine must be >= 0");
    if (!(tol_ > 0.0)) tol_ = 10.0 * n * 2.220446049250313e-16;
    require_memory(ctx, ((size_t)maxiters + (lazy_dense ? 7 : 10) + extra_n2) * n * n);
    Pstore_ = Mat(ctx, n, n * maxiters);
    E_ = E;
    Einv_ = square(ctx, n); F_ = square(ctx, n); Z_ = square(ctx, n); Zi_ = square(ctx, n); Y_ = square(ctx, n);
    if (!lazy_dense) { W_ = square(ctx, n); T_ = square(ctx, n); Res_ = square(ctx, n); }
    piv_ = DevArr<int>(ctx, n);
    ctl_ = DevArr<SignCtl>(ctx, 1);
    part_ = DevArr<double>(ctx, 3 * SIGN_PARTS);
    nrm_ = DevArr<double>(ctx, 2);
    DRE_HIP(hipMemsetAsync(ctl_.p, 0, sizeof(SignCtl), ctx->stream));
    // E^-1 and log|det E| once per solve
    copy_mat(ctx, E, Einv_);
    gj_invert(ctx, Einv_, piv_.p, ctl_.p);
    frob2_device(ctx, E, nrm_.p);
    SignCtl h;
    read_ctl(&h);
    if (h.singular) throw Error(ERR_SINGULAR, "dense path: E is singular (zero pivot in the Gauss-Jordan inversion)");
    logdetE_ = h.logdet;
}

void SignLyap::ensure_dense_work() {
    if (W_.p) return;
    require_memory(c_, (size_t)3 * n_ * n_);
    W_ = square(c_, n_); T_ = square(c_, n_); Res_ = square(c_, n_);
}

void SignLyap::read_ctl(SignCtl* h) {
    DRE_HIP(hipMemcpyAsync(h, ctl_.p, sizeof(SignCtl), hipMemcpyDeviceToHost, c_->stream));
    c_->sync();
}

void SignLyap::factor(const Mat& F) {
    const int n = n_;
    DRE_REQUIRE(F.rows == n && F.cols == n, "dense path: F must be n x n");
    copy_mat(c_, F, F_);
    copy_mat(c_, F, Z_);
    copy_mat(c_, F, Zi_);
    cs_.clear();
    iters_ = 0;
    bool scale = true;
    SignCtl h;
    for (int k = 0; k < maxiters_; ++k) {
        gj_invert(c_, Zi_, piv_.p, ctl_.p);
        read_ctl(&h);
        if (h.singular) throw Error(ERR_SINGULAR, "dense path: singular Z_" + std::to_string(k) + " in the sign iteration (F singular?)");
        const double cfac = scale ? std::exp((h.logdet - logdetE_) / n) : 1.0;
        Mat P = Pstore_.colsview(k * n, n);
        gemm(c_, false, false, 1.0, Zi_, E_, 0.0, P, nullptr, "sign_gemm");            // P_k = Z_k^-1 E
        gemm(c_, false, false, 1.0, E_, P, 0.0, Y_, nullptr, "sign_gemm");             // E P_k
        {
            TimedScope ts(c_, "sign_update", 40.0 * n * n, 0.0);
            hipLaunchKernelGGL(k_sign_update, dim3(SIGN_PARTS), dim3(256), 0, c_->stream, n, Z_.p, Zi_.p, (const double*)Y_.p, (const double*)E_.p, cfac,
                               part_.p);
            hipLaunchKernelGGL(k_sign_decide, dim3(1), dim3(256), 0, c_->stream, SIGN_PARTS, (const double*)part_.p, (const double*)nrm_.p, tol_, ctl_.p);
        }
        cs_.push_back(cfac);
        iters_ = k + 1;
        read_ctl(&h);
        if (h.done == 1) return;
        if (h.done == 2)
            throw Error(ERR_NOT_STABLE, "dense path: the pencil is not c-stable (sign iteration stagnated at ||Z + E|| / ||E|| = " + std::to_string(h.dist) + ")");
        if (h.done == 3) throw Error(ERR_NOT_STABLE, "dense path: the sign iteration produced non-finite values (pencil not c-stable?)");
        if (h.dist < SCALE_OFF) scale = false;
    }
    throw Error(ERR_NOT_STABLE, "dense path: the sign iteration did not reach -E in " + std::to_string(maxiters_) + " iterations (||Z + E|| / ||E|| = " +
                                    std::to_string(h.dist) + "); the pencil is not c-stable");
}

void SignLyap::replay(const Mat& R, Mat& X) {
    const int n = n_;
    copy_mat(c_, R, W_);
    for (int k = 0; k < iters_; ++k) {
        const Mat P = Pstore_.colsview(k * n, n);
        const double cf = cs_[(size_t)k];
        gemm(c_, false, false, 1.0, W_, P, 0.0, T_, nullptr, "sign_gemm");                     // W P
        gemm(c_, true, false, 0.5 * cf, P, T_, 1.0 / (2.0 * cf), W_, nullptr, "sign_gemm");    // W/(2c) + (c/2) P' W P
        comb(c_, Y_, 1.0, W_, 0.0, nullptr, 0.0, nullptr, true);
        std::swap(W_, Y_);
    }
    gemm(c_, false, false, 1.0, W_, Einv_, 0.0, T_, nullptr, "sign_gemm");                     // X = E^-T (W/2) E^-1
    gemm(c_, true, false, 0.5, Einv_, T_, 0.0, Y_, nullptr, "sign_gemm");
    comb(c_, X, 1.0, Y_, 0.0, nullptr, 0.0, nullptr, true);
}

double SignLyap::residual(const Mat& R, const Mat& X) {
    const int n = n_;
    gemm(c_, false, false, 1.0, X, E_, 0.0, T_, nullptr, "sign_gemm");       // X E
    gemm(c_, true, false, 1.0, F_, T_, 0.0, Y_, nullptr, "sign_gemm");       // F' X E
    TimedScope ts(c_, "sign_residual", 24.0 * n * n, 0.0);
    hipLaunchKernelGGL(k_res_sym, dim3(SIGN_PARTS), dim3(256), 0, c_->stream, n, (const double*)R.p, (const double*)Y_.p, Res_.p, part_.p);
    hipLaunchKernelGGL(k_res_finish, dim3(1), dim3(256), 0, c_->stream, SIGN_PARTS, (const double*)part_.p, (const double*)(nrm_.p + 1), ctl_.p);
    SignCtl h;
    read_ctl(&h);
    return h.res;
}

SignStats SignLyap::solve(const Mat& R, Mat& X) {
    const int n = n_;
    DRE_REQUIRE(R.rows == n && R.cols == n && R.ld == n && X.rows == n && X.cols == n && X.ld == n, "dense path: R and X must be n x n");
    DRE_REQUIRE(iters_ > 0, "dense path: factor() first");
    ensure_dense_work();
    frob2_device(c_, R, nrm_.p + 1);
    SignStats s;
    s.iters = iters_;
    replay(R, X);
    s.res0 = s.res = residual(R, X);
    const double target = 100.0 * n * 2.220446049250313e-16;
    Mat dX = square(c_, n);
    while (s.res > target && s.refinements < max_refine_) {
        replay(Res_, dX);
        comb(c_, X, 1.0, X, 1.0, &dX);
        s.res = residual(R, X);
        ++s.refinements;
    }
    return s;
}

// ---- Rosenbrock drivers (dense_ros{1,2,3,4}.jl of the reference) ------------------------------------------------
DenseGdreResult dense_gdre_solve(Ctx* ctx, const Mat& E, const Mat& A, const Mat& B, const Mat& C, const Mat& X0, double t0, double tf, double dt,
                                 int order, bool save_state, int maxiters, double tol, int max_refine) {
    const int n = E.rows, m = B.cols;
    DRE_REQUIRE(order >= 1 && order <= 4, "dense path: order must be 1 .. 4");
    DRE_REQUIRE(E.cols == n && A.rows == n && A.cols == n && B.rows == n && C.cols == n && X0.rows == n && X0.cols == n,
                "dense path: E, A, X0 must be n x n, B n x m, C q x n");
    DRE_REQUIRE(dt != 0.0 && std::isfinite(dt), "dense path: dt must be finite and nonzero");
    const int nsteps = (int)std::floor((tf - t0) / dt + 1e-9);
    DRE_REQUIRE(nsteps >= 0, "tspan and dt point in opposite directions");
    DenseGdreResult out;
    for (int i = 0; i <= nsteps; ++i) out.t.push_back(t0 + i * dt);
    // the sign solver's own (maxiters + 10) n^2, the driver's matrices (16 n^2 for Ros4) and the saved states
    SignLyap lyap(ctx, E, maxiters, tol, max_refine, 16 + (save_state ? (size_t)nsteps : 1));
    auto sq = [&] { return Mat(ctx, n, n); };
    Mat X = sq(), CtC = sq(), Acl = sq(), gF = sq(), T = sq(), AXE = sq(), Racc = sq(), Rs = sq(), K1 = sq(), K2 = sq(), K3 = sq(), K4 = sq();
    Mat XB(ctx, n, m), V1(ctx, n, m), V2(ctx, n, m);
    copy_mat(ctx, X0, X);
    gemm(ctx, true, false, 1.0, C, C, 0.0, CtC, nullptr, "dense_ros");
    // Kt = (B'XE)' = E'XB  (X symmetric)
    auto feedback = [&](const Mat& Xs) {
        Mat Kt(ctx, n, m);
        gemm(ctx, false, false, 1.0, Xs, B, 0.0, XB, nullptr, "dense_ros");
        gemm(ctx, true, false, 1.0, E, XB, 0.0, Kt, nullptr, "dense_ros");
        return Kt;
    };
    auto save = [&](const Mat& Xs) { Mat c = sq(); copy_mat(ctx, Xs, c); out.X.push_back(c); };
    // Y = E' M E
    auto EtME = [&](const Mat& M, Mat& Y) {
        gemm(ctx, false, false, 1.0, M, E, 0.0, T, nullptr, "dense_ros");
        gemm(ctx, true, false, 1.0, E, T, 0.0, Y, nullptr, "dense_ros");
    };
    auto solve = [&](const Mat& Rsym, Mat& Xout) { out.solves.push_back(lyap.solve(Rsym, Xout)); };
    save(X);
    Mat Kt = feedback(X);
    out.Kt.push_back(Kt);
    const double gamma2 = 1.0 + 1.0 / std::sqrt(2.0);
    for (int i = 1; i <= nsteps; ++i) {
        const double tau = out.t[(size_t)i - 1] - out.t[(size_t)i];
        // Acl = A - B K
        copy_mat(ctx, A, Acl);
        gemm(ctx, false, true, -1.0, B, Kt, 1.0, Acl, nullptr, "dense_ros");
        // R of the first stage (Ros2..4): C'C + A'XE + E'XA - K'K
        auto first_rhs = [&]() {
            gemm(ctx, false, false, 1.0, X, E, 0.0, T, nullptr, "dense_ros");
            gemm(ctx, true, false, 1.0, A, T, 0.0, AXE, nullptr, "dense_ros");
            copy_mat(ctx, CtC, Racc);
            gemm(ctx, false, true, -1.0, Kt, Kt, 1.0, Racc, nullptr, "dense_ros");
            comb(ctx, Racc, 1.0, Racc, 2.0, &AXE);        // sym(R + 2 A'XE) = C'C + A'XE + E'XA - K'K
            comb(ctx, Rs, 1.0, Racc, 0.0, nullptr, 0.0, nullptr, true);
        };
        if (order == 1) {
            comb(ctx, gF, 1.0, Acl, -1.0 / (2.0 * tau), &E);                                 // F = (A - BK) - E/(2 tau)
            lyap.factor(gF);
            copy_mat(ctx, CtC, Racc);                                                        // R = C'C + K'K + E'XE / tau
            gemm(ctx, false, true, 1.0, Kt, Kt, 1.0, Racc, nullptr, "dense_ros");
            EtME(X, K2);
            comb(ctx, Rs, 1.0, Racc, 1.0 / tau, &K2, 0.0, nullptr, true);
            solve(Rs, X);
        } else if (order == 2) {
            comb(ctx, gF, gamma2 * tau, Acl, -0.5, &E);                                       // gF = gamma tau (A - BK) - E/2
            lyap.factor(gF);
            first_rhs();
            solve(Rs, K1);
            gemm(ctx, false, false, 1.0, K1, B, 0.0, XB, nullptr, "dense_ros");             // V1 = E'K1B = (B'K1E)'
            gemm(ctx, true, false, 1.0, E, XB, 0.0, V1, nullptr, "dense_ros");
            EtME(K1, Racc);
            comb(ctx, Racc, -(2.0 - 1.0 / gamma2), Racc);
            gemm(ctx, false, true, -tau * tau, V1, V1, 1.0, Racc, nullptr, "dense_ros");
            comb(ctx, Rs, 1.0, Racc, 0.0, nullptr, 0.0, nullptr, true);
            solve(Rs, K2);
            comb(ctx, X, 1.0, X, tau / 2.0, &K2, (tau / 2.0) * (4.0 - 1.0 / gamma2), &K1);  // X + tau/2 (Kt2 + (4 - 1/gamma) K1)
        } else if (order == 3) {
            const double g = 7.886751345948129e-1, a21 = 1.267949192431123;
            const double c21 = -1.607695154586736, c31 = -3.464101615137755, c32 = -1.732050807568877;
            const double m1 = 2.0, m2 = 5.773502691896258e-1, m3 = 4.226497308103742e-1;
            comb(ctx, gF, 1.0, Acl, -1.0 / (2.0 * g * tau), &E);                            // gF = (A - BK) - E/(2 gamma tau)
            lyap.factor(gF);
            first_rhs();
            solve(Rs, K1);
            gemm(ctx, false, false, 1.0, K1, E, 0.0, T, nullptr, "dense_ros");              // RX = (A - BK)' K1 E
            gemm(ctx, true, false, 1.0, Acl, T, 0.0, AXE, nullptr, "dense_ros");
            EtME(K1, Racc);
            comb(ctx, Rs, 2.0 * a21, AXE, c21 / tau, &Racc, 0.0, nullptr, true);           // sym(a21 (RX + RX') + c21/tau E'K1E)
            solve(Rs, K2);                                                                   // K21
            comb(ctx, K3, (c31 + c32) / tau, K1, c32 / tau, &K2);
            EtME(K3, Racc);
            comb(ctx, Rs, 2.0 * a21, AXE, 1.0, &Racc, 0.0, nullptr, true);
            solve(Rs, K3);                                                                   // K31
            comb(ctx, X, 1.0, X, m1 + m2 + m3, &K1, m2, &K2);
            comb(ctx, X, 1.0, X, m3, &K3);
        } else {
            comb(ctx, gF, tau / 2.0, Acl, -0.5, &E);                                         // gF = (tau (A - BK) - E)/2
            lyap.factor(gF);
            first_rhs();
            solve(Rs, K1);
            Mat EK1E = AXE;                                                                  // (A'XE is dead from here on)
            EtME(K1, EK1E);
            gemm(ctx, false, false, 1.0, K1, B, 0.0, XB, nullptr, "dense_ros");             // V1 = E'K1B
            gemm(ctx, true, false, 1.0, E, XB, 0.0, V1, nullptr, "dense_ros");
            comb(ctx, Racc, -2.0, EK1E);
            gemm(ctx, false, true, -tau * tau, V1, V1, 1.0, Racc, nullptr, "dense_ros");
            comb(ctx, Rs, 1.0, Racc, 0.0, nullptr, 0.0, nullptr, true);
            solve(Rs, K2);                                                                   // K21
            comb(ctx, K2, 1.0, K2, -1.0, &K1);                                               // K2 = K21 - K1
            const double al = (24.0 / 25.0) * tau, be = (3.0 / 25.0) * tau;
            EtME(K2, K4);                                                                    // EK2E (in K4 until K4 is formed)
            gemm(ctx, false, false, 1.0, K2, B, 0.0, XB, nullptr, "dense_ros");             // V2 = E'K2B
            gemm(ctx, true, false, 1.0, E, XB, 0.0, V2, nullptr, "dense_ros");
            comb(ctx, Racc, 245.0 / 25.0, EK1E, 36.0 / 25.0, &K4);
            gemm(ctx, false, true, -(426.0 / 625.0) * tau * tau, V1, V1, 1.0, Racc, nullptr, "dense_ros");
            gemm(ctx, false, true, -be * be, V2, V2, 1.0, Racc, nullptr, "dense_ros");
            gemm(ctx, false, true, -2.0 * al * be, V2, V1, 1.0, Racc, nullptr, "dense_ros");   // -al be (TMP + TMP') under sym
            comb(ctx, Rs, 1.0, Racc, 0.0, nullptr, 0.0, nullptr, true);
            solve(Rs, K3);                                                                   // K31
            comb(ctx, K3, 1.0, K3, -17.0 / 25.0, &K1);                                       // K3 = K31 - 17/25 K1
            comb(ctx, Racc, -981.0 / 125.0, EK1E, -177.0 / 125.0, &K4);
            EtME(K3, Rs);
            comb(ctx, Racc, 1.0, Racc, -0.2, &Rs);
            comb(ctx, Rs, 1.0, Racc, 0.0, nullptr, 0.0, nullptr, true);
            solve(Rs, K4);                                                                   // K41
            comb(ctx, K4, 1.0, K4, 1.0, &K3);                                                // K4 = K41 + K3
            comb(ctx, X, 1.0, X, tau * 19.0 / 18.0, &K1, tau * 0.25, &K2);
            comb(ctx, X, 1.0, X, tau * 25.0 / 216.0, &K3, tau * 125.0 / 216.0, &K4);
        }
        if (save_state) save(X);
        Kt = feedback(X);
        out.Kt.push_back(Kt);
    }
    if (!save_state && nsteps > 0) save(X);         // (no step: X0 is the only state, as t and K have one entry)
    ctx->sync();
    return out;
}

}  // namespace dre
