// Device bodies of the register-panel Gauss-Jordan inversion: the one text of the pivot rule and its ties, the elimination order and the
// log|det| accumulation.  k_gj_panel, k_gj_swap and k_gj_unpivot of dense_gj.hip call them with the whole matrix, k_bgj_panel, k_bgj_swap
// and k_bgj_unpivot of dense_batch.hip with one member's slices.
#pragma once
#include "dense_gj.hpp"

namespace dre {

static constexpr int GJ_THREADS = 512;

// Panel: columns k .. k+kb-1 of A, all n rows, in registers (thread t owns rows t, t + 512, ...).  Step jj: pivot search over rows
// >= j = k + jj, interchange of rows j and p (through LDS), scaling of the pivot row, elimination of column j from every other row.  On exit
// the panel columns hold the columns of the accumulated transform M, and Pn (n x kb) = M - I on the panel's rows: the trailing update of
// every other column c is A(:, c) += Pn W(:, c) with W = A(k:k+kb, :) after the interchanges.
template <int NB, int R>
__device__ __forceinline__ void gj_panel_body(int n, int k, int kb, double* __restrict__ A, int lda, double* __restrict__ Pn,
                                              int* __restrict__ piv, GjCtl* ctl) {
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

// the panel's row interchanges applied to every column outside it (with_panel: to the panel's columns too), and W(:, c) = A(k:k+kb, c) (ld nb)
// for the trailing update; 256 threads per workgroup, one column per thread
__device__ __forceinline__ void gj_swap_body(int n, int k, int kb, int nb, double* __restrict__ A, int lda, const int* __restrict__ piv,
                                             double* __restrict__ W, const GjCtl* ctl, int with_panel) {
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

// inv(A) = M P_{n-1} ... P_0: the column interchanges in reverse order, one row per thread
__device__ __forceinline__ void gj_unpivot_body(int n, double* __restrict__ A, int lda, const int* __restrict__ piv, const GjCtl* ctl) {
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

}  // namespace dre
