// Device bodies of the complex register-panel Gauss-Jordan inversion (dense_cgj.hip): the complex counterparts of
// dense_gj_body.hpp on planar storage, a member being two n x n real planes Ar and Ai of one leading dimension.  The host model is
// tests/_cgj_model.py.
#pragma once
#include "dense_gj_body.hpp"

namespace dre {

// 1 / (pr + i pi) by Smith's formula: no pr^2 + pi^2, so that a pivot of modulus 2^600 (or 2^-600) inverts without overflow (underflow).
// A purely real pivot gives an exactly zero imaginary part, a purely imaginary one an exactly zero real part.
__device__ __forceinline__ void cgj_reciprocal(double pr, double pi, double& dr, double& di) {
    if (fabs(pr) >= fabs(pi)) {
        const double r = pi / pr, den = pr + pi * r;
        dr = 1.0 / den; di = -r / den;
    } else {
        const double r = pr / pi, den = pi + pr * r;
        dr = r / den; di = -1.0 / den;
    }
}

// Panel: columns k .. k+kb-1 of both planes, all n rows, in registers (thread t owns rows t, t + 512, ...).  Step jj: pivot search by
// |re| + |im| over rows >= j = k + jj, interchange of rows j and p (through LDS), scaling of the pivot row by the pivot's reciprocal (Smith's formula, NB threads),
// elimination of column j from every other row.  On exit the panel's columns hold the columns of the accumulated transform M in both planes,
// and Pt (n x 2kb, ld n) = [Re M | Im M]: the trailing update of every other column is the real product [Cr | Ci] += Pt Wt with Wt of
// cgj_swap_body, which has moved the panel's rows of those columns into Wt and left zeros behind.  (The real body keeps those rows and
// subtracts the identity from Pn instead; M - I rounds M's diagonal block away when the matrix is scaled by 2^600 and its inverse by 2^-600.)
template <int NB, int R>
__device__ __forceinline__ void cgj_panel_body(int n, int k, int kb, double* __restrict__ Ar, double* __restrict__ Ai, int lda,
                                               double* __restrict__ Pt, int* __restrict__ piv, GjCtl* ctl) {
    if (ctl->singular) return;
    __shared__ double prow[2][2][NB], jrow[2][2][NB], srow[2][2][NB];
    __shared__ double redv[GJ_THREADS / 64];
    __shared__ int redi[GJ_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double ar[R][NB], ai[R][NB];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int i = tid + r * GJ_THREADS;
#pragma unroll
        for (int c = 0; c < NB; ++c) {
            const bool in = i < n && c < kb;
            ar[r][c] = in ? Ar[i + (size_t)(k + c) * lda] : 0.0;
            ai[r][c] = in ? Ai[i + (size_t)(k + c) * lda] : 0.0;
        }
    }
    double ldacc = 0.0;
    // fully unrolled and predicated on the uniform jj < kb, as in gj_panel_body: a loop exit would move the panel to scratch
#pragma clang loop unroll(full)
    for (int jj = 0; jj < NB; ++jj) {
        if (jj < kb) {
        const int j = k + jj, buf = jj & 1;
        double best = -1.0;
        int bi = n;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = tid + r * GJ_THREADS;
            const double v = fabs(ar[r][jj]) + fabs(ai[r][jj]);
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
                for (int c = 0; c < NB; ++c) { prow[buf][0][c] = ar[r][c]; prow[buf][1][c] = ai[r][c]; }
            }
            if (i == j) {
#pragma unroll
                for (int c = 0; c < NB; ++c) { jrow[buf][0][c] = ar[r][c]; jrow[buf][1][c] = ai[r][c]; }
            }
        }
        __syncthreads();
        // the scaled pivot row, once per panel column by thread c: srow[c] = prow[c] / pivot, and the pivot's reciprocal in its own column
        if (tid < NB) {
            double dr, di;
            cgj_reciprocal(prow[buf][0][jj], prow[buf][1][jj], dr, di);
            const double qr = prow[buf][0][tid], qi = prow[buf][1][tid];
            srow[buf][0][tid] = tid == jj ? dr : qr * dr - qi * di;
            srow[buf][1][tid] = tid == jj ? di : qr * di + qi * dr;
        }
        if (tid == 0) { ldacc += log(hypot(prow[buf][0][jj], prow[buf][1][jj])); piv[j] = p; }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int i = tid + r * GJ_THREADS;
            if (i >= n) continue;
            if (i == p && p != j) {
#pragma unroll
                for (int c = 0; c < NB; ++c) { ar[r][c] = jrow[buf][0][c]; ai[r][c] = jrow[buf][1][c]; }
            }
            if (i == j) {
#pragma unroll
                for (int c = 0; c < NB; ++c) { ar[r][c] = srow[buf][0][c]; ai[r][c] = srow[buf][1][c]; }
            } else {
                // a(i, c) -= f srow[c]; column j itself becomes -f / pivot
                const double fr = ar[r][jj], fi = ai[r][jj];
#pragma unroll
                for (int c = 0; c < NB; ++c) {
                    const double sr = srow[buf][0][c], si = srow[buf][1][c];
                    ar[r][c] = (c == jj ? 0.0 : ar[r][c]) - (fr * sr - fi * si);
                    ai[r][c] = (c == jj ? 0.0 : ai[r][c]) - (fr * si + fi * sr);
                }
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
                Ar[i + (size_t)(k + c) * lda] = ar[r][c];
                Ai[i + (size_t)(k + c) * lda] = ai[r][c];
                Pt[i + (size_t)c * n] = ar[r][c];
                Pt[i + (size_t)(kb + c) * n] = ai[r][c];
            }
        }
    }
    if (tid == 0) ctl->logdet += ldacc;
}

// The panel's row interchanges applied to both planes of every column outside it, and Wt (2kb x 2n, ld 2nb) for the trailing update: with
// W = A(k:k+kb, :) after the interchanges, Wt = [[Wr, Wi], [-Wi, Wr]], and A(k:k+kb, :) = 0 (the update writes M W there).  The panel's own
// columns of Wt are zero, so that one product over all 2n columns leaves the panel's columns as the panel kernel wrote them.  256 threads per
// workgroup, one column per thread.
__device__ __forceinline__ void cgj_swap_body(int n, int k, int kb, int nb, double* __restrict__ Ar, double* __restrict__ Ai, int lda,
                                              const int* __restrict__ piv, double* __restrict__ Wt, const GjCtl* ctl) {
    if (ctl->singular) return;
    const int col = blockIdx.x * blockDim.x + threadIdx.x;
    if (col >= n) return;
    const size_t ldw = (size_t)2 * nb;
    double* Wre = Wt + (size_t)col * ldw;                 // column col of [Wr; -Wi]
    double* Wim = Wt + ((size_t)n + col) * ldw;           // column col of [Wi; Wr]
    if (col >= k && col < k + kb) {
        for (int c = 0; c < 2 * kb; ++c) { Wre[c] = 0.0; Wim[c] = 0.0; }
        return;
    }
    double* Rc = Ar + (size_t)col * lda;
    double* Ic = Ai + (size_t)col * lda;
    for (int jj = 0; jj < kb; ++jj) {
        const int j = k + jj, p = piv[j];
        if (p != j && p > j && p < n) {
            const double t = Rc[j]; Rc[j] = Rc[p]; Rc[p] = t;
            const double u = Ic[j]; Ic[j] = Ic[p]; Ic[p] = u;
        }
    }
    for (int c = 0; c < kb; ++c) {
        const double wr = Rc[k + c], wi = Ic[k + c];
        Wre[c] = wr; Wre[kb + c] = -wi;
        Wim[c] = wi; Wim[kb + c] = wr;
        Rc[k + c] = 0.0; Ic[k + c] = 0.0;
    }
}

// inv(A) = M P_{n-1} ... P_0: the column interchanges in reverse order on both planes, one row per thread
__device__ __forceinline__ void cgj_unpivot_body(int n, double* __restrict__ Ar, double* __restrict__ Ai, int lda, const int* __restrict__ piv,
                                                 const GjCtl* ctl) {
    if (ctl->singular) return;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int j = n - 1; j >= 0; --j) {
        const int p = piv[j];
        if (p != j && p > j && p < n) {
            const size_t oj = i + (size_t)j * lda, op = i + (size_t)p * lda;
            const double t = Ar[oj]; Ar[oj] = Ar[op]; Ar[op] = t;
            const double u = Ai[oj]; Ai[oj] = Ai[op]; Ai[op] = u;
        }
    }
}

}  // namespace dre
