// In-place blocked Gauss-Jordan inversion with row pivoting, the inversion of the dense path:
//   gj_invert        a register-resident panel kernel (pivot search, row interchanges, elimination inside the panel, log|det|; n <= 4096) or
//                    the multi-workgroup tournament panel (any n), and rank-nb updates on the MFMA GEMM.
// The host model of the tournament panel is tests/_tslu_model.py.
#include "dense_gj.hpp"

#include "dense.hpp"
#include "dense_gj_body.hpp"
#include "profiling.hpp"

namespace dre {

// the tournament panel's width: 64 columns do not fit the selection round's registers at one row per thread (604 bytes of scratch), so the
// trailing update runs at K = 32 as the register panel's does for n <= 1536
static constexpr int GJ_TSLU_NB = 32;

// ---- Gauss-Jordan inversion ------------------------------------------------------------------------------------------------------
// Panel kernel: one workgroup, the whole panel in registers (gj_panel_body of dense_gj_body.hpp)
template <int NB, int R>
__global__ __launch_bounds__(GJ_THREADS) void k_gj_panel(int n, int k, int kb, double* __restrict__ A, int lda, double* __restrict__ Pn,
                                                         int* __restrict__ piv, GjCtl* ctl) {
    gj_panel_body<NB, R>(n, k, kb, A, lda, Pn, piv, ctl);
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
__global__ __launch_bounds__(GJ_THREADS) void k_gj_tslu(int k, int kb, const double* __restrict__ A, int lda, int* __restrict__ piv, GjCtl* ctl,
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

// the panel's row interchanges applied to every column outside it (with_panel: to the panel's columns too), and W for the trailing update
__global__ __launch_bounds__(256) void k_gj_swap(int n, int k, int kb, int nb, double* __restrict__ A, int lda, const int* __restrict__ piv,
                                                 double* __restrict__ W, const GjCtl* ctl, int with_panel) {
    gj_swap_body(n, k, kb, nb, A, lda, piv, W, ctl, with_panel);
}

// Tournament panel, after the interchanges: A(k:k+kb, J) <- P^-1 and A(i, J) <- -A(i, J) P^-1 for every other row i (the columns J of the
// Gauss-Jordan transform M), Pn = M - I on the panel's rows.  64 rows per workgroup, a quarter of the kb output columns per wave.
template <int NB>
__global__ __launch_bounds__(256) void k_gj_apply(int n, int k, int kb, double* __restrict__ A, int lda, double* __restrict__ Pn,
                                                  const double* __restrict__ Pinv, const GjCtl* ctl) {
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

// inv(A) = M P_{n-1} ... P_0: the column interchanges in reverse order
__global__ __launch_bounds__(256) void k_gj_unpivot(int n, double* __restrict__ A, int lda, const int* __restrict__ piv, const GjCtl* ctl) {
    gj_unpivot_body(n, A, lda, piv, ctl);
}

__global__ void k_ctl_reset(GjCtl* ctl) { ctl->logdet = 0.0; ctl->singular = 0; }

template <int NB, int R>
static void launch_panel(Ctx* ctx, int n, int k, int kb, double* A, int lda, double* Pn, int* piv, GjCtl* ctl) {
    hipLaunchKernelGGL((k_gj_panel<NB, R>), dim3(1), dim3(GJ_THREADS), 0, ctx->stream, n, k, kb, A, lda, Pn, piv, ctl);
}

// the register panel: one workgroup per panel, nb shrinking with n (n <= GJ_REGISTER_MAX_N)
static void gj_invert_register(Ctx* ctx, Mat& A, int* piv, GjCtl* ctl) {
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
                               (const GjCtl*)ctl, 0);
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
static void gj_invert_tournament(Ctx* ctx, Mat& A, int* piv, GjCtl* ctl) {
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
                               (const GjCtl*)ctl, 1);
        }
        {
            TimedScope ts(ctx, "gj_apply", 24.0 * n * kb, 2.0 * n * kb * kb);
            hipLaunchKernelGGL((k_gj_apply<NB>), dim3(ceil_div(n, 64)), dim3(256), 0, ctx->stream, n, k, kb, A.p, A.ld, Pn.p, (const double*)Pinv.p,
                               (const GjCtl*)ctl);
        }
        gemm(ctx, false, false, n, k, kb, 1.0, Pn.p, n, W.p, NB, 1.0, A.p, A.ld, nullptr, "gj_update");
        const int c1 = k + kb;
        gemm(ctx, false, false, n, n - c1, kb, 1.0, Pn.p, n, W.p + (size_t)c1 * NB, NB, 1.0, A.p + (size_t)c1 * A.ld, A.ld, nullptr, "gj_update");
    }
}

void gj_check_order(const Ctx* ctx, int order, const char* who) {
    DRE_REQUIRE(ctx->dense_gj_panel != 1 || order <= GJ_REGISTER_MAX_N, std::string(who) + ": the register panel (dense_gj_panel = 1) inverts matrices " +
                    "of order <= " + std::to_string(GJ_REGISTER_MAX_N) + ", order = " + std::to_string(order));
}

void gj_invert(Ctx* ctx, Mat& A, int* piv, GjCtl* ctl) {
    const int n = A.rows;
    DRE_REQUIRE(A.cols == n && n >= 1 && n <= DENSE_MAX_N, "gj_invert: square matrix of order 1 .. " + std::to_string(DENSE_MAX_N) + " expected");
    const int mode = ctx->dense_gj_panel;
    DRE_REQUIRE(mode >= 0 && mode <= 2, "dense_gj_panel must be 0, 1 or 2");
    gj_check_order(ctx, n, "gj_invert");
    hipLaunchKernelGGL(k_ctl_reset, dim3(1), dim3(1), 0, ctx->stream, ctl);
    if (mode == 2 || (mode == 0 && n > GJ_REGISTER_MAX_N)) {
        gj_invert_tournament<GJ_TSLU_NB>(ctx, A, piv, ctl);
    } else {
        gj_invert_register(ctx, A, piv, ctl);
    }
    {
        TimedScope ts(ctx, "gj_unpivot", 16.0 * n * n, 0.0);
        hipLaunchKernelGGL(k_gj_unpivot, dim3(ceil_div(n, 256)), dim3(256), 0, ctx->stream, n, A.p, A.ld, (const int*)piv, (const GjCtl*)ctl);
    }
    DRE_HIP(hipGetLastError());
}

void require_memory(Ctx* ctx, size_t doubles) {
    size_t fr = 0, total = 0;
    DRE_HIP(hipMemGetInfo(&fr, &total));
    const size_t need = doubles * sizeof(double);
    const size_t avail = fr + ctx->pool.cached_bytes();       // free device memory + the pool's released (reusable) buffers, not its live ones
    if (need > avail)
        throw Error(ERR_ALLOC, "dense path: " + std::to_string(need >> 20) + " MiB of device memory needed, " + std::to_string(avail >> 20) +
                                   " MiB available");
}

}  // namespace dre
