// Device bodies of the dense GARE solver's element-wise kernels: the one text of the Hamiltonian's assembly, the structured update, the step
// rule, the extraction operands and the residual.  The k_are_* kernels of dense_are.hip call them with the whole operands, the k_bare_*
// kernels of dense_are_batch.hip with one member's slices (base pointers already offset); what the two callers obtain differently, the
// scaling factor c and the partial-sum slice, comes in as an argument.  The host model is tests/_hamiltonian_sign_model.py.
#pragma once
#include "dense_device.hpp"

namespace dre {

// g is KERNEL_GRID_STRIDE (dense_device.hpp): the grid-stride loop's first index and step, formed by the calling kernel.
static constexpr double ARE_SCALE_OFF = 1e-2;    // tests/_hamiltonian_sign_model.py: SCALE_OFF, STAG_WINDOW
static constexpr int ARE_STAG_WINDOW = 3;

// Z0 = [[A, -sym(G)], [-sym(Q), -A']] into Z and Zi (ld 2n; A, G, Q ld n)
__device__ __forceinline__ void are_assemble_body(GridStride g, int n, const double* __restrict__ A, const double* __restrict__ G, const double* __restrict__ Q,
                                                  double* __restrict__ Z, double* __restrict__ Zi) {
    const size_t L = 2 * (size_t)n, tot = (size_t)n * n;
    for (size_t idx = g.first; idx < tot; idx += g.step) {
        const size_t i = idx % n, j = idx / n, t = j + i * n;
        const double a = A[idx], at = A[t], g = -0.5 * (G[idx] + G[t]), q = -0.5 * (Q[idx] + Q[t]);
        const size_t p11 = i + j * L, p12 = i + (n + j) * L, p21 = (n + i) + j * L, p22 = (n + i) + (n + j) * L;
        Z[p11] = a; Zi[p11] = a;
        Z[p12] = g; Zi[p12] = g;
        Z[p21] = q; Zi[p21] = q;
        Z[p22] = -at; Zi[p22] = -at;
    }
}

// Z_{k+1} = struct((Z_k / c + c Y) / 2) with Y = K Z_k^-1 K in Zi, written to Z and to Zi (the next inversion's operand), and the partial sums
// of ||Z_{k+1} - Z_k||^2 and ||Z_{k+1}||^2 per workgroup.  Thread idx = (i, j) owns the orbits {Z11(i,j), Z22(j,i)} and, for i <= j,
// {Z12(i,j), Z12(j,i)} and {Z21(i,j), Z21(j,i)}: it reads and writes only its own orbits, so the structured average runs in place.
__device__ __forceinline__ void are_update_body(GridStride g, int n, double* __restrict__ Z, double* __restrict__ Zi, double c, double* __restrict__ part) {
    const double h0 = 0.5 / c, h1 = 0.5 * c;
    const size_t L = 2 * (size_t)n, tot = (size_t)n * n;
    double sd = 0.0, sz = 0.0;
    for (size_t idx = g.first; idx < tot; idx += g.step) {
        const size_t i = idx % n, j = idx / n;
        {   // Z11(i,j) and Z22(j,i):  Z11 := (Z11 - Z22')/2,  Z22 := -Z11'
            const size_t pa = i + j * L, pb = (n + j) + (n + i) * L;
            const double a = Z[pa], b = Z[pb];
            const double s = 0.5 * ((h0 * a + h1 * Zi[pa]) - (h0 * b + h1 * Zi[pb]));
            sd += (s - a) * (s - a) + (s + b) * (s + b);
            sz += 2.0 * s * s;
            Z[pa] = s; Zi[pa] = s;
            Z[pb] = -s; Zi[pb] = -s;
        }
        if (i <= j) {   // Z12 and Z21 symmetrised
#pragma unroll
            for (int blk = 0; blk < 2; ++blk) {
                const size_t r0 = blk ? n : 0, c0 = blk ? 0 : n;
                const size_t pa = (r0 + i) + (c0 + j) * L, pb = (r0 + j) + (c0 + i) * L;
                const double a = Z[pa], b = Z[pb];
                const double s = 0.5 * ((h0 * a + h1 * Zi[pa]) + (h0 * b + h1 * Zi[pb]));
                if (i < j) {
                    sd += (s - a) * (s - a) + (s - b) * (s - b);
                    sz += 2.0 * s * s;
                } else {
                    sd += (s - a) * (s - a);
                    sz += s * s;
                }
                Z[pa] = s; Zi[pa] = s;
                Z[pb] = s; Zi[pb] = s;
            }
        }
    }
    store_partials(part, sd, sz);
}

// the step rule of the sign iteration (tests/_hamiltonian_sign_model.py: sign_iteration) on the relative step d: returns done (0 running,
// 1 converged, 2 stagnated, 3 non-finite) and keeps the smallest step, the count since it and the scaling switch up to date
__device__ __forceinline__ int are_step_rule(double d, double tol, double& best, int& since, int& scale) {
    if (!isfinite(d)) return 3;
    if (d <= tol) return 1;
    if (d < best) {
        best = d; since = 0;
    } else if (!scale && ++since >= ARE_STAG_WINDOW) {          // (the scaled phase is not monotone: its first steps often grow)
        return 2;
    }
    if (d < ARE_SCALE_OFF) scale = 0;
    return 0;
}

// extraction operands: M = [Z12; Z22 + E'] into Zi(:, 0:n), rhs = -[Z11 + E; Z21] into Zi(:, n:2n)  (ld 2n; E ld n)
__device__ __forceinline__ void are_extract_ops_body(GridStride g, int n, const double* __restrict__ Z, const double* __restrict__ E, double* __restrict__ Zi) {
    const size_t L = 2 * (size_t)n, tot = (size_t)n * n;
    for (size_t idx = g.first; idx < tot; idx += g.step) {
        const size_t i = idx % n, j = idx / n;
        const double e = E[idx], et = E[j + i * n];
        Zi[i + j * L] = Z[i + (n + j) * L];                                  // Z12
        Zi[(n + i) + j * L] = Z[(n + i) + (n + j) * L] + et;                 // Z22 + E'
        Zi[i + (n + j) * L] = -(Z[i + j * L] + e);                           // -(Z11 + E)
        Zi[(n + i) + (n + j) * L] = -Z[(n + i) + j * L];                     // -Z21
    }
}

// the filter's extraction operands from the transposed blocks: M_f = [Z21'; Z22' + E] into Zi(:, 0:n), rhs_f = -[Z11' + E'; Z12'] into Zi(:, n:2n)
// (ld 2n; E ld n).  One workgroup of 256 threads per 32 x 32 tile of the n x n blocks, tile = (blockIdx.x, blockIdx.y): the source tile (rows
// j0.., columns i0..) is read along its columns into LDS (33 doubles per row: no bank conflicts on the transposed read-out) and written along
// the destination's columns, so both sides of each of the four transpositions are coalesced.  The untransposed E of the second block is read
// at the destination index.
__device__ __forceinline__ void are_extract_ops_t_body(int n, const double* __restrict__ Z, const double* __restrict__ E, double* __restrict__ Zi) {
    __shared__ double tile[32][33];
    const size_t L = 2 * (size_t)n, N = (size_t)n;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;                      // 32 x 8
    const size_t i0 = (size_t)blockIdx.x * 32, j0 = (size_t)blockIdx.y * 32;     // destination rows i0.., columns j0..
#pragma unroll 1
    for (int blk = 0; blk < 4; ++blk) {
        // blk 0: Z21' -> (0, 0);  1: Z22' + E -> (n, 0);  2: -(Z11 + E)' -> (0, n);  3: -Z12' -> (n, n)
        const size_t sr = blk < 2 ? N : 0, sc = (blk == 1 || blk == 3) ? N : 0;
        const size_t dr = (blk & 1) ? N : 0, dc = blk < 2 ? 0 : N;
        const size_t js = j0 + tx;                                               // source row
        for (int k = ty; k < 32; k += 8) {
            const size_t is = i0 + k;                                            // source column
            double v = 0.0;
            if (js < N && is < N) {
                v = Z[(sr + js) + (sc + is) * L];
                if (blk == 2) v += E[js + is * N];
            }
            tile[k][tx] = v;
        }
        __syncthreads();
        const size_t id = i0 + tx;                                               // destination row
        for (int k = ty; k < 32; k += 8) {
            const size_t jd = j0 + k;                                            // destination column
            if (id < N && jd < N) {
                double v = tile[tx][k];
                if (blk == 1) v += E[id + jd * N];
                Zi[(dr + id) + (dc + jd) * L] = blk < 2 ? v : -v;
            }
        }
        __syncthreads();
    }
}

// Res = sym(Q) + AXE + AXE' - sym(XGX) and the partial sums of ||Res||^2, ||Q||^2, ||AXE||^2, ||XGX||^2 (all n x n, ld n)
__device__ __forceinline__ void are_residual_body(GridStride g, int n, const double* __restrict__ Q, const double* __restrict__ AXE, const double* __restrict__ XGX,
                                                  double* __restrict__ Res, double* __restrict__ part) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    const size_t tot = (size_t)n * n;
    for (size_t idx = g.first; idx < tot; idx += g.step) {
        const size_t i = idx % n, j = idx / n, t = j + i * n;
        const double v = 0.5 * (Q[idx] + Q[t]) + (AXE[idx] + AXE[t]) - 0.5 * (XGX[idx] + XGX[t]);     // (exactly symmetric)
        Res[idx] = v;
        s0 += v * v; s1 += Q[idx] * Q[idx]; s2 += AXE[idx] * AXE[idx]; s3 += XGX[idx] * XGX[idx];
    }
    store_partials(part, s0, s1, s2, s3);
}

// the scaled residual ||R||_F / (||Q||_F + 2 ||A'XE||_F + ||E'XGXE||_F) from the four sums of are_residual_body; *fro = ||R||_F
__device__ __forceinline__ double are_scaled_residual(const double (&s)[4], double* fro) {
    const double r = sqrt(s[0]), den = sqrt(s[1]) + 2.0 * sqrt(s[2]) + sqrt(s[3]);
    *fro = r;
    return den > 0.0 ? r / den : r;
}

}  // namespace dre
