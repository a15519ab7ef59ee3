// Device bodies of the sign-function Lyapunov solver's element-wise kernels: the one text of the update of Z, the stopping rule, the
// residual and its norm.  k_sign_update, k_sign_decide, k_res_sym and k_res_finish of dense_sign.hip call them with the whole operands, the
// k_bsign_* / k_bres_* kernels of dense_batch.hip with one member's slices (base pointers already offset).  The scaling factor c comes in as
// an argument: the single path forms it on the host, the batched path on the device.  The host model is tests/_sign_model.py.
#pragma once
#include "dense_device.hpp"

namespace dre {

// g is KERNEL_GRID_STRIDE (dense_device.hpp): the grid-stride loop's first index and step, formed by the calling kernel.
static constexpr double SCALE_OFF = 1e-2;        // tests/_sign_model.py: SCALE_OFF, STAG_STEP, STAG_DIST
static constexpr double STAG_STEP = 1e-8;
static constexpr double STAG_DIST = 1e-4;

// Z_{k+1} = Z_k / (2c) + (c/2) Y  (Y = E P_k), written to Z and to Zi (the next inversion's operand); partial sums of ||Z_{k+1} + E||^2,
// ||Z_{k+1} - Z_k||^2 and ||Z_{k+1}||^2 per workgroup
__device__ __forceinline__ void sign_update_body(GridStride g, int n, double* __restrict__ Z, double* __restrict__ Zi, const double* __restrict__ Y,
                                                 const double* __restrict__ E, double c, double* __restrict__ part) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    const size_t tot = (size_t)n * n;
    for (size_t idx = g.first; idx < tot; idx += g.step) {
        const double z = Z[idx], zn = z / (2.0 * c) + (0.5 * c) * Y[idx];
        const double a = zn + E[idx], b = zn - z;
        s0 += a * a; s1 += b * b; s2 += zn * zn;
        Z[idx] = zn; Zi[idx] = zn;
    }
    store_partials(part, s0, s1, s2);
}

// the decision of the sign iteration on e = ||Z + E|| / ||E|| and d = ||Z_{k+1} - Z_k|| / ||Z_{k+1}||: 0 running, 1 converged, 2 stagnated
// away from -E (not c-stable), 3 non-finite
__device__ __forceinline__ int sign_decision(double e, double d, double tol) {
    return !isfinite(e) || !isfinite(d) ? 3 : (e <= tol ? 1 : ((d <= STAG_STEP && e > STAG_DIST) ? 2 : 0));
}

// Res = R + G + G' (G = F'XE) and its partial sums of squares
__device__ __forceinline__ void res_sym_body(GridStride g, int n, const double* __restrict__ Rm, const double* __restrict__ G, double* __restrict__ Res,
                                             double* __restrict__ part) {
    double s = 0.0;
    const size_t tot = (size_t)n * n;
    for (size_t idx = g.first; idx < tot; idx += g.step) {
        const int i = idx % n, j = idx / n;
        const double v = Rm[idx] + G[idx] + G[j + (size_t)i * n];
        Res[idx] = v;
        s += v * v;
    }
    store_partials(part, s);
}

// ||Res||_F / ||R||_F from the two sums of squares (||Res||_F for R = 0)
__device__ __forceinline__ double relative_residual(double res2, double nR2) { return nR2 > 0.0 ? sqrt(res2 / nR2) : sqrt(res2); }

}  // namespace dre
