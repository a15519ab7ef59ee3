// Transfer function of dense descriptor systems at arbitrary complex points (transfer_eval.hip):
//   H(s_k) = C (s_k E - A)^-1 B,  s_k = sigma_k + i omega_k,
// for K points of one or several systems of one (n, m, q), the point on the member axis of the batched dense path as in freq_response.hpp.
//
// Method, per member (s, k) = system s at point k, member index s K + k, on planar complex storage (dense_cgj.hpp):
//   1. k_tf_assemble writes the planes  Zr = sigma E - A,  Zi = omega E;
//   2. cgj_invert_batched inverts the stack in place with the complex register panel (n <= GJ_REGISTER_MAX_N): X = [Xr | Xi];
//   3. gemm_strided forms  Y = X B  (B real: Yr = Xr B, Yi = Xi B);
//   4. one refinement step with the residual from E and A (the assembled matrix is not kept):
//        Rr = B + A Yr - sigma E Yr + omega E Yi,   Ri = A Yi - sigma E Yi - omega E Yr
//      (sigma and omega per member from a device array), then  [Yr | Yi] += [Xr | Xi] [[Rr, Ri], [-Ri, Rr]]  as one real product;
//   5. gemm_strided forms  Re H = C Yr  and  Im H = C Yi.
// The refinement step is there for the reason freq_response.hpp gives: the blocked inversion is accurate norm-wise only.
// Cost per point: 8 n^3 real flops (n^3 complex multiply-adds; the real embedding of freq_response does 16 n^3), half as many panels of
// half the height, and 2 n^2 doubles for the matrix instead of 4 n^2.  Failures, masks, chunks and the bit-for-bit independence of a
// member are freq_response's: both run on the one driver of freq_sweep.hpp.
#pragma once
#include <vector>

#include "freq_response.hpp"

namespace dre {

// ERR_INVALID before any launch: no systems, K < 1, a non-finite sigma or omega, mismatched shapes, n > GJ_REGISTER_MAX_N, chunk < 0 or
// > 65535.  ERR_ALLOC before any launch: the chunk (chunk = 0: even one member) does not fit the free device memory.
FreqResponse transfer_eval(Ctx* ctx, const std::vector<FreqSystem>& sys, const std::vector<double>& s_re, const std::vector<double>& s_im,
                           int chunk /* 0 = auto */);

}  // namespace dre
