// Frequency response of dense descriptor systems (freq_response.hip):  H(i w) = C (i w E - A)^-1 B  for K frequencies of
// one or several systems of one (n, m, q), the frequency on the member axis of the batched dense path (dense_batch.hpp).
//
// Method, per member (s, k) = system s at frequency w_k, member index s K + k:
//   1. k_fr_assemble writes the real form of i w E - A, the 2n x 2n matrix  M = [[-A, -w E], [w E, -A]];
//   2. gj_invert_batched inverts the stack in place (register panel: 2n <= GJ_REGISTER_MAX_N);
//   3. gemm_strided forms  Y = M^-1[:, 0:n] B  (2n x m):  (i w E - A)(Y[0:n] + i Y[n:2n]) = B;
//   4. one refinement step:  R = [B; 0] - M Y = [B + A Yr + w E Yi; A Yi - w E Yr]  from E and A (four strided GEMMs on the shared operands,
//      w per member from a device array), then  Y += M^-1 R.  M itself is not kept;
//   5. gemm_strided forms  Re H = C Y[0:n]  and  Im H = C Y[n:2n].
// Why the refinement step: the blocked inversion (rank-nb trailing updates) is accurate norm-wise, errors of order eps |M^-1| everywhere in
// M^-1.  Where the response has decayed, H = C M^-1 B is small beside |C| |M^-1| |B| and inherits that absolute error: at n = 371 and w = 1e3
// (|H| / (|C| |M^-1| |B|) = 1e-2, cond = 15) the unrefined H is off by 9e-13 relative, where a complex LU solve and numpy.linalg.inv (an LU with
// triangular solves, which keeps small entries small) give 4e-16.  One step with the residual in working precision brings it to 1e-15; it
// costs 16 n^2 m flops per frequency beside the inversion's 16 n^3.  On well-scaled responses it changes the result by less than the spread
// between the embedding inverse and a complex LU solve (both track cond * eps), so a second step buys nothing.
//
// Why the real embedding and not the n x n Schur form  A + w^2 E A^-1 E = (A - i w E) A^-1 (A + i w E):  that form is 8 x cheaper and would
// reach n <= 4096, but its condition number is about that of i w E - A SQUARED, and it needs a regular A.  The known cost of the embedding is
// 16 n^3 flops per frequency (2 (2n)^3); a native complex Gauss-Jordan panel would need a quarter of that.
//
// E may be singular (descriptor systems of index 1 and above): nothing here inverts E, unlike the sign-function entry points.  A member whose
// i w E - A is singular (w on a pole; exactly zero or non-finite pivot, a NaN in its system) gets ERR_SINGULAR in its status and NaN in its H;
// the other members go on.  A member's result is bit for bit independent of the other members and of the chunk it falls in.
// Validation, chunk plan, chunk loop, read-backs and per-member status are the driver's that transfer_eval shares (freq_sweep.hpp).
#pragma once
#include <vector>

#include "dense_batch.hpp"
#include "freq_chunk.hpp"

namespace dre {

struct FreqSystem { Mat E, A, B, C; };     // E, A: n x n; B: n x m; C: q x n

struct FreqResponse {
    std::vector<double> re, im;            // q x m per member, column-major, member-major
    std::vector<BatchMemberStatus> status; // per member
    int chunk = 0;                         // members per chunk
    int chunks = 0;
};

// ERR_INVALID before any launch: no systems, K < 1, a non-finite frequency, mismatched shapes, 2n > GJ_REGISTER_MAX_N, chunk < 0 or > 65535.
// ERR_ALLOC before any launch: the chunk (chunk = 0: even one member) does not fit the free device memory.
FreqResponse freq_response(Ctx* ctx, const std::vector<FreqSystem>& sys, const std::vector<double>& omega, int chunk /* 0 = auto */);

}  // namespace dre
