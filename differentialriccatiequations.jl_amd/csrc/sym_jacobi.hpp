// Whole-device symmetric eigensolver: two-sided cyclic block Jacobi on v_mfma_f64_16x16x4_f64 (sym_jacobi.hip).  See DESIGN.md §9.6; the host
// model of exactly this iteration is tests/_block_jacobi_model.py.
#pragma once
#include "dense.hpp"

namespace dre {

constexpr int BJ_BLOCK = 16;          // block size b; a pivot block is 2 b x 2 b
constexpr int BJ_MAX_SWEEPS = 30;     // block sweeps before DRE_ERR_INTERNAL

// Device-side control block, one per member: written only by the one-workgroup-per-member decide kernel after every sweep, read by the kernels
// enqueued after it on the same stream and read back once per sweep.
struct BjCtl {
    double off;        // off(A) = Frobenius norm of the off-diagonal part
    double norm;       // ||A||_F
    int sweeps;        // block sweeps done
    int done;          // off <= tol * norm
    int nonfinite;     // ||A||_F is not finite
    int failed;        // BJ_MAX_SWEEPS sweeps without convergence
};

struct BjStats { long sweeps = 0, rounds = 0; };

// padded order: a multiple of the block size, at least two blocks (a single block has no partner to be diagonalised with)
inline int bj_padded_order(int q) { const int p = (q + BJ_BLOCK - 1) / BJ_BLOCK; return (p < 2 ? 2 : p) * BJ_BLOCK; }

// Eigen-decomposition of the symmetric q x q matrix S (full storage, left untouched) in the form sym_eig returns: j = q, nref = 0, Z the q x q
// eigenvectors, w the eigenvalues on the host (unsorted, column i of Z belongs to w[i]), snorm = ||S||_F.  tol <= 0: q eps.  Converged when
// off(A) <= tol ||A||_F.  DRE_ERR_INVALID for a non-finite S, DRE_ERR_INTERNAL after BJ_MAX_SWEEPS sweeps.
// An entry whose square overflows (|a| above about 1e154) makes the norm non-finite and is reported as DRE_ERR_INVALID like a NaN or an infinity.
SymEig sym_eig_jacobi(Ctx* ctx, const Mat& S, double tol = 0.0, BjStats* stats = nullptr);

// Diagnostic: with the environment variable DRE_SYM_EIG_DUMP=<directory> set, every matrix that reaches sym_eig(..., want_eig = true) is written to
// <directory>/S_<count>_<order>.f64 (column-major doubles, synchronising) before it is diagonalised, so that tools/time_sym_eig.py can time the
// eigensolvers on the matrices the compressions really see.  Unset: nothing happens.
void sym_eig_dump_input(Ctx* ctx, const Mat& S);

}  // namespace dre
