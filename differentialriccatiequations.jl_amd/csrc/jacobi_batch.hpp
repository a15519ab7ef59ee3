// Block Jacobi for an ensemble of same-size problems in shared launches: the batch types and entry points of the symmetric eigensolver
// (sym_jacobi.hip) and of the SVD (svd_jacobi.hip).  See DESIGN.md §9.9.  There is one kernel set: member b sits on the grid's y axis, and
// sym_eig_jacobi / svd_jacobi are batches of one, so every output of a member is bit for bit what the single call returns for it, whatever the
// other members are.  A member that is finished, non-finite or out of sweeps is skipped by every later launch (its workgroups return at
// entry); the others go on.
#pragma once
#include <string>
#include <vector>

#include "dense_batch.hpp"
#include "svd_jacobi.hpp"
#include "sym_jacobi.hpp"

namespace dre {

constexpr int JACOBI_BATCH_MAX = 65535;      // members at most (the grid's y axis)

struct SymEigBatch {
    std::vector<SymEig> eig;                 // per member what sym_eig_jacobi returns (empty for a failed member)
    std::vector<BjStats> stats;
    std::vector<BatchMemberStatus> status;   // code 0, DRE_ERR_INVALID (non-finite) or DRE_ERR_INTERNAL (no convergence), with the message
};

struct SvdBatch {
    std::vector<SvdResult> svd;              // per member what svd_jacobi returns (empty for a failed member); U, S, V are views of shared stacks
    std::vector<SvjStats> stats;
    std::vector<BatchMemberStatus> status;
};

// S[b]: symmetric q x q, one q for all members (left untouched).  tol <= 0: q eps.  Limits (1 <= batch <= 65535, equal shapes, the single
// call's order limit) and the memory check come before any launch (DRE_ERR_INVALID / DRE_ERR_ALLOC of the call).  who: prefix of the messages.
SymEigBatch sym_eig_jacobi_batch(Ctx* ctx, const std::vector<Mat>& S, double tol = 0.0, const char* who = "sym_eig_jacobi_batch");

// A[b]: one shape for all members (left untouched), the limits of svd_jacobi.  tol <= 0: sqrt(max(m, w)) eps.  The rotation rule, floor, sweep
// caps, zero-column rule and numerical rank are per member, exactly those of svd_jacobi.
SvdBatch svd_jacobi_batch(Ctx* ctx, const std::vector<Mat>& A, double tol = 0.0, const char* who = "svd_jacobi_batch");

// The driver behind svd_jacobi (single) and svd_jacobi_batch, for a caller that words the failures itself: status[b].msg is only the "what"
// of a member's failure, without "who" and the member's number.  single: the kernel-timer tags and the trace line of svd_jacobi.
SvdBatch svd_jacobi_run(Ctx* ctx, const std::vector<Mat>& A, double tol, const char* who, bool single);

}  // namespace dre
