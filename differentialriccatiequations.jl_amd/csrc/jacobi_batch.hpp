// Member-indexed block Jacobi: the symmetric eigensolver of sym_jacobi.hip and the SVD of svd_jacobi.hip for an ensemble of same-size problems in
// shared launches (jacobi_batch.hip).  See DESIGN.md §9.9.  Member b sits on the grid's y axis; a workgroup of member b does that member's
// arithmetic of the single solver in the same order, so every output of a member is bit for bit what the single call returns for it, whatever
// the other members are.  A member that is finished, non-finite or out of sweeps is skipped by every later launch (its workgroups return at
// entry); the others go on.
#pragma once
#include <string>
#include <vector>

#include "dense_batch.hpp"
#include "svd_jacobi.hpp"
#include "sym_jacobi.hpp"

namespace dre {

constexpr int JACOBI_BATCH_MAX = 65535;      // members at most (the grid's y axis)

// Device-side control blocks, one per member: BjCtl / SvjCtl with the padding word used for "out of sweeps".  ctl[b] is written only by the
// one-workgroup-per-member decide / init / fold kernels and read by the kernels enqueued after them on the same stream.
struct BjbCtl {
    double off, norm;
    int sweeps, done, nonfinite, failed;     // failed: BJ_MAX_SWEEPS sweeps without convergence
};
struct SvjbCtl {
    double norm, pad0_;
    int sweeps, done, nonfinite, failed;     // failed: SVJ_MAX_SWEEPS sweeps with rotations
};

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

}  // namespace dre
