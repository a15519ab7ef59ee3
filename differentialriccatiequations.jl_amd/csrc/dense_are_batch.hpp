// Batched dense GARE solver (dense_are_batch.hip): dense_gare_solve's algorithm (dense_are.hip) on the stacks of dense_batch.hpp, B
// Riccati equations of one (n, m, q) in one chain of shared launches, member b on a grid axis.  See DESIGN.md §9.4.
#pragma once
#include <vector>

#include "dense_are.hpp"
#include "dense_batch.hpp"

namespace dre {

// The words of AreCtl (dense_are.hip) that BatchCtl does not have, one per member, behind the B BatchCtl blocks in one device allocation
// (all 2 B blocks come back in one copy).  BatchCtl carries the rest: s.gj (the inversion), s.done (0 running, 1 converged, 2 stagnated,
// 3 non-finite, 4 singular Z_k, 5 out of maxiters), s.step, s.res (the accepted iterate's scaled residual), logdetE, res0, fail, iters,
// scale, refine (another Newton-Kleinman step is due), nref.
struct AreBatchCtl {
    double best;        // smallest relative step so far
    double resnorm;     // ||R||_F of the last residual evaluation
    double cand;        // scaled residual of the last residual evaluation (the candidate's, in the refinement)
    int since;          // unscaled iterations since the last new minimum of the step
    int accept;         // the last refinement step decreased the residual: the candidate replaces X
};

// Q_b + A_b'X_b E_b + E_b'X_b A_b - E_b'X_b G_b X_b E_b = 0 for b < batch, G_b = B_b Rinv_b B_b', Q_b = Ct_b S_b Ct_b'.  Stacks: E, A n x n*B;
// Bm n x m*B; Ct n x q*B; Rinv m x m*B and S q x q*B or null (identity for every member).  2n <= GJ_REGISTER_MAX_N.  No member's failure
// throws: status[b] gets the code and a message that names the member, the member is dropped from every later launch and the others go
// on.  out[b].X is empty for a failed member.  Throws Error(ERR_INVALID) on argument errors and Error(ERR_ALLOC) from the up-front memory
// check, before any kernel.
void dense_gare_solve_batched(Ctx* ctx, int batch, const Mat& E, const Mat& A, const Mat& Bm, const Mat* Rinv, const Mat& Ct, const Mat* S, int m,
                              int q, int maxiters, double tol, int max_refine, std::vector<DenseGareResult>& out,
                              std::vector<BatchMemberStatus>& status);
// device memory of that call in doubles, the operand stacks included (the formula of DESIGN.md §9.4)
size_t dense_gare_batched_doubles(int batch, int n, int m, int q, int maxiters, int max_refine);

}  // namespace dre
