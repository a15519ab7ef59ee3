// Ros1 with X carried as a dense symmetric n x n matrix between the time steps (dense_x.hip): what the driver (gdre.hip) needs of it.
#pragma once
#include <memory>

#include "engine.hpp"
#include "side_worker.hpp"

namespace dre {

// the context's parked thread number `slot` (created on first use, joined when the context goes)
SideWorker& parked_worker(Ctx* ctx, int slot);

// State of one run.  Its destructor joins what the parked thread still does for the run (the deferred group base of the first dense step, a
// prefetched side set-up) and the side stream behind it: declare it behind everything the steps were given by reference (options, factor cache).
struct DenseXState;
std::shared_ptr<DenseXState> dense_x_new(Ctx* ctx, SideWorker* worker);
// the current X (X0, or a block list: warm start + increments) as a dense matrix, with its feedback K' and the first solve's iteration hint
void dense_x_start(Ctx* ctx, const GdreProblem& prob, DenseXState& sx, const LDLt& X, const Mat& Kt, int hint);
// One Ros1 step on the dense state.  Returns false (state untouched) when the fast chain cannot take the step.
bool ros1_dense_step(Ctx* ctx, const GdreProblem& prob, const GaleOperator& op_base, double tau, const AdiOptions& adi, FactorCache* cache, DenseXState& sx,
                     AdiResult& ar, bool more_steps);
const Mat& dense_x_X(const DenseXState& sx);
const Mat& dense_x_Kt(const DenseXState& sx);      // K' = E' X B of the last step
void dense_x_report(DenseXState& sx);              // the trace switches' end-of-run lines
// the last X of a run for the result: kept dense and factored on demand (final_x_lazy; returns null), or factored here
LDLtP dense_x_final(Ctx* ctx, DenseXState& sx, double ctf, bool steps_on, GdreResult& out);
// LDL' form of a dense symmetric X: compress!(lowrank(I, X))  (LDLt.jl:204-225; S = I X I' is X itself)
LDLtP dense_to_ldlt(Ctx* ctx, int n, const Mat& Xd, double ctf);

}  // namespace dre
