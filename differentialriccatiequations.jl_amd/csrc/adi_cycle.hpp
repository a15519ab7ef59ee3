// Operator products of a real Cyclic shift list on the dense-inverse path (adi_cycle.hip): what the dense-X time step (dense_x.hip) sets up
// on its side stream — the SMW products and packed stacks of every shift, and the group chain's K-independent base and per-step fold.
#pragma once
#include <complex>
#include <functional>
#include <memory>
#include <vector>

#include "engine.hpp"
#include "engine_internal.hpp"

namespace dre {

// SMW products of every shift of a real Cyclic list for the low-rank factor (U, Vt) of `op`, and the SMW-folded packed stacks of the
// fast chain (dense.hip).  Factors, dense inverses and stacked inverses come from the cache (built on first use).
struct CycleOps {
    std::vector<const double*> wks_pos; // per position of the cycle: [N K' Sinv; E'N K' Sinv] (2n x m, leading dimension 2n) of its shift, or null (no low-rank part)
    std::vector<const double*> gpack;   // group chain: packed group stack per start position (index = start / g), empty = not available
    int group_g = 0;
    bool single_built = true;           // the single-iteration packed stacks (k_adi_fast) exist; false: build_single makes them on demand
    std::function<void(Ctx*)> build_single;
    std::vector<double*> pack;          // per position of the cycle
    std::vector<std::shared_ptr<FactorEntry<double>>> fe;
    std::vector<Mat> keep;
    std::vector<BufP> keepb;
    DevArr<int> serr;
    DevArr<long long> serr8;      // the breakdown flag as an 8-byte word (read back together with the control block)
};
// false: some shift cannot take the dense-inverse path (complex, or its inverse was rejected by the condition estimate)
bool cycle_ops_prepare(Ctx* ctx, const GaleOperator& op, const std::vector<std::complex<double>>& values, FactorCache* cache, CycleOps& co,
                       std::vector<Mat>* wks_store = nullptr /* persistent 2n x m buffers per position of the cycle (group chain) */,
                       const std::vector<Mat>* spack = nullptr /* packed stacks per position (group chain): thin products without k_gemm */,
                       bool defer_single = false /* the single-iteration packs are only needed by a fallback chunk: build on demand */);

// ---- group chain (dense.hip, k_adi_group): see adi_cycle.hip for the algebra ----
struct GroupLeftDesc { const double* Mtx; int ldm; const double* v; int ldv; double* out; int ldo; double scale; int kind; int pad; };   // kind 0: out = scale Mtx v (null Mtx: copy), 1: M = scale v' PsiT'
struct GroupBase {
    int g = 0, n = 0, m = 0;
    uint64_t tag = 0;
    std::vector<double> mus;            // the cycle this base was built for
    std::vector<int> starts;            // start positions (multiples of g)
    std::vector<Mat> G0;                // per start: (2 g n) x n  rows [i n, (i+1) n) = Om0_i, rows [(g + i) n, ...) = Pi0_{i+1}
    std::vector<Mat> D;                 // per start: (g m) x n    rows [i m, (i+1) m) = D_i
    std::vector<Mat> spack;             // per position of the cycle: stack_s = [N_s; E'N_s; B'N_s] in the MFMA A-operand order
    std::vector<Mat> wks;               // persistent [N K' Sinv; E'N K' Sinv] per position of the cycle (2n x m): the descriptors point into them
    std::vector<Mat> XL, Yt, Mb;        // per start: left factors (2 g n) x (m g), Y' (m g) x n, the M(j, i) blocks (m x m each, g*g slots)
    std::vector<Mat> pack;              // packed effective group stacks
    DevArr<GroupLeftDesc> table;        // descriptors of the left-factor launch (built once per run)
    std::vector<GroupLeftDesc> host_table;
    int ndesc = 0;
};
int group_size_for(Ctx* ctx, int ncycle, int n, int m);
// K-independent part, once per run (every shift of the cycle has its stacked inverse)
void group_base_build(Ctx* ctx, const GaleOperator& op, const std::vector<std::complex<double>>& values, const CycleOps& co, GroupBase& gb, int g);
// K-dependent part, once per time step (side stream): copies, g - 1 thin levels, the rows of Y, fold + packing
void group_ops_prepare(Ctx* ctx, const std::vector<std::complex<double>>& values, CycleOps& co, GroupBase& gb);

}  // namespace dre
