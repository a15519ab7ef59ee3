// In-place complex Gauss-Jordan inversion with row pivoting on a stack of planar complex matrices (dense_cgj.hip).
// Layout: a member is two adjacent n x n real planes [Zr | Zi], ld n, member stride 2 n^2: at the same time an n x 2n real matrix, so that
// the rank-kb trailing update of a complex Gauss-Jordan step is ONE real product on gemm_strided,
//   [Cr | Ci] += [Pr | Pi] [[Wr, Wi], [-Wi, Wr]]        (n x 2kb) (2kb x 2n),
// with exactly the complex flop count (8 n^2 kb) and C read once.
#pragma once
#include "dense_batch.hpp"
#include "dense_gj.hpp"

namespace dre {

// width of the complex register panel at order n: R = ceil(n / 512) rows per thread in two planes, R x nb complex numbers per thread
// (no scratch in any instantiation).  fr_panel_nb_c of freq_chunk.hpp is the same table.
int cgj_batch_nb(int n);

// Stack of n x n complex inverses in place with the register panel (1 <= n <= GJ_REGISTER_MAX_N, batch <= 65535): member b's planes at
// Z + b 2 n^2, its interchanges in piv + b n, log|det| and the singular flag in ctl[b].s.gj.  Ptilde (n x 2nb per member, ld n) and Wtilde
// (2nb x 2n per member, ld 2nb) are work stacks of batch * 2 n nb and batch * 4 n nb doubles, nb = cgj_batch_nb(n).  A member that the mask
// leaves out, or whose inversion met an exactly zero or non-finite pivot, is left alone from there on.  No synchronisation.
void cgj_invert_batched(Ctx* ctx, int batch, int n, double* Z, int* piv, BatchCtl* ctl, int mode, double* Ptilde, double* Wtilde);

}  // namespace dre
