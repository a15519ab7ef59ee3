// Device SVD: one-sided (Hestenes) block Jacobi, Gram and update products on v_mfma_f64_16x16x4_f64 (svd_jacobi.hip).  See DESIGN.md §9.8; the
// host model of exactly this iteration is tests/_svd_jacobi_model.py.
//
// Accuracy contract: norm-wise, like a LAPACK driver — errors of order eps sigma_1 in the singular values, the residual and the orthogonality
// of U (over the columns kept) and V.  There is NO claim of high relative accuracy for tiny singular values: the Gram matrix of every block
// pair is formed explicitly.
#pragma once
#include "dense.hpp"

namespace dre {

constexpr int SVJ_MAX_SWEEPS = 60;      // block sweeps before DRE_ERR_INTERNAL (the cap of host_svd_left)
constexpr int SVJ_MAX_W = 4096;         // the shorter dimension at most
constexpr int SVJ_SLAB = 64;            // rows of a slab staged through LDS

// Device-side control block (shaped like BjCtl), one per member: written only by the one-workgroup-per-member init kernel at the entry and
// fold kernel after every sweep, read by the kernels enqueued after them on the same stream and read back once per sweep.
struct SvjCtl {
    double norm;       // ||A||_F
    double pad0_;
    int sweeps;        // block sweeps done
    int done;          // the last sweep rotated nothing
    int nonfinite;     // ||A||_F is not finite
    int failed;        // SVJ_MAX_SWEEPS sweeps with rotations
};

struct SvjStats { long sweeps = 0, rounds = 0, rank = 0; };

struct SvdResult {
    Mat U, S, V;       // U m x k, S k x 1 (descending), V w x k with k = min(m, w):  A ~ U diag(S) V'
    std::vector<double> s;   // S on the host
    double norm = 0.0;       // ||A||_F
};

// A (m x w, left untouched; min(m, w) <= SVJ_MAX_W, max(m, w) <= DENSE_MAX_N).  tol <= 0: sqrt(max(m, w)) eps.  A column pair (r, c) counts as
// orthogonal when |g_r'g_c| <= tol ||g_r|| ||g_c||, and pairs with ||g_r|| ||g_c|| <= (tol ||A||_F)^2 are left alone.  The columns of U (of V for
// a wide input) that belong to sigma <= tol ||A||_F are zero columns; stats->rank counts the others.  DRE_ERR_INVALID for a non-finite A or a shape beyond the
// limits (before any launch), DRE_ERR_ALLOC from the memory check (before any launch), DRE_ERR_INTERNAL after SVJ_MAX_SWEEPS sweeps.
SvdResult svd_jacobi(Ctx* ctx, const Mat& A, double tol = 0.0, SvjStats* stats = nullptr);

}  // namespace dre
