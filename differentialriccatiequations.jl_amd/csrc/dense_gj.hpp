// In-place Gauss-Jordan inversion with row pivoting (dense_gj.hip), and the small host-side helpers that the dense sign-function family
// (dense_sign.hip, dense_sign_lr.hip, dense_are.hip, dre_dense_invert of api_dense.hip) shares.  See DESIGN.md, "Dense path".
#pragma once
#include <algorithm>
#include <limits>

#include "common.hpp"

namespace dre {

// Order limits of the dense path.  DENSE_MAX_N is the index limit: every device kernel the dense path launches (dense_gj.hip, dense_sign.hip, the
// element-wise copies and norms of dense.hip, the GEMM family of gemm.hip) forms element offsets inside an n x n operand either in size_t or as an int
// row / column index below n, and every int product it forms (row + col * ld of the n x n, n x nb and nb x n operands, the
// k * n column offset of a stored P_k) stays below 2^31 - 1 while n <= 46340 = floor(sqrt(2^31 - 1)).  Below that limit the device memory
// decides (require_memory).  GJ_REGISTER_MAX_N is the limit of the register panel, which keeps ceil(n / 512) rows per thread in registers
// (dense_gj_panel = 1 refuses larger n; the default 0 switches to the tournament panel above it).
#define DENSE_MAX_N 46340
#define GJ_REGISTER_MAX_N 4096

// Device-side control words of the inversion (a caller that needs them reads them back: read_back).
struct GjCtl {
    double logdet;      // log |det| of the last inverted matrix (sum of log |pivot|)
    int singular;       // the inversion met an exactly zero (or non-finite) pivot column
};

// A <- inv(A) in place (n x n, n <= DENSE_MAX_N); ctl->logdet = log|det A|, ctl->singular set on a zero pivot; piv[0..n) the row interchanges
// (LAPACK style: row j was swapped with row piv[j] >= j).  The panel follows ctx->dense_gj_panel (0 auto, 1 register, 2 tournament; the
// tournament panel's width is 32).  No synchronisation.
void gj_invert(Ctx* ctx, Mat& A, int* piv_dev, GjCtl* ctl_dev);

// DRE_ERR_INVALID when the context insists on the register panel (dense_gj_panel = 1) and the order of the matrices `who` will invert is beyond it
void gj_check_order(const Ctx* ctx, int order, const char* who);

// DRE_ERR_ALLOC unless `doubles` doubles fit in the free device memory plus the pool's released buffers (no allocation, no kernel)
void require_memory(Ctx* ctx, size_t doubles);

constexpr double DBL_EPS = std::numeric_limits<double>::epsilon();
constexpr int NORM_PARTS = 256;      // workgroups of the fused element-wise + partial-norm kernels (dense_device.hpp: store_partials, load_partials)

// grid of an element-wise kernel with a grid-stride loop: 256 threads per workgroup, at most 1024 workgroups
inline unsigned grid_for(size_t tot) { return (unsigned)std::max<size_t>(1, std::min<size_t>(1024, (tot + 255) / 256)); }

// one object from the device to the host, behind everything enqueued on the context's stream (synchronising)
template <class T>
T read_back(Ctx* ctx, const T* dev) {
    T h;
    DRE_HIP(hipMemcpyAsync(&h, dev, sizeof(T), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    return h;
}

}  // namespace dre
