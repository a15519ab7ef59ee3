// Batched complex Gauss-Jordan inversion on planar storage (dense_cgj.hpp): the register panel of dense_cgj_body.hpp per
// member and panel, the interchanges, and one real rank-2kb update per panel on gemm_strided.  A translation unit of its own: the eight
// panel instantiations take minutes to compile.
#include "dense_cgj.hpp"

#include "dense.hpp"
#include "dense_cgj_body.hpp"
#include "profiling.hpp"

namespace dre {

// member b = blockIdx.x: planes at Z + b 2 n^2 and Z + b 2 n^2 + n^2
template <int NB, int R>
__global__ __launch_bounds__(GJ_THREADS) void k_bcgj_panel(int n, int k, int kb, double* __restrict__ Z, double* __restrict__ Pt,
                                                           int* __restrict__ piv, BatchCtl* ctl, int mode) {
    const int b = blockIdx.x;
    if (batch_off(BatchMask{ctl, mode, 0}, b)) return;
    const size_t nn = (size_t)n * n;
    double* Zr = Z + (size_t)b * 2 * nn;
    cgj_panel_body<NB, R>(n, k, kb, Zr, Zr + nn, n, Pt + (size_t)b * n * 2 * NB, piv + (size_t)b * n, &ctl[b].s.gj);
}

__global__ __launch_bounds__(256) void k_bcgj_swap(int n, int k, int kb, int nb, double* __restrict__ Z, const int* __restrict__ piv,
                                                   double* __restrict__ Wt, const BatchCtl* ctl, int mode) {
    const int b = blockIdx.y;
    if (batch_off(BatchMask{ctl, mode, 0}, b)) return;
    const size_t nn = (size_t)n * n;
    double* Zr = Z + (size_t)b * 2 * nn;
    cgj_swap_body(n, k, kb, nb, Zr, Zr + nn, n, piv + (size_t)b * n, Wt + (size_t)b * 4 * nb * n, &ctl[b].s.gj);
}

__global__ __launch_bounds__(256) void k_bcgj_unpivot(int n, double* __restrict__ Z, const int* __restrict__ piv, const BatchCtl* ctl, int mode) {
    const int b = blockIdx.y;
    if (batch_off(BatchMask{ctl, mode, 0}, b)) return;
    const size_t nn = (size_t)n * n;
    double* Zr = Z + (size_t)b * 2 * nn;
    cgj_unpivot_body(n, Zr, Zr + nn, n, piv + (size_t)b * n, &ctl[b].s.gj);
}

__global__ void k_bcgj_reset(int batch, BatchCtl* ctl) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch || ctl[b].fail) return;
    ctl[b].s.gj.logdet = 0.0;
    ctl[b].s.gj.singular = 0;
}

int cgj_batch_nb(int n) {
    const int R = ceil_div(n, GJ_THREADS);
    return R <= 1 ? 32 : (R <= 3 ? 16 : (R <= 5 ? 8 : 4));
}

template <int NB, int R>
static void launch_cpanel(Ctx* ctx, int batch, int n, int k, int kb, double* Z, double* Pt, int* piv, BatchCtl* ctl, int mode) {
    hipLaunchKernelGGL((k_bcgj_panel<NB, R>), dim3(batch), dim3(GJ_THREADS), 0, ctx->stream, n, k, kb, Z, Pt, piv, ctl, mode);
}

void cgj_invert_batched(Ctx* ctx, int batch, int n, double* Z, int* piv, BatchCtl* ctl, int mode, double* Pt, double* Wt) {
    DRE_REQUIRE(n >= 1 && n <= GJ_REGISTER_MAX_N, "complex dense path: the register panel inverts matrices of order 1 .. " +
                                                      std::to_string(GJ_REGISTER_MAX_N) + ", order = " + std::to_string(n));
    DRE_REQUIRE(batch >= 1 && batch <= 65535, "complex dense path: batch must be in 1 .. 65535");
    mode |= BM_GJ;
    const int R = ceil_div(n, GJ_THREADS), nb = cgj_batch_nb(n);
    const size_t nn = (size_t)n * n;
    const BatchMask mask{ctl, mode, 0};
    hipLaunchKernelGGL(k_bcgj_reset, dim3(ceil_div(batch, 256)), dim3(256), 0, ctx->stream, batch, ctl);
    for (int k = 0; k < n; k += nb) {
        const int kb = std::min(nb, n - k);
        {
            TimedScope ts(ctx, "batch_cgj_panel", 32.0 * batch * n * kb, 8.0 * batch * n * kb * kb);
            switch (R) {
                case 1: launch_cpanel<32, 1>(ctx, batch, n, k, kb, Z, Pt, piv, ctl, mode); break;
                case 2: launch_cpanel<16, 2>(ctx, batch, n, k, kb, Z, Pt, piv, ctl, mode); break;
                case 3: launch_cpanel<16, 3>(ctx, batch, n, k, kb, Z, Pt, piv, ctl, mode); break;
                case 4: launch_cpanel<8, 4>(ctx, batch, n, k, kb, Z, Pt, piv, ctl, mode); break;
                case 5: launch_cpanel<8, 5>(ctx, batch, n, k, kb, Z, Pt, piv, ctl, mode); break;
                case 6: launch_cpanel<4, 6>(ctx, batch, n, k, kb, Z, Pt, piv, ctl, mode); break;
                case 7: launch_cpanel<4, 7>(ctx, batch, n, k, kb, Z, Pt, piv, ctl, mode); break;
                default: launch_cpanel<4, 8>(ctx, batch, n, k, kb, Z, Pt, piv, ctl, mode); break;
            }
            hipLaunchKernelGGL(k_bcgj_swap, dim3(ceil_div(n, 256), batch), dim3(256), 0, ctx->stream, n, k, kb, nb, Z, (const int*)piv, Wt,
                               (const BatchCtl*)ctl, mode);
        }
        // one real rank-2kb update of all 2n columns of [Zr | Zi]: the panel's columns of Wt are zero
        gemm_strided(ctx, batch, false, false, n, 2 * n, 2 * kb, 1.0, Pt, n, (size_t)n * 2 * nb, Wt, 2 * nb, (size_t)4 * nb * n, 1.0, Z, n, 2 * nn, mask,
                     "batch_cgj_update");
    }
    {
        TimedScope ts(ctx, "batch_cgj_unpivot", 32.0 * batch * n * n, 0.0);
        hipLaunchKernelGGL(k_bcgj_unpivot, dim3(ceil_div(n, 256), batch), dim3(256), 0, ctx->stream, n, Z, (const int*)piv, (const BatchCtl*)ctl, mode);
    }
    DRE_HIP(hipGetLastError());
}

}  // namespace dre
