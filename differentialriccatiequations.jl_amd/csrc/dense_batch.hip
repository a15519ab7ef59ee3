// Batched dense path: B independent problems of one order n in shared launches, member b on a grid axis.
//   gj_invert_batched        the register-panel Gauss-Jordan inversion of dense_gj.hip on a stack (the bodies are dense_gj_body.hpp's, shared with dense_gj.hip);
//   BatchedSignLyap          SignLyap on a stack of pencils, the iteration's decisions taken per member on the device (the element-wise bodies
//                            and the stopping rule are dense_sign_body.hpp's, shared with dense_sign.hip);
//   dense_gdre_solve_batched Ros1 / Ros2 on stacks: the stage program of dense_ros.hpp behind a stack back end, and what is this driver's own.
// The strided MFMA GEMM is gemm_strided of gemm.hip.  A member's arithmetic never looks at B, at its position or at another member's data.
#include "dense_batch.hpp"

#include <cmath>

#include "dense.hpp"
#include "dense_gj_body.hpp"
#include "dense_ros.hpp"
#include "dense_sign_body.hpp"
#include "profiling.hpp"

namespace dre {

// ---- inversion ---------------------------------------------------------------------------------------------------------------------
template <int NB, int R>
__global__ __launch_bounds__(GJ_THREADS) void k_bgj_panel(int n, int k, int kb, double* __restrict__ A, double* __restrict__ Pn,
                                                          int* __restrict__ piv, BatchCtl* ctl, int mode) {
    const int b = blockIdx.x;
    if (batch_off(BatchMask{ctl, mode, 0}, b)) return;
    gj_panel_body<NB, R>(n, k, kb, A + (size_t)b * n * n, n, Pn + (size_t)b * n * NB, piv + (size_t)b * n, &ctl[b].s.gj);
}

__global__ __launch_bounds__(256) void k_bgj_swap(int n, int k, int kb, int nb, double* __restrict__ A, const int* __restrict__ piv,
                                                  double* __restrict__ W, const BatchCtl* ctl, int mode) {
    const int b = blockIdx.y;
    if (batch_off(BatchMask{ctl, mode, 0}, b)) return;
    gj_swap_body(n, k, kb, nb, A + (size_t)b * n * n, n, piv + (size_t)b * n, W + (size_t)b * nb * n, &ctl[b].s.gj, 0);
}

__global__ __launch_bounds__(256) void k_bgj_unpivot(int n, double* __restrict__ A, const int* __restrict__ piv, const BatchCtl* ctl, int mode) {
    const int b = blockIdx.y;
    if (batch_off(BatchMask{ctl, mode, 0}, b)) return;
    gj_unpivot_body(n, A + (size_t)b * n * n, n, piv + (size_t)b * n, &ctl[b].s.gj);
}

__global__ void k_bgj_reset(int batch, BatchCtl* ctl) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch || ctl[b].fail) return;
    ctl[b].s.gj.logdet = 0.0;
    ctl[b].s.gj.singular = 0;
}

int gj_batch_nb(int n) {
    const int R = ceil_div(n, GJ_THREADS);
    return R <= 3 ? 32 : (R <= 5 ? 16 : 8);          // the table of gj_invert_register
}

template <int NB, int R>
static void launch_bpanel(Ctx* ctx, int batch, int n, int k, int kb, double* A, double* Pn, int* piv, BatchCtl* ctl, int mode) {
    hipLaunchKernelGGL((k_bgj_panel<NB, R>), dim3(batch), dim3(GJ_THREADS), 0, ctx->stream, n, k, kb, A, Pn, piv, ctl, mode);
}

void gj_invert_batched(Ctx* ctx, int batch, int n, double* A, int* piv, BatchCtl* ctl, int mode, double* Pn, double* W) {
    DRE_REQUIRE(n >= 1 && n <= GJ_REGISTER_MAX_N, "batched dense path: the register panel inverts matrices of order 1 .. " +
                                                      std::to_string(GJ_REGISTER_MAX_N) + ", order = " + std::to_string(n));
    DRE_REQUIRE(batch >= 1 && batch <= 65535, "batched dense path: batch must be in 1 .. 65535");
    mode |= BM_GJ;
    const int R = ceil_div(n, GJ_THREADS), nb = gj_batch_nb(n);
    const size_t nn = (size_t)n * n;
    const BatchMask mask{ctl, mode, 0};
    hipLaunchKernelGGL(k_bgj_reset, dim3(ceil_div(batch, 256)), dim3(256), 0, ctx->stream, batch, ctl);
    for (int k = 0; k < n; k += nb) {
        const int kb = std::min(nb, n - k);
        {
            TimedScope ts(ctx, "batch_gj_panel", 16.0 * batch * n * kb, 2.0 * batch * n * kb * kb);
            switch (R) {
                case 1: launch_bpanel<32, 1>(ctx, batch, n, k, kb, A, Pn, piv, ctl, mode); break;
                case 2: launch_bpanel<32, 2>(ctx, batch, n, k, kb, A, Pn, piv, ctl, mode); break;
                case 3: launch_bpanel<32, 3>(ctx, batch, n, k, kb, A, Pn, piv, ctl, mode); break;
                case 4: launch_bpanel<16, 4>(ctx, batch, n, k, kb, A, Pn, piv, ctl, mode); break;
                case 5: launch_bpanel<16, 5>(ctx, batch, n, k, kb, A, Pn, piv, ctl, mode); break;
                case 6: launch_bpanel<8, 6>(ctx, batch, n, k, kb, A, Pn, piv, ctl, mode); break;
                case 7: launch_bpanel<8, 7>(ctx, batch, n, k, kb, A, Pn, piv, ctl, mode); break;
                default: launch_bpanel<8, 8>(ctx, batch, n, k, kb, A, Pn, piv, ctl, mode); break;
            }
            hipLaunchKernelGGL(k_bgj_swap, dim3(ceil_div(n, 256), batch), dim3(256), 0, ctx->stream, n, k, kb, nb, A, (const int*)piv, W,
                               (const BatchCtl*)ctl, mode);
        }
        // rank-kb updates of the columns left and right of the panel
        gemm_strided(ctx, batch, false, false, n, k, kb, 1.0, Pn, n, (size_t)n * nb, W, nb, (size_t)nb * n, 1.0, A, n, nn, mask, "batch_gj_update");
        const int c1 = k + kb;
        gemm_strided(ctx, batch, false, false, n, n - c1, kb, 1.0, Pn, n, (size_t)n * nb, W + (size_t)c1 * nb, nb, (size_t)nb * n, 1.0,
                     A + (size_t)c1 * n, n, nn, mask, "batch_gj_update");
    }
    {
        TimedScope ts(ctx, "batch_gj_unpivot", 16.0 * batch * n * n, 0.0);
        hipLaunchKernelGGL(k_bgj_unpivot, dim3(ceil_div(n, 256), batch), dim3(256), 0, ctx->stream, n, A, (const int*)piv, (const BatchCtl*)ctl, mode);
    }
    DRE_HIP(hipGetLastError());
}

// ---- element-wise kernels, member = blockIdx.y; the bodies shared with dense_sign.hip are dense_sign_body.hpp's -------------------------
// k_sign_update per member; the scaling factor c_k comes from the member's own log|det Z_k| and log|det E| on the device, and the replay's
// coefficients c/2 and 1/(2c) of iteration k are left in coef for the strided GEMM
__global__ __launch_bounds__(256) void k_bsign_update(int n, double* __restrict__ Z, double* __restrict__ Zi, const double* __restrict__ Y,
                                                      const double* __restrict__ E, double* __restrict__ part, double* __restrict__ coef,
                                                      int maxiters, BatchMask mask) {
    const int b = blockIdx.y;
    if (batch_off(mask, b)) return;
    const BatchCtl& cb = mask.ctl[b];
    const double c = cb.scale ? exp((cb.s.gj.logdet - cb.logdetE) / n) : 1.0;
    const size_t tot = (size_t)n * n, o = (size_t)b * tot;
    sign_update_body(KERNEL_GRID_STRIDE, n, Z + o, Zi + o, Y + o, E + o, c, part + (size_t)b * 3 * NORM_PARTS);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double* cf = coef + ((size_t)b * maxiters + mask.k) * 2;
        cf[0] = 0.5 * c; cf[1] = 1.0 / (2.0 * c);
    }
}

// k_sign_decide per member (one workgroup each): the stopping norm, the decision, and what the single path's host loop does with it
__global__ __launch_bounds__(256) void k_bsign_decide(const double* __restrict__ part, const double* __restrict__ nrm, double tol, int k,
                                                      int maxiters, BatchCtl* ctl) {
    const int b = blockIdx.x;
    BatchCtl* c = ctl + b;
    if (c->fail || c->s.done) return;
    if (c->s.gj.singular) {                  // singular Z_k
        if (threadIdx.x == 0) { c->fail = ERR_SINGULAR; c->s.done = 4; c->iters = k; }
        return;
    }
    double s[3];
    load_partials(NORM_PARTS, part + (size_t)b * 3 * NORM_PARTS, s);
    if (threadIdx.x == 0) {
        const double e = sqrt(s[0] / nrm[2 * b]), d = sqrt(s[1] / s[2]);
        int done = sign_decision(e, d, tol);
        if (done == 0 && k + 1 >= maxiters) done = 5;
        c->s.dist = e; c->s.step = d; c->s.done = done; c->iters = k + 1;
        if (done > 1) c->fail = ERR_NOT_STABLE;
        if (e < SCALE_OFF) c->scale = 0;
    }
}

__global__ void k_bctl_begin_factor(int batch, BatchCtl* ctl) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch || ctl[b].fail) return;
    ctl[b].s.done = 0; ctl[b].s.dist = 0.0; ctl[b].s.step = 0.0; ctl[b].iters = 0; ctl[b].scale = 1;
}

// after the inversion of E: a singular E drops the member, the others keep log|det E|
__global__ void k_bctl_after_E(int batch, BatchCtl* ctl) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch || ctl[b].fail) return;
    if (ctl[b].s.gj.singular) ctl[b].fail = ERR_SINGULAR; else ctl[b].logdetE = ctl[b].s.gj.logdet;
}

// ||M_b||_F^2 into nrm[2 b + slot]
__global__ __launch_bounds__(256) void k_bsumsq(int n, const double* __restrict__ M, double* __restrict__ part, BatchMask mask) {
    const int b = blockIdx.y;
    if (batch_off(mask, b)) return;
    const size_t tot = (size_t)n * n, o = (size_t)b * tot;
    double s = 0.0;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < tot; idx += (size_t)gridDim.x * blockDim.x) { const double v = M[o + idx]; s += v * v; }
    store_partials(part + (size_t)b * 3 * NORM_PARTS, s);
}
__global__ __launch_bounds__(256) void k_bsumsq_finish(const double* __restrict__ part, double* __restrict__ nrm, int slot, BatchMask mask) {
    const int b = blockIdx.x;
    if (batch_off(mask, b)) return;
    double s[1];
    load_partials(NORM_PARTS, part + (size_t)b * 3 * NORM_PARTS, s);
    if (threadIdx.x == 0) nrm[2 * b + slot] = s[0];
}

// k_res_sym per member
__global__ __launch_bounds__(256) void k_bres_sym(int n, const double* __restrict__ Rm, const double* __restrict__ G, double* __restrict__ Res,
                                                  double* __restrict__ part, BatchMask mask) {
    const int b = blockIdx.y;
    if (batch_off(mask, b)) return;
    const size_t tot = (size_t)n * n, o = (size_t)b * tot;
    res_sym_body(KERNEL_GRID_STRIDE, n, Rm + o, G + o, Res + o, part + (size_t)b * 3 * NORM_PARTS);
}
// k_res_finish per member, and the refinement decision of SignLyap::solve: phase 0 is the residual of the first replay, phase 1 the one
// after a refinement step
__global__ __launch_bounds__(256) void k_bres_finish(const double* __restrict__ part, const double* __restrict__ nrm, double target, int max_refine,
                                                     int phase, BatchCtl* ctl, BatchMask mask) {
    const int b = blockIdx.x;
    if (batch_off(mask, b)) return;
    double s[1];
    load_partials(NORM_PARTS, part + (size_t)b * 3 * NORM_PARTS, s);
    if (threadIdx.x == 0) {
        BatchCtl* c = ctl + b;
        const double res = relative_residual(s[0], nrm[2 * b + 1]);
        c->s.res = res;
        if (phase == 0) { c->res0 = res; c->nref = 0; } else c->nref += 1;
        c->refine = (res > target && c->nref < max_refine) ? 1 : 0;
    }
}

// k_comb per member (rows x cols members, every operand with ld = rows)
__global__ __launch_bounds__(256) void k_bcomb(int rows, int cols, double a0, const double* M0, double a1, const double* M1, double a2,
                                               const double* M2, double* out, int sym, BatchMask mask) {
    const int b = blockIdx.y;
    if (batch_off(mask, b)) return;
    const size_t tot = (size_t)rows * cols, o = (size_t)b * tot;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < tot; idx += (size_t)gridDim.x * blockDim.x) {
        double v = a0 * M0[o + idx] + (M1 ? a1 * M1[o + idx] : 0.0) + (M2 ? a2 * M2[o + idx] : 0.0);
        if (sym) {
            const int i = idx % rows, j = idx / rows;
            const size_t t = o + j + (size_t)i * rows;
            v = 0.5 * (v + a0 * M0[t] + (M1 ? a1 * M1[t] : 0.0) + (M2 ? a2 * M2[t] : 0.0));
        }
        out[o + idx] = v;
    }
}

// W_b <- (W_b + W_b')/2 in place: the thread of element (i, j), i < j, owns both (the replay's symmetrisation; masked members keep their W
// where it is, which an out-of-place symmetrisation with swapped buffers would not)
__global__ __launch_bounds__(256) void k_bsym_inplace(int n, double* W, BatchMask mask) {
    const int b = blockIdx.y;
    if (batch_off(mask, b)) return;
    const size_t tot = (size_t)n * n, o = (size_t)b * tot;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < tot; idx += (size_t)gridDim.x * blockDim.x) {
        const int i = idx % n, j = idx / n;
        if (i < j) {
            const size_t t = o + j + (size_t)i * n;
            const double v = 0.5 * (W[o + idx] + W[t]);
            W[o + idx] = v; W[t] = v;
        }
    }
}

void comb_batched(Ctx* ctx, int batch, int rows, int cols, double* out, double a0, const double* M0, double a1, const double* M1, double a2,
                  const double* M2, bool sym, BatchMask mask, const char* tag) {
    DRE_REQUIRE(!sym || rows == cols, "comb_batched: sym needs square members");
    const size_t tot = (size_t)rows * cols;
    if (!tot) return;
    TimedScope ts(ctx, tag, 8.0 * batch * (2 + (M1 != nullptr) + (M2 != nullptr)) * (double)tot, 0.0);
    hipLaunchKernelGGL(k_bcomb, dim3(grid_for(tot), batch), dim3(256), 0, ctx->stream, rows, cols, a0, M0, a1, M1, a2, M2, out, sym ? 1 : 0, mask);
}

// ---- BatchedSignLyap ----------------------------------------------------------------------------------------------------------------
namespace {
// a stack with its member shape
struct Stk {
    Mat m; int r = 0, c = 0;
    Stk() = default;
    Stk(Ctx* ctx, int batch, int rows, int cols) : m(ctx, rows, cols * batch), r(rows), c(cols) {}
    Stk(const Mat& M, int rows, int cols) : m(M), r(rows), c(cols) {}
    size_t stride() const { return (size_t)r * c; }
};
void sgemm(Ctx* ctx, int batch, bool tA, bool tB, double alpha, const Stk& A, const Stk& B, double beta, Stk& C, BatchMask mask, const char* tag,
           const double* coef = nullptr, size_t coef_stride = 0) {
    const int M = tA ? A.c : A.r, K = tA ? A.r : A.c, N = tB ? B.r : B.c, K2 = tB ? B.c : B.r;
    DRE_REQUIRE(K == K2 && C.r == M && C.c == N, "batched gemm: shape mismatch");
    gemm_strided(ctx, batch, tA, tB, M, N, K, alpha, A.m.p, A.r, A.stride(), B.m.p, B.r, B.stride(), beta, C.m.p, C.r, C.stride(), mask, tag, coef, coef_stride);
}
void scomb(Ctx* ctx, int batch, Stk& out, double a0, const Stk& M0, double a1, const Stk* M1, double a2, const Stk* M2, bool sym, BatchMask mask) {
    comb_batched(ctx, batch, out.r, out.c, out.m.p, a0, M0.m.p, a1, M1 ? M1->m.p : nullptr, a2, M2 ? M2->m.p : nullptr, sym, mask);
}
void scopy(Ctx* ctx, int batch, const Stk& src, Stk& dst, BatchMask mask) { scomb(ctx, batch, dst, 1.0, src, 0.0, nullptr, 0.0, nullptr, false, mask); }

// The stack back end of the stage program dense_ros.hpp, for dense_gdre_solve_batched: sgemm with the tag "batch_dense_ros", scomb, scopy
// and lyap's factor / solve.  mask goes to every launch (the driver sets it); solves collects one statistics vector per solve.
struct StkRosOps {
    using M = Stk;
    Ctx* ctx;
    int batch;
    BatchedSignLyap& lyap;
    BatchMask mask;
    std::vector<std::vector<SignStats>> solves;       // per solve, per member
    void gemm(bool tA, bool tB, double alpha, const Stk& A, const Stk& B, double beta, Stk& C) {
        sgemm(ctx, batch, tA, tB, alpha, A, B, beta, C, mask, "batch_dense_ros");
    }
    void comb(Stk& out, double a0, const Stk& M0, double a1, const Stk* M1, double a2, const Stk* M2, bool sym) {
        scomb(ctx, batch, out, a0, M0, a1, M1, a2, M2, sym, mask);
    }
    void copy(const Stk& src, Stk& dst) { scopy(ctx, batch, src, dst, mask); }
    void factor(const Stk& F) { lyap.factor(F.m); }
    void solve(const Stk& R, Stk& X) {
        solves.emplace_back();
        lyap.solve(R.m, X.m, solves.back());
    }
};
}  // namespace

BatchedSignLyap::BatchedSignLyap(Ctx* ctx, int batch, const Mat& E, int maxiters, double tol, int max_refine, size_t extra_n2)
    : c_(ctx), B_(batch), n_(E.rows), maxiters_(maxiters), max_refine_(max_refine), tol_(tol) {
    const int n = n_;
    DRE_REQUIRE(batch >= 1 && batch <= 65535, "batched dense path: batch must be in 1 .. 65535");
    DRE_REQUIRE(n >= 1 && n <= GJ_REGISTER_MAX_N, "batched dense path: order 1 .. " + std::to_string(GJ_REGISTER_MAX_N) +
                                                      " (the register panel), n = " + std::to_string(n));
    DRE_REQUIRE(E.ld == n && (size_t)E.cols == (size_t)n * batch, "batched dense path: E must be an n x n*B stack");
    DRE_REQUIRE(maxiters >= 1 && maxiters <= 1000, "dense path: maxiters must be in 1 .. 1000");
    DRE_REQUIRE(max_refine >= 0, "dense path: max_refine must be >= 0");
    if (!(tol_ > 0.0)) tol_ = 10.0 * n * DBL_EPS;
    nn_ = (size_t)n * n;
    require_memory(ctx, doubles_needed(batch, n, maxiters, extra_n2));
    DRE_REQUIRE((size_t)n * maxiters * batch <= 2147483647u, "batched dense path: batch * maxiters * n exceeds the index range of a stack");
    const int nb = gj_batch_nb(n);
    Pstore_ = Mat(ctx, n, n * maxiters * batch);
    E_ = E;
    auto sq = [&] { return Mat(ctx, n, n * batch); };
    Einv_ = sq(); F_ = sq(); Z_ = sq(); Zi_ = sq(); Y_ = sq(); W_ = sq(); T_ = sq(); Res_ = sq(); dX_ = sq();
    Pn_ = Mat(ctx, n, nb * batch); Wp_ = Mat(ctx, nb, n * batch);
    piv_ = DevArr<int>(ctx, (size_t)n * batch);
    ctl_ = DevArr<BatchCtl>(ctx, batch);
    part_ = DevArr<double>(ctx, (size_t)3 * NORM_PARTS * batch);
    nrm_ = DevArr<double>(ctx, (size_t)2 * batch);
    coef_ = DevArr<double>(ctx, (size_t)2 * maxiters * batch);
    h_.resize((size_t)batch);
    status_.resize((size_t)batch);
    DRE_HIP(hipMemsetAsync(ctl_.p, 0, sizeof(BatchCtl) * batch, ctx->stream));
    // E^-1 and log|det E| once per solve
    Stk Es(E_, n, n), Ei(Einv_, n, n);
    scopy(ctx, batch, Es, Ei, BatchMask{});
    gj_invert_batched(ctx, batch, n, Einv_.p, piv_.p, ctl_.p, BM_GJ, Pn_.p, Wp_.p);
    hipLaunchKernelGGL(k_bctl_after_E, dim3(ceil_div(batch, 256)), dim3(256), 0, ctx->stream, batch, ctl_.p);
    hipLaunchKernelGGL(k_bsumsq, dim3(NORM_PARTS, batch), dim3(256), 0, ctx->stream, n, (const double*)E_.p, part_.p, BatchMask{});
    hipLaunchKernelGGL(k_bsumsq_finish, dim3(batch), dim3(256), 0, ctx->stream, (const double*)part_.p, nrm_.p, 0, BatchMask{});
    DRE_HIP(hipGetLastError());
    fetch();
}

void BatchedSignLyap::fetch() {
    DRE_HIP(hipMemcpyAsync(h_.data(), ctl_.p, sizeof(BatchCtl) * (size_t)B_, hipMemcpyDeviceToHost, c_->stream));
    c_->sync();
    for (int b = 0; b < B_; ++b) {
        const BatchCtl& h = h_[(size_t)b];
        BatchMemberStatus& st = status_[(size_t)b];
        if (!h.fail || st.code) continue;
        st.code = h.fail;
        const std::string who = "batched dense path, member " + std::to_string(b) + ": ";
        if (h.fail == ERR_SINGULAR && h.s.done != 4) st.msg = who + "E is singular (zero pivot in the Gauss-Jordan inversion)";
        else st.msg = who + sign_failure(h.s.done, h.iters, h.s.dist, maxiters_);
    }
}

void BatchedSignLyap::factor(const Mat& F) {
    const int n = n_, B = B_;
    DRE_REQUIRE(F.rows == n && F.ld == n && (size_t)F.cols == (size_t)n * B, "batched dense path: F must be an n x n*B stack");
    Stk Fs(F, n, n), Fk(F_, n, n), Z(Z_, n, n), Zi(Zi_, n, n), Es(E_, n, n), Y(Y_, n, n);
    hipLaunchKernelGGL(k_bctl_begin_factor, dim3(ceil_div(B, 256)), dim3(256), 0, c_->stream, B, ctl_.p);
    scopy(c_, B, Fs, Fk, live());
    scopy(c_, B, Fs, Z, live());
    scopy(c_, B, Fs, Zi, live());
    max_iters_live_ = 0;
    for (int k = 0; k < maxiters_; ++k) {
        const BatchMask mk{ctl_.p, BM_FACTOR, k};
        gj_invert_batched(c_, B, n, Zi_.p, piv_.p, ctl_.p, BM_FACTOR, Pn_.p, Wp_.p);
        // P_k = Z_k^-1 E at member b's slot k of the store, E P_k
        gemm_strided(c_, B, false, false, n, n, n, 1.0, Zi_.p, n, nn_, E_.p, n, nn_, 0.0, Pstore_.p + (size_t)k * nn_, n, nn_ * maxiters_, mk, "batch_sign_gemm");
        gemm_strided(c_, B, false, false, n, n, n, 1.0, E_.p, n, nn_, Pstore_.p + (size_t)k * nn_, n, nn_ * maxiters_, 0.0, Y_.p, n, nn_, mk, "batch_sign_gemm");
        {
            TimedScope ts(c_, "batch_sign_update", 40.0 * B * n * n, 0.0);
            hipLaunchKernelGGL(k_bsign_update, dim3(NORM_PARTS, B), dim3(256), 0, c_->stream, n, Z_.p, Zi_.p, (const double*)Y_.p, (const double*)E_.p,
                               part_.p, coef_.p, maxiters_, mk);
            hipLaunchKernelGGL(k_bsign_decide, dim3(B), dim3(256), 0, c_->stream, (const double*)part_.p, (const double*)nrm_.p, tol_, k, maxiters_, ctl_.p);
        }
        DRE_HIP(hipGetLastError());
        fetch();
        bool running = false;
        for (int b = 0; b < B; ++b) running = running || (!h_[(size_t)b].fail && !h_[(size_t)b].s.done);
        if (!running) break;
    }
    for (int b = 0; b < B; ++b)
        if (!h_[(size_t)b].fail) max_iters_live_ = std::max(max_iters_live_, h_[(size_t)b].iters);
}

void BatchedSignLyap::replay(const Mat& R, Mat& X, int extra_mode) {
    const int n = n_, B = B_;
    Stk Rs(R, n, n), W(W_, n, n), T(T_, n, n), Y(Y_, n, n), Ei(Einv_, n, n), Xs(X, n, n);
    const BatchMask m0{ctl_.p, extra_mode, 0};
    scopy(c_, B, Rs, W, m0);
    for (int k = 0; k < max_iters_live_; ++k) {
        const BatchMask mk{ctl_.p, BM_REPLAY | extra_mode, k};
        const double* P = Pstore_.p + (size_t)k * nn_;
        gemm_strided(c_, B, false, false, n, n, n, 1.0, W_.p, n, nn_, P, n, nn_ * maxiters_, 0.0, T_.p, n, nn_, mk, "batch_sign_gemm");                 // W P
        gemm_strided(c_, B, true, false, n, n, n, 0.0, P, n, nn_ * maxiters_, T_.p, n, nn_, 0.0, W_.p, n, nn_, mk, "batch_sign_gemm",                   // W/(2c) + (c/2) P' W P
                     coef_.p + (size_t)2 * k, (size_t)2 * maxiters_);
        TimedScope ts(c_, "batch_comb", 16.0 * B * n * n, 0.0);
        hipLaunchKernelGGL(k_bsym_inplace, dim3(grid_for(nn_), B), dim3(256), 0, c_->stream, n, W_.p, mk);
    }
    sgemm(c_, B, false, false, 1.0, W, Ei, 0.0, T, m0, "batch_sign_gemm");                     // X = E^-T (W/2) E^-1
    sgemm(c_, B, true, false, 0.5, Ei, T, 0.0, Y, m0, "batch_sign_gemm");
    scomb(c_, B, Xs, 1.0, Y, 0.0, nullptr, 0.0, nullptr, true, m0);
}

void BatchedSignLyap::residual(const Mat& R, const Mat& X, int extra_mode, int phase) {
    const int n = n_, B = B_;
    Stk Xs(X, n, n), Es(E_, n, n), Fk(F_, n, n), T(T_, n, n), Y(Y_, n, n);
    const BatchMask m0{ctl_.p, extra_mode, 0};
    sgemm(c_, B, false, false, 1.0, Xs, Es, 0.0, T, m0, "batch_sign_gemm");       // X E
    sgemm(c_, B, true, false, 1.0, Fk, T, 0.0, Y, m0, "batch_sign_gemm");         // F' X E
    TimedScope ts(c_, "batch_sign_residual", 24.0 * B * n * n, 0.0);
    hipLaunchKernelGGL(k_bres_sym, dim3(NORM_PARTS, B), dim3(256), 0, c_->stream, n, (const double*)R.p, (const double*)Y_.p, Res_.p, part_.p, m0);
    hipLaunchKernelGGL(k_bres_finish, dim3(B), dim3(256), 0, c_->stream, (const double*)part_.p, (const double*)nrm_.p, 100.0 * n * DBL_EPS, max_refine_,
                       phase, ctl_.p, m0);
}

void BatchedSignLyap::solve(const Mat& R, Mat& X, std::vector<SignStats>& stats) {
    const int n = n_, B = B_;
    DRE_REQUIRE(R.rows == n && R.ld == n && (size_t)R.cols == (size_t)n * B && X.rows == n && X.ld == n && (size_t)X.cols == (size_t)n * B,
                "batched dense path: R and X must be n x n*B stacks");
    stats.assign((size_t)B, SignStats{});
    if (max_iters_live_ == 0) return;              // no live member
    hipLaunchKernelGGL(k_bsumsq, dim3(NORM_PARTS, B), dim3(256), 0, c_->stream, n, (const double*)R.p, part_.p, live());
    hipLaunchKernelGGL(k_bsumsq_finish, dim3(B), dim3(256), 0, c_->stream, (const double*)part_.p, nrm_.p, 1, live());
    replay(R, X, BM_LIVE);
    residual(R, X, BM_LIVE, 0);
    DRE_HIP(hipGetLastError());
    fetch();
    Stk Xs(X, n, n), dX(dX_, n, n);
    for (;;) {
        bool any = false;
        for (int b = 0; b < B; ++b) any = any || (!h_[(size_t)b].fail && h_[(size_t)b].refine);
        if (!any) break;
        replay(Res_, dX_, BM_REFINE);
        scomb(c_, B, Xs, 1.0, Xs, 1.0, &dX, 0.0, nullptr, false, BatchMask{ctl_.p, BM_REFINE, 0});
        residual(R, X, BM_REFINE, 1);
        DRE_HIP(hipGetLastError());
        fetch();
    }
    for (int b = 0; b < B; ++b) {
        const BatchCtl& h = h_[(size_t)b];
        if (h.fail) continue;
        SignStats& s = stats[(size_t)b];
        s.iters = h.iters; s.refinements = h.nref; s.res0 = h.res0; s.res = h.s.res;
    }
}

// ---- Rosenbrock drivers on stacks ----------------------------------------------------------------------------------------------------
// square stacks beside the solver's: the driver's ten (X, C'C, A - BK, F, T, A'XE, R, sym R, K1, K2), the operands E, A, X0, the saved
// states (X0 and every step's, or X0 alone: the last state is a view of X)
static size_t gdre_extra_n2(int nsteps, bool save_state) { return 10 + 3 + (save_state ? (size_t)nsteps + 1 : 1); }

// the solver's stacks and the square stacks above; B, K(t_i) for every time point, X B, V1 and one spare n x m stack; C
size_t dense_gdre_batched_doubles(int batch, int n, int m, int q, int nsteps, int order, bool save_state, int maxiters) {
    (void)order;
    return BatchedSignLyap::doubles_needed(batch, n, maxiters, gdre_extra_n2(nsteps, save_state)) +
           (size_t)batch * ((size_t)n * m * ((size_t)nsteps + 4) + (size_t)q * n);
}

void dense_gdre_solve_batched(Ctx* ctx, int batch, const Mat& E, const Mat& A, const Mat& Bm, const Mat& C, const Mat& X0, int m, int q, double t0,
                              double tf, double dt, int order, bool save_state, int maxiters, double tol, int max_refine,
                              std::vector<DenseGdreResult>& out, std::vector<BatchMemberStatus>& status) {
    const int n = E.rows, B = batch;
    DRE_REQUIRE(order == 1 || order == 2, "batched dense path: only Ros1 and Ros2 (order 1, 2) are batched; order = " + std::to_string(order) +
                                              " runs through the single-problem call");
    const std::vector<double> t = dense_time_grid(t0, tf, dt);
    const int nsteps = (int)t.size() - 1;
    require_memory(ctx, dense_gdre_batched_doubles(B, n, m, q, nsteps, order, save_state, maxiters));
    BatchedSignLyap lyap(ctx, B, E, maxiters, tol, max_refine, gdre_extra_n2(nsteps, save_state));
    StkRosOps ops{ctx, B, lyap, BatchMask{}, {}};       // before the first factorisation every member takes part (K(t_0) needs no solve)
    const Stk Es(E, n, n), As(A, n, n), Bs(Bm, n, m), Cs(C, q, n), X0s(X0, n, n);
    auto sq = [&] { return Stk(ctx, B, n, n); };
    Stk X = sq(), CtC = sq();
    RosWork<Stk> w{sq(), sq(), sq(), sq(), sq(), sq(), sq(), sq(), Stk(), Stk(), Stk(ctx, B, n, m), Stk(ctx, B, n, m), Stk()};   // (Ros1, Ros2: no K3, K4, V2)
    const RosOperands<Stk> p{Es, As, Bs, CtC};
    ops.copy(X0s, X);
    ops.gemm(true, false, 1.0, Cs, Cs, 0.0, CtC);
    auto feedback = [&](const Stk& Xs) {
        Stk Kt(ctx, B, n, m);
        ros_EtKB(ops, p, w, Xs, Kt);
        return Kt;
    };
    std::vector<Stk> Kts, Xsaved;
    std::vector<int> steps_done((size_t)B, 0);
    auto save = [&](const Stk& Xs) { Stk c = sq(); ops.copy(Xs, c); Xsaved.push_back(c); };
    save(X);
    Stk Kt = feedback(X);
    Kts.push_back(Kt);
    ops.mask = lyap.live();
    for (int i = 1; i <= nsteps; ++i) {
        bool any = false;
        for (int b = 0; b < B; ++b) any = any || lyap.alive(b);
        if (!any) break;
        const double tau = t[(size_t)i - 1] - t[(size_t)i];
        ros_stages(ops, order, tau, p, X, Kt, w);
        ros_combine(ops, order, tau, X, w);
        for (int b = 0; b < B; ++b)
            if (lyap.alive(b)) steps_done[(size_t)b] = i;
        if (save_state) save(X);
        Kt = feedback(X);
        Kts.push_back(Kt);
    }
    ctx->sync();
    // member b's slices of the stacks, up to its last completed step
    const int per_step = order == 1 ? 1 : 2;
    out.assign((size_t)B, DenseGdreResult{});
    status = lyap.status();
    for (int b = 0; b < B; ++b) {
        DenseGdreResult& r = out[(size_t)b];
        const int done = steps_done[(size_t)b];
        for (int i = 0; i <= done; ++i) {
            r.t.push_back(t[(size_t)i]);
            r.Kt.push_back(Kts[(size_t)i].m.colsview(b * m, m));
        }
        r.X.push_back(Xsaved[0].m.colsview(b * n, n));
        if (save_state) {
            for (int i = 1; i <= done; ++i) r.X.push_back(Xsaved[(size_t)i].m.colsview(b * n, n));
        } else if (done > 0) {
            r.X.push_back(X.m.colsview(b * n, n));      // (a failed member's X was not touched after its last completed step)
        }
        for (int j = 0; j < done * per_step; ++j) r.solves.push_back(ops.solves[(size_t)j][(size_t)b]);
    }
}

}  // namespace dre
