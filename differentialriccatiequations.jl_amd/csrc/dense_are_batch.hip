// Batched dense GARE solver: the algorithm of dense_are.hip, statement by statement, on stacks laid out as in
// dense_batch.hpp (member b at base + b * rows * cols), member b = blockIdx.y of every launch:
//   Z0_b = [[A_b, -G_b], [-Q_b, -A_b']], K_b = diag(E_b, E_b')   assembled per member from the factors of G_b and Q_b;
//   Z_{k+1} = struct((Z_k / c_k + c_k K Z_k^-1 K) / 2)           gj_invert_batched at order 2n, the eight K_a W_ab K_b products through
//                                                                gemm_strided on block views, c_k, scaling off, convergence and the
//                                                                stagnation window decided per member on the device;
//   (Z_inf + K)[I; XE] = 0                                       Householder QR member by member (qr_factor has no batched form), everything
//                                                                behind it on stacks;
//   Newton-Kleinman refinement                                   BatchedSignLyap on the gathered sub-batch of the members that need a step.
// The element-wise kernels are thin wrappers: the bodies live in dense_are_body.hpp, shared with dense_are.hip, and a wrapper here only
// applies the member's mask and offsets the base pointers.  A member's arithmetic never looks at B, at its position or at another member's data: no atomics, per-member
// grids and partial-sum buffers, fixed-order sums.  Offsets into the stacks are formed in size_t.
#include "dense_are_batch.hpp"

#include <cmath>
#include <cstring>
#include <memory>

#include "dense.hpp"
#include "dense_are_body.hpp"
#include "profiling.hpp"

namespace dre {

// ---- control blocks ------------------------------------------------------------------------------------------------------------------
__global__ void k_bare_ctl_init(BatchCtl* ctl, AreBatchCtl* ext) {
    const int b = blockIdx.y;
    if (threadIdx.x != 0) return;
    BatchCtl& c = ctl[b];
    c.s.gj.logdet = 0.0; c.s.gj.singular = 0; c.s.done = 0; c.s.dist = 0.0; c.s.step = 0.0; c.s.res = 0.0;
    c.logdetE = 0.0; c.res0 = 0.0; c.fail = 0; c.iters = 0; c.scale = 1; c.refine = 0; c.nref = 0; c.pad = 0;
    AreBatchCtl& e = ext[b];
    e.best = INFINITY; e.resnorm = 0.0; e.cand = 0.0; e.since = 0; e.accept = 0;
}

// after an inversion outside the sign iteration: a zero pivot drops the member (phase 0: E_b, phase 1: the extraction's R factor), after
// E_b the others keep log|det E_b|
__global__ void k_bare_ctl_after_inverse(BatchCtl* ctl, int phase) {
    const int b = blockIdx.y;
    if (threadIdx.x != 0 || ctl[b].fail) return;
    if (ctl[b].s.gj.singular) ctl[b].fail = ERR_SINGULAR;
    else if (phase == 0) ctl[b].logdetE = ctl[b].s.gj.logdet;
}

// ---- the kernels of dense_are.hip per member: bodies of dense_are_body.hpp on the member's slices ------------------------------------------
__global__ __launch_bounds__(256) void k_bare_assemble(int n, const double* __restrict__ A, const double* __restrict__ G, const double* __restrict__ Q,
                                                       double* __restrict__ Z, double* __restrict__ Zi, BatchMask mask) {
    const int b = blockIdx.y;
    if (batch_off(mask, b)) return;
    const size_t tot = (size_t)n * n, o = (size_t)b * tot, oz = (size_t)b * 4 * tot;
    are_assemble_body(KERNEL_GRID_STRIDE, n, A + o, G + o, Q + o, Z + oz, Zi + oz);
}

// c = (|det Z_k| / |det K|)^(1/2n) from the member's own log|det Z_k| and log|det E| while its scaling is on.  The mask (BM_FACTOR) leaves
// out a member whose inversion met a zero pivot: k_bare_decide reports it.
__global__ __launch_bounds__(256) void k_bare_update(int n, double* __restrict__ Z, double* __restrict__ Zi, double* __restrict__ part, BatchMask mask) {
    const int b = blockIdx.y;
    if (batch_off(mask, b)) return;
    const BatchCtl& cb = mask.ctl[b];
    const double logdetK = 2.0 * cb.logdetE;
    const double c = cb.scale ? exp((cb.s.gj.logdet - logdetK) / (2.0 * n)) : 1.0;
    const size_t tot = (size_t)n * n, oz = (size_t)b * 4 * tot;
    are_update_body(KERNEL_GRID_STRIDE, n, Z + oz, Zi + oz, c, part + (size_t)b * 2 * NORM_PARTS);
}

// one workgroup per member: the decision, and what the single path's host loop does with it: a failure sets the member's code, so that it
// drops out of every later launch; running out of maxiters is done = 5
__global__ __launch_bounds__(256) void k_bare_decide(const double* __restrict__ part, double tol, int k, int maxiters, BatchCtl* ctl, AreBatchCtl* ext) {
    const int b = blockIdx.y;
    BatchCtl* c = ctl + b;
    if (c->fail || c->s.done) return;        // (uniform in the workgroup, read before the barriers of load_partials)
    if (c->s.gj.singular) {                  // singular Z_k
        if (threadIdx.x == 0) { c->fail = ERR_SINGULAR; c->s.done = 4; c->iters = k; }
        return;
    }
    double s[2];                             // ||Z_{k+1} - Z_k||^2, ||Z_{k+1}||^2
    load_partials(NORM_PARTS, part + (size_t)b * 2 * NORM_PARTS, s);
    if (threadIdx.x != 0) return;
    AreBatchCtl* e = ext + b;
    const double d = sqrt(s[0] / s[1]);
    c->s.step = d; c->iters = k + 1;
    int done = are_step_rule(d, tol, e->best, e->since, c->scale);
    if (done == 0 && k + 1 >= maxiters) done = 5;
    if (done) c->s.done = done;
    if (done > 1) c->fail = ERR_NOT_STABLE;
}

__global__ __launch_bounds__(256) void k_bare_extract_ops(int n, const double* __restrict__ Z, const double* __restrict__ E, double* __restrict__ Zi,
                                                          BatchMask mask) {
    const int b = blockIdx.y;
    if (batch_off(mask, b)) return;
    const size_t tot = (size_t)n * n, oz = (size_t)b * 4 * tot;
    are_extract_ops_body(KERNEL_GRID_STRIDE, n, Z + oz, E + (size_t)b * tot, Zi + oz);
}

__global__ __launch_bounds__(256) void k_bare_residual(int n, const double* __restrict__ Q, const double* __restrict__ AXE, const double* __restrict__ XGX,
                                                       double* __restrict__ Res, double* __restrict__ part, BatchMask mask) {
    const int b = blockIdx.y;
    if (batch_off(mask, b)) return;
    const size_t tot = (size_t)n * n, o = (size_t)b * tot;
    are_residual_body(KERNEL_GRID_STRIDE, n, Q + o, AXE + o, XGX + o, Res + o, part + (size_t)b * 4 * NORM_PARTS);
}

// the scaled residual per member, and the refinement loop's decision of dense_gare_solve.  phase 0: the residual of the extracted X;
// phase 1: the residual of the candidate X + D, which replaces X only when it is smaller.  A live member that the mask leaves out took no
// step: its accept word is cleared.
__global__ __launch_bounds__(256) void k_bare_residual_finish(const double* __restrict__ part, double target, int max_refine, int phase, BatchCtl* ctl,
                                                              AreBatchCtl* ext, BatchMask mask) {
    const int b = blockIdx.y;
    if (batch_off(mask, b)) {
        if (threadIdx.x == 0 && !ctl[b].fail) ext[b].accept = 0;
        return;
    }
    double s[4];
    load_partials(NORM_PARTS, part + (size_t)b * 4 * NORM_PARTS, s);
    if (threadIdx.x != 0) return;
    BatchCtl* c = ctl + b;
    AreBatchCtl* e = ext + b;
    const double res = are_scaled_residual(s, &e->resnorm);
    e->cand = res;
    if (phase == 0) {
        c->res0 = res; c->s.res = res; c->nref = 0; e->accept = 0;
        c->refine = (res > target && max_refine > 0) ? 1 : 0;
    } else {
        c->nref += 1;
        if (res < c->s.res) {
            c->s.res = res; e->accept = 1;
            c->refine = (res > target && c->nref < max_refine) ? 1 : 0;
        } else {                             // stopped decreasing: keep the better iterate
            e->accept = 0; c->refine = 0;
        }
    }
}

// X_b <- Xn_b for the members whose last step was accepted
__global__ __launch_bounds__(256) void k_bare_accept(int n, const double* __restrict__ Xn, double* __restrict__ X, const AreBatchCtl* ext, BatchMask mask) {
    const int b = blockIdx.y;
    if (batch_off(mask, b) || !ext[b].accept) return;
    const size_t tot = (size_t)n * n, o = (size_t)b * tot;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < tot; idx += (size_t)gridDim.x * blockDim.x) X[o + idx] = Xn[o + idx];
}

// dst_j = src_{idx[j]}: the members that take a refinement step, gathered into a contiguous sub-batch (j = blockIdx.y)
__global__ __launch_bounds__(256) void k_bare_gather(int n, const double* __restrict__ src, double* __restrict__ dst, const int* __restrict__ idx) {
    const size_t tot = (size_t)n * n, os = (size_t)idx[blockIdx.y] * tot, od = (size_t)blockIdx.y * tot;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += (size_t)gridDim.x * blockDim.x) dst[od + i] = src[os + i];
}
// Xn_{idx[j]} = X_{idx[j]} + D_j: the sub-batch's steps scattered back as candidates
__global__ __launch_bounds__(256) void k_bare_scatter_step(int n, const double* __restrict__ X, const double* __restrict__ D, double* __restrict__ Xn,
                                                           const int* __restrict__ idx, BatchMask mask) {
    const int b = idx[blockIdx.y];
    if (batch_off(mask, b)) return;
    const size_t tot = (size_t)n * n, o = (size_t)b * tot, od = (size_t)blockIdx.y * tot;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < tot; i += (size_t)gridDim.x * blockDim.x) Xn[o + i] = X[o + i] + D[od + i];
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
namespace {

size_t panel_doubles(int n) { return std::max((size_t)n * gj_batch_nb(n), (size_t)2 * n * gj_batch_nb(2 * n)); }

// the B BatchCtl blocks and the B AreBatchCtl blocks in one allocation, fetched in one copy
struct Controls {
    Ctx* c; int B;
    DevArr<double> raw;
    std::vector<double> host;
    Controls(Ctx* ctx, int batch) : c(ctx), B(batch), raw(ctx, (size_t)batch * words()), host((size_t)batch * words()) {}
    static constexpr size_t words() { return (sizeof(BatchCtl) + sizeof(AreBatchCtl)) / sizeof(double); }
    BatchCtl* ctl() const { return reinterpret_cast<BatchCtl*>(raw.p); }
    AreBatchCtl* ext() const { return reinterpret_cast<AreBatchCtl*>(raw.p + (size_t)B * sizeof(BatchCtl) / sizeof(double)); }
    void fetch() {
        DRE_HIP(hipMemcpyAsync(host.data(), raw.p, host.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        c->sync();
    }
    BatchCtl h(int b) const { BatchCtl v; std::memcpy(&v, (const char*)host.data() + (size_t)b * sizeof(BatchCtl), sizeof v); return v; }
    AreBatchCtl he(int b) const {
        AreBatchCtl v;
        std::memcpy(&v, (const char*)host.data() + (size_t)B * sizeof(BatchCtl) + (size_t)b * sizeof(AreBatchCtl), sizeof v);
        return v;
    }
    // the refinement's closed loop of member b failed in the sub-batch: drop the member (one control block written back)
    void drop(int b, int code) {
        BatchCtl v = h(b);
        v.fail = code; v.refine = 0;
        std::memcpy((char*)host.data() + (size_t)b * sizeof(BatchCtl), &v, sizeof v);
        DRE_HIP(hipMemcpyAsync(ctl() + b, (const char*)host.data() + (size_t)b * sizeof(BatchCtl), sizeof v, hipMemcpyHostToDevice, c->stream));
    }
};
static_assert(sizeof(BatchCtl) % sizeof(double) == 0 && sizeof(AreBatchCtl) % sizeof(double) == 0, "control blocks are whole doubles");

// G_b = F_b In_b F_b' (In null: F_b F_b') for a stack of n x w factors
void form_gram_batched(Ctx* ctx, int batch, int n, int w, const Mat& F, const Mat* In, Mat& G) {
    const size_t nn = (size_t)n * n, nw = (size_t)n * w;
    if (w == 0) { DRE_HIP(hipMemsetAsync(G.p, 0, nn * batch * sizeof(double), ctx->stream)); return; }
    if (In) {
        Mat FI(ctx, n, w * batch);
        gemm_strided(ctx, batch, false, false, n, w, w, 1.0, F.p, n, nw, In->p, w, (size_t)w * w, 0.0, FI.p, n, nw, BatchMask{}, "batch_are");
        gemm_strided(ctx, batch, false, true, n, n, w, 1.0, FI.p, n, nw, F.p, n, nw, 0.0, G.p, n, nn, BatchMask{}, "batch_are");
    } else {
        gemm_strided(ctx, batch, false, true, n, n, w, 1.0, F.p, n, nw, F.p, n, nw, 0.0, G.p, n, nn, BatchMask{}, "batch_are");
    }
}

}  // namespace

// Per member: the single path's 24 n^2 (Z, Zi; the extraction's QR, whose 7 n^2 exist for one member at a time; E^-1, G, Q, X; the residual's
// five) and, with refinement, its (maxiters + 12) n^2 (BatchedSignLyap's (maxiters + 10) n^2, F and the candidate; the gathered E, F, R and D
// of the sub-batch take the place of Z and Zi, which are released before); the operand stacks E, A, B, Ct, Rinv, S; the panel's work stacks
// Pn and W, sized for the larger of the two inversion orders n and 2n.
size_t dense_gare_batched_doubles(int batch, int n, int m, int q, int maxiters, int max_refine) {
    const size_t nn = (size_t)n * n;
    return (size_t)batch * ((24 + 2) * nn + (max_refine > 0 ? ((size_t)maxiters + 12) * nn : 0) + (size_t)n * ((size_t)m + q) + (size_t)m * m +
                            (size_t)q * q + 2 * panel_doubles(n));
}

void dense_gare_solve_batched(Ctx* ctx, int batch, const Mat& E, const Mat& A, const Mat& Bm, const Mat* Rinv, const Mat& Ct, const Mat* S, int m,
                              int q, int maxiters, double tol, int max_refine, std::vector<DenseGareResult>& out,
                              std::vector<BatchMemberStatus>& status) {
    const int n = E.rows, n2 = 2 * n, B = batch;
    DRE_REQUIRE(B >= 1 && B <= 65535, "batched dense GARE: batch must be in 1 .. 65535");
    DRE_REQUIRE(n >= 1 && n2 <= GJ_REGISTER_MAX_N, "batched dense GARE: the register panel inverts the Hamiltonian of order 2n <= " +
                                                       std::to_string(GJ_REGISTER_MAX_N) + ", 2n = " + std::to_string(n2));
    DRE_REQUIRE(m >= 0 && q >= 0, "batched dense GARE: m, q >= 0");
    DRE_REQUIRE(E.ld == n && A.rows == n && A.ld == n && (size_t)E.cols == (size_t)n * B && (size_t)A.cols == (size_t)n * B,
                "batched dense GARE: E and A must be n x n*B stacks");
    DRE_REQUIRE(Bm.rows == n && Bm.ld == n && (size_t)Bm.cols == (size_t)m * B && Ct.rows == n && Ct.ld == n && (size_t)Ct.cols == (size_t)q * B,
                "batched dense GARE: B must be an n x m*B stack and Ct an n x q*B stack");
    DRE_REQUIRE(!Rinv || (Rinv->rows == m && Rinv->ld == std::max(m, 1) && (size_t)Rinv->cols == (size_t)m * B), "batched dense GARE: Rinv must be an m x m*B stack");
    DRE_REQUIRE(!S || (S->rows == q && S->ld == std::max(q, 1) && (size_t)S->cols == (size_t)q * B), "batched dense GARE: S must be a q x q*B stack");
    DRE_REQUIRE(maxiters >= 1 && maxiters <= 1000, "dense GARE: maxiters must be in 1 .. 1000");
    DRE_REQUIRE(max_refine >= 0, "dense GARE: max_refine must be >= 0");
    require_memory(ctx, dense_gare_batched_doubles(B, n, m, q, maxiters, max_refine) -
                            (size_t)B * (2 * (size_t)n * n + (size_t)n * ((size_t)m + q) + (Rinv ? (size_t)m * m : 0) + (S ? (size_t)q * q : 0)));   // (the operands exist)
    DRE_REQUIRE((size_t)n2 * B <= 2147483647u, "batched dense GARE: batch * 2n exceeds the column range of a stack");
    const double tol2 = tol > 0.0 ? tol : 10.0 * n2 * DBL_EPS;
    const size_t nn = (size_t)n * n, nn4 = 4 * nn;
    const dim3 per_member(1, B), blk(256);

    out.assign((size_t)B, DenseGareResult{});
    status.assign((size_t)B, BatchMemberStatus{});
    Controls cb(ctx, B);
    BatchCtl* ctl = cb.ctl();
    AreBatchCtl* ext = cb.ext();
    const BatchMask live{ctl, BM_LIVE, 0};
    auto who = [](int b) { return "batched dense GARE, member " + std::to_string(b) + ": "; };
    // the control blocks -> status (a member's first failure is the one that is kept)
    auto note_failures = [&] {
        for (int b = 0; b < B; ++b) {
            const BatchCtl h = cb.h(b);
            BatchMemberStatus& st = status[(size_t)b];
            if (!h.fail || st.code) continue;
            st.code = h.fail;
            if (h.fail == ERR_SINGULAR)
                st.msg = who(b) + (h.s.done == 0   ? std::string("E is singular (zero pivot in the Gauss-Jordan inversion)")
                                   : h.s.done == 4 ? gare_sign_failure(4, h.iters, h.s.step, maxiters)
                                                   : std::string("[Z12; Z22 + E'] is rank deficient (no stable deflating subspace of dimension n)"));
            else
                st.msg = who(b) + gare_sign_failure(h.s.done, h.iters, h.s.step, maxiters);
        }
    };
    auto any_alive = [&] {
        for (int b = 0; b < B; ++b)
            if (!status[(size_t)b].code) return true;
        return false;
    };

    auto sq = [&] { return Mat(ctx, n, n * B); };
    Mat G = sq(), Q = sq(), Einv = sq(), T = sq(), X = sq();
    DRE_REQUIRE(panel_doubles(n) * B <= 2147483647u, "batched dense GARE: batch * 2n * panel width exceeds the index range of a stack");
    Mat Pn(ctx, 1, (int)(panel_doubles(n) * B)), Wp(ctx, 1, Pn.cols);
    DevArr<int> piv(ctx, (size_t)n2 * B);
    DevArr<double> part(ctx, (size_t)4 * NORM_PARTS * B);
    hipLaunchKernelGGL(k_bare_ctl_init, per_member, dim3(64), 0, ctx->stream, ctl, ext);
    form_gram_batched(ctx, B, n, m, Bm, Rinv, G);
    form_gram_batched(ctx, B, n, q, Ct, S, Q);
    // E^-1 and log|det K| = 2 log|det E| per member
    comb_batched(ctx, B, n, n, Einv.p, 1.0, E.p, 0.0, nullptr, 0.0, nullptr, false, BatchMask{}, "batch_are_copy");
    gj_invert_batched(ctx, B, n, Einv.p, piv.p, ctl, BM_GJ, Pn.p, Wp.p);
    hipLaunchKernelGGL(k_bare_ctl_after_inverse, per_member, dim3(64), 0, ctx->stream, ctl, 0);

    // ---- sign iteration on the Hamiltonian pencils ----
    Mat Z(ctx, n2, n2 * B), Zi(ctx, n2, n2 * B);
    {
        TimedScope ts(ctx, "batch_are_assemble", 8.0 * 12 * B * nn, 0.0);
        hipLaunchKernelGGL(k_bare_assemble, dim3(grid_for(nn), B), blk, 0, ctx->stream, n, (const double*)A.p, (const double*)G.p, (const double*)Q.p, Z.p,
                           Zi.p, live);
    }
    DRE_HIP(hipGetLastError());
    for (int k = 0; k < maxiters; ++k) {
        const BatchMask mk{ctl, BM_FACTOR, k};
        gj_invert_batched(ctx, B, n2, Zi.p, piv.p, ctl, BM_FACTOR, Pn.p, Wp.p);
        // Zi <- K Zi K block by block: W_ab <- K_a W_ab K_b with K_0 = E, K_1 = E'
        for (int b = 0; b < 2; ++b) {
            for (int a = 0; a < 2; ++a) {
                double* W = Zi.p + (size_t)a * n + (size_t)b * n * n2;
                gemm_strided(ctx, B, false, b == 1, n, n, n, 1.0, W, n2, nn4, E.p, n, nn, 0.0, T.p, n, nn, mk, "batch_are_kwk");
                gemm_strided(ctx, B, a == 1, false, n, n, n, 1.0, E.p, n, nn, T.p, n, nn, 0.0, W, n2, nn4, mk, "batch_are_kwk");
            }
        }
        {
            TimedScope ts(ctx, "batch_are_update", 8.0 * 4 * 4.0 * B * nn, 0.0);
            hipLaunchKernelGGL(k_bare_update, dim3(NORM_PARTS, B), blk, 0, ctx->stream, n, Z.p, Zi.p, part.p, mk);
            hipLaunchKernelGGL(k_bare_decide, per_member, blk, 0, ctx->stream, (const double*)part.p, tol2, k, maxiters, ctl, ext);
        }
        DRE_HIP(hipGetLastError());
        cb.fetch();
        note_failures();
        bool running = false;
        for (int b = 0; b < B; ++b) running = running || (!cb.h(b).fail && !cb.h(b).s.done);
        if (!running) break;
    }
    for (int b = 0; b < B; ++b) out[(size_t)b].iters = cb.h(b).iters;

    // ---- extraction: [Z12; Z22 + E'] Y = -[Z11 + E; Z21] by Householder QR, X = sym(Y E^-1) ----
    if (any_alive()) {
        {
            TimedScope ts(ctx, "batch_are_extract_ops", 8.0 * 10 * B * nn, 0.0);
            hipLaunchKernelGGL(k_bare_extract_ops, dim3(grid_for(nn), B), blk, 0, ctx->stream, n, (const double*)Z.p, (const double*)E.p, Zi.p, live);
        }
        Mat Rs = sq();
        for (int b = 0; b < B; ++b) {            // (qr_factor and qr_apply_q have no batched form: member by member on the member's view)
            if (status[(size_t)b].code) continue;
            Mat Zb = Zi.colsview(b * n2, n2);
            Mat M = Zb.colsview(0, n), rhs = Zb.colsview(n, n), Rb = Rs.colsview(b * n, n);
            QRFact f = qr_factor(ctx, M);
            qr_apply_q(ctx, f, rhs, true);                                            // Q' rhs
            copy_mat(ctx, f.R, Rb);
        }
        gj_invert_batched(ctx, B, n, Rs.p, piv.p, ctl, BM_GJ, Pn.p, Wp.p);            // R^-1
        hipLaunchKernelGGL(k_bare_ctl_after_inverse, per_member, dim3(64), 0, ctx->stream, ctl, 1);
        // Y = R^-1 (Q' rhs)(0:n, :), Y E^-1, X = sym(Y E^-1)
        gemm_strided(ctx, B, false, false, n, n, n, 1.0, Rs.p, n, nn, Zi.p + (size_t)n * n2, n2, nn4, 0.0, T.p, n, nn, live, "batch_are_extract");
        gemm_strided(ctx, B, false, false, n, n, n, 1.0, T.p, n, nn, Einv.p, n, nn, 0.0, Rs.p, n, nn, live, "batch_are_extract");
        comb_batched(ctx, B, n, n, X.p, 1.0, Rs.p, 0.0, nullptr, 0.0, nullptr, true, live, "batch_are_sym");
    }
    Z = Mat(); Zi = Mat(); Pn = Mat(); Wp = Mat();      // (back to the pool for the refinement)

    // ---- residual and Newton-Kleinman refinement ----
    Mat XE = sq(), AXE = sq(), GXE = sq(), XGX = sq(), Res = sq();
    const double target = 100.0 * n * DBL_EPS;
    // Res_b = R(Xc_b) and the decision, for the members of `mode`
    auto eval = [&](const Mat& Xc, int mode, int phase) {
        const BatchMask mm{ctl, mode, 0};
        gemm_strided(ctx, B, false, false, n, n, n, 1.0, Xc.p, n, nn, E.p, n, nn, 0.0, XE.p, n, nn, mm, "batch_are_residual");      // X E
        gemm_strided(ctx, B, true, false, n, n, n, 1.0, A.p, n, nn, XE.p, n, nn, 0.0, AXE.p, n, nn, mm, "batch_are_residual");      // A' X E
        gemm_strided(ctx, B, false, false, n, n, n, 1.0, G.p, n, nn, XE.p, n, nn, 0.0, GXE.p, n, nn, mm, "batch_are_residual");     // G X E
        gemm_strided(ctx, B, true, false, n, n, n, 1.0, XE.p, n, nn, GXE.p, n, nn, 0.0, XGX.p, n, nn, mm, "batch_are_residual");    // E' X G X E
        TimedScope ts(ctx, "batch_are_residual_sym", 48.0 * B * nn, 0.0);
        hipLaunchKernelGGL(k_bare_residual, dim3(NORM_PARTS, B), blk, 0, ctx->stream, n, (const double*)Q.p, (const double*)AXE.p, (const double*)XGX.p,
                           Res.p, part.p, mm);
        hipLaunchKernelGGL(k_bare_residual_finish, per_member, blk, 0, ctx->stream, (const double*)part.p, target, max_refine, phase, ctl, ext, mm);
    };
    eval(X, BM_LIVE, 0);
    DRE_HIP(hipGetLastError());
    cb.fetch();
    note_failures();
    if (max_refine > 0) {
        Mat F, Xn;
        for (;;) {
            std::vector<int> idx;                    // the members that take a step now
            for (int b = 0; b < B; ++b)
                if (!cb.h(b).fail && cb.h(b).refine) idx.push_back(b);
            if (idx.empty()) break;
            const int Bs = (int)idx.size();
            if (F.empty()) { F = sq(); Xn = sq(); }
            const BatchMask mr{ctl, BM_REFINE, 0};
            comb_batched(ctx, B, n, n, F.p, 1.0, A.p, -1.0, GXE.p, 0.0, nullptr, false, mr, "batch_are_axpby");      // F = A - G X E
            DevArr<int> didx(ctx, (size_t)Bs);
            DRE_HIP(hipMemcpyAsync(didx.p, idx.data(), sizeof(int) * (size_t)Bs, hipMemcpyHostToDevice, ctx->stream));
            Mat Es(ctx, n, n * Bs), Fs(ctx, n, n * Bs), Rsub(ctx, n, n * Bs), Ds(ctx, n, n * Bs);
            {
                TimedScope ts(ctx, "batch_are_gather", 48.0 * Bs * nn, 0.0);
                const dim3 g(grid_for(nn), Bs);
                hipLaunchKernelGGL(k_bare_gather, g, blk, 0, ctx->stream, n, (const double*)E.p, Es.p, (const int*)didx.p);
                hipLaunchKernelGGL(k_bare_gather, g, blk, 0, ctx->stream, n, (const double*)F.p, Fs.p, (const int*)didx.p);
                hipLaunchKernelGGL(k_bare_gather, g, blk, 0, ctx->stream, n, (const double*)Res.p, Rsub.p, (const int*)didx.p);
            }
            DRE_HIP(hipGetLastError());
            {
                BatchedSignLyap lyap(ctx, Bs, Es, maxiters, tol, max_refine);
                lyap.factor(Fs);                                                      // NOT_STABLE: X_b is not the stabilizing solution
                std::vector<SignStats> st;
                lyap.solve(Rsub, Ds, st);                                             // F'DE + E'DF = -R(X)
                for (int j = 0; j < Bs; ++j) {
                    const BatchMemberStatus& ls = lyap.status()[(size_t)j];
                    if (!ls.code) continue;
                    const int b = idx[(size_t)j];
                    status[(size_t)b].code = ls.code;
                    status[(size_t)b].msg = who(b) + "Newton-Kleinman refinement, closed loop A - GXE: " + ls.msg;
                    cb.drop(b, ls.code);
                }
            }
            {
                TimedScope ts(ctx, "batch_are_axpby", 24.0 * Bs * nn, 0.0);
                hipLaunchKernelGGL(k_bare_scatter_step, dim3(grid_for(nn), Bs), blk, 0, ctx->stream, n, (const double*)X.p, (const double*)Ds.p, Xn.p,
                                   (const int*)didx.p, live);
            }
            eval(Xn, BM_REFINE, 1);
            {
                TimedScope ts(ctx, "batch_are_axpby", 16.0 * Bs * nn, 0.0);
                hipLaunchKernelGGL(k_bare_accept, dim3(grid_for(nn), B), blk, 0, ctx->stream, n, (const double*)Xn.p, X.p, (const AreBatchCtl*)ext, live);
            }
            DRE_HIP(hipGetLastError());
            cb.fetch();
        }
    }
    ctx->sync();
    for (int b = 0; b < B; ++b) {
        if (status[(size_t)b].code) continue;
        const BatchCtl h = cb.h(b);
        DenseGareResult& r = out[(size_t)b];
        r.X = X.colsview(b * n, n);
        r.refinements = h.nref; r.res0 = h.res0; r.res = h.s.res;
    }
}

}  // namespace dre
