// Device SVD: one-sided (Hestenes) cyclic block Jacobi (host model: tests/_svd_jacobi_model.py).
//
// The m x w matrix (m >= w; a wide input is transposed on the way in, U and V are swapped at the exit) is padded with zero columns to
// W = 16 p (p >= 2) and cut into p column blocks of 16: the working copy G (m x W), V = I (W x W).  A sweep is the p - 1 (p even) or p (p odd:
// one block sits out per round) rounds of the round-robin tournament of the blocks.  ONE launch per round (k_svjb_round): one workgroup of 256
// per block pair (i, j) forms H = [G_i G_j]'[G_i G_j] (32 x 32, v_mfma_f64_16x16x4_f64, row slabs of 64 through LDS), diagonalises it by cyclic
// Jacobi in LDS (J accumulated) and, if anything was rotated, applies [G_i G_j] <- [G_i G_j] J and [V_i V_j] <- [V_i V_j] J on MFMA.  The pairs
// of a round own disjoint columns, so G and V are updated in place; kernel boundaries are the only synchronisation between workgroups.  After
// every sweep a one-workgroup kernel folds the `rotated` flags into the control block, which the host reads once per sweep; a sweep without a
// rotation ends the iteration.
//
// Every launch carries the member b = blockIdx.y of an ensemble of same-shape matrices (jacobi_common.hpp); svd_jacobi is a batch of one.
// Every member has its own control block, `rotated` flags and partial sums; nothing is summed across members and there are no atomics, so a
// member's result does not depend on the others.  The host reads the B control blocks in one copy per sweep.
//
// Index arithmetic: row and column indices are ints below max(m, W) <= DENSE_MAX_N; every element offset and every member stride is a size_t.
#include <cmath>
#include <numeric>

#include "dense_gj.hpp"
#include "jacobi_common.hpp"
#include "profiling.hpp"

namespace dre {

namespace {

constexpr int LDX = SVJ_SLAB + 1;     // leading dimension of a 64 x 32 row slab in LDS

// rows [r0, r0 + 64) of the column blocks c0 and c1 (first columns) of M (rows x ., leading dimension ld) into Xs; rows beyond `rows` are zero
__device__ inline void svj_load_slab(const double* __restrict__ M, int rows, size_t ld, int c0, int c1, int r0, double* Xs) {
    for (int e = threadIdx.x; e < SVJ_SLAB * PB; e += 256) {
        const int i = e & (SVJ_SLAB - 1), j = e >> 6;
        const int row = r0 + i, col = (j < SB ? c0 : c1) + (j & (SB - 1));
        Xs[i + LDX * j] = row < rows ? M[(size_t)row + (size_t)col * ld] : 0.0;
    }
}

// [M_c0 M_c1] <- [M_c0 M_c1] J, slab by slab: wave w owns the rows 16 w .. 16 w + 15 of the slab in both column tiles
__device__ inline void svj_apply(double* __restrict__ M, int rows, size_t ld, int c0, int c1, const double* J, double* Xs) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lr = lane & 15, lk = lane >> 4;
    for (int r0 = 0; r0 < rows; r0 += SVJ_SLAB) {
        svj_load_slab(M, rows, ld, c0, c1, r0, Xs);
        __syncthreads();
        // MFMA operand maps: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15]; D: column lane & 15, row (lane >> 4) + 4 reg
        v4d acc0 = {0.0, 0.0, 0.0, 0.0}, acc1 = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k0 = 0; k0 < PB; k0 += 4) {
            const double a = Xs[(wave * 16 + lr) + LDX * (k0 + lk)];
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, J[(k0 + lk) + LDP * lr], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, J[(k0 + lk) + LDP * (16 + lr)], acc1, 0, 0, 0);
        }
        // (a wave reads and writes its own 16 rows of the slab only)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            Xs[(wave * 16 + lk + 4 * r) + LDX * lr] = acc0[r];
            Xs[(wave * 16 + lk + 4 * r) + LDX * (16 + lr)] = acc1[r];
        }
        __syncthreads();
        for (int e = tid; e < SVJ_SLAB * PB; e += 256) {
            const int i = e & (SVJ_SLAB - 1), j = e >> 6;
            const int row = r0 + i, col = (j < SB ? c0 : c1) + (j & (SB - 1));
            if (row < rows) M[(size_t)row + (size_t)col * ld] = Xs[i + LDX * j];
        }
        __syncthreads();
    }
}

// ---- one round -------------------------------------------------------------------------------------------------------------------------------
// grid (np pairs of the round, B).  Gs: m x W per member (leading dimension ldg, member stride sg), Vs: W x W per member (stride sv); pairs: the
// round's block pairs (bi < bj); rotateds: this round's np flags of member b at rotateds + b * rstride.
// A rotation (r, c) is done when h_rc != 0, h_rr h_cc > 0, |h_rc| > tol sqrt(h_rr h_cc) and sqrt(h_rr h_cc) > (tol ||A||_F)^2; a skipped rotation is
// the exact identity, so a zero padding column stays a zero column of G and a unit column of V.
__global__ __launch_bounds__(256) void k_svjb_round(int m, int W, double* __restrict__ Gs, size_t ldg, size_t sg, double* __restrict__ Vs, size_t sv,
                                                    const int* __restrict__ pairs, const SvjCtl* __restrict__ ctls, double tol,
                                                    int* __restrict__ rotateds, size_t rstride) {
    __shared__ double Xs[LDX * PB], H[PB * LDP], J[PB * LDP], cs[2 * SB];
    __shared__ int flag;
    const SvjCtl* ctl = ctls + blockIdx.y;
    if (member_off(*ctl)) return;          // (uniform in the workgroup)
    double* G = Gs + (size_t)blockIdx.y * sg;
    double* V = Vs + (size_t)blockIdx.y * sv;
    int* rotated = rotateds + (size_t)blockIdx.y * rstride;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, wr = wave >> 1, wc = wave & 1, lr = lane & 15, lk = lane >> 4;
    const int c0 = pairs[2 * blockIdx.x] * SB, c1 = pairs[2 * blockIdx.x + 1] * SB;
    const double floor_ = (tol * ctl->norm) * (tol * ctl->norm);

    // 1. H = X'X, X = [G_i G_j]: wave (wr, wc) owns the tile (wr, wc); both operands come from the same slab
    v4d acc = {0.0, 0.0, 0.0, 0.0};
    for (int r0 = 0; r0 < m; r0 += SVJ_SLAB) {
        svj_load_slab(G, m, ldg, c0, c1, r0, Xs);
        __syncthreads();
#pragma unroll
        for (int k0 = 0; k0 < SVJ_SLAB; k0 += 4)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Xs[(k0 + lk) + LDX * (wr * 16 + lr)], Xs[(k0 + lk) + LDX * (wc * 16 + lr)], acc, 0, 0, 0);
        __syncthreads();
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) H[(wr * 16 + lk + 4 * r) + LDP * (wc * 16 + lr)] = acc[r];
    for (int e = tid; e < PB * PB; e += 256) J[(e & (PB - 1)) + LDP * (e >> 5)] = (e & (PB - 1)) == (e >> 5) ? 1.0 : 0.0;
    if (tid == 0) flag = 0;
    __syncthreads();

    // 2. cyclic Jacobi on H, J accumulated
    const int any = cyclic_jacobi_32(H, J, cs, &flag, INNER_MAX, [tol, floor_](double app, double aqq, double apq) {
        const double prod = app * aqq;
        if (!(apq != 0.0 && prod > 0.0)) return false;
        const double g = sqrt(prod);
        return fabs(apq) > tol * g && g > floor_;
    });
    if (tid == 0) rotated[blockIdx.x] = any;
    if (!any) return;                // (uniform in the workgroup)

    // 3. [G_i G_j] <- [G_i G_j] J,  [V_i V_j] <- [V_i V_j] J
    svj_apply(G, m, ldg, c0, c1, J, Xs);
    svj_apply(V, W, (size_t)W, c0, c1, J, Xs);
}

// ---- control -------------------------------------------------------------------------------------------------------------------------------
// grid (NORM_PARTS, B): the partial sums of member b in parts + NORM_PARTS b
__global__ __launch_bounds__(256) void k_svjb_sumsq(int rows, int cols, const double* __restrict__ As, size_t ld, size_t stride, double* __restrict__ parts) {
    const double* A = As + (size_t)blockIdx.y * stride;
    double s = 0.0;
    const size_t tot = (size_t)rows * (size_t)cols;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < tot; idx += (size_t)gridDim.x * blockDim.x) {
        const double x = A[idx % (size_t)rows + (idx / (size_t)rows) * ld];
        s += x * x;
    }
    store_partials(parts + (size_t)blockIdx.y * gridDim.x, s);
}

// grid (B)
__global__ __launch_bounds__(256) void k_svjb_init(int nparts, const double* __restrict__ parts, SvjCtl* ctls) {
    SvjCtl* ctl = ctls + blockIdx.x;
    double s[1];
    load_partials(nparts, parts + (size_t)blockIdx.x * nparts, s);
    if (threadIdx.x == 0) {
        const double norm = sqrt(s[0]);
        ctl->norm = norm; ctl->pad0_ = 0.0;
        ctl->sweeps = 0; ctl->done = 0; ctl->failed = 0;
        ctl->nonfinite = isfinite(norm) ? 0 : 1;
    }
}

// grid (B): n flags per member at rotateds + b * n; a member still rotating after SVJ_MAX_SWEEPS sweeps is dropped here
__global__ __launch_bounds__(256) void k_svjb_fold(int n, const int* __restrict__ rotateds, SvjCtl* ctls) {
    SvjCtl* ctl = ctls + blockIdx.x;
    if (member_off(*ctl)) return;          // (uniform in the workgroup)
    const int* rotated = rotateds + (size_t)blockIdx.x * n;
    int any = 0;
    for (int i = threadIdx.x; i < n; i += 256) any |= rotated[i];
    any = __syncthreads_or(any);
    if (threadIdx.x == 0) {
        ctl->sweeps += 1; ctl->done = any ? 0 : 1;
        ctl->failed = any && ctl->sweeps >= SVJ_MAX_SWEEPS ? 1 : 0;
    }
}

// ---- exit ----------------------------------------------------------------------------------------------------------------------------------
// grid (w, B), one workgroup per column: sig[b w + c] = ||G_b(:, c)||
__global__ __launch_bounds__(256) void k_svjb_colnorm(int m, const double* __restrict__ Gs, size_t ldg, size_t sg, double* __restrict__ sig) {
    __shared__ double red[17];
    const double* g = Gs + (size_t)blockIdx.y * sg + (size_t)blockIdx.x * ldg;
    double s = 0.0;
    for (int i = threadIdx.x; i < m; i += 256) s += g[i] * g[i];
    s = block_sum(s, red);
    if (threadIdx.x == 0) sig[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = sqrt(s);
}

// grid (., B): U(:, j) = G(:, perm[j]) / sig[j] where sig[j] > thr = tol ||A_b||_F, a zero column otherwise;  Vout(:, j) = V(0 .. w, perm[j]).
// perm and sig are w per member, U m x w, Vout w x w per member (contiguous)
__global__ __launch_bounds__(256) void k_svjb_gather(int m, int w, const double* __restrict__ Gs, size_t ldg, size_t sg, const double* __restrict__ Vs, size_t ldv,
                                                     size_t sv, const int* __restrict__ perms, const double* __restrict__ sigs, double tol,
                                                     const SvjCtl* __restrict__ ctls, double* __restrict__ Us, double* __restrict__ Vouts) {
    const SvjCtl* ctl = ctls + blockIdx.y;
    if (ctl->nonfinite | ctl->failed) return;
    const double thr = tol * ctl->norm;
    const double* G = Gs + (size_t)blockIdx.y * sg;
    const double* V = Vs + (size_t)blockIdx.y * sv;
    const int* perm = perms + (size_t)blockIdx.y * w;
    const double* sig = sigs + (size_t)blockIdx.y * w;
    double* U = Us + (size_t)blockIdx.y * (size_t)m * (size_t)w;
    double* Vout = Vouts + (size_t)blockIdx.y * (size_t)w * (size_t)w;
    const size_t ldu = (size_t)m, ldvo = (size_t)w;
    const size_t h = (size_t)m + (size_t)w, tot = h * (size_t)w;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < tot; idx += (size_t)gridDim.x * blockDim.x) {
        const int j = (int)(idx / h), i = (int)(idx % h);
        const size_t src = (size_t)perm[j];
        if (i < m) U[(size_t)i + (size_t)j * ldu] = sig[j] > thr ? G[(size_t)i + src * ldg] / sig[j] : 0.0;
        else Vout[(size_t)(i - m) + (size_t)j * ldvo] = V[(size_t)(i - m) + src * ldv];
    }
}

// a rows x cols view (contiguous columns) at `off` doubles into a stack
Mat stack_view(const DevArr<double>& st, size_t off, int rows, int cols) {
    Mat m;
    m.buf = st.buf; m.p = st.p + off; m.rows = rows; m.cols = cols; m.ld = rows > 0 ? rows : 1;
    return m;
}

}  // namespace

SvdBatch svd_jacobi_run(Ctx* ctx, const std::vector<Mat>& A, double tol, const char* who, bool single) {
    check_batch(A, who);
    const int B = (int)A.size(), rows = A[0].rows, cols = A[0].cols;
    const int m = std::max(rows, cols), w = std::min(rows, cols);
    const bool wide = rows < cols;
    DRE_REQUIRE(rows >= 0 && cols >= 0, std::string(who) + ": negative shape");
    DRE_REQUIRE(w <= SVJ_MAX_W, std::string(who) + ": the shorter dimension is limited to 4096");
    DRE_REQUIRE(m <= DENSE_MAX_N, std::string(who) + ": the longer dimension is beyond the device's 32-bit index limit");
    DRE_REQUIRE(std::isfinite(tol), std::string(who) + ": tol is not finite");
    SvdBatch out;
    out.svd.resize((size_t)B); out.stats.resize((size_t)B); out.status.resize((size_t)B);
    if (w == 0) {
        for (auto& r : out.svd) { r.U = Mat(ctx, rows, 0); r.S = Mat(ctx, 0, 1); r.V = Mat(ctx, cols, 0); }
        return out;
    }
    const int p = std::max(2, ceil_div(w, SB)), W = p * SB, nrounds = p - 1 + (p & 1), np = p / 2;
    const size_t sg = (size_t)m * W, sv = (size_t)W * W, ldg = (size_t)m, nrot = (size_t)nrounds * np;
    // per member: G, V, the outputs, partial sums and the small arrays
    require_memory(ctx, (size_t)B * (sg + sv + 2 * (size_t)m * w + (size_t)w * w + NORM_PARTS + 4 * (size_t)W + (size_t)(W / SB) * (W / SB)));

    const std::vector<int> tab = rr_schedule(p, false);
    DevArr<int> dtab(ctx, tab.size());
    dtab.upload(ctx, tab);

    // G_b = [A_b 0] (m x W; a wide member is transposed on the way in), V_b = I
    DevArr<double> G(ctx, (size_t)B * sg), V(ctx, (size_t)B * sv), part(ctx, (size_t)B * NORM_PARTS), dsig(ctx, (size_t)B * w);
    DevArr<int> rotated(ctx, (size_t)B * nrot), dperm(ctx, (size_t)B * w);
    DevArr<SvjCtl> ctl(ctx, (size_t)B);
    if (W != w) DRE_HIP(hipMemsetAsync(G.p, 0, (size_t)B * sg * sizeof(double), ctx->stream));
    if (wide) {
        for (int b = 0; b < B; ++b) { Mat left = stack_view(G, (size_t)b * sg, m, w); transpose_mat(ctx, A[(size_t)b], left); }
    } else {
        std::vector<CopyDesc> cp((size_t)B);
        for (int b = 0; b < B; ++b) cp[(size_t)b] = CopyDesc{A[(size_t)b].p, G.p + (size_t)b * sg, m, w, A[(size_t)b].ld, m};
        copy_batched(ctx, cp);
    }
    hipLaunchKernelGGL(k_jb_eye, dim3(grid_for(sv), B), dim3(256), 0, ctx->stream, W, V.p, sv);
    {
        TimedScope ts(ctx, single ? "svj_norm" : "svjb_norm", 8.0 * B * m * w, 0.0, 2);
        hipLaunchKernelGGL(k_svjb_sumsq, dim3(NORM_PARTS, B), dim3(256), 0, ctx->stream, m, w, (const double*)G.p, ldg, sg, part.p);
        hipLaunchKernelGGL(k_svjb_init, dim3(B), dim3(256), 0, ctx->stream, NORM_PARTS, (const double*)part.p, ctl.p);
    }
    std::vector<SvjCtl> h((size_t)B);
    fetch_ctl(ctx, ctl, h);
    if (!(tol > 0.0)) tol = std::sqrt((double)m) * DBL_EPS;
    auto judge = [&] {
        bool live = false;
        for (int b = 0; b < B; ++b) {
            if (h[(size_t)b].done || out.status[(size_t)b].code) continue;
            if (h[(size_t)b].nonfinite) out.status[(size_t)b] = {ERR_INVALID, "the matrix has non-finite entries"};
            else if (h[(size_t)b].failed) out.status[(size_t)b] = {ERR_INTERNAL, "no convergence in " + std::to_string(h[(size_t)b].sweeps) + " sweeps"};
            else live = true;
        }
        return live;
    };
    bool live = judge();
    while (live) {
        {
            TimedScope ts(ctx, single ? "svj_round" : "svjb_round", 16.0 * B * nrounds * ((double)m + W) * W, 2.0 * B * nrounds * np * (3.0 * m + 2.0 * W) * PB * PB,
                          nrounds);
            for (int r = 0; r < nrounds; ++r)
                hipLaunchKernelGGL(k_svjb_round, dim3(np, B), dim3(256), 0, ctx->stream, m, W, G.p, ldg, sg, V.p, sv, (const int*)(dtab.p + (size_t)r * 2 * np),
                                   (const SvjCtl*)ctl.p, tol, rotated.p + (size_t)r * np, nrot);
        }
        hipLaunchKernelGGL(k_svjb_fold, dim3(B), dim3(256), 0, ctx->stream, (int)nrot, (const int*)rotated.p, ctl.p);
        fetch_ctl(ctx, ctl, h);
        live = judge();
    }
    DRE_HIP(hipGetLastError());

    // sigma = column norms of every member in one copy, sorted per member on the host (stable, descending); the permutations in one upload
    hipLaunchKernelGGL(k_svjb_colnorm, dim3(w, B), dim3(256), 0, ctx->stream, m, (const double*)G.p, ldg, sg, dsig.p);
    std::vector<double> sig((size_t)B * w), ssort((size_t)B * w);
    DRE_HIP(hipMemcpyAsync(sig.data(), dsig.p, sig.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    ctx->sync();
    std::vector<int> perm((size_t)B * w);
    for (int b = 0; b < B; ++b) {
        int* pb = perm.data() + (size_t)b * w;
        const double* sb = sig.data() + (size_t)b * w;
        std::iota(pb, pb + w, 0);
        if (out.status[(size_t)b].code) continue;          // (a dropped member's columns are not looked at)
        std::stable_sort(pb, pb + w, [&](int a, int c) { return sb[a] > sb[c]; });
        SvdResult& r = out.svd[(size_t)b];
        r.s.resize((size_t)w);
        for (int j = 0; j < w; ++j) r.s[(size_t)j] = ssort[(size_t)b * w + j] = sb[pb[j]];
        const double thr = tol * h[(size_t)b].norm;
        long rank = 0;
        for (int j = 0; j < w; ++j) rank += r.s[(size_t)j] > thr ? 1 : 0;
        r.norm = h[(size_t)b].norm;
        out.stats[(size_t)b].sweeps = h[(size_t)b].sweeps;
        out.stats[(size_t)b].rounds = (long)nrounds * h[(size_t)b].sweeps;
        out.stats[(size_t)b].rank = rank;
    }
    dperm.upload(ctx, perm);
    DevArr<double> Ss(ctx, (size_t)B * w), Us(ctx, (size_t)B * m * w), Vo(ctx, (size_t)B * w * w);
    Ss.upload(ctx, ssort);
    hipLaunchKernelGGL(k_svjb_gather, dim3(grid_for(((size_t)m + w) * w), B), dim3(256), 0, ctx->stream, m, w, (const double*)G.p, ldg, sg, (const double*)V.p,
                       (size_t)W, sv, (const int*)dperm.p, (const double*)Ss.p, tol, (const SvjCtl*)ctl.p, Us.p, Vo.p);
    DRE_HIP(hipGetLastError());
    ctx->sync();
    for (int b = 0; b < B; ++b) {
        if (out.status[(size_t)b].code) continue;
        SvdResult& r = out.svd[(size_t)b];
        const SvjStats& st = out.stats[(size_t)b];
        r.S = stack_view(Ss, (size_t)b * w, w, 1);
        r.U = stack_view(Us, (size_t)b * m * w, m, w);
        r.V = stack_view(Vo, (size_t)b * w * w, w, w);
        if (wide) std::swap(r.U, r.V);
        if (!env_trace("compress")) continue;
        if (single) std::fprintf(stderr, "[svd_jacobi] %d x %d: %ld sweeps, %ld rounds, rank %ld\n", m, w, st.sweeps, st.rounds, st.rank);
        else std::fprintf(stderr, "[svd_jacobi_batch] member %d, %d x %d: %ld sweeps, rank %ld\n", b, rows, cols, st.sweeps, st.rank);
    }
    return out;
}

SvdBatch svd_jacobi_batch(Ctx* ctx, const std::vector<Mat>& A, double tol, const char* who) {
    SvdBatch out = svd_jacobi_run(ctx, A, tol, who, false);
    name_members(out.status, who);
    return out;
}

SvdResult svd_jacobi(Ctx* ctx, const Mat& A, double tol, SvjStats* stats) {
    if (stats) *stats = SvjStats{};
    SvdBatch r = svd_jacobi_run(ctx, {A}, tol, "svd_jacobi", true);
    if (r.status[0].code) throw Error(r.status[0].code, "svd_jacobi: " + r.status[0].msg);
    if (stats) *stats = r.stats[0];
    return std::move(r.svd[0]);
}

}  // namespace dre
