// Operator products of a real Cyclic shift list on the dense-inverse path: SMW products and packed stacks per shift (cycle_ops_prepare), and the
// group chain's K-independent base and per-step fold (group_base_build, group_ops_prepare).  Used by the dense-X time step (dense_x.hip).
#include "adi_cycle.hpp"

#include <algorithm>
#include <cstring>
#include <map>

#include "hostla.hpp"
#include "profiling.hpp"

namespace dre {

typedef double v4d __attribute__((ext_vector_type(4)));
// 16-row strip of  W = Apk X  (X: n x ncols <= 32, column-major), K split over the four waves; returns this thread's element (row lk + 4 wave,
// column 16 j + lr) of both column tiles in v0 / v1
__device__ __forceinline__ void group_thin_tile(const double* __restrict__ Apk_strip, const double* __restrict__ X, int ldx, int n, int ncols,
                                                double (*part)[2][4][64], double& v0, double& v1) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lk = lane >> 4, lr = lane & 15;
    const int kst = (n + 3) >> 2, per = (kst + 3) >> 2;
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const int t0 = wv * per, t1 = min(kst, t0 + per);
    const bool c0ok = lr < ncols, c1ok = 16 + lr < ncols;
    const double* __restrict__ ap = Apk_strip + lane;
    const double* __restrict__ x0 = X + (size_t)(c0ok ? lr : 0) * ldx;
    const double* __restrict__ x1 = X + (size_t)(c1ok ? 16 + lr : 0) * ldx;
    v4d acc0 = (v4d){0.0, 0.0, 0.0, 0.0}, acc1 = (v4d){0.0, 0.0, 0.0, 0.0};
    for (int tb = t0; tb < t1; tb += 24) {
        double av[24], b0[24], b1[24];
#pragma unroll
        for (int u = 0; u < 24; ++u) {
            const int t = min(tb + u, t1 - 1);
            const int c = min(4 * t + lk, n - 1);
            av[u] = ap[(size_t)t * 64]; b0[u] = x0[c]; b1[u] = x1[c];
        }
#pragma unroll
        for (int u = 0; u < 24; ++u) {
            const bool kok = (tb + u < t1) && 4 * (tb + u) + lk < n;
            const double a = kok ? av[u] : 0.0;
            acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (kok && c0ok) ? b0[u] : 0.0, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, (kok && c1ok) ? b1[u] : 0.0, acc1, 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) { part[wave][0][r][lane] = acc0[r]; part[wave][1][r][lane] = acc1[r]; }
    __syncthreads();
    v0 = ((part[0][0][wave][lane] + part[1][0][wave][lane]) + part[2][0][wave][lane]) + part[3][0][wave][lane];
    v1 = ((part[0][1][wave][lane] + part[1][1][wave][lane]) + part[2][1][wave][lane]) + part[3][1][wave][lane];
}
// W_s = stack_s X for every shift s of the cycle in one launch (X: n x ncols <= 32, the same for all): the SMW products N K', E'N K', B'N K'
struct StackThinBatch { const double* Apk[16]; double* W[16]; };
__global__ __launch_bounds__(256) void k_stack_thin(int M, int n, int ncols, const double* __restrict__ X, int ldx, int ldw, StackThinBatch bt) {
    __shared__ double part[4][2][4][64];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lk = lane >> 4, lr = lane & 15;
    const int kst = (n + 3) >> 2;
    double v0, v1;
    group_thin_tile(bt.Apk[blockIdx.y] + (size_t)blockIdx.x * kst * 64, X, ldx, n, ncols, part, v0, v1);
    const int orow = blockIdx.x * 16 + lk + 4 * wave;
    if (orow >= M) return;
    double* __restrict__ W = bt.W[blockIdx.y];
    if (lr < ncols) W[orow + (size_t)lr * ldw] = v0;
    if (16 + lr < ncols) W[orow + (size_t)(16 + lr) * ldw] = v1;
}
static void ensure_stack(Ctx* ctx, const GaleOperator& op, FactorEntry<double>& fe) {
    const Pencil& P = *op.P;
    const int n = P.n, mm = op.has_lr ? op.U.cols : 0;
    if (!fe.stack.empty() && fe.stack_m == mm && (!mm || fe.stack_U == (const void*)op.U.p)) return;
    Mat stk(ctx, 2 * n + mm, n);
    { Mat top = stk.view(0, 0, n, n); copy_mat(ctx, fe.dinv, top); }
    { Mat mid = stk.view(n, 0, n, n); spmm(ctx, P, P.valEt.p, fe.dinv, mid, 1.0, 0.0, nullptr); }
    if (mm) { Mat bot = stk.view(2 * n, 0, mm, n); gemm(ctx, true, false, 1.0, op.U, fe.dinv, 0.0, bot, nullptr, "gemm_dinv"); }
    fe.stack = stk; fe.stack_U = (const void*)op.U.p; fe.stack_m = mm;
}
// Acceptance norms of the batched set-up below, as partial sums the host adds up: out[17 z] = ||F + mu_z E||_F^2 (value arrays),
// out[17 z + 1 .. 17 z + 16] = sums of squares of sixteen column slabs of N_z (n x n, leading dimension ldw)
struct SetupNormZ { double mu[MF_ZMAX]; };
__global__ __launch_bounds__(256) void k_setup_norms_z(int nnz, const double* __restrict__ valF, const double* __restrict__ valE, SetupNormZ mz, int n,
                                                       const double* __restrict__ W, int ldw, long wz, double* __restrict__ out) {
    const int z = blockIdx.x, part = blockIdx.y, tid = threadIdx.x;
    double s = 0.0;
    if (part == 0) {
        const double mu = mz.mu[z];
        for (int i = tid; i < nnz; i += 256) { const double v = valF[i] + mu * valE[i]; s += v * v; }
    } else {
        const double* __restrict__ Wz = W + (size_t)z * wz;
        const int cw = (n + 15) / 16, c0 = (part - 1) * cw, c1 = min(n, c0 + cw);
        for (int c = c0; c < c1; ++c)
            for (int r = tid; r < n; r += 256) { const double v = Wz[r + (size_t)c * ldw]; s += v * v; }
    }
    __shared__ double sh[4];
    s = wave_sum_d(s);
    if ((tid & 63) == 0) sh[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) out[17 * z + part] = (sh[0] + sh[1]) + (sh[2] + sh[3]);
}
// Set-up of a whole real Cyclic list on the dense-inverse path (n <= dense_inv_max_n) in SHARED launches: every missing factorisation
// (mf_factor_batch: one launch per tree level for all shifts), the explicit inverses N_z = M_z^-1 through one batched solve with the identity
// as common right-hand side (mf_solve_batch), the stacked inverses [N_z; E'N_z; U'N_z] of all shifts as ONE matrix (one SpMM, one GEMM) and
// the acceptance norms — ~25 launches instead of ~30 per shift on helper streams (1.6 of the 2.2 ms of the first time step at n = 371).
// Fills the factor cache; shifts it cannot take (already cached, more than MF_ZMAX, sweeps without the matrix cores) go through get_factor.
static void cycle_setup_batched(Ctx* ctx, const GaleOperator& op, const std::vector<std::complex<double>>& values, FactorCache* cache) {
    const Pencil& P = *op.P;
    const int n = P.n, mm = op.has_lr ? op.U.cols : 0;
    if (!cache->enabled || !P.use_mfma_sweeps || n > ctx->dense_inv_max_n || ctx->setup_batched <= 0) return;
    const std::vector<double> todo = distinct_real_shifts(values, MF_ZMAX, [&](size_t, double mu) { return cache->real.count(std::make_tuple(op.tag, mu, 0.0)) > 0; });
    const int g = (int)todo.size();
    if (g < 2) return;
    std::vector<std::shared_ptr<FactorEntry<double>>> fes;
    std::vector<Factor<double>*> fp;
    std::vector<const Factor<double>*> cf;
    for (int z = 0; z < g; ++z) { fes.push_back(std::make_shared<FactorEntry<double>>()); fp.push_back(&fes.back()->f); cf.push_back(&fes.back()->f); }
    mf_factor_batch<double>(ctx, P, op.valFt.p, P.valEt.p, 1.0, todo.data(), fp.data(), g);
    Mat STK(ctx, 2 * n + mm, n * g), Id(ctx, n, n);
    set_identity(ctx, Id, 1.0);
    if (!mf_solve_batch(ctx, P, cf.data(), g, Id.p, Id.ld, n, STK.p, STK.ld, n)) return;       // (the factors are dropped: get_factor redoes them one by one)
    DevArr<double> nr(ctx, (size_t)17 * g);
    SetupNormZ mz; std::memset(&mz, 0, sizeof(mz));
    for (int z = 0; z < g; ++z) mz.mu[z] = todo[(size_t)z];
    hipLaunchKernelGGL(k_setup_norms_z, dim3((unsigned)g, 17), dim3(256), 0, ctx->stream, P.nnz, (const double*)op.valFt.p, (const double*)P.valEt.p, mz, n,
                       (const double*)STK.p, STK.ld, (long)n * STK.ld, nr.p);
    {
        Mat top = STK.view(0, 0, n, n * g), mid = STK.view(n, 0, n, n * g);
        spmm(ctx, P, P.valEt.p, top, mid, 1.0, 0.0, nullptr);
        if (mm) { Mat bot = STK.view(2 * n, 0, mm, n * g); gemm(ctx, true, false, 1.0, op.U, top, 0.0, bot, nullptr, "gemm_dinv"); }
    }
    std::vector<double> hp((size_t)17 * g), h((size_t)2 * g, 0.0);
    ctx_fetch(ctx, nr.p, hp.size() * sizeof(double), hp.data());
    for (int z = 0; z < g; ++z) { h[2 * z] = hp[17 * z]; for (int i = 1; i <= 16; ++i) h[2 * z + 1] += hp[17 * z + i]; }
    const std::vector<double> gr = mf_check_batch(ctx, cf);
    for (int z = 0; z < g; ++z) {
        auto& fe = *fes[(size_t)z];
        fe.growth = gr[(size_t)z]; fe.checked = true;
        fe.f.allow_topinv = true;
        const double cond_est = std::sqrt(h[2 * z]) * std::sqrt(h[2 * z + 1]);
        if (cond_est == cond_est && cond_est < 1e7 && fe.f.nperturbed <= 0) {
            fe.stack = STK.view(0, z * n, 2 * n + mm, n); fe.stack_U = (const void*)op.U.p; fe.stack_m = mm;
            fe.dinv = STK.view(0, z * n, n, n); fe.dense = true;
        }
        const auto key = std::make_tuple(op.tag, todo[(size_t)z], 0.0);
        cache->real[key] = fes[(size_t)z]; cache->fresh.push_back(key); cache->nfactor++;
    }
}
bool cycle_ops_prepare(Ctx* ctx, const GaleOperator& op, const std::vector<std::complex<double>>& values, FactorCache* cache, CycleOps& co, std::vector<Mat>* wks_store,
                       const std::vector<Mat>* spack, bool defer_single) {
    const Pencil& P = *op.P;
    const int n = P.n, m = op.has_lr ? op.U.cols : 0;
    if (m > 32) return false;
    std::map<double, double*> by_mu;
    std::map<double, const double*> wks_by_mu;
    std::vector<GemmBatchDesc> descs;
    std::vector<SmwBatch> hb;
    std::vector<const double*> stacks, wks; std::vector<double*> outs;
    for (auto& mu : values) if (mu.imag() != 0.0) return false;
    cycle_setup_batched(ctx, op, values, cache);
    {
        // Every factorisation and dense inverse of the cycle is enqueued before the single read-back of the acceptance norms.  Each of
        // them is a chain of ~25 small kernels (assembly, one factorisation launch per tree level, n unit right-hand sides, norms) that
        // uses a few CUs: the chains of different shifts go to different helper streams and run side by side.
        DeferredDense dd;
        dd.cap = std::min<int>((int)values.size(), 256);
        dd.norms = DevArr<double>(ctx, (size_t)2 * dd.cap);
        int todo = 0;
        for (auto& mu : values) if (!cache->enabled || !cache->real.count(std::make_tuple(op.tag, mu.real(), mu.imag()))) ++todo;
        const int nh = (cache->enabled && todo > 1) ? std::min(todo, std::max(0, ctx->setup_streams)) : 0;
        if (nh > 1) {
            helpers_grow(ctx, nh);
            // (the look-ahead of the ADI, engine.hip Prefetcher::next_helper, also copies pivot_static onto its helpers; this list does not)
            if (!ctx->helper_e0) DRE_HIP(hipEventCreateWithFlags(&ctx->helper_e0, hipEventDisableTiming));
            DRE_HIP(hipEventRecord(ctx->helper_e0, ctx->stream));         // the operator's value arrays are ready here
            for (int h = 0; h < nh; ++h) {
                Ctx* hc = ctx->helpers[(size_t)h].get();
                hc->dense_inv_max_n = ctx->dense_inv_max_n; hc->top_inverse_max_rows = ctx->top_inverse_max_rows; hc->mf_subtree = ctx->mf_subtree;
                hc->pivot_growth_warn = ctx->pivot_growth_warn; hc->pivot_growth_fail = ctx->pivot_growth_fail;
                hc->timer->enabled = ctx->timer && ctx->timer->enabled;
                DRE_HIP(hipStreamWaitEvent(hc->stream, ctx->helper_e0, 0));
            }
            int j = 0;
            for (auto& mu : values) {
                if (cache->real.count(std::make_tuple(op.tag, mu.real(), mu.imag()))) continue;
                (void)get_factor<double>(ctx->helpers[(size_t)(j % nh)].get(), op, cache, cache->real, mu, true, &dd);
                ++j;
            }
            for (int h = 0; h < nh; ++h) {
                DRE_HIP(hipEventRecord(ctx->helper_ev[(size_t)h], ctx->helpers[(size_t)h]->stream));
                DRE_HIP(hipStreamWaitEvent(ctx->stream, ctx->helper_ev[(size_t)h], 0));
            }
        } else {
            for (auto& mu : values) (void)get_factor<double>(ctx, op, cache, cache->real, mu, true, &dd);
        }
        finalize_dense(ctx, dd);
    }
    size_t pos_idx = 0;
    for (auto& mu : values) {
        const size_t pos = pos_idx++;
        auto fe = get_factor<double>(ctx, op, cache, cache->real, mu, true);
        if (!fe->dense) return false;
        ensure_stack(ctx, op, *fe);
        co.fe.push_back(fe);
        auto bm = by_mu.find(mu.real());
        if (bm == by_mu.end()) {
            Mat pk(ctx, (int)(adi_fast_pack_doubles(n) / 64), 64);
            co.keep.push_back(pk);
            const double* wksp = nullptr;
            if (m) {
                Mat WK(ctx, 2 * n + m, m);
                Mat WKS = (wks_store && pos < wks_store->size()) ? (*wks_store)[pos] : Mat(ctx, 2 * n, m);
                auto sinv = std::make_shared<Buf>(ctx, (size_t)m * m * sizeof(double));
                co.keep.push_back(WK); co.keep.push_back(WKS); co.keepb.push_back(sinv);
                descs.push_back({fe->stack.p, op.Vt.p, WK.p, nullptr, 1.0, 2 * n + m, m, n, fe->stack.ld, op.Vt.ld, WK.ld, 0});
                hb.push_back({WK.p, (double*)sinv->p, WKS.p});
                wksp = WKS.p;
            }
            stacks.push_back(fe->stack.p); wks.push_back(wksp); outs.push_back(pk.p);
            bm = by_mu.emplace(mu.real(), pk.p).first;
            wks_by_mu[mu.real()] = wksp;
        }
        co.pack.push_back(bm->second);
        co.wks_pos.push_back(wks_by_mu[mu.real()]);
    }
    if (m) {
        co.serr8 = DevArr<long long>(ctx, 1);
        co.serr = DevArr<int>();
        co.serr.buf = co.serr8.buf; co.serr.p = (int*)co.serr8.p; co.serr.n = 2;     // the kernels write the low word
        DRE_HIP(hipMemsetAsync(co.serr8.p, 0, sizeof(long long), ctx->stream));
        if (spack && spack->size() == values.size() && m <= 32 && descs.size() <= 16 && descs.size() == values.size()) {
            // WK_s = stack_s K' for every shift in one launch on the packed stacks (the general batched GEMM spends 31 us on these 749 x 371 x 7 products)
            StackThinBatch tb;
            for (size_t i = 0; i < 16; ++i) { const size_t j = i < descs.size() ? i : 0; tb.Apk[i] = (*spack)[j].p; tb.W[i] = descs[j].C; }
            TimedScope ts(ctx, "gemm_dinv", 8.0 * descs.size() * (2.0 * n + m) * n, 2.0 * descs.size() * (2.0 * n + m) * n * (double)m);
            hipLaunchKernelGGL(k_stack_thin, dim3(ceil_div(2 * n + m, 16), (unsigned)descs.size()), dim3(256), 0, ctx->stream, 2 * n + m, n, m, (const double*)op.Vt.p,
                               op.Vt.ld, 2 * n + m, tb);
        } else gemm_batched(ctx, descs, "gemm_dinv");
        smw_sinv_fold_batched(ctx, n, m, op.alpha, hb.data(), (int)hb.size(), co.serr.p);
    }
    if (defer_single) {
        co.single_built = false;
        co.build_single = [n, m, stacks, wks, outs](Ctx* c) { adi_fast_build(c, n, m, stacks, 2 * n + m, wks, 2 * n, outs); };
    } else adi_fast_build(ctx, n, m, stacks, 2 * n + m, wks, 2 * n, outs);
    return true;
}

// ---- group chain (dense.hip, k_adi_group): operator products of g consecutive ADI iterations --------------------------------------
// With N_s = (A' + (mu_s - 1/(2 tau)) E')^-1 (K independent, kept per shift as stack_s = [N_s; E'N_s; B'N_s]) the shifted operator of a time
// step is a rank-m correction (Sherman-Morrison-Woodbury, smw.jl:20-43):  A_s = N_s + a_s b_s',  P_s = I - 2 mu_s E'A_s = P0_s + c_s b_s'
// with a_s = -(N_s K' Sinv_s), c_s = 2 mu_s (E'N_s K' Sinv_s), b_s' = B'N_s.  For the g shifts s_0 .. s_{g-1} of a group (index i for s_i):
//   Pi_i = P_{i-1} ... P_0 = Pi0_i + X_i Y_i',      Om_i = A_i Pi_i = Om0_i + [N_i X_i, a_i] Y_{i+1}',
//   X_i  block j (j < i)  = Phi(j+1, i) c_j,        Phi(a, b) = P0_{b-1} ... P0_a   (K independent; Pi0_i = Phi(0, i), Om0_i = N_i Phi(0, i)),
//   Y_{i+1} = [Y_i, y_i],  y_i = Pi_i' b_i = D_i' + sum_{j<i} y_j M(j, i),   D_i = b_i' Phi(0, i),   M(j, i) = c_j' Psi(j, i),   Psi(j, i) = Phi(j+1, i)' b_i.
// Everything K independent (Phi, N Phi, Psi, D: GroupBase) is formed ONCE per run — one stacked product stack_b Phi(a, b) delivers
// N_b Phi(a, b), the next Phi(a, b+1) and Psi(a-1, b)' at once — and a time step costs three launches on the side stream: the left-factor
// blocks (independent thin products, no recursion), the rows of Y, and the fold + packing of the effective group stack.
// out(16-row strip) = scale * Mtx(strip, :) v   (v: n x m, m <= 16), K split over the four waves;  kind 1: the m x m matrix scale * v' P' with P = Mtx (m x n)
__global__ __launch_bounds__(256) void k_group_left(int n, int m, const GroupLeftDesc* __restrict__ table) {
    __shared__ double part[4][4][64];
    const GroupLeftDesc d = table[blockIdx.y];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lk = lane >> 4, lr = lane & 15;
    if (d.kind == 1) {
        if (blockIdx.x > 0) return;
        // M[u, v] = scale * sum_r vv[r, u] * PsiT[v, r]
        for (int e = tid; e < m * m; e += 256) {
            const int u = e % m, vv = e / m;
            double sacc = 0.0;
            for (int r = 0; r < n; ++r) sacc += d.v[r + (size_t)u * d.ldv] * d.Mtx[vv + (size_t)r * d.ldm];
            d.out[u + (size_t)vv * d.ldo] = d.scale * sacc;
        }
        return;
    }
    const int row0 = blockIdx.x * 16;
    if (row0 >= n) return;
    if (!d.Mtx) {
        for (int e = tid; e < 16 * m; e += 256) {
            const int r = row0 + (e & 15), c = e >> 4;
            if (r < n) d.out[r + (size_t)c * d.ldo] = d.scale * d.v[r + (size_t)c * d.ldv];
        }
        return;
    }
    const int row = row0 + lr;
    const bool rok = row < n, cok = lr < m;
    const int kst = (n + 3) >> 2, per = (kst + 3) >> 2;
    const int wv = __builtin_amdgcn_readfirstlane(wave);
    const int t0 = wv * per, t1 = min(kst, t0 + per);
    const double* __restrict__ ap = d.Mtx + (rok ? row : 0);
    const double* __restrict__ xp = d.v + (size_t)(cok ? lr : 0) * d.ldv;
    v4d acc = (v4d){0.0, 0.0, 0.0, 0.0};
    for (int tb = t0; tb < t1; tb += 24) {
        double av[24], bv[24];
#pragma unroll
        for (int u = 0; u < 24; ++u) {
            const int c = min(4 * min(tb + u, t1 - 1) + lk, n - 1);
            av[u] = ap[(size_t)c * d.ldm]; bv[u] = xp[c];
        }
#pragma unroll
        for (int u = 0; u < 24; ++u) {
            const bool kok = (tb + u < t1) && 4 * (tb + u) + lk < n;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64((kok && rok) ? av[u] : 0.0, (kok && cok) ? bv[u] : 0.0, acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) part[wave][r][lane] = acc[r];
    __syncthreads();
    const double vsum = ((part[0][wave][lane] + part[1][wave][lane]) + part[2][wave][lane]) + part[3][wave][lane];
    const int orow = row0 + lk + 4 * wave;
    if (orow < n && lr < m) d.out[orow + (size_t)lr * d.ldo] = d.scale * vsum;
}
// rows of Y' = [y_0 .. y_{g-1}]':  y_i = D_i' + sum_{j<i} y_j M(j, i).  One thread per (row, component v); the g levels are sequential, the
// row's earlier y_j go through LDS (32 rows per workgroup, 8 component slots per row).
struct GroupYOne { const double* D; const double* Mb; double* Yt; };
struct GroupYBatch { GroupYOne s[8]; };
__global__ __launch_bounds__(256) void k_group_y(int n, int m, int g, int ldd, GroupYBatch bt) {
    __shared__ double ysh[32][ADI_GROUP_MAX_G][8];
    __shared__ double msh[ADI_GROUP_MAX_G * ADI_GROUP_MAX_G][8][8];
    const GroupYOne& o = bt.s[blockIdx.y];
    const int rl = threadIdx.x >> 3, v = threadIdx.x & 7;
    const int rr = blockIdx.x * 32 + rl;
    const int r = m * g;
    for (int e = threadIdx.x; e < g * g * 64; e += 256) {
        const int ji = e >> 6, u = (e >> 3) & 7, vv = e & 7;
        msh[ji][u][vv] = (u < m && vv < m) ? o.Mb[(size_t)ji * m * m + u + (size_t)vv * m] : 0.0;
    }
    __syncthreads();
    const bool ok = rr < n && v < m;
    for (int i = 0; i < g; ++i) {
        double acc = ok ? o.D[(size_t)i * m + v + (size_t)rr * ldd] : 0.0;
        for (int j = 0; j < i; ++j)
#pragma unroll
            for (int u = 0; u < 8; ++u) acc += ysh[rl][j][u] * msh[j * g + i][u][v];
        ysh[rl][i][v] = ok ? acc : 0.0;
        if (ok) o.Yt[(size_t)i * m + v + (size_t)rr * r] = acc;
        __syncthreads();
    }
}
// Packed effective group stack in one pass:  out = pack(G0 + XL Yt).  The rank-r product of a 16 x 16 tile is computed TRANSPOSED, so that the
// accumulator layout is the packed layout (acc[q] = K-step 4 tt + q, position lane) — the trick of k_eff_stack_mfma (dense.hip).
struct GroupFoldOne { const double* G0; const double* XL; const double* Yt; double* out; };
struct GroupFoldBatch { GroupFoldOne s[8]; };
__global__ __launch_bounds__(256) void k_group_fold(int n, int nblk, int nstrip, int kst, int r, int ldg, int ldx, GroupFoldBatch bt) {
    const GroupFoldOne& o = bt.s[blockIdx.z];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, lk = lane >> 4, lr = lane & 15;
    const int tt = blockIdx.x * 4 + wave;                          // column tile: K-steps 4 tt .. 4 tt + 3
    const int ntile = (kst + 3) >> 2;
    if (tt >= ntile) return;
    const int hs = blockIdx.y, b = hs / nstrip, s = hs - b * nstrip;
    const int rowl = 16 * s + lr;                                  // row within the block (B-operand column index j = lr)
    const bool rok = rowl < n;
    const size_t grow = (size_t)b * n + (rok ? rowl : 0);
    const int colA = 16 * tt + lr;                                 // A operand: A[i = lr][k] = Yt[k, 16 tt + lr]
    const bool cok = colA < n;
    v4d acc = (v4d){0.0, 0.0, 0.0, 0.0};
    const int ksteps = (r + 3) >> 2;
    for (int kk = 0; kk < ksteps; ++kk) {
        const int q = 4 * kk + lk;
        const bool qok = q < r;
        const double ya = (qok && cok) ? o.Yt[q + (size_t)colA * r] : 0.0;
        const double xb = (qok && rok) ? o.XL[grow + (size_t)q * ldx] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ya, xb, acc, 0, 0, 0);
    }
    // acc[q] = (XL Yt)[row = rowl, col = 16 tt + 4 q + lk]   (transposed tile: D'[i = lk + 4 q][j = lr])
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int t = 4 * tt + q, col = 4 * t + lk;
        if (t < kst) {
            const double base = (rok && col < n) ? o.G0[grow + (size_t)col * ldg] : 0.0;
            o.out[((size_t)hs * kst + t) * 64 + lane] = (rok && col < n) ? base + acc[q] : 0.0;
        }
    }
}
// next = prev - two_mu * W_mid  (n x n);  prev = null: identity
__global__ __launch_bounds__(256) void k_group_next_phi(int n, double two_mu, const double* __restrict__ prev, int ldp, const double* __restrict__ Wmid, int ldw,
                                                       double* __restrict__ next, int ldn) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (size_t)n * n) return;
    const int r = idx % n, c = idx / n;
    const double p = prev ? prev[r + (size_t)c * ldp] : (r == c ? 1.0 : 0.0);
    next[r + (size_t)c * ldn] = p - two_mu * Wmid[r + (size_t)c * ldw];
}
int group_size_for(Ctx* ctx, int ncycle, int n, int m) {
    if (ctx->adi_group == 0 || n > ctx->adi_group_max_n || m < 1 || m > 8) return 0;
    if (ctx->adi_group > 1) return (ncycle % ctx->adi_group == 0 && ctx->adi_group <= ADI_GROUP_MAX_G && m * (ctx->adi_group - 1) <= 32) ? ctx->adi_group : 0;
    for (int g = std::min(5, ADI_GROUP_MAX_G); g >= 2; --g) if (ncycle % g == 0 && m * (g - 1) <= 32) return g;      // auto: the largest divisor of the cycle length up to 5
    return 0;
}
// (2n + m) x n stack -> A-operand order: strip of 16 rows x K-step of 4 columns = 64 consecutive doubles (one coalesced 512-byte fragment load)
__global__ __launch_bounds__(256) void k_pack_rows(int M, int n, int kst, const double* __restrict__ src, int lds_, double* __restrict__ out) {
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t >= kst) return;
    const int row = 16 * blockIdx.y + (lane & 15), col = 4 * t + (lane >> 4);
    out[((size_t)blockIdx.y * kst + t) * 64 + lane] = (row < M && col < n) ? src[row + (size_t)col * lds_] : 0.0;
}
// Level i of the thin recursion, one launch for all start positions:  W = stack_{s_i} X_i  (X_i: n x m i, the left factor of Pi_i, in XL block
// row g + i - 1), one workgroup per 16-row strip of the packed stack, K split over the four waves, two column tiles; the epilogue writes the
// three row ranges of W where they are needed:  top -> XV_i (XL block row i),  mid -> X_{i+1} = X_i - 2 mu W_mid (XL block row g + i),
// bottom (b_i' X_i, m x m i) -> the blocks M(j, i) of the Y recursion.
struct GroupLevelOne { const double* Apk; double* XL; double* Mb; double two_mu; };
struct GroupLevelBatch { GroupLevelOne s[8]; };
__global__ __launch_bounds__(256) void k_group_level_gemm(int n, int m, int g, int i, int ldx, GroupLevelBatch bt) {
    __shared__ double part[4][2][4][64];
    const GroupLevelOne& o = bt.s[blockIdx.y];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, lk = lane >> 4, lr = lane & 15;
    const int M = 2 * n + m, ncols = m * i, kst = (n + 3) >> 2;
    const double* __restrict__ Xi = o.XL + (size_t)(g + i - 1) * n;
    double vv2[2];
    group_thin_tile(o.Apk + (size_t)blockIdx.x * kst * 64, Xi, ldx, n, ncols, part, vv2[0], vv2[1]);
    const int orow = blockIdx.x * 16 + lk + 4 * wave;
    if (orow >= M) return;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const double v = vv2[j];
        const int col = 16 * j + lr;
        if (col >= ncols) continue;
        if (orow < n) o.XL[(size_t)i * n + orow + (size_t)col * ldx] = v;                                            // XV_i
        else if (orow < 2 * n) {
            const int r = orow - n;
            o.XL[(size_t)(g + i) * n + r + (size_t)col * ldx] = Xi[r + (size_t)col * ldx] - o.two_mu * v;           // X_{i+1}
        } else {
            const int vv = orow - 2 * n, jj = col / m, u = col - jj * m;
            o.Mb[(size_t)(jj * g + i) * m * m + u + (size_t)vv * m] = v;                                               // M(jj, i)[u, vv]
        }
    }
}
void group_base_build(Ctx* ctx, const GaleOperator& op, const std::vector<std::complex<double>>& values, const CycleOps& co, GroupBase& gb, int g) {
    const int n = op.P->n, m = op.U.cols, c = (int)values.size();
    gb = GroupBase();
    gb.g = g; gb.n = n; gb.m = m; gb.tag = op.tag;
    for (auto& v : values) gb.mus.push_back(v.real());
    const int r = m * g, M = 2 * n + m, kst = adi_fast_kst(n), nstripM = ceil_div(M, 16);
    std::vector<GroupLeftDesc> tab;
    const unsigned nn_blocks = (unsigned)(((size_t)n * n + 255) / 256);
    for (int pos = 0; pos < c; ++pos) {
        gb.wks.push_back(Mat(ctx, 2 * n, m));
        const FactorEntry<double>& fe = *co.fe[(size_t)pos];
        Mat pk(ctx, nstripM * kst, 64);
        hipLaunchKernelGGL(k_pack_rows, dim3(ceil_div(kst, 4), nstripM), dim3(256), 0, ctx->stream, M, n, kst, (const double*)fe.stack.p, fe.stack.ld, pk.p);
        gb.spack.push_back(pk);
    }
    for (int p = 0; p < c; p += g) {
        gb.starts.push_back(p);
        Mat G0(ctx, 2 * g * n, n), D(ctx, g * m, n), XL(ctx, 2 * g * n, r), Yt(ctx, r, n), Mb(ctx, m * m, g * g);
        fill_mat(ctx, XL, 0.0); fill_mat(ctx, Yt, 0.0); fill_mat(ctx, Mb, 0.0);
        Mat W(ctx, M, n);
        for (int b = 0; b < g; ++b) {       // Phi(0, b) = Pi0_b:  stack_b Pi0_b = [Om0_b; E'N_b Pi0_b; D_b],  Pi0_{b+1} = Pi0_b - 2 mu_b (mid)
            const FactorEntry<double>& fe = *co.fe[(size_t)(p + b)];
            const double two_mu = 2.0 * values[(size_t)(p + b)].real();
            Mat top, mid, bot, prev;
            if (b == 0) { top = fe.stack.view(0, 0, n, n); mid = fe.stack.view(n, 0, n, n); bot = fe.stack.view(2 * n, 0, m, n); }
            else {
                prev = G0.view((g + b - 1) * n, 0, n, n);
                gemm(ctx, false, false, 1.0, fe.stack, prev, 0.0, W, nullptr, "gemm_group_base");
                top = W.view(0, 0, n, n); mid = W.view(n, 0, n, n); bot = W.view(2 * n, 0, m, n);
            }
            Mat nxt = G0.view((g + b) * n, 0, n, n);
            hipLaunchKernelGGL(k_group_next_phi, dim3(nn_blocks), dim3(256), 0, ctx->stream, n, two_mu, b == 0 ? (const double*)nullptr : (const double*)prev.p,
                               b == 0 ? 0 : prev.ld, (const double*)mid.p, mid.ld, nxt.p, nxt.ld);
            Mat om = G0.view(b * n, 0, n, n); copy_mat(ctx, top, om);
            Mat dd = D.view(b * m, 0, m, n); copy_mat(ctx, bot, dd);
        }
        // the K-dependent blocks that are plain copies:  XV_i block i = a_i = -(N K' Sinv)_i,  X_{i+1} block i = c_i = 2 mu_i (E'N K' Sinv)_i
        for (int i = 0; i < g; ++i) {
            const Mat& w = gb.wks[(size_t)(p + i)];
            tab.push_back({nullptr, 0, w.p, w.ld, XL.p + (size_t)i * n + (size_t)(i * m) * XL.ld, XL.ld, -1.0, 0, 0});
            tab.push_back({nullptr, 0, w.p + n, w.ld, XL.p + (size_t)(g + i) * n + (size_t)(i * m) * XL.ld, XL.ld, 2.0 * values[(size_t)(p + i)].real(), 0, 0});
        }
        gb.G0.push_back(G0); gb.D.push_back(D); gb.XL.push_back(XL); gb.Yt.push_back(Yt); gb.Mb.push_back(Mb);
        gb.pack.push_back(Mat(ctx, (int)((size_t)g * adi_fast_pack_doubles(n) / 64), 64));
    }
    gb.ndesc = (int)tab.size();
    gb.table = DevArr<GroupLeftDesc>(ctx, tab.size());
    gb.host_table = std::move(tab);                      // stays alive with the base: the upload is asynchronous
    DRE_HIP(hipMemcpyAsync(gb.table.p, gb.host_table.data(), gb.host_table.size() * sizeof(GroupLeftDesc), hipMemcpyHostToDevice, ctx->stream));
}
void group_ops_prepare(Ctx* ctx, const std::vector<std::complex<double>>& values, CycleOps& co, GroupBase& gb) {
    const int n = gb.n, m = gb.m, g = gb.g, r = m * g;
    const int ns = (int)gb.starts.size();
    TimedScope tsall(ctx, "group_prepare", 8.0 * ns * ((g - 1) * (2.0 * n + m) * n + 4.0 * g * n * (double)n), 2.0 * ns * 2.0 * g * n * (double)n * r, g + 2);
    hipLaunchKernelGGL(k_group_left, dim3(ceil_div(n, 16), gb.ndesc), dim3(256), 0, ctx->stream, n, m, (const GroupLeftDesc*)gb.table.p);
    for (int i = 1; i < g; ++i) {
        GroupLevelBatch lb;
        for (int q = 0; q < 8; ++q) {
            const int qq = q < ns ? q : 0, pos = gb.starts[(size_t)qq] + i;
            lb.s[q] = {gb.spack[(size_t)pos].p, gb.XL[(size_t)qq].p, gb.Mb[(size_t)qq].p, 2.0 * values[(size_t)pos].real()};
        }
        hipLaunchKernelGGL(k_group_level_gemm, dim3(ceil_div(2 * n + m, 16), ns), dim3(256), 0, ctx->stream, n, m, g, i, gb.XL[0].ld, lb);
    }
    {
        GroupYBatch yb;
        for (int q = 0; q < 8; ++q) { const int qq = q < ns ? q : 0; yb.s[q] = {gb.D[(size_t)qq].p, gb.Mb[(size_t)qq].p, gb.Yt[(size_t)qq].p}; }
        hipLaunchKernelGGL(k_group_y, dim3(ceil_div(n, 32), ns), dim3(256), 0, ctx->stream, n, m, g, gb.D[0].ld, yb);
    }
    co.gpack.clear();
    {
        const int nstrip = adi_fast_nstrip(n), kst = adi_fast_kst(n);
        GroupFoldBatch ft;
        for (int q = 0; q < 8; ++q) { const int qq = q < ns ? q : 0; ft.s[q] = {gb.G0[(size_t)qq].p, gb.XL[(size_t)qq].p, gb.Yt[(size_t)qq].p, gb.pack[(size_t)qq].p}; }
        hipLaunchKernelGGL(k_group_fold, dim3(ceil_div((kst + 3) / 4, 4), 2 * g * nstrip, ns), dim3(256), 0, ctx->stream, n, 2 * g, nstrip, kst, r,
                           gb.G0[0].ld, gb.XL[0].ld, ft);
        for (int q = 0; q < ns; ++q) co.gpack.push_back(gb.pack[(size_t)q].p);
    }
    co.group_g = g;
    DRE_HIP(hipGetLastError());
}

}  // namespace dre
