// Whole-device symmetric eigensolver: two-sided cyclic block Jacobi (host model: tests/_block_jacobi_model.py).
//
// The q x q matrix is padded with zero rows and columns to Q = 16 p (p >= 2) and cut into p x p blocks of 16 x 16.  A sweep is the p - 1 (p even)
// or p (p odd: one block sits out per round) rounds of the round-robin tournament of the blocks; the floor(p / 2) block pairs of a round are
// disjoint, so their 32 x 32 pivot blocks are diagonalised independently (k_bjb_pivot, one workgroup each, J_P to global memory, A untouched) and
// the whole similarity transformation of the round, A <- J' A J and V <- V J with J = blockdiag(J_P), is one launch (k_bjb_update: one workgroup
// per 32 x 32 super-block, both products on v_mfma_f64_16x16x4_f64, every super-block read and written once).  Kernel boundaries are the only
// synchronisation between workgroups.  After every sweep off(A)^2 and ||A||_F^2 are summed in two launches (store_partials / load_partials) into
// the control block, which the host reads once per sweep.
//
// Every launch carries the member b = blockIdx.y of an ensemble of same-order matrices (jacobi_common.hpp); sym_eig_jacobi is a batch of one.
// Every member has its own control block, `rotated` flags, partial sums and J buffer; nothing is summed across members and there are no
// atomics, so a member's result does not depend on the others.  The host reads the B control blocks in one copy per sweep.
//
// Index arithmetic: block, row and column indices are ints below the padded order Q <= DENSE_MAX_N; every element offset and every member
// stride is a size_t.
#include <cmath>

#include "dense_gj.hpp"
#include "jacobi_common.hpp"
#include "profiling.hpp"

namespace dre {

namespace {

// ---- pivot blocks ------------------------------------------------------------------------------------------------------------------------
// grid (m pairs, B); Jbuf and rotated: m slices per member.  One workgroup per block pair (bi, bj) of the round: gathers the 32 x 32 pivot
// block [A_ii A_ij; A_ji A_jj] into LDS, diagonalises it by cyclic Jacobi and leaves J (column-major, 32 x 32) in Jbuf and "a rotation was
// done" in rotated.  A rotation (r, c) is done when |a_rc| > (tol / Q) ||A||_F; a skipped rotation is the exact identity, so a zero padding
// row stays a unit row of J.
__global__ __launch_bounds__(256) void k_bjb_pivot(int Q, const double* __restrict__ As, size_t stride, const int* __restrict__ pairs,
                                                   const BjCtl* __restrict__ ctls, double tol, double* __restrict__ Jbufs, int* __restrict__ rotateds) {
    __shared__ double G[PB * LDP], J[PB * LDP], cs[2 * SB];
    __shared__ int flag;
    const BjCtl* ctl = ctls + blockIdx.y;
    const bool off = member_off(*ctl);
    const double* A = As + (size_t)blockIdx.y * stride;
    double* Jbuf = Jbufs + (size_t)blockIdx.y * (size_t)gridDim.x * (PB * PB);
    int* rotated = rotateds + (size_t)blockIdx.y * gridDim.x;
    const int tid = threadIdx.x;
    const int bi = pairs[2 * blockIdx.x], bj = pairs[2 * blockIdx.x + 1];
    const double thr = tol / (double)Q * ctl->norm;
    for (int e = tid; e < PB * PB; e += 256) {
        const int i = e & (PB - 1), j = e >> 5;
        const int gi = (i < SB ? bi : bj) * SB + (i & (SB - 1)), gj = (j < SB ? bi : bj) * SB + (j & (SB - 1));
        G[i + LDP * j] = A[(size_t)gi + (size_t)gj * (size_t)Q];
        J[i + LDP * j] = i == j ? 1.0 : 0.0;
    }
    // (uniform in the workgroup.  Asked behind the gather, which is harmless for a member that is off: the control block is then loaded beside
    // `pairs` and the arguments, not alone in front of them, which takes two dependent loads out of every launch of this latency-bound kernel)
    if (off) return;
    if (tid == 0) flag = 0;
    __syncthreads();
    const int any = cyclic_jacobi_32(G, J, cs, &flag, INNER_MAX, [thr](double, double, double apq) { return fabs(apq) > thr; });
    double* Jo = Jbuf + (size_t)blockIdx.x * (PB * PB);
    for (int e = tid; e < PB * PB; e += 256) Jo[e] = J[(e & (PB - 1)) + LDP * (e >> 5)];
    if (tid == 0) rotated[blockIdx.x] = any;
}

// ---- the similarity transformation of a round ---------------------------------------------------------------------------------------------
// grid (super-blocks, B).  One workgroup per 32 x 32 super-block X of A or V:  X <- L' X R  with L, R one of the round's J_P or the identity.
// m block pairs, `sit` the block that sits out (-1: none), p blocks.  Workgroups, in order:
//   m * m          A_PQ <- J_P' A_PQ J_Q                     (P, Q block pairs)
//   2 m if sit     A_sQ <- A_sQ J_Q,  A_Ps <- J_P' A_Ps      (16 x 32 and 32 x 16: the absent half is zero in LDS and not written)
//   ceil(p/2) * m  V_tQ <- V_tQ J_Q                          (t: two block rows of V)
// A pair whose pivot block needed no rotation has J = I exactly: its factor is skipped, and a super-block with both factors skipped is left alone.
// Four waves, wave (wr, wc) owns the 16 x 16 tile (wr, wc) of the super-block in both products.
__global__ __launch_bounds__(256) void k_bjb_update(int Q, int p, int m, int sit, const int* __restrict__ pairs, const double* __restrict__ Jbufs,
                                                    const int* __restrict__ rotateds, double* __restrict__ As, double* __restrict__ Vs, size_t stride,
                                                    const BjCtl* __restrict__ ctls) {
    __shared__ double Xs[PB * LDP], Ts[PB * LDP], JL[PB * LDP], JR[PB * LDP];
    const bool off = member_off(ctls[blockIdx.y]);          // (asked with the `rotated` flags below, as in k_bjb_pivot)
    const double* Jbuf = Jbufs + (size_t)blockIdx.y * (size_t)m * (PB * PB);
    const int* rotated = rotateds + (size_t)blockIdx.y * m;
    double* A = As + (size_t)blockIdx.y * stride;
    double* V = Vs + (size_t)blockIdx.y * stride;
    const int tid = threadIdx.x;
    int b = blockIdx.x;
    int rb0, rb1, cb0, cb1, L = -1, R = -1;
    double* M = A;
    if (b < m * m) {
        L = b / m; R = b % m;
        rb0 = pairs[2 * L]; rb1 = pairs[2 * L + 1]; cb0 = pairs[2 * R]; cb1 = pairs[2 * R + 1];
    } else {
        b -= m * m;
        if (sit >= 0 && b < 2 * m) {
            if (b < m) { R = b; rb0 = sit; rb1 = -1; cb0 = pairs[2 * R]; cb1 = pairs[2 * R + 1]; }
            else { L = b - m; rb0 = pairs[2 * L]; rb1 = pairs[2 * L + 1]; cb0 = sit; cb1 = -1; }
        } else {
            if (sit >= 0) b -= 2 * m;
            const int t = b / m;
            R = b % m; M = V;
            rb0 = 2 * t; rb1 = 2 * t + 1 < p ? 2 * t + 1 : -1; cb0 = pairs[2 * R]; cb1 = pairs[2 * R + 1];
        }
    }
    if (L >= 0 && !rotated[L]) L = -1;
    if (R >= 0 && !rotated[R]) R = -1;
    if (off || (L < 0 && R < 0)) return;          // (uniform in the workgroup)
    for (int e = tid; e < PB * PB; e += 256) {
        const int i = e & (PB - 1), j = e >> 5;
        const int br = (i >> 4) ? rb1 : rb0, bc = (j >> 4) ? cb1 : cb0;
        double x = 0.0;
        if (br >= 0 && bc >= 0) x = M[(size_t)(br * SB + (i & 15)) + (size_t)(bc * SB + (j & 15)) * (size_t)Q];
        Xs[i + LDP * j] = x;
        if (L >= 0) JL[i + LDP * j] = Jbuf[(size_t)L * (PB * PB) + e];
        if (R >= 0) JR[i + LDP * j] = Jbuf[(size_t)R * (PB * PB) + e];
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63, wr = wave >> 1, wc = wave & 1;
    const int lr = lane & 15, lk = lane >> 4;
    // T = L' X  (MFMA operand maps: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][j = lane & 15]; D: column lane & 15, row (lane >> 4) + 4 reg)
    if (L >= 0) {
        v4d acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k0 = 0; k0 < PB; k0 += 4)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(JL[(k0 + lk) + LDP * (wr * 16 + lr)], Xs[(k0 + lk) + LDP * (wc * 16 + lr)], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) Ts[(wr * 16 + lk + 4 * r) + LDP * (wc * 16 + lr)] = acc[r];
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) Ts[(wr * 16 + lk + 4 * r) + LDP * (wc * 16 + lr)] = Xs[(wr * 16 + lk + 4 * r) + LDP * (wc * 16 + lr)];
    }
    __syncthreads();          // (T complete; every read of Xs is done, so the result may go there)
    if (R >= 0) {
        v4d acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k0 = 0; k0 < PB; k0 += 4)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Ts[(wr * 16 + lr) + LDP * (k0 + lk)], JR[(k0 + lk) + LDP * (wc * 16 + lr)], acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) Xs[(wr * 16 + lk + 4 * r) + LDP * (wc * 16 + lr)] = acc[r];
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) Xs[(wr * 16 + lk + 4 * r) + LDP * (wc * 16 + lr)] = Ts[(wr * 16 + lk + 4 * r) + LDP * (wc * 16 + lr)];
    }
    __syncthreads();
    for (int e = tid; e < PB * PB; e += 256) {
        const int i = e & (PB - 1), j = e >> 5;
        const int br = (i >> 4) ? rb1 : rb0, bc = (j >> 4) ? cb1 : cb0;
        if (br >= 0 && bc >= 0) M[(size_t)(br * SB + (i & 15)) + (size_t)(bc * SB + (j & 15)) * (size_t)Q] = Xs[i + LDP * j];
    }
}

// ---- norms and the decision -----------------------------------------------------------------------------------------------------------------
// grid (NORM_PARTS, B): the partial sums of member b in parts + 2 NORM_PARTS b
__global__ __launch_bounds__(256) void k_bjb_norms(int Q, const double* __restrict__ As, size_t stride, double* __restrict__ parts,
                                                   const BjCtl* __restrict__ ctls) {
    const bool off = member_off(ctls[blockIdx.y]);
    const double* A = As + (size_t)blockIdx.y * stride;
    double s_off = 0.0, s_diag = 0.0;
    const size_t tot = (size_t)Q * (size_t)Q;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < tot; idx += (size_t)gridDim.x * blockDim.x) {
        const double x = A[idx];
        if (idx % (size_t)Q == idx / (size_t)Q) s_diag += x * x; else s_off += x * x;
    }
    if (off) return;          // (uniform in the workgroup; asked behind the loads, as in k_bjb_pivot)
    store_partials(parts + (size_t)blockIdx.y * (2 * gridDim.x), s_off, s_diag);
}

// grid (B); a member still rotating after BJ_MAX_SWEEPS sweeps is dropped here
__global__ __launch_bounds__(256) void k_bjb_decide(int nparts, const double* __restrict__ parts, double tol, int count, BjCtl* ctls) {
    BjCtl* ctl = ctls + blockIdx.x;
    const bool off = member_off(*ctl);
    double s[2];
    load_partials(nparts, parts + (size_t)blockIdx.x * (2 * nparts), s);
    if (threadIdx.x == 0 && !off) {          // (asked behind the loads, as in k_bjb_pivot)
        const double off = sqrt(s[0]), norm = sqrt(s[0] + s[1]);
        ctl->off = off; ctl->norm = norm;
        ctl->nonfinite = isfinite(norm) ? 0 : 1;
        ctl->done = isfinite(norm) && off <= tol * norm ? 1 : 0;
        ctl->sweeps += count;
        ctl->failed = isfinite(norm) && !ctl->done && ctl->sweeps >= BJ_MAX_SWEEPS ? 1 : 0;
    }
}

// grid (ceil(q / 256), B): w[b q + i] = A_b(i, i)
__global__ void k_bjb_diag(int q, int Q, const double* __restrict__ As, size_t stride, double* __restrict__ w) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < q) w[(size_t)blockIdx.y * q + i] = As[(size_t)blockIdx.y * stride + (size_t)i + (size_t)i * (size_t)Q];
}

// The driver of sym_eig_jacobi (single) and sym_eig_jacobi_batch.  status[b].msg is only the "what" of a member's failure.  single: the
// kernel-timer tags and the trace line of sym_eig_jacobi, which also takes any tol as it comes.
SymEigBatch bj_run(Ctx* ctx, const std::vector<Mat>& S, double tol, const char* who, bool single) {
    check_batch(S, who);
    const int B = (int)S.size(), q = S[0].rows;
    DRE_REQUIRE(S[0].rows == S[0].cols, std::string(who) + ": square matrices expected");
    DRE_REQUIRE(q <= DENSE_MAX_N - 2 * BJ_BLOCK, std::string(who) + ": order beyond the device's 32-bit index limit");
    DRE_REQUIRE(single || std::isfinite(tol), std::string(who) + ": tol is not finite");
    SymEigBatch out;
    out.eig.resize((size_t)B); out.stats.resize((size_t)B); out.status.resize((size_t)B);
    for (auto& e : out.eig) e.q = q;
    if (q == 0) return out;
    if (!(tol > 0.0)) tol = q * DBL_EPS;
    const int Q = bj_padded_order(q), p = Q / BJ_BLOCK, nrounds = p - 1 + (p & 1), m = p / 2;
    const size_t QQ = (size_t)Q * Q;
    // per member: A, V, the result's Z, the J buffer, the partial sums, the eigenvalues
    require_memory(ctx, (size_t)B * (2 * QQ + (size_t)q * q + (size_t)m * PB * PB + 2 * NORM_PARTS + q));

    const std::vector<int> tab = rr_schedule(p, true);
    DevArr<int> dtab(ctx, tab.size());
    dtab.upload(ctx, tab);

    DevArr<double> A(ctx, (size_t)B * QQ), V(ctx, (size_t)B * QQ), Jbuf(ctx, (size_t)B * m * PB * PB), part(ctx, (size_t)B * 2 * NORM_PARTS);
    DevArr<int> rotated(ctx, (size_t)B * m);
    DevArr<BjCtl> ctl(ctx, (size_t)B);
    if (Q != q) DRE_HIP(hipMemsetAsync(A.p, 0, (size_t)B * QQ * sizeof(double), ctx->stream));
    {
        std::vector<CopyDesc> cp((size_t)B);
        for (int b = 0; b < B; ++b) cp[(size_t)b] = CopyDesc{S[(size_t)b].p, A.p + (size_t)b * QQ, q, q, S[(size_t)b].ld, Q};
        copy_batched(ctx, cp);
    }
    hipLaunchKernelGGL(k_jb_eye, dim3(grid_for(QQ), B), dim3(256), 0, ctx->stream, Q, V.p, QQ);
    DRE_HIP(hipMemsetAsync(ctl.p, 0, sizeof(BjCtl) * (size_t)B, ctx->stream));

    const char* tag_norm = single ? "bj_norm" : "bjb_norm";
    const char* tag_pivot = single ? "bj_pivot" : "bjb_pivot";
    const char* tag_update = single ? "bj_update" : "bjb_update";
    std::vector<BjCtl> h((size_t)B);
    auto measure = [&](int count) {
        TimedScope ts(ctx, tag_norm, 8.0 * B * Q * Q, 0.0, 2);
        hipLaunchKernelGGL(k_bjb_norms, dim3(NORM_PARTS, B), dim3(256), 0, ctx->stream, Q, (const double*)A.p, QQ, part.p, (const BjCtl*)ctl.p);
        hipLaunchKernelGGL(k_bjb_decide, dim3(B), dim3(256), 0, ctx->stream, NORM_PARTS, (const double*)part.p, tol, count, ctl.p);
        fetch_ctl(ctx, ctl, h);
    };
    // the outcomes of the last measurement: a dropped member's code and message
    auto judge = [&](bool entry) {
        bool live = false;
        for (int b = 0; b < B; ++b) {
            const BjCtl& c = h[(size_t)b];
            if (c.done || out.status[(size_t)b].code) continue;
            if (c.nonfinite)
                out.status[(size_t)b] = {ERR_INVALID, entry ? "the matrix has non-finite entries" : "non-finite values in sweep " + std::to_string(c.sweeps)};
            else if (c.failed)
                out.status[(size_t)b] = {ERR_INTERNAL, "no convergence in " + std::to_string(c.sweeps) + " sweeps (off / norm = " + std::to_string(c.off / c.norm) + ")"};
            else live = true;
        }
        return live;
    };
    measure(0);
    bool live = judge(true);
    const unsigned vjobs = (unsigned)((p + 1) / 2) * (unsigned)m;
    while (live) {
        for (int r = 0; r < nrounds; ++r) {
            const int* t = dtab.p + (size_t)r * (2 * m + 1);
            const int sit = tab[(size_t)r * (2 * m + 1) + 2 * m];
            {
                TimedScope ts(ctx, tag_pivot, 16.0 * B * m * PB * PB, 0.0);
                hipLaunchKernelGGL(k_bjb_pivot, dim3(m, B), dim3(256), 0, ctx->stream, Q, (const double*)A.p, QQ, t, (const BjCtl*)ctl.p, tol, Jbuf.p, rotated.p);
            }
            {
                const unsigned grid = (unsigned)m * (unsigned)m + (sit >= 0 ? 2u * (unsigned)m : 0u) + vjobs;
                TimedScope ts(ctx, tag_update, 32.0 * B * Q * Q, 8.0 * PB * (double)B * Q * Q * 1.5);
                hipLaunchKernelGGL(k_bjb_update, dim3(grid, B), dim3(256), 0, ctx->stream, Q, p, m, sit, t, (const double*)Jbuf.p, (const int*)rotated.p, A.p, V.p,
                                   QQ, (const BjCtl*)ctl.p);
            }
        }
        measure(1);
        live = judge(false);
    }
    DRE_HIP(hipGetLastError());

    DevArr<double> dw(ctx, (size_t)B * q);
    hipLaunchKernelGGL(k_bjb_diag, dim3(ceil_div(q, 256), B), dim3(256), 0, ctx->stream, q, Q, (const double*)A.p, QQ, dw.p);
    std::vector<double> w((size_t)B * q);
    DRE_HIP(hipMemcpyAsync(w.data(), dw.p, w.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    std::vector<CopyDesc> cp;
    for (int b = 0; b < B; ++b) {
        if (out.status[(size_t)b].code) continue;
        SymEig& e = out.eig[(size_t)b];
        e.j = q; e.nref = 0; e.snorm = h[(size_t)b].norm;
        e.Z = Mat(ctx, q, q);
        cp.push_back(CopyDesc{V.p + (size_t)b * QQ, e.Z.p, q, q, Q, e.Z.ld});
        out.stats[(size_t)b].sweeps = h[(size_t)b].sweeps;
        out.stats[(size_t)b].rounds = (long)nrounds * h[(size_t)b].sweeps;
    }
    copy_batched(ctx, cp);
    ctx->sync();
    for (int b = 0; b < B; ++b)
        if (!out.status[(size_t)b].code) out.eig[(size_t)b].w.assign(w.begin() + (size_t)b * q, w.begin() + (size_t)(b + 1) * q);
    if (env_trace("compress")) {
        for (int b = 0; b < B; ++b) {
            const BjCtl& c = h[(size_t)b];
            if (!single) std::fprintf(stderr, "[sym_eig_jacobi_batch] member %d, q=%d: %d sweeps, status %d\n", b, q, c.sweeps, out.status[(size_t)b].code);
            else if (!out.status[0].code)
                std::fprintf(stderr, "[sym_eig_jacobi] q=%d: %d sweeps, %ld rounds, off / norm = %.2e\n", q, c.sweeps, out.stats[0].rounds, c.norm > 0 ? c.off / c.norm : 0.0);
        }
    }
    return out;
}

}  // namespace

void sym_eig_dump_input(Ctx* ctx, const Mat& S) {
    const char* dir = std::getenv("DRE_SYM_EIG_DUMP");
    if (!dir || !*dir || S.rows == 0 || S.rows != S.cols) return;
    static std::atomic<long> count{0};
    const int q = S.rows;
    std::vector<double> h((size_t)q * q);
    DRE_HIP(hipMemcpy2DAsync(h.data(), (size_t)q * sizeof(double), S.p, (size_t)S.ld * sizeof(double), (size_t)q * sizeof(double), q, hipMemcpyDeviceToHost,
                             ctx->stream));
    ctx->sync();
    const std::string path = std::string(dir) + "/S_" + std::to_string(count++) + "_" + std::to_string(q) + ".f64";
    if (FILE* f = std::fopen(path.c_str(), "wb")) { (void)std::fwrite(h.data(), sizeof(double), h.size(), f); std::fclose(f); }
}

SymEigBatch sym_eig_jacobi_batch(Ctx* ctx, const std::vector<Mat>& S, double tol, const char* who) {
    SymEigBatch out = bj_run(ctx, S, tol, who, false);
    name_members(out.status, who);
    return out;
}

SymEig sym_eig_jacobi(Ctx* ctx, const Mat& S, double tol, BjStats* stats) {
    DRE_REQUIRE(S.rows == S.cols, "sym_eig_jacobi: square matrix expected");
    if (stats) *stats = BjStats{};
    SymEigBatch r = bj_run(ctx, {S}, tol, "sym_eig_jacobi", true);
    if (r.status[0].code) throw Error(r.status[0].code, "sym_eig_jacobi: " + r.status[0].msg);
    if (stats) *stats = r.stats[0];
    return std::move(r.eig[0]);
}

}  // namespace dre
