// C ABI of libdre_hip, the dense family: everything from dre_dense_gale_solve to dre_balance_lr_batched (sign-function and doubling solvers,
// inversion, frequency / transfer / time response, the kept sign and Sylvester factorisations, SVD and balanced truncation, single and
// batched).  The dense accessors of dre_gdre_result (dre_gdre_result_X_dense, _dense_stats, _step_stats) live here, beside the drivers that
// fill them; every other accessor of that handle is in api_lowrank.hip.
#include "abi.hpp"

#include <algorithm>
#include <cstring>
#include <functional>

#include "balance.hpp"
#include "dense_adaptive.hpp"
#include "dense_are.hpp"
#include "dense_are_batch.hpp"
#include "dense_cgj.hpp"
#include "dense_doubling.hpp"
#include "dense_sign_lr.hpp"
#include "freq_response.hpp"
#include "jacobi_batch.hpp"
#include "time_response.hpp"
#include "transfer_eval.hpp"

using namespace dre;

// (iters, refinements | res0, res) of one solve into the caller's info arrays; member b of a batched call (or the second of a pair) at 2 b
template <typename Stats>
static void solve_info(const Stats& s, int64_t* iinfo, double* dinfo, size_t b = 0) {
    if (iinfo) { iinfo[2 * b] = s.iters; iinfo[2 * b + 1] = s.refinements; }
    if (dinfo) { dinfo[2 * b] = s.res0; dinfo[2 * b + 1] = s.res; }
}

// The continuous (GARE, dense_are.hip) and the discrete (DARE, dense_doubling.hip) Riccati entries take the same operands and return the same
// things: one body each for solve, solve_pair and residual over the solver function.  Rinv and S are optional.
struct AreOperands { const dre_dense *E, *A, *B, *Rinv, *Ct, *S; };
template <typename Solve>
static int are_solve(dre_ctx* ctx, Solve solve, const char* who, const AreOperands& a, int maxiters, double tol, int max_refine, dre_dense** X,
                     int64_t* iinfo, double* dinfo) {
    return guarded_out<dre_dense>(ctx, [&](DenseOut& o) {
        DRE_REQUIRE(a.E && a.A && a.B && a.Ct && X, std::string(who) + ": null argument");
        auto r = solve(&ctx->c, a.E->m, a.A->m, a.B->m, opt_mat(a.Rinv), a.Ct->m, opt_mat(a.S), maxiters, tol, max_refine);
        solve_info(r, iinfo, dinfo);
        put(o, X, std::move(r.X));
    });
}
template <typename Solve>
static int are_solve_pair(dre_ctx* ctx, Solve solve, const char* who, const AreOperands& a, int maxiters, double tol, int max_refine, dre_dense** X,
                          dre_dense** Y, int64_t* iinfo, double* dinfo) {
    return guarded_out<dre_dense>(ctx, [&](DenseOut& o) {
        DRE_REQUIRE(a.E && a.A && a.B && a.Ct && X && Y, std::string(who) + ": null argument");
        auto r = solve(&ctx->c, a.E->m, a.A->m, a.B->m, opt_mat(a.Rinv), a.Ct->m, opt_mat(a.S), maxiters, tol, max_refine);
        solve_info(r.X, iinfo, dinfo, 0);
        solve_info(r.Y, iinfo, dinfo, 1);
        put(o, X, std::move(r.X.X));
        put(o, Y, std::move(r.Y.X));
    });
}
template <typename Residual>
static int are_residual(dre_ctx* ctx, Residual residual, const char* who, const AreOperands& a, const dre_dense* X, dre_dense** Res, double* norm,
                        double* scaled) {
    return guarded_out<dre_dense>(ctx, [&](DenseOut& o) {
        DRE_REQUIRE(a.E && a.A && a.B && a.Ct && X && Res, std::string(who) + ": null argument");
        double fro = 0.0, sc = 0.0;
        put(o, Res, residual(&ctx->c, a.E->m, a.A->m, a.B->m, opt_mat(a.Rinv), a.Ct->m, opt_mat(a.S), X->m, &fro, &sc));
        if (norm) *norm = fro;
        if (scaled) *scaled = sc;
    });
}

extern "C" {

// ---- dense path (dense_sign.hip, dense_gj.hip, dense_are.hip) ---------------------------------------------------------------------------------------------------
int dre_dense_gale_solve(dre_ctx* ctx, const dre_dense* E, const dre_dense* F, const dre_dense* R, int maxiters, double tol, int max_refine,
                         dre_dense** X, int64_t* iinfo, double* dinfo) {
    return guarded_out<dre_dense>(ctx, [&](DenseOut& o) {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(E && F && R && X, "dre_dense_gale_solve: null argument");
        const int n = E->m.rows;
        DRE_REQUIRE(F->m.rows == n && F->m.cols == n && R->m.rows == n && R->m.cols == n, "dre_dense_gale_solve: E, F, R must be n x n");
        SignLyap lyap(c, E->m, maxiters, tol, max_refine);
        lyap.factor(F->m);
        const SignStats s = lyap.solve(R->m, put(o, X, Mat(c, n, n))->m);
        c->sync();
        solve_info(s, iinfo, dinfo);
    });
}
// a dense driver's result (single, adaptive, one member of a batch) as the handle the result accessors read; d is emptied
static dre_gdre_result* wrap_dense_result(AbiOut<dre_gdre_result>& o, dre_gdre_result** slot, DenseGdreResult& d, int n, int m) {
    dre_gdre_result* r = o.make(slot);
    r->dense = true; r->n = n; r->m = m;
    r->r.t = std::move(d.t); r->r.Kt = std::move(d.Kt);
    r->Xd = std::move(d.X); r->solves = std::move(d.solves);
    return r;
}
int dre_dense_gdre_solve(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* C, const dre_dense* X0,
                         double t0, double tf, double dt, int order, int save_state, int maxiters, double tol, int max_refine,
                         dre_gdre_result** out) {
    return guarded_out<dre_gdre_result>(ctx, [&](AbiOut<dre_gdre_result>& o) {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(E && A && B && C && X0 && out, "dre_dense_gdre_solve: null argument");
        DenseGdreResult d = dense_gdre_solve(c, E->m, A->m, B->m, C->m, X0->m, t0, tf, dt, order, save_state != 0, maxiters, tol, max_refine);
        wrap_dense_result(o, out, d, E->m.rows, B->m.cols);
    });
}
int dre_dense_gdre_solve_adaptive(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* C, const dre_dense* X0,
                                  double t0, double tf, double dt0, int order, double rtol, double atol, double dt_min, double dt_max, int64_t max_steps,
                                  const double* tstops, int ntstops, int save_state, int maxiters, double tol, int max_refine, dre_gdre_result** out) {
    return guarded_out<dre_gdre_result>(ctx, [&](AbiOut<dre_gdre_result>& o) {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(E && A && B && C && X0 && out, "dre_dense_gdre_solve_adaptive: null argument");
        DRE_REQUIRE(ntstops >= 0 && (ntstops == 0 || tstops), "dre_dense_gdre_solve_adaptive: ntstops must be >= 0, with tstops given when it is positive");
        StepControl sc;
        sc.rtol = rtol; sc.atol = atol; sc.dt_min = dt_min; sc.dt_max = dt_max; sc.max_steps = (long)max_steps;
        sc.tstops.assign(tstops, tstops + ntstops);
        DenseAdaptiveResult d = dense_gdre_solve_adaptive(c, E->m, A->m, B->m, C->m, X0->m, t0, tf, dt0, order, sc, save_state != 0, maxiters, tol, max_refine);
        dre_gdre_result* r = wrap_dense_result(o, out, d.r, E->m.rows, B->m.cols);
        r->adaptive = true; r->accepted = d.accepted; r->rejected = d.rejected; r->step_err = std::move(d.err);
    });
}
int dre_gdre_result_step_stats(const dre_gdre_result* r, int64_t* accepted_rejected, double* err) {
    if (!r || !r->adaptive) return DRE_ERR_INVALID;
    if (accepted_rejected) { accepted_rejected[0] = r->accepted; accepted_rejected[1] = r->rejected; }
    if (err) std::memcpy(err, r->step_err.data(), r->step_err.size() * sizeof(double));
    return DRE_OK;
}
int dre_dense_invert(dre_ctx* ctx, dre_dense* A, int32_t* piv, double* logabsdet) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(A, "dre_dense_invert: null argument");
        const int n = A->m.rows;
        DRE_REQUIRE(A->m.cols == n && n >= 1 && n <= DENSE_MAX_N, "dre_dense_invert: square matrix of order 1 .. " + std::to_string(DENSE_MAX_N) + " expected");
        DevArr<int> pv(c, n);
        DevArr<GjCtl> ctl(c, 1);
        DRE_HIP(hipMemsetAsync(ctl.p, 0, sizeof(GjCtl), c->stream));
        gj_invert(c, A->m, pv.p, ctl.p);
        const GjCtl h = read_back(c, ctl.p);
        if (h.singular) throw Error(ERR_SINGULAR, "dre_dense_invert: singular matrix (exactly zero or non-finite pivot)");
        if (piv) { DRE_HIP(hipMemcpyAsync(piv, pv.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, c->stream)); c->sync(); }
        if (logabsdet) *logabsdet = h.logdet;
    });
}
int dre_dense_gare_solve(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* Rinv, const dre_dense* Ct,
                         const dre_dense* S, int maxiters, double tol, int max_refine, dre_dense** X, int64_t* iinfo, double* dinfo) {
    return are_solve(ctx, dense_gare_solve, "dre_dense_gare_solve", {E, A, B, Rinv, Ct, S}, maxiters, tol, max_refine, X, iinfo, dinfo);
}
int dre_dense_gare_solve_pair(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* Rinv, const dre_dense* Ct,
                              const dre_dense* S, int maxiters, double tol, int max_refine, dre_dense** X, dre_dense** Y, int64_t* iinfo, double* dinfo) {
    return are_solve_pair(ctx, dense_gare_solve_pair, "dre_dense_gare_solve_pair", {E, A, B, Rinv, Ct, S}, maxiters, tol, max_refine, X, Y, iinfo, dinfo);
}
int dre_dense_gare_residual(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* Rinv, const dre_dense* Ct,
                            const dre_dense* S, const dre_dense* X, dre_dense** Res, double* norm) {
    const auto residual = [](Ctx* c, const Mat& E, const Mat& A, const Mat& B, const Mat* Rinv, const Mat& Ct, const Mat* S, const Mat& X, double* fro,
                             double*) { return dense_gare_residual(c, E, A, B, Rinv, Ct, S, X, fro); };
    return are_residual(ctx, residual, "dre_dense_gare_residual", {E, A, B, Rinv, Ct, S}, X, Res, norm, nullptr);
}
int dre_dense_stein_solve(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* Q, int dual, int maxiters, double tol, dre_dense** X,
                          int64_t* iinfo, double* dinfo) {
    return guarded_out<dre_dense>(ctx, [&](DenseOut& o) {
        DRE_REQUIRE(E && A && Q && X, "dre_dense_stein_solve: null argument");
        DenseSteinResult r = dense_stein_solve(&ctx->c, E->m, A->m, Q->m, dual != 0, maxiters, tol);
        solve_info(SignStats{r.iters, 0, r.step, r.step}, iinfo, dinfo);          // (no refinement; the last step stands for both residual words)
        put(o, X, std::move(r.X));
    });
}
int dre_dense_stein_residual(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* Q, const dre_dense* X, int dual, dre_dense** Res,
                             double* norm, double* scaled) {
    return guarded_out<dre_dense>(ctx, [&](DenseOut& o) {
        DRE_REQUIRE(E && A && Q && X && Res, "dre_dense_stein_residual: null argument");
        put(o, Res, dense_stein_residual(&ctx->c, E->m, A->m, Q->m, X->m, dual != 0, norm, scaled));
    });
}
int dre_dense_dare_solve(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* Rinv, const dre_dense* Ct,
                         const dre_dense* S, int maxiters, double tol, int max_refine, dre_dense** X, int64_t* iinfo, double* dinfo) {
    return are_solve(ctx, dense_dare_solve, "dre_dense_dare_solve", {E, A, B, Rinv, Ct, S}, maxiters, tol, max_refine, X, iinfo, dinfo);
}
int dre_dense_dare_solve_pair(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* Rinv, const dre_dense* Ct,
                              const dre_dense* S, int maxiters, double tol, int max_refine, dre_dense** X, dre_dense** Y, int64_t* iinfo, double* dinfo) {
    return are_solve_pair(ctx, dense_dare_solve_pair, "dre_dense_dare_solve_pair", {E, A, B, Rinv, Ct, S}, maxiters, tol, max_refine, X, Y, iinfo, dinfo);
}
int dre_dense_dare_residual(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* Rinv, const dre_dense* Ct,
                            const dre_dense* S, const dre_dense* X, dre_dense** Res, double* norm, double* scaled) {
    return are_residual(ctx, dense_dare_residual, "dre_dense_dare_residual", {E, A, B, Rinv, Ct, S}, X, Res, norm, scaled);
}
int dre_gdre_result_X_dense(dre_ctx* ctx, const dre_gdre_result* r, int i, dre_dense** X) {
    return guarded_out<dre_dense>(ctx, [&](DenseOut& o) {
        DRE_REQUIRE(r && r->dense, "dre_gdre_result_X_dense: not a dense result");
        DRE_REQUIRE(i >= 0 && i < (int)r->Xd.size(), "state index out of range");
        Ctx* c = &ctx->c;
        copy_mat(c, r->Xd[(size_t)i], put(o, X, Mat(c, r->n, r->n))->m);
        c->sync();
    });
}
int dre_gdre_result_dense_stats(const dre_gdre_result* r, int64_t* iters, int64_t* refinements, double* residuals) {
    if (!r || !r->dense) return DRE_ERR_INVALID;
    for (size_t j = 0; j < r->solves.size(); ++j) {
        const SignStats& s = r->solves[j];
        if (iters) iters[j] = s.iters;
        if (refinements) refinements[j] = s.refinements;
        if (residuals) { residuals[2 * j] = s.res0; residuals[2 * j + 1] = s.res; }
    }
    return DRE_OK;
}

// ---- batched dense path (dense_batch.hip) ---------------------------------------------------------------------------------------------
const char* dre_batch_member_error(dre_ctx* ctx, int b) {
    if (!ctx || b < 0 || b >= (int)ctx->batch_errors.size()) return "";
    return ctx->batch_errors[(size_t)b].c_str();
}
// Real and complex batched inversion in place (dense_batch.hip, dense_cgj.hip): one body over np, the planes of a member (1: A; 2: [Re | Im], member
// b's planes side by side at b * np * n^2), and the inversion.  nb_of and invert are the real or the complex pair of functions.
static int invert_batched(dre_ctx* ctx, const char* who, int np, dre_dense* const* const* A, const char* const* names, int batch, int32_t* piv,
                          double* logabsdet, int32_t* status, int (*nb_of)(int), decltype(gj_invert_batched)* invert) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(A[0] && A[np - 1] && status && batch >= 1 && A[0][0], std::string(who) + ": null argument or batch < 1");
        const int n = A[0][0]->m.rows;
        check_batch_order(batch, n, who);
        for (int k = 0; k < np; ++k) check_members(batch, A[k], n, n, who, names[k]);
        const int nb = nb_of(n);
        require_memory(c, (size_t)batch * ((size_t)np * n * n + (size_t)(np + np * np) * n * nb + n));
        Mat S(c, n, np * n * batch);
        auto plane = [&](int b, int k) { return S.colsview((np * b + k) * n, n); };
        for (int b = 0; b < batch; ++b)
            for (int k = 0; k < np; ++k) { Mat v = plane(b, k); copy_mat(c, A[k][b]->m, v); }
        Mat Pn(c, n, np * nb * batch), W(c, np * nb, np * n * batch);
        DevArr<int> pv(c, (size_t)n * batch);
        DevArr<BatchCtl> ctl(c, batch);
        DRE_HIP(hipMemsetAsync(ctl.p, 0, sizeof(BatchCtl) * batch, c->stream));
        invert(c, batch, n, S.p, pv.p, ctl.p, BM_GJ, Pn.p, W.p);
        std::vector<BatchCtl> h((size_t)batch);
        DRE_HIP(hipMemcpyAsync(h.data(), ctl.p, sizeof(BatchCtl) * batch, hipMemcpyDeviceToHost, c->stream));
        if (piv) DRE_HIP(hipMemcpyAsync(piv, pv.p, (size_t)n * batch * sizeof(int), hipMemcpyDeviceToHost, c->stream));
        c->sync();
        std::vector<BatchMemberStatus> st((size_t)batch);
        for (int b = 0; b < batch; ++b) {
            if (h[(size_t)b].s.gj.singular) {
                st[(size_t)b].code = ERR_SINGULAR;
                st[(size_t)b].msg = std::string(who) + ", member " + std::to_string(b) + ": singular matrix (exactly zero or non-finite pivot)";
                continue;
            }
            for (int k = 0; k < np; ++k) copy_mat(c, plane(b, k), A[k][b]->m);
            if (logabsdet) logabsdet[b] = h[(size_t)b].s.gj.logdet;
        }
        c->sync();
        report_members(ctx, st, status);
    });
}
int dre_dense_invert_batched(dre_ctx* ctx, int batch, dre_dense* const* A, int32_t* piv, double* logabsdet, int32_t* status) {
    const char* name = "A";
    return invert_batched(ctx, "dre_dense_invert_batched", 1, &A, &name, batch, piv, logabsdet, status, gj_batch_nb, gj_invert_batched);
}
// ---- frequency response (freq_response.hip) --------------------------------------------------------------------------------------------
// the two sweeps' entry points: collect the systems, run `sweep` (freq_response or transfer_eval on them), copy H, info and the members' outcomes
// out.  noun: what the K points are called in the caller's messages
static void sweep_entry(dre_ctx* ctx, const char* who, const char* noun, bool args_ok, int nsys, const dre_dense* const* E, const dre_dense* const* A,
                        const dre_dense* const* B, const dre_dense* const* C, int K, double* H_re, double* H_im, int32_t* status, int64_t* info,
                        const std::function<FreqResponse(const std::vector<FreqSystem>&)>& sweep) {
    DRE_REQUIRE(nsys >= 1, std::string(who) + ": no systems (nsys < 1)");
    DRE_REQUIRE(K >= 1, std::string(who) + ": at least one " + noun + " is needed (K >= 1)");
    DRE_REQUIRE(E && A && B && C && args_ok && H_re && H_im && status, std::string(who) + ": null argument");
    std::vector<FreqSystem> sys((size_t)nsys);
    for (int s = 0; s < nsys; ++s) {
        DRE_REQUIRE(E[s] && A[s] && B[s] && C[s], std::string(who) + ": null operand in system " + std::to_string(s));
        sys[(size_t)s] = FreqSystem{E[s]->m, A[s]->m, B[s]->m, C[s]->m};
    }
    const FreqResponse r = sweep(sys);
    std::memcpy(H_re, r.re.data(), r.re.size() * sizeof(double));
    std::memcpy(H_im, r.im.data(), r.im.size() * sizeof(double));
    if (info) { info[0] = r.chunk; info[1] = r.chunks; }
    report_members(ctx, r.status, status);
}
int dre_freq_response_batched(dre_ctx* ctx, int nsys, const dre_dense* const* E, const dre_dense* const* A, const dre_dense* const* B,
                              const dre_dense* const* C, int K, const double* omega, int chunk, double* H_re, double* H_im, int32_t* status,
                              int64_t* info) {
    return guarded(ctx, [&] {
        sweep_entry(ctx, "dre_freq_response_batched", "frequency", omega != nullptr, nsys, E, A, B, C, K, H_re, H_im, status, info,
                    [&](const std::vector<FreqSystem>& sys) { return freq_response(&ctx->c, sys, std::vector<double>(omega, omega + K), chunk); });
    });
}
int dre_freq_response(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* C, int K, const double* omega,
                      int chunk, double* H_re, double* H_im, int32_t* status, int64_t* info) {
    return dre_freq_response_batched(ctx, 1, &E, &A, &B, &C, K, omega, chunk, H_re, H_im, status, info);
}

// ---- complex inversion and the transfer function at complex points (dense_cgj.hip, transfer_eval.hip) -----------------------------------
int dre_dense_invert_complex_batched(dre_ctx* ctx, int batch, dre_dense* const* Are, dre_dense* const* Aim, int32_t* piv, double* logabsdet,
                                     int32_t* status) {
    dre_dense* const* const planes[2] = {Are, Aim};
    const char* const names[2] = {"Are", "Aim"};
    return invert_batched(ctx, "dre_dense_invert_complex_batched", 2, planes, names, batch, piv, logabsdet, status, cgj_batch_nb, cgj_invert_batched);
}
int dre_transfer_eval_batched(dre_ctx* ctx, int nsys, const dre_dense* const* E, const dre_dense* const* A, const dre_dense* const* B,
                              const dre_dense* const* C, int K, const double* s_re, const double* s_im, int chunk, double* H_re, double* H_im,
                              int32_t* status, int64_t* info) {
    return guarded(ctx, [&] {
        sweep_entry(ctx, "dre_transfer_eval_batched", "point", s_re && s_im, nsys, E, A, B, C, K, H_re, H_im, status, info,
                    [&](const std::vector<FreqSystem>& sys) {
                        return transfer_eval(&ctx->c, sys, std::vector<double>(s_re, s_re + K), std::vector<double>(s_im, s_im + K), chunk);
                    });
    });
}
int dre_transfer_eval(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* C, int K, const double* s_re,
                      const double* s_im, int chunk, double* H_re, double* H_im, int32_t* status, int64_t* info) {
    return dre_transfer_eval_batched(ctx, 1, &E, &A, &B, &C, K, s_re, s_im, chunk, H_re, H_im, status, info);
}

// ---- time response: step, impulse, simulate (time_response.hip) --------------------------------------------------------------------------
int dre_time_response(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* C, int method, double dt, int K,
                      int kind, const double* U, int S, const double* X0, int block, double* Y, int64_t* info) {
    return guarded(ctx, [&] {
        DRE_REQUIRE(E && A && B && C && Y, "dre_time_response: null argument");
        const TimeResponse r = time_response(&ctx->c, E->m, A->m, B->m, C->m, method, dt, K, kind, U, S, X0, block);
        std::memcpy(Y, r.Y.data(), r.Y.size() * sizeof(double));
        if (info) { info[0] = r.block; info[1] = r.blocks; info[2] = r.squarings; info[3] = r.launches; }
    });
}

int dre_dense_gale_solve_batched(dre_ctx* ctx, int batch, const dre_dense* const* E, const dre_dense* const* F, const dre_dense* const* R,
                                 int maxiters, double tol, int max_refine, dre_dense** X, int64_t* iinfo, double* dinfo, int32_t* status) {
    return guarded_out<dre_dense>(ctx, [&](DenseOut& o) {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(E && F && R && X && status && batch >= 1 && E[0], "dre_dense_gale_solve_batched: null argument or batch < 1");
        const int n = E[0]->m.rows;
        check_batch_order(batch, n, "dre_dense_gale_solve_batched");
        check_members(batch, E, n, n, "dre_dense_gale_solve_batched", "E");
        check_members(batch, F, n, n, "dre_dense_gale_solve_batched", "F");
        check_members(batch, R, n, n, "dre_dense_gale_solve_batched", "R");
        DRE_REQUIRE(maxiters >= 1 && maxiters <= 1000, "dense path: maxiters must be in 1 .. 1000");
        require_memory(c, BatchedSignLyap::doubles_needed(batch, n, maxiters, 4));       // + the stacks of E, F, R and X
        for (int b = 0; b < batch; ++b) X[b] = nullptr;
        Mat Es = pack_stack(c, batch, E, n, n), Fs = pack_stack(c, batch, F, n, n), Rs = pack_stack(c, batch, R, n, n);
        Mat Xs(c, n, n * batch);
        BatchedSignLyap lyap(c, batch, Es, maxiters, tol, max_refine, 4);
        lyap.factor(Fs);
        std::vector<SignStats> stats;
        lyap.solve(Rs, Xs, stats);
        for (int b = 0; b < batch; ++b) {
            if (!lyap.alive(b)) continue;
            copy_mat(c, Xs.colsview(b * n, n), put(o, X + b, Mat(c, n, n))->m);
            solve_info(stats[(size_t)b], iinfo, dinfo, (size_t)b);
        }
        c->sync();
        report_members(ctx, lyap.status(), status);
    });
}
int dre_dense_gdre_solve_batched(dre_ctx* ctx, int batch, const dre_dense* const* E, const dre_dense* const* A, const dre_dense* const* B,
                                 const dre_dense* const* C, const dre_dense* const* X0, double t0, double tf, double dt, int order,
                                 int save_state, int maxiters, double tol, int max_refine, dre_gdre_result** out, int32_t* status) {
    return guarded_out<dre_gdre_result>(ctx, [&](AbiOut<dre_gdre_result>& o) {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(E && A && B && C && X0 && out && status && batch >= 1 && E[0] && B[0] && C[0],
                    "dre_dense_gdre_solve_batched: null argument or batch < 1");
        dense_check_order(order);
        DRE_REQUIRE(order <= 2, "dre_dense_gdre_solve_batched: only Ros1 and Ros2 (order 1, 2) are batched; order " + std::to_string(order) +
                                    " runs through dre_dense_gdre_solve");
        const int n = E[0]->m.rows, m = B[0]->m.cols, q = C[0]->m.rows;
        check_batch_order(batch, n, "dre_dense_gdre_solve_batched");
        check_members(batch, E, n, n, "dre_dense_gdre_solve_batched", "E");
        check_members(batch, A, n, n, "dre_dense_gdre_solve_batched", "A");
        check_members(batch, B, n, m, "dre_dense_gdre_solve_batched", "B");
        check_members(batch, C, q, n, "dre_dense_gdre_solve_batched", "C");
        check_members(batch, X0, n, n, "dre_dense_gdre_solve_batched", "X0");
        const int nsteps = (int)dense_time_grid(t0, tf, dt).size() - 1;
        DRE_REQUIRE(maxiters >= 1 && maxiters <= 1000, "dense path: maxiters must be in 1 .. 1000");
        require_memory(c, dense_gdre_batched_doubles(batch, n, m, q, nsteps, order, save_state != 0, maxiters));
        for (int b = 0; b < batch; ++b) out[b] = nullptr;
        Mat Es = pack_stack(c, batch, E, n, n), As = pack_stack(c, batch, A, n, n), Bs = pack_stack(c, batch, B, n, m),
            Cs = pack_stack(c, batch, C, q, n), Xs = pack_stack(c, batch, X0, n, n);
        std::vector<DenseGdreResult> res;
        std::vector<BatchMemberStatus> st;
        dense_gdre_solve_batched(c, batch, Es, As, Bs, Cs, Xs, m, q, t0, tf, dt, order, save_state != 0, maxiters, tol, max_refine, res, st);
        for (int b = 0; b < batch; ++b) wrap_dense_result(o, out + b, res[(size_t)b], n, m);
        report_members(ctx, st, status);
    });
}

// dre_dense_gare_solve per member (dense_are_batch.hip).  Unlike the three calls above the return value is the first failed member's code.
int dre_dense_gare_solve_batched(dre_ctx* ctx, int batch, const dre_dense* const* E, const dre_dense* const* A, const dre_dense* const* B,
                                 const dre_dense* const* Rinv, const dre_dense* const* Ct, const dre_dense* const* S, int maxiters, double tol,
                                 int max_refine, dre_dense** X, int64_t* iinfo, double* dinfo, int32_t* status) {
    int first_fail = DRE_OK;
    const int rc = guarded_out<dre_dense>(ctx, [&](DenseOut& o) {
        Ctx* c = &ctx->c;
        const char* who = "dre_dense_gare_solve_batched";
        DRE_REQUIRE(E && A && B && Ct && X && status && batch >= 1 && E[0] && B[0] && Ct[0], std::string(who) + ": null argument or batch < 1");
        DRE_REQUIRE(batch <= 65535, std::string(who) + ": batch must be in 1 .. 65535");
        const int n = E[0]->m.rows, m = B[0]->m.cols, q = Ct[0]->m.cols;
        DRE_REQUIRE(n >= 1 && 2 * n <= DENSE_MAX_N, std::string(who) + ": E must be square of order 1 .. " + std::to_string(DENSE_MAX_N / 2));
        check_members(batch, E, n, n, who, "E");
        check_members(batch, A, n, n, who, "A");
        check_members(batch, B, n, m, who, "B");
        check_members(batch, Ct, n, q, who, "Ct");
        // the inner matrices are optional per member: the array or single entries may be null (identity)
        bool anyR = false, anyS = false;
        for (int b = 0; b < batch; ++b) {
            if (Rinv && Rinv[b]) {
                anyR = true;
                DRE_REQUIRE(Rinv[b]->m.rows == m && Rinv[b]->m.cols == m, std::string(who) + ": Rinv of member " + std::to_string(b) + " must be m x m");
            }
            if (S && S[b]) {
                anyS = true;
                DRE_REQUIRE(S[b]->m.rows == q && S[b]->m.cols == q, std::string(who) + ": S of member " + std::to_string(b) + " must be q x q");
            }
        }
        // the batched inversion is the register panel's whatever dense_gj_panel says: gj_check_order's refusal, in its wording
        DRE_REQUIRE(2 * n <= GJ_REGISTER_MAX_N, std::string(who) + " (the Hamiltonian of order 2n): the register panel inverts matrices of order <= " +
                                                    std::to_string(GJ_REGISTER_MAX_N) + ", order = " + std::to_string(2 * n));
        DRE_REQUIRE(maxiters >= 1 && maxiters <= 1000, "dense GARE: maxiters must be in 1 .. 1000");
        DRE_REQUIRE(max_refine >= 0, "dense GARE: max_refine must be >= 0");
        require_memory(c, dense_gare_batched_doubles(batch, n, m, q, maxiters, max_refine));
        for (int b = 0; b < batch; ++b) X[b] = nullptr;
        Mat Es = pack_stack(c, batch, E, n, n), As = pack_stack(c, batch, A, n, n), Bs = pack_stack(c, batch, B, n, m),
            Cs = pack_stack(c, batch, Ct, n, q);
        auto pack_inner = [&](const dre_dense* const* h, int w) {
            Mat St(c, w, w * batch), I(c, w, w);
            set_identity(c, I);
            for (int b = 0; b < batch; ++b) {
                Mat v = St.colsview(b * w, w);
                copy_mat(c, h[b] ? h[b]->m : I, v);
            }
            return St;
        };
        Mat Rs, Ss;
        if (anyR && m > 0) Rs = pack_inner(Rinv, m);
        if (anyS && q > 0) Ss = pack_inner(S, q);
        std::vector<DenseGareResult> res;
        std::vector<BatchMemberStatus> st;
        dense_gare_solve_batched(c, batch, Es, As, Bs, Rs.p ? &Rs : nullptr, Cs, Ss.p ? &Ss : nullptr, m, q, maxiters, tol, max_refine, res, st);
        for (int b = 0; b < batch; ++b) {
            const DenseGareResult& r = res[(size_t)b];
            solve_info(r, iinfo, dinfo, (size_t)b);
            if (st[(size_t)b].code) {
                if (first_fail == DRE_OK) first_fail = st[(size_t)b].code;
                continue;
            }
            copy_mat(c, r.X, put(o, X + b, Mat(c, n, n))->m);
        }
        c->sync();
        report_members(ctx, st, status);
    });
    return rc != DRE_OK ? rc : first_fail;
}
// ---- factored sign-function Lyapunov solver (dense_sign_lr.hip) -----------------------------------------------------------------------
int dre_sign_create(dre_ctx* ctx, const dre_dense* E, const dre_dense* F, int maxiters, double tol, dre_sign** out) {
    return guarded_out<dre_sign>(ctx, [&](AbiOut<dre_sign>& o) {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(E && F && out, "dre_sign_create: null argument");
        const int n = E->m.rows;
        DRE_REQUIRE(F->m.rows == n && F->m.cols == n, "dre_sign_create: E and F must be n x n");
        dre_sign* h = o.make(out);
        Mat Ec(c, n, E->m.cols);            // the handle outlives the caller's E
        copy_mat(c, E->m, Ec);
        h->s = std::make_unique<SignLyap>(c, Ec, maxiters, tol, 0, 0, true);
        h->s->factor(F->m);
    });
}
int dre_sign_info(const dre_sign* s, int64_t* n_iters) {
    if (!s || !n_iters) return DRE_ERR_INVALID;
    *n_iters = s->s->iters();
    return DRE_OK;
}
// primal (F'XE + E'XF = -R / -G S G') and dual (F Y E' + E Y F' = ..., 109) solves on the same kept factorisation: one body per pair
static int sign_solve_lr(dre_ctx* ctx, bool dual, dre_sign* s, const dre_dense* G, const dre_dense* S, double rtol, int max_width, int max_refine,
                         dre_dense** L, dre_dense** D, int64_t* ii, double* dd, const char* null_msg) {
    return guarded_out<dre_dense>(ctx, [&](DenseOut& o) {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(s && G && S && L && D, null_msg);
        Mat &Lm = o.make(L)->m, &Dm = o.make(D)->m;
        const SignLrStats st = dual ? s->s->solve_lr_t(G->m, S->m, rtol, max_width, max_refine, Lm, Dm)
                                    : s->s->solve_lr(G->m, S->m, rtol, max_width, max_refine, Lm, Dm);
        c->sync();
        if (ii) { ii[0] = st.rank; ii[1] = st.peak_width; ii[2] = st.compressions; ii[3] = st.refinements; }
        if (dd) { dd[0] = st.res0; dd[1] = st.res; }
    });
}
static int sign_solve_dense(dre_ctx* ctx, bool dual, dre_sign* s, const dre_dense* R, int max_refine, dre_dense** X, int64_t* iinfo, double* dinfo,
                            const char* null_msg) {
    return guarded_out<dre_dense>(ctx, [&](DenseOut& o) {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(s && R && X && max_refine >= 0, null_msg);
        const int n = s->s->n();
        Mat& Xm = put(o, X, Mat(c, n, n))->m;
        s->s->set_max_refine(max_refine);
        const SignStats st = dual ? s->s->solve_t(R->m, Xm) : s->s->solve(R->m, Xm);
        c->sync();
        solve_info(st, iinfo, dinfo);
    });
}
int dre_sign_solve_lr(dre_ctx* ctx, dre_sign* s, const dre_dense* G, const dre_dense* S, double rtol, int max_width, int max_refine,
                      dre_dense** L, dre_dense** D, int64_t* ii, double* dd) {
    return sign_solve_lr(ctx, false, s, G, S, rtol, max_width, max_refine, L, D, ii, dd, "dre_sign_solve_lr: null argument");
}
int dre_sign_solve_dense(dre_ctx* ctx, dre_sign* s, const dre_dense* R, int max_refine, dre_dense** X, int64_t* iinfo, double* dinfo) {
    return sign_solve_dense(ctx, false, s, R, max_refine, X, iinfo, dinfo, "dre_sign_solve_dense: null argument or negative max_refine");
}
int dre_sign_solve_dense_t(dre_ctx* ctx, dre_sign* s, const dre_dense* R, int max_refine, dre_dense** Y, int64_t* iinfo, double* dinfo) {
    return sign_solve_dense(ctx, true, s, R, max_refine, Y, iinfo, dinfo, "dre_sign_solve_dense_t: null argument or negative max_refine");
}
int dre_sign_solve_lr_t(dre_ctx* ctx, dre_sign* s, const dre_dense* G, const dre_dense* S, double rtol, int max_width, int max_refine,
                        dre_dense** L, dre_dense** D, int64_t* ii, double* dd) {
    return sign_solve_lr(ctx, true, s, G, S, rtol, max_width, max_refine, L, D, ii, dd, "dre_sign_solve_lr_t: null argument");
}
int dre_sign_free(dre_ctx*, dre_sign* s) { delete s; return DRE_OK; }

// ---- dense generalized Sylvester solver (dense_sylvester.hip, 119) ---------------------------------------------------------------------
static void sylvester_info(const SylvStats& st, int64_t* iinfo, double* dinfo) {
    solve_info(st, iinfo, dinfo);
    if (dinfo) dinfo[2] = st.step;
}
int dre_dense_sylvester_solve(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* F, const dre_dense* B, const dre_dense* C,
                              int transposed, int maxiters, double tol, int max_refine, dre_dense** X, int64_t* iinfo, double* dinfo) {
    return guarded_out<dre_dense>(ctx, [&](DenseOut& o) {
        DRE_REQUIRE(A && B && C && X, "dre_dense_sylvester_solve: null argument");
        DenseSylvesterResult r = dense_sylvester_solve(&ctx->c, opt_mat(E), A->m, opt_mat(F), B->m, C->m, transposed != 0, maxiters, tol, max_refine);
        sylvester_info(r.st, iinfo, dinfo);
        put(o, X, std::move(r.X));
    });
}
int dre_dense_sylvester_residual(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* F, const dre_dense* B, const dre_dense* C,
                                 const dre_dense* X, int transposed, dre_dense** Res, double* norm, double* scaled) {
    return guarded_out<dre_dense>(ctx, [&](DenseOut& o) {
        DRE_REQUIRE(A && B && C && X && Res, "dre_dense_sylvester_residual: null argument");
        put(o, Res, dense_sylvester_residual(&ctx->c, opt_mat(E), A->m, opt_mat(F), B->m, C->m, X->m, transposed != 0, norm, scaled));
    });
}
int dre_sylvester_create(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* F, const dre_dense* B, int maxiters, double tol,
                         dre_sylvester** out) {
    return guarded_out<dre_sylvester>(ctx, [&](AbiOut<dre_sylvester>& o) {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(A && B && out, "dre_sylvester_create: null argument");
        const int n = A->m.rows, m = B->m.rows;
        DRE_REQUIRE(n >= 1 && m >= 1 && A->m.cols == n && B->m.cols == m && (!E || (E->m.rows == n && E->m.cols == n)) &&
                        (!F || (F->m.rows == m && F->m.cols == m)),
                    "dre_sylvester_create: E and A must be n x n, F and B m x m");
        DRE_REQUIRE(n <= DENSE_MAX_N && m <= DENSE_MAX_N, "dre_sylvester_create: orders of at most " + std::to_string(DENSE_MAX_N) + " expected");
        dre_sylvester* h = o.make(out);
        Mat Ec(c, n, n), Fc(c, m, m);            // the handle outlives the caller's E and F
        if (E) copy_mat(c, E->m, Ec); else set_identity(c, Ec);
        if (F) copy_mat(c, F->m, Fc); else set_identity(c, Fc);
        h->s = std::make_unique<SignSylvester>(c, Ec, Fc, maxiters, tol, 0);
        h->s->factor(A->m, B->m);
    });
}
int dre_sylvester_solve(dre_ctx* ctx, dre_sylvester* s, const dre_dense* C, int transposed, int max_refine, dre_dense** X, int64_t* iinfo, double* dinfo) {
    return guarded_out<dre_dense>(ctx, [&](DenseOut& o) {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(s && C && X && max_refine >= 0, "dre_sylvester_solve: null argument or negative max_refine");
        Mat& Xm = put(o, X, Mat(c, s->s->n(), s->s->m()))->m;
        s->s->set_max_refine(max_refine);
        const SylvStats st = transposed ? s->s->solve_t(C->m, Xm) : s->s->solve(C->m, Xm);
        c->sync();
        sylvester_info(st, iinfo, dinfo);
    });
}
int dre_sylvester_iters(const dre_sylvester* s, int64_t* n_iters) {
    if (!s || !n_iters) return DRE_ERR_INVALID;
    *n_iters = s->s->iters();
    return DRE_OK;
}
int dre_sylvester_destroy(dre_ctx*, dre_sylvester* s) { delete s; return DRE_OK; }

// device SVD and balanced truncation (110)
int dre_svd_jacobi(dre_ctx* ctx, const dre_dense* A, double tol, dre_dense** U, dre_dense** S, dre_dense** V, int64_t* stats) {
    return guarded_out<dre_dense>(ctx, [&](DenseOut& o) {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(A && U && S && V, "dre_svd_jacobi: null argument");
        SvjStats st;
        SvdResult r = svd_jacobi(c, A->m, tol, &st);
        c->sync();
        put(o, U, r.U); put(o, S, r.S); put(o, V, r.V);
        if (stats) { stats[0] = st.sweeps; stats[1] = st.rounds; stats[2] = st.rank; }
    });
}
// what the balance calls share: the six info words and three figures, and the six outputs (hsv, T, W, Ar, Br, Cr); member b of the batched
// call at ii + 6 b, dd + 3 b and slot[i] + b
static void balance_info(const BalanceResult& r, int64_t* ii, double* dd, size_t b = 0) {
    if (ii) { int64_t* p = ii + 6 * b; p[0] = r.order; p[1] = r.rank; p[2] = r.r_c; p[3] = r.r_o; p[4] = r.dropped; p[5] = r.sweeps; }
    if (dd) { double* p = dd + 3 * b; p[0] = r.eye_err; p[1] = r.bound; p[2] = r.neg_max; }
}
static void balance_out(DenseOut& o, const BalanceResult& r, dre_dense** const* slot, size_t b = 0) {
    const Mat* src[6] = {&r.hsv, &r.T, &r.W, &r.Ar, &r.Br, &r.Cr};
    for (int i = 0; i < 6; ++i) put(o, slot[i] + b, *src[i]);
}
int dre_balance_lr(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* C, const dre_dense* Lc, const dre_dense* Dc,
                   const dre_dense* Lo, const dre_dense* Do, int order, double tol, dre_dense** hsv, dre_dense** T, dre_dense** W, dre_dense** Ar,
                   dre_dense** Br, dre_dense** Cr, int64_t* ii, double* dd) {
    return guarded_out<dre_dense>(ctx, [&](DenseOut& o) {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(E && A && B && C && Lc && Dc && Lo && Do && hsv && T && W && Ar && Br && Cr, "dre_balance_lr: null argument");
        BalanceResult r = balance_lr(c, E->m, A->m, B->m, C->m, Lc->m, Dc->m, Lo->m, Do->m, order, tol);
        c->sync();
        dre_dense** const slot[6] = {hsv, T, W, Ar, Br, Cr};
        balance_out(o, r, slot);
        balance_info(r, ii, dd);
    });
}
// LQG balanced truncation from the two Riccati solutions (113)
int dre_lqg_balance(dre_ctx* ctx, const dre_dense* E, const dre_dense* A, const dre_dense* B, const dre_dense* C, const dre_dense* X, const dre_dense* Y,
                    int order, double tol, dre_dense** mu, dre_dense** T, dre_dense** W, dre_dense** Ar, dre_dense** Br, dre_dense** Cr, dre_dense** Kr,
                    dre_dense** Lr, dre_dense** Ac, int64_t* ii, double* dd) {
    return guarded_out<dre_dense>(ctx, [&](DenseOut& o) {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(E && A && B && C && X && Y && mu && T && W && Ar && Br && Cr && Kr && Lr && Ac, "dre_lqg_balance: null argument");
        LqgBalanceResult l = lqg_balance(c, E->m, A->m, B->m, C->m, X->m, Y->m, order, tol);
        const BalanceResult& r = l.bal;
        c->sync();
        dre_dense** const slot[6] = {mu, T, W, Ar, Br, Cr};
        balance_out(o, r, slot);
        put(o, Kr, l.Kr); put(o, Lr, l.Lr); put(o, Ac, l.Ac);
        balance_info(r, ii, dd);
    });
}

// batched block Jacobi and ensemble balanced truncation (111)
int dre_sym_eig_jacobi_batched(dre_ctx* ctx, int batch, const dre_dense* const* S, double tol, dre_dense** values, dre_dense** vectors, int64_t* stats,
                               int32_t* status) {
    return guarded_out<dre_dense>(ctx, [&](DenseOut& o) {
        Ctx* c = &ctx->c;
        const char* who = "dre_sym_eig_jacobi_batched";
        DRE_REQUIRE(S && values && vectors && status && batch >= 1, std::string(who) + ": null argument or batch < 1");
        for (int b = 0; b < batch; ++b) values[b] = vectors[b] = nullptr;
        SymEigBatch r = sym_eig_jacobi_batch(c, member_mats(batch, S, who, "S"), tol, who);
        // ascending order and the output format of dre_sym_eig_jacobi, per member; the eigenvalues of all members go up in one copy
        const int q = r.eig[0].q;
        std::vector<double> w((size_t)batch * q);
        DevArr<double> dw(c, w.size());
        for (int b = 0; b < batch; ++b) {
            if (r.status[(size_t)b].code) continue;
            const SymEig& e = r.eig[(size_t)b];
            std::vector<int> ids(e.j);
            for (int i = 0; i < e.j; ++i) ids[i] = i;
            std::sort(ids.begin(), ids.end(), [&](int a, int d) { return e.w[a] < e.w[d]; });
            for (int i = 0; i < e.j; ++i) w[(size_t)b * q + i] = e.w[ids[i]];
            put(o, vectors + b, sym_eig_backtransform(c, e, ids));
        }
        dw.upload(c, w);
        for (int b = 0; b < batch; ++b) {
            if (r.status[(size_t)b].code) continue;
            Mat& W = o.make(values + b)->m;
            W.buf = dw.buf; W.p = dw.p + (size_t)b * q;
            W.rows = q; W.cols = 1; W.ld = q > 0 ? q : 1;
            if (stats) { stats[2 * b] = r.stats[(size_t)b].sweeps; stats[2 * b + 1] = r.stats[(size_t)b].rounds; }
        }
        c->sync();
        report_members(ctx, r.status, status);
    });
}
int dre_svd_jacobi_batched(dre_ctx* ctx, int batch, const dre_dense* const* A, double tol, dre_dense** U, dre_dense** S, dre_dense** V, int64_t* stats,
                           int32_t* status) {
    return guarded_out<dre_dense>(ctx, [&](DenseOut& o) {
        Ctx* c = &ctx->c;
        const char* who = "dre_svd_jacobi_batched";
        DRE_REQUIRE(A && U && S && V && status && batch >= 1, std::string(who) + ": null argument or batch < 1");
        for (int b = 0; b < batch; ++b) U[b] = S[b] = V[b] = nullptr;
        SvdBatch r = svd_jacobi_batch(c, member_mats(batch, A, who, "A"), tol, who);
        c->sync();
        for (int b = 0; b < batch; ++b) {
            if (r.status[(size_t)b].code) continue;
            put(o, U + b, r.svd[(size_t)b].U); put(o, S + b, r.svd[(size_t)b].S); put(o, V + b, r.svd[(size_t)b].V);
            if (stats) { stats[3 * b] = r.stats[(size_t)b].sweeps; stats[3 * b + 1] = r.stats[(size_t)b].rounds; stats[3 * b + 2] = r.stats[(size_t)b].rank; }
        }
        report_members(ctx, r.status, status);
    });
}
int dre_balance_lr_batched(dre_ctx* ctx, int batch, const dre_dense* const* E, const dre_dense* const* A, const dre_dense* const* B,
                           const dre_dense* const* C, const dre_dense* const* Lc, const dre_dense* const* Dc, const dre_dense* const* Lo,
                           const dre_dense* const* Do, int order, double tol, dre_dense** hsv, dre_dense** T, dre_dense** W, dre_dense** Ar,
                           dre_dense** Br, dre_dense** Cr, int64_t* ii, double* dd, int32_t* status) {
    return guarded_out<dre_dense>(ctx, [&](DenseOut& o) {
        Ctx* c = &ctx->c;
        const char* who = "dre_balance_lr_batched";
        DRE_REQUIRE(E && A && B && C && Lc && Dc && Lo && Do && hsv && T && W && Ar && Br && Cr && status && batch >= 1,
                    std::string(who) + ": null argument or batch < 1");
        dre_dense** outs[6] = {hsv, T, W, Ar, Br, Cr};
        for (int b = 0; b < batch; ++b)
            for (dre_dense** slot : outs) slot[b] = nullptr;
        const dre_dense* const* ins[8] = {E, A, B, C, Lc, Dc, Lo, Do};
        std::vector<BalanceMember> mem((size_t)batch);
        for (int b = 0; b < batch; ++b) {
            for (auto* in : ins) DRE_REQUIRE(in[b], std::string(who) + ": a handle of member " + std::to_string(b) + " is null");
            mem[(size_t)b] = BalanceMember{&E[b]->m, &A[b]->m, &B[b]->m, &C[b]->m, &Lc[b]->m, &Dc[b]->m, &Lo[b]->m, &Do[b]->m};
        }
        BalanceBatch r = balance_lr_batch(c, mem, order, tol, who);
        c->sync();
        for (int b = 0; b < batch; ++b) {
            if (r.status[(size_t)b].code) continue;
            balance_out(o, r.res[(size_t)b], outs, (size_t)b);
            balance_info(r.res[(size_t)b], ii, dd, (size_t)b);
        }
        report_members(ctx, r.status, status);
    });
}

}  // extern "C"
