// C ABI of libdre_hip, the sparse low-rank family: shift factor and solve (with the two complex-split kernels), LDLt, ADI and its stepwise
// protocol, the communicator, GDRE and its result accessors (with k_traj_export).  The dense accessors of dre_gdre_result
// (dre_gdre_result_X_dense, _dense_stats, _step_stats) live in api_dense.hip, beside the solvers that fill them.
#include "abi.hpp"

#include <atomic>
#include <cstring>

#include "comm.hpp"

using namespace dre;

// one LDLt result: the factor is complete before the handle is made, so making and committing stand together
static void put_ldlt(dre_ldlt** slot, LDLtP x, const dre_pencil* pen) {
    AbiOut<dre_ldlt> o;
    put(o, slot, std::move(x), pen);
    o.commit();
}
// a result of the shift solves, in solver order -> a fresh handle in the user's order
static void put_user(Ctx* c, DenseOut& o, dre_dense** slot, const dre_pencil* pen, const Mat& solver) {
    Mat u = to_user_order(c, pen, solver);
    copy_mat(c, u, put(o, slot, Mat(c, u.rows, u.cols))->m);
}

extern "C" {

int dre_shift_factor(dre_ctx* ctx, const dre_pencil* p, double cA, double cE_re, double cE_im, dre_factor** out) {
    return guarded_out<dre_factor>(ctx, [&](AbiOut<dre_factor>& o) {
        const Pencil& P = *p->p;
        DRE_REQUIRE(P.has_device, "pencil was created host-only");
        dre_factor* f = o.make(out);
        f->pen = p;
        f->is_cplx = cE_im != 0.0;
        if (f->is_cplx) { mf_factor<cplx>(&ctx->c, P, P.valAt.p, P.valEt.p, cplx{cA, 0.0}, cplx{cE_re, cE_im}, f->fc); mf_check(&ctx->c, f->fc); }
        else { mf_factor<double>(&ctx->c, P, P.valAt.p, P.valEt.p, cA, cE_re, f->fr); mf_check(&ctx->c, f->fr); }
    });
}

__global__ void k_split_cplx(int rows, int cols, const cplx* __restrict__ src, int lds_, double* __restrict__ re, int ldr,
                             double* __restrict__ im, int ldi) {
    size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (size_t)rows * cols) return;
    int r = id % rows, c = id / rows;
    cplx z = src[r + (size_t)c * lds_];
    re[r + (size_t)c * ldr] = z.re;
    im[r + (size_t)c * ldi] = z.im;
}
__global__ void k_make_cplx(int rows, int cols, const double* __restrict__ src, int lds_, cplx* __restrict__ dst, int ldd) {
    size_t id = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (size_t)rows * cols) return;
    int r = id % rows, c = id / rows;
    dst[r + (size_t)c * ldd] = {src[r + (size_t)c * lds_], 0.0};
}

int dre_shift_solve(dre_ctx* ctx, const dre_factor* f, const dre_dense* B, dre_dense** X_re, dre_dense** X_im) {
    return guarded_out<dre_dense>(ctx, [&](DenseOut& o) {
        Ctx* c = &ctx->c;
        const Pencil& P = *f->pen->p;
        Mat Bs = to_solver_order(c, f->pen, B->m);
        const int n = P.n, k = Bs.cols;
        if (!f->is_cplx) {
            Mat W(c, n, k);
            copy_mat(c, Bs, W);
            mf_solve<double>(c, P, f->fr, W.p, W.ld, k);
            put_user(c, o, X_re, f->pen, W);
            if (X_im) *X_im = nullptr;
        } else {
            DRE_REQUIRE(X_im != nullptr, "complex factor needs an imaginary output");
            DevArr<cplx> W(c, (size_t)n * std::max(k, 1));
            size_t tot = (size_t)n * k;
            if (tot) hipLaunchKernelGGL(k_make_cplx, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, n, k, Bs.p, Bs.ld, W.p, n);
            mf_solve<cplx>(c, P, f->fc, W.p, n, k);
            Mat re(c, n, k), im(c, n, k);
            if (tot) hipLaunchKernelGGL(k_split_cplx, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, c->stream, n, k, W.p, n, re.p, re.ld, im.p, im.ld);
            put_user(c, o, X_re, f->pen, re); put_user(c, o, X_im, f->pen, im);
            c->sync();
        }
    });
}
int dre_shift_solve_smw(dre_ctx* ctx, const dre_factor* f, double alpha, const dre_dense* U, const dre_dense* Vt, const dre_dense* B,
                        dre_dense** X_re, dre_dense** X_im) {
    return guarded_out<dre_dense>(ctx, [&](DenseOut& o) {
        Ctx* c = &ctx->c;
        const Pencil& P = *f->pen->p;
        DRE_REQUIRE(U && Vt && B && X_re, "dre_shift_solve_smw: null argument");
        Mat Us = to_solver_order(c, f->pen, U->m), Vs = to_solver_order(c, f->pen, Vt->m), Bs = to_solver_order(c, f->pen, B->m);
        if (!f->is_cplx) {
            put_user(c, o, X_re, f->pen, smw_solve(c, P, f->fr, alpha, Us, Vs, Bs));
            c->sync();
            if (X_im) *X_im = nullptr;
        } else {
            DRE_REQUIRE(X_im != nullptr, "complex factor needs an imaginary output");
            Mat re, im;
            smw_solve(c, P, f->fc, alpha, Us, Vs, Bs, re, im);
            put_user(c, o, X_re, f->pen, re); put_user(c, o, X_im, f->pen, im);
            c->sync();
        }
    });
}
int dre_factor_growth(dre_ctx* ctx, const dre_factor* f, double* growth) {
    return guarded(ctx, [&] { *growth = f->is_cplx ? mf_check(&ctx->c, f->fc) : mf_check(&ctx->c, f->fr); });
}
int dre_factor_perturbed(dre_ctx* ctx, const dre_factor* f, int64_t* count) {
    return guarded(ctx, [&] {
        if (f->is_cplx) { if (f->fc.nperturbed < 0) mf_check(&ctx->c, f->fc); *count = f->fc.nperturbed; }
        else { if (f->fr.nperturbed < 0) mf_check(&ctx->c, f->fr); *count = f->fr.nperturbed; }
    });
}
int dre_factor_free(dre_ctx*, dre_factor* f) { delete f; return DRE_OK; }

// ---- LDLt --------------------------------------------------------------------------------------
int dre_ldlt_create(dre_ctx* ctx, const dre_pencil* p, const dre_dense* L, const dre_dense* D, double alpha, dre_ldlt** out) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(D->m.rows == D->m.cols && D->m.rows == L->m.cols, "lowrank: D must be k x k with k = size(L, 2)");
        Mat Ls = to_solver_order(c, p, L->m);
        if (!p) { Ls = Mat(c, L->m.rows, L->m.cols); copy_mat(c, L->m, Ls); }
        Mat Dc(c, D->m.rows, D->m.cols);
        copy_mat(c, D->m, Dc);
        put_ldlt(out, ldlt_make(c, L->m.rows, Ls, Dc, alpha, false), p);
    });
}
int dre_ldlt_zero(dre_ctx* ctx, const dre_pencil* p, int n, dre_ldlt** out) {
    return guarded(ctx, [&] { put_ldlt(out, ldlt_zero(n), p); });
}
int dre_ldlt_free(dre_ctx*, dre_ldlt* x) { delete x; return DRE_OK; }
int dre_ldlt_info(const dre_ldlt* x, int* n, int* rank, int* nblocks) {
    *n = x->x->n; *rank = x->x->rank(); *nblocks = (int)x->x->blocks.size();
    return DRE_OK;
}
int dre_ldlt_add(dre_ctx* ctx, const dre_ldlt* a, const dre_ldlt* b, dre_ldlt** out) {
    return guarded(ctx, [&] {
        DRE_REQUIRE(a->pen == b->pen, "LDLt operands live in different orderings");
        LDLtP x = ldlt_add(a->x, b->x);
        if (x.get() == a->x.get() || x.get() == b->x.get()) x = std::make_shared<LDLt>(*x);
        put_ldlt(out, x, a->pen);
    });
}
int dre_ldlt_scale(dre_ctx* ctx, const dre_ldlt* a, double alpha, dre_ldlt** out) {
    return guarded(ctx, [&] { put_ldlt(out, ldlt_scale(a->x, alpha), a->pen); });
}
int dre_ldlt_concatenate(dre_ctx* ctx, dre_ldlt* x) { return guarded(ctx, [&] { ldlt_concatenate(&ctx->c, *x->x); }); }
int dre_ldlt_compress(dre_ctx* ctx, dre_ldlt* x) { return guarded(ctx, [&] { ldlt_compress(&ctx->c, *x->x); }); }
int dre_ldlt_compress_tol(dre_ctx* ctx, dre_ldlt* x, double abs_tol) {
    return guarded(ctx, [&] { ldlt_compress(&ctx->c, *x->x, 4.0, false, abs_tol > 0.0 ? abs_tol : -1.0); });
}
int dre_ldlt_compress_fast(dre_ctx* ctx, dre_ldlt* x) { return guarded(ctx, [&] { ldlt_compress(&ctx->c, *x->x, 4.0, false, -1.0); }); }
int dre_ldlt_canonicalize(dre_ctx* ctx, dre_ldlt* x) {
    return guarded(ctx, [&] {
        LDLt& X = *x->x;
        if (X.blocks.size() > 1 || (X.blocks.size() == 1 && !X.blocks[0].diag && X.blocks[0].L.cols > 0)) ldlt_compress(&ctx->c, X, 4.0, true);
    });
}
int dre_ldlt_norm(dre_ctx* ctx, dre_ldlt* x, double* out) { return guarded(ctx, [&] { *out = ldlt_norm_accurate(&ctx->c, *x->x); }); }
int dre_ldlt_destructure(dre_ctx* ctx, dre_ldlt* x, double* alpha, double* Lh, int ldl, double* Dh, int ldd) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        ldlt_destructure(c, *x->x);
        const LBlock& b = x->x->blocks[0];
        if (alpha) *alpha = b.alpha;
        if (Lh) { Mat Lu = to_user_order(c, x->pen, b.L); download_mat(c, Lu, Lh, ldl); }
        if (Dh) download_mat(c, b.D, Dh, ldd);
    });
}

// ---- GALE / ADI --------------------------------------------------------------------------------
int dre_adi_default_options(dre_adi_options* o) {
    std::memset(o, 0, sizeof(*o));
    o->maxiters = 100; o->reltol = -1.0; o->abstol = -1.0; o->ignore_initial_guess = 0; o->compression_interval = 10;
    o->compression = 1; o->shift_kind = 1; o->n_history = 2; o->nshifts = 0; o->shifts_re = nullptr; o->shifts_im = nullptr;
    o->compress_tolfac = 4.0;
    o->compress_exact = 0;
    o->heuristic_kplus = 0; o->heuristic_kminus = 0;
    o->shift_fn = nullptr; o->shift_user = nullptr;
    return DRE_OK;
}
static AdiOptions convert_options(const dre_adi_options* o) {
    AdiOptions a;
    if (!o) return a;
    a.maxiters = o->maxiters; a.reltol = o->reltol; a.abstol = o->abstol; a.ignore_initial_guess = o->ignore_initial_guess != 0;
    a.compression_interval = o->compression_interval; a.compression = o->compression != 0;
    a.compress_tolfac = o->compress_tolfac > 0 ? o->compress_tolfac : 4.0;
    a.compress_exact = o->compress_exact != 0;
    a.inner_solve = o->inner_solve; a.inner_user = o->inner_user;
    if (o->shift_kind == 0) {
        a.shifts.kind = ShiftSpec::CYCLIC;
        DRE_REQUIRE(o->nshifts > 0 && o->shifts_re, "Cyclic shifts need at least one value");
        for (int i = 0; i < o->nshifts; ++i) a.shifts.values.emplace_back(o->shifts_re[i], o->shifts_im ? o->shifts_im[i] : 0.0);
    } else if (o->shift_kind == 2) {
        a.shifts.kind = ShiftSpec::HEURISTIC;
        DRE_REQUIRE(o->nshifts > 0 && o->heuristic_kplus > 0 && o->heuristic_kminus > 0, "Heuristic(nshifts, k+, k-) must be positive");
        a.shifts.h_nshifts = o->nshifts; a.shifts.h_kplus = o->heuristic_kplus; a.shifts.h_kminus = o->heuristic_kminus;
    } else if (o->shift_kind == 3) {
        a.shifts.kind = ShiftSpec::USER;
        DRE_REQUIRE(o->shift_fn != nullptr, "shift_kind 3 (user-defined strategy) needs shift_fn");
        DRE_REQUIRE(o->n_history > 0, "shift_kind 3: n_history must be positive");
        a.shifts.user_fn = o->shift_fn; a.shifts.user_data = o->shift_user; a.shifts.n_history = o->n_history;
    } else {
        a.shifts.kind = ShiftSpec::PROJECTION;
        DRE_REQUIRE(o->n_history > 0 && o->n_history % 2 == 0, "History must be even");   // projection.jl:28-32
        a.shifts.n_history = o->n_history;
    }
    return a;
}
static std::atomic<uint64_t> g_tag_counter{1ull << 40};     // operator identities for the factor caches (unique across threads)
static GaleOperator make_operator(Ctx* c, const dre_pencil* p, double cA, double cE, double lr_alpha, const dre_dense* U, const dre_dense* Vt) {
    const Pencil& P = *p->p;
    DRE_REQUIRE(P.has_device, "pencil was created host-only");
    GaleOperator op;
    op.P = &P;
    op.valFt = DevArr<double>(c, P.nnz);
    vals_axpby(c, P.nnz, cA, P.valAt.p, cE, P.valEt.p, op.valFt.p);
    op.tag = g_tag_counter++;
    op.cA = cA; op.cE = cE;
    if (U && Vt) {
        DRE_REQUIRE(U->m.rows == P.n && Vt->m.rows == P.n && U->m.cols == Vt->m.cols, "low-rank factors must be n x m");
        op.has_lr = true; op.alpha = lr_alpha;
        op.U = to_solver_order(c, p, U->m);
        op.Vt = to_solver_order(c, p, Vt->m);
    }
    return op;
}
// The sketch of a wide factor (ldlt.hip sketch_compress) is chosen from what earlier compressions at the same order left in the context:
// the rank hint and the fallback counters.  A solve entered through the ABI starts from a clean slate, so that two identical calls return
// identical bits whatever ran on the context before (the explicit compression entry dre_ldlt_compress_fast keeps the history: that is
// its documented behaviour).
static void reset_sketch_history(Ctx* c, int n) {
    const long skey = -(4000000000L + (long)n);
    c->band_hint.erase(skey); c->band_hint.erase(skey - 1); c->band_hint.erase(skey - 2);
}
int dre_gale_solve(dre_ctx* ctx, const dre_pencil* p, double cA, double cE, double lr_alpha, const dre_dense* U, const dre_dense* Vt,
                   dre_ldlt* C, const dre_ldlt* X0, const dre_adi_options* opt, dre_adi_result** out) {
    return guarded_out<dre_adi_result>(ctx, [&](AbiOut<dre_adi_result>& o) {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(C->pen == p && (!X0 || X0->pen == p), "LDLt operands must be created with the same pencil");
        GaleOperator op = make_operator(c, p, cA, cE, lr_alpha, U, Vt);
        AdiOptions ao = convert_options(opt);
        dre_adi_result* r = o.make(out);
        r->pen = p;
        reset_sketch_history(c, p->p->n);
        r->r = adi_solve(c, op, *C->x, X0 ? X0->x : nullptr, ao, nullptr);
    });
}
// ---- stepwise protocol: init / step! / isdone / solve! on the solver object (src/lyapunov/adi.jl:29-141) -------------------------
struct dre_adi_solver {
    std::shared_ptr<AdiRun> run;
    const dre_pencil* pen = nullptr;
};
int dre_adi_init(dre_ctx* ctx, const dre_pencil* p, double cA, double cE, double lr_alpha, const dre_dense* U, const dre_dense* Vt,
                 dre_ldlt* C, const dre_ldlt* X0, const dre_adi_options* opt, dre_adi_solver** out) {
    return guarded_out<dre_adi_solver>(ctx, [&](AbiOut<dre_adi_solver>& o) {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(C->pen == p && (!X0 || X0->pen == p), "LDLt operands must be created with the same pencil");
        GaleOperator op = make_operator(c, p, cA, cE, lr_alpha, U, Vt);
        AdiOptions ao = convert_options(opt);
        dre_adi_solver* s = o.make(out);
        s->pen = p;
        reset_sketch_history(c, p->p->n);
        s->run = adi_begin(c, op, *C->x, X0 ? X0->x : nullptr, ao, nullptr);
    });
}
int dre_adi_step(dre_ctx* ctx, dre_adi_solver* s) { return guarded(ctx, [&] { adi_advance(*s->run, 1); }); }
int dre_adi_solve(dre_ctx* ctx, dre_adi_solver* s) {
    return guarded(ctx, [&] { while (!adi_isdone(*s->run)) adi_advance(*s->run, 1 << 30); });
}
int dre_adi_isdone(const dre_adi_solver* s, int* done) { *done = adi_isdone(*s->run) ? 1 : 0; return DRE_OK; }
int dre_adi_state(const dre_adi_solver* s, int64_t* iters, double* res_norm, double* abstol) {
    int it = 0; double rn = 0, at = 0;
    adi_peek(*s->run, &it, &rn, &at);
    if (iters) *iters = it;
    if (res_norm) *res_norm = rn;
    if (abstol) *abstol = at;
    return DRE_OK;
}
int dre_adi_shifts(const dre_adi_solver* s, int64_t from, int64_t* count, double* re, double* im) {
    auto v = adi_shifts_since(*s->run, (int)from);
    if (count) *count = (int64_t)v.size();
    for (size_t i = 0; i < v.size(); ++i) { if (re) re[i] = v[i].real(); if (im) im[i] = v[i].imag(); }
    return DRE_OK;
}
int dre_adi_snapshot(dre_ctx* ctx, dre_adi_solver* s, dre_ldlt** X, dre_ldlt** residual) {
    return guarded_out<dre_ldlt>(ctx, [&](AbiOut<dre_ldlt>& o) {
        LDLtP x, r;
        adi_snapshot(*s->run, X ? &x : nullptr, residual ? &r : nullptr);
        if (X) put(o, X, x, s->pen);
        if (residual) put(o, residual, r, s->pen);
    });
}
int dre_adi_finish(dre_ctx* ctx, dre_adi_solver* s, dre_adi_result** out) {
    return guarded_out<dre_adi_result>(ctx, [&](AbiOut<dre_adi_result>& o) {
        dre_adi_result* r = o.make(out);
        r->pen = s->pen;
        r->r = adi_finish(*s->run);
    });
}
int dre_adi_free(dre_adi_solver* s) { delete s; return DRE_OK; }

int dre_heuristic_ritz(dre_ctx* ctx, const dre_pencil* p, double cA, double cE, double lr_alpha, const dre_dense* U, const dre_dense* Vt,
                       int kplus, int kminus, double* plus_re, double* plus_im, double* minus_re, double* minus_im) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        GaleOperator op = make_operator(c, p, cA, cE, lr_alpha, U, Vt);
        std::vector<std::complex<double>> rp, rm;
        heuristic_ritz(c, op, kplus, kminus, rp, rm);
        for (int i = 0; i < kplus; ++i) { plus_re[i] = rp[i].real(); plus_im[i] = rp[i].imag(); }
        for (int i = 0; i < kminus; ++i) { minus_re[i] = rm[i].real(); minus_im[i] = rm[i].imag(); }
    });
}
int dre_gale_residual(dre_ctx* ctx, const dre_pencil* p, double cA, double cE, double lr_alpha, const dre_dense* U, const dre_dense* Vt,
                      dre_ldlt* C, dre_ldlt* X, dre_ldlt** out) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        GaleOperator op = make_operator(c, p, cA, cE, lr_alpha, U, Vt);
        put_ldlt(out, gale_residual(c, op, *C->x, X ? X->x : nullptr), p);
    });
}
int dre_ldlt_dot(dre_ctx* ctx, const dre_ldlt* a, const dre_ldlt* b, double* out) {
    return guarded(ctx, [&] {
        DRE_REQUIRE(a->pen == b->pen, "dot: both operands must be created with the same pencil (same row ordering)");
        *out = ldlt_dot(&ctx->c, *a->x, *b->x);
    });
}
int dre_gale_apply(dre_ctx* ctx, const dre_pencil* p, double cA, double cE, double lr_alpha, const dre_dense* U, const dre_dense* Vt,
                   const dre_ldlt* X, dre_ldlt** out) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(X->pen == p, "LDLt operand must be created with the same pencil");
        GaleOperator op = make_operator(c, p, cA, cE, lr_alpha, U, Vt);
        put_ldlt(out, lyapunov_apply(c, op, X->x), p);
    });
}
int dre_gare_residual(dre_ctx* ctx, const dre_pencil* p, dre_ldlt* X, const dre_dense* Ct, const dre_dense* S, double gamma, const dre_dense* B,
                      const dre_dense* Rinv, double beta, dre_ldlt** out) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(X->pen == p, "LDLt operand must be created with the same pencil");
        DRE_REQUIRE(Ct->m.rows == p->p->n && B->m.rows == p->p->n && S->m.rows == Ct->m.cols && Rinv->m.rows == B->m.cols, "dre_gare_residual: shape mismatch");
        Mat Cs = to_solver_order(c, p, Ct->m), Bs = to_solver_order(c, p, B->m);
        put_ldlt(out, gare_residual_dev(c, *p->p, *X->x, Cs, S->m, gamma, Bs, Rinv->m, beta), p);
    });
}
int dre_ldlt_feedback(dre_ctx* ctx, const dre_pencil* p, dre_ldlt* X, const dre_dense* B, dre_dense** Kt) {
    return guarded_out<dre_dense>(ctx, [&](DenseOut& o) {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(X->pen == p && B->m.rows == p->p->n, "dre_ldlt_feedback: operand mismatch");
        Mat Bs = to_solver_order(c, p, B->m);
        Mat Ks = ldlt_feedback_dev(c, *p->p, *X->x, Bs);
        Mat Ku = to_user_order(c, p, Ks);
        copy_mat(c, Ku, put(o, Kt, Mat(c, Ku.rows, Ku.cols))->m);
    });
}
int dre_adi_result_info(const dre_adi_result* r, int64_t* info, double* dinfo) {
    info[0] = r->r.iters; info[1] = r->r.converged; info[2] = r->r.warnings; info[3] = (int64_t)r->r.norms.size(); info[4] = r->r.rhs_cols;
    dinfo[0] = r->r.res_norm; dinfo[1] = r->r.abstol; dinfo[2] = r->r.initial_norm;
    return DRE_OK;
}
int dre_adi_result_history(const dre_adi_result* r, double* norms, int32_t* norm_iters, double* sre, double* sim) {
    for (size_t i = 0; i < r->r.norms.size(); ++i) { if (norms) norms[i] = r->r.norms[i]; if (norm_iters) norm_iters[i] = r->r.norm_iters[i]; }
    for (size_t i = 0; i < r->r.shifts.size(); ++i) { if (sre) sre[i] = r->r.shifts[i].real(); if (sim) sim[i] = r->r.shifts[i].imag(); }
    return DRE_OK;
}
int dre_adi_result_take_x(dre_adi_result* r, dre_ldlt** X) { put_ldlt(X, r->r.X, r->pen); return DRE_OK; }
int dre_adi_result_take_residual(dre_adi_result* r, dre_ldlt** R) { put_ldlt(R, r->r.residual, r->pen); return DRE_OK; }
int dre_adi_result_free(dre_adi_result* r) { delete r; return DRE_OK; }

// ---- communicator (RCCL over xGMI, comm.hip) ----------------------------------------------------
int dre_comm_unique_id(dre_ctx* ctx, void* id128) { return guarded(ctx, [&] { DRE_REQUIRE(id128, "null id buffer"); comm_unique_id(id128); }); }
int dre_comm_init(dre_ctx* ctx, int nranks, int rank, const void* id128) {
    return guarded(ctx, [&] {
        const int emu = ctx->c.comm ? ctx->c.comm->emulate : 0;
        ctx->c.comm = comm_init(&ctx->c, nranks, rank, id128);
        ctx->c.comm->emulate = emu;
    });
}
int dre_comm_init_host(dre_ctx* ctx, int nranks, int rank, dre_comm_allgather_fn allgather, dre_comm_allreduce_fn allreduce, void* user) {
    return guarded(ctx, [&] {
        const int emu = ctx->c.comm ? ctx->c.comm->emulate : 0;
        ctx->c.comm = comm_init_host(&ctx->c, nranks, rank, allgather, allreduce, user);
        ctx->c.comm->emulate = emu;
    });
}
int dre_comm_free(dre_ctx* ctx) {
    return guarded(ctx, [&] { if (ctx->c.comm) { DRE_HIP(hipStreamSynchronize(ctx->c.stream)); ctx->c.comm.reset(); } });
}
int dre_comm_info(dre_ctx* ctx, int64_t* info) {
    const Comm* c = ctx->c.comm.get();
    info[0] = c ? c->nranks : 1; info[1] = c ? c->rank : 0; info[2] = c ? (int64_t)c->ncalls : 0;
    info[3] = c ? (int64_t)c->bytes_gathered : 0; info[4] = c ? (int64_t)c->bytes_reduced : 0; info[5] = c ? c->emulate : 0;
    return DRE_OK;
}
int dre_comm_allgather(dre_ctx* ctx, const void* send_dev, void* recv_dev, size_t count) {
    return guarded(ctx, [&] {
        DRE_REQUIRE(ctx->c.comm, "dre_comm_allgather: no communicator (dre_comm_init)");
        comm_allgather(&ctx->c, *ctx->c.comm, (const double*)send_dev, (double*)recv_dev, count);
    });
}
int dre_comm_allreduce_sum(dre_ctx* ctx, void* buf_dev, size_t count) {
    return guarded(ctx, [&] {
        DRE_REQUIRE(ctx->c.comm, "dre_comm_allreduce_sum: no communicator (dre_comm_init)");
        comm_allreduce_sum(&ctx->c, *ctx->c.comm, (double*)buf_dev, count);
    });
}

// ---- GDRE --------------------------------------------------------------------------------------
int dre_gdre_solve(dre_ctx* ctx, const dre_pencil* p, const dre_dense* B, const dre_dense* C, dre_ldlt* X0, double t0, double tf,
                   double dt, int order, int save_state, const dre_adi_options* opt, dre_gdre_result** out) {
    return guarded_out<dre_gdre_result>(ctx, [&](AbiOut<dre_gdre_result>& o) {
        Ctx* c = &ctx->c;
        const Pencil& P = *p->p;
        DRE_REQUIRE(P.has_device, "pencil was created host-only");
        DRE_REQUIRE(X0->pen == p, "X0 must be created with the same pencil");
        DRE_REQUIRE(B->m.rows == P.n && C->m.cols == P.n, "B must be n x m and C must be q x n");
        GdreProblem prob;
        prob.P = &P;
        prob.B = to_solver_order(c, p, B->m);
        Mat Ct(c, P.n, C->m.rows);
        transpose_mat(c, C->m, Ct);
        prob.Ct = to_solver_order(c, p, Ct);
        prob.X0 = X0->x;
        prob.t0 = t0; prob.tf = tf;
        AdiOptions ao = convert_options(opt);
        dre_gdre_result* r = o.make(out);
        r->pen = p; r->m = B->m.cols;
        reset_sketch_history(c, p->p->n);
        r->r = gdre_solve(c, prob, order, dt, save_state != 0, ao);
    });
}
int dre_gdre_result_info(const dre_gdre_result* r, int64_t* info) {
    if (r->dense) {
        info[0] = (int64_t)r->r.t.size(); info[1] = (int64_t)r->Xd.size(); info[2] = 0; info[3] = 0;
        info[4] = (int64_t)r->solves.size(); info[5] = r->m; info[6] = r->n;
        return DRE_OK;
    }
    info[0] = (int64_t)r->r.t.size(); info[1] = (int64_t)r->r.X.size(); info[2] = r->r.adi_iters; info[3] = r->r.nfactor;
    info[4] = (int64_t)r->r.gale.size(); info[5] = r->m; info[6] = r->pen->p->n;
    return DRE_OK;
}
int dre_gdre_result_times(const dre_gdre_result* r, double* t) {
    std::memcpy(t, r->r.t.data(), r->r.t.size() * sizeof(double));
    return DRE_OK;
}
int dre_gdre_result_K(dre_ctx* ctx, const dre_gdre_result* r, int i, double* K_host, int ld) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        DRE_REQUIRE(i >= 0 && i < (int)r->r.Kt.size(), "K index out of range");
        Mat Ktu = to_user_order(c, r->pen, r->r.Kt[i]);      // n x m
        Mat K(c, Ktu.cols, Ktu.rows);
        transpose_mat(c, Ktu, K);
        download_mat(c, K, K_host, ld);
    });
}
// K(t_i)(j, old) = Kt_i(iperm[old], j) for up to 64 time points per launch (the table of factors travels as kernel arguments): the whole
// trajectory leaves the solver ordering in one pass instead of a permutation and a transposition launch per time point
struct KTrajBatch { const double* Kt[64]; int ld[64]; };
__global__ void k_traj_export(int n, int m, const int* __restrict__ iperm, KTrajBatch bt, double* __restrict__ out) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= n * m) return;
    const int j = idx % m, old = idx / m;
    const int src = iperm ? iperm[old] : old;
    out[(size_t)blockIdx.y * n * m + idx] = bt.Kt[blockIdx.y][src + (size_t)j * bt.ld[blockIdx.y]];
}
static void export_trajectory(Ctx* c, const dre_gdre_result* r, double* K_dev) {
    const int nt = (int)r->r.Kt.size();
    if (nt == 0) return;
    const int n = r->r.Kt[0].rows, m = r->r.Kt[0].cols;
    if (n * m == 0) return;
    for (int i0 = 0; i0 < nt; i0 += 64) {
        KTrajBatch bt;
        const int nb = std::min(64, nt - i0);
        for (int i = 0; i < 64; ++i) {
            const Mat& K = r->r.Kt[(size_t)(i0 + std::min(i, nb - 1))];
            DRE_REQUIRE(K.rows == n && K.cols == m, "K trajectory: inconsistent shapes");
            bt.Kt[i] = K.p; bt.ld[i] = K.ld;
        }
        hipLaunchKernelGGL(k_traj_export, dim3((unsigned)((n * m + 255) / 256), (unsigned)nb), dim3(256), 0, c->stream, n, m,
                           r->pen ? (const int*)r->pen->p->iperm.p : (const int*)nullptr, bt, K_dev + (size_t)i0 * n * m);
    }
    DRE_HIP(hipGetLastError());
}
int dre_gdre_result_K_device(dre_ctx* ctx, const dre_gdre_result* r, double* K_dev) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        export_trajectory(c, r, K_dev);
        c->sync();
    });
}
int dre_gdre_result_K_all(dre_ctx* ctx, const dre_gdre_result* r, double* K_host) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        const int nt = (int)r->r.Kt.size();
        if (nt == 0) return;
        const size_t tot = (size_t)nt * r->r.Kt[0].rows * r->r.Kt[0].cols;
        if (tot == 0) return;
        DevArr<double> stage(c, tot);
        export_trajectory(c, r, stage.p);
        DRE_HIP(hipMemcpyAsync(K_host, stage.p, tot * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        c->sync();
    });
}
int dre_gdre_result_X(const dre_gdre_result* r, int i, dre_ldlt** X) {
    if (r->dense || i < 0 || i >= (int)r->r.X.size()) return DRE_ERR_INVALID;
    // a final X the solve left in dense form is factored here, once, on the stream of the solve's context (gdre.hip, gdre_result_x); the
    // handle is const for the caller, the cache behind it is not
    GdreResult& res = const_cast<dre_gdre_result*>(r)->r;
    Ctx* const c = res.final_x ? res.final_x->ctx : nullptr;
    LDLtP x;
    try { x = gdre_result_x(res, i); }
    catch (const Error& e) { if (c) c->last_error = e.what(); else g_noctx_error = e.what(); return e.code; }
    catch (const std::exception& e) { if (c) c->last_error = e.what(); else g_noctx_error = e.what(); return DRE_ERR_INTERNAL; }
    put_ldlt(X, x, r->pen);
    return DRE_OK;
}
// the first four and two words that dre_gdre_result_gale and dre_gdre_result_gales_all report of one inner solve
static void gale_info(const AdiResult& a, int64_t* ii, double* dd) {
    if (ii) { ii[0] = a.iters; ii[1] = a.converged; ii[2] = a.warnings; ii[3] = a.rhs_cols; }
    if (dd) { dd[0] = a.res_norm; dd[1] = a.abstol; }
}
int dre_gdre_result_gale(const dre_gdre_result* r, int j, int64_t* iinfo, double* dinfo) {
    if (r->dense) return DRE_ERR_INVALID;
    if (j < 0 || j >= (int)r->r.gale.size()) return DRE_ERR_INVALID;
    gale_info(r->r.gale[j], iinfo, dinfo);
    return DRE_OK;
}
int dre_gdre_result_gale_history(const dre_gdre_result* r, int j, int64_t* counts, double* norms, int32_t* norm_iters, double* sre, double* sim) {
    if (r->dense) return DRE_ERR_INVALID;
    if (j < 0 || j >= (int)r->r.gale.size()) return DRE_ERR_INVALID;
    const AdiResult& g = r->r.gale[j];
    if (counts) { counts[0] = (int64_t)g.norms.size(); counts[1] = (int64_t)g.shifts.size(); }
    for (size_t i = 0; i < g.norms.size(); ++i) { if (norms) norms[i] = g.norms[i]; if (norm_iters) norm_iters[i] = g.norm_iters[i]; }
    for (size_t i = 0; i < g.shifts.size(); ++i) { if (sre) sre[i] = g.shifts[i].real(); if (sim) sim[i] = g.shifts[i].imag(); }
    return DRE_OK;
}
int dre_gdre_result_gales_all(const dre_gdre_result* r, int64_t* iinfo, double* dinfo, double* norms, int32_t* norm_iters, double* sre, double* sim) {
    if (r->dense) return DRE_ERR_INVALID;
    size_t on = 0, os = 0;
    for (size_t j = 0; j < r->r.gale.size(); ++j) {
        const AdiResult& g = r->r.gale[j];
        gale_info(g, iinfo ? iinfo + 6 * j : nullptr, dinfo ? dinfo + 2 * j : nullptr);
        if (iinfo) { iinfo[6 * j + 4] = (int64_t)g.norms.size(); iinfo[6 * j + 5] = (int64_t)g.shifts.size(); }
        for (size_t i = 0; i < g.norms.size(); ++i) { if (norms) norms[on + i] = g.norms[i]; if (norm_iters) norm_iters[on + i] = g.norm_iters[i]; }
        for (size_t i = 0; i < g.shifts.size(); ++i) { if (sre) sre[os + i] = g.shifts[i].real(); if (sim) sim[os + i] = g.shifts[i].imag(); }
        on += g.norms.size(); os += g.shifts.size();
    }
    return DRE_OK;
}
int dre_gdre_result_free(dre_gdre_result* r) { delete r; return DRE_OK; }

}  // extern "C"
