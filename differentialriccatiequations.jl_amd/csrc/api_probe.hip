// C ABI of libdre_hip, the test and diagnostic surface: the four probes that run internal entry points on caller-supplied operands, and nothing
// else.  No product path calls them and none of them launches a kernel of its own (the host tests read this file to prove it: each probe's
// text runs from its banner to the next one).
#include "abi.hpp"

#include <cstring>
#include <limits>

#include "gemm_probe_check.hpp"

using namespace dre;

extern "C" {

// ---- dre_gemm_probe: the internal GEMM entry points one by one (test and diagnostic surface) ------------------------------------------
namespace {
int64_t probe_cap(const dre_dense* d) {          // elements of the buffer from the matrix's first element on
    if (!d || !d->m.buf || !d->m.p) return -1;
    const char* base = (const char*)d->m.buf->p;
    const char* p = (const char*)d->m.p;
    if (p < base || (size_t)(p - base) > d->m.buf->bytes) return -1;
    return (int64_t)((d->m.buf->bytes - (size_t)(p - base)) / sizeof(double));
}
void probe_check(const dre_gemm_view* v, const char* what, int64_t count = 1, int64_t stride = 0) {
    DRE_REQUIRE(v && v->buf, std::string("dre_gemm_probe: missing view ") + what);
    DRE_REQUIRE(probe_view_fits(probe_cap(v->buf), v->offset, v->ld, v->rows, v->cols, count, stride),
                std::string("dre_gemm_probe: view ") + what + " does not lie inside its buffer");
}
double* probe_ptr(const dre_gemm_view* v) { return v->buf->m.p + v->offset; }
void probe_mat(const dre_gemm_view* v, Mat& m) { m.buf = v->buf->m.buf; m.p = probe_ptr(v); m.rows = v->rows; m.cols = v->cols; m.ld = v->ld; }
}  // namespace

int dre_gemm_probe(dre_ctx* ctx, int kind, int transA, int transB, double alpha, const dre_gemm_view* A, const dre_gemm_view* B, double beta,
                   const dre_gemm_view* C, const dre_gemm_probe_options* opt, int* splits_out) {
    return guarded(ctx, [&] {
        Ctx* c = &ctx->c;
        const dre_gemm_probe_options none = {};
        const dre_gemm_probe_options& o = opt ? *opt : none;
        const bool tA = transA != 0, tB = transB != 0;
        DRE_REQUIRE(kind >= DRE_PROBE_GEMM && kind <= DRE_PROBE_GEMM_SYM, "dre_gemm_probe: unknown kind");
        const int batch = o.batch > 0 ? o.batch : 1;
        DRE_REQUIRE(o.batch >= 0 && batch <= 65535, "dre_gemm_probe: batch");
        const bool stacked = kind == DRE_PROBE_GEMM_STRIDED || kind == DRE_PROBE_GEMM_Z;
        // what each kind can take
        const bool takes_done = kind == DRE_PROBE_GEMM || kind == DRE_PROBE_GEMM_THIN || kind == DRE_PROBE_GEMM_ROWS || kind == DRE_PROBE_GEMM_Z;
        const bool takes_count = kind == DRE_PROBE_GEMM_BATCHED || kind == DRE_PROBE_GEMM_ROWS || kind == DRE_PROBE_GEMM_SYM;
        DRE_REQUIRE(!o.use_done || takes_done, "dre_gemm_probe: this kind takes no done flag");
        DRE_REQUIRE(!o.use_count || takes_count, "dre_gemm_probe: this kind takes no device-side count");
        DRE_REQUIRE(!o.tile_sumsq || kind == DRE_PROBE_GEMM, "dre_gemm_probe: tile_sumsq belongs to gemm");
        DRE_REQUIRE((!o.member_on && !o.coef) || kind == DRE_PROBE_GEMM_STRIDED, "dre_gemm_probe: member_on and coef belong to gemm_strided");
        DRE_REQUIRE(!o.rowmap || kind == DRE_PROBE_GEMM_ROWS || kind == DRE_PROBE_GEMM_Z, "dre_gemm_probe: rowmap belongs to the reduce kinds");
        DRE_REQUIRE(stacked || o.batch <= 1, "dre_gemm_probe: this kind takes no batch");
        DRE_REQUIRE((o.nprod == 0 && !o.prod) || kind == DRE_PROBE_GEMM_BATCHED, "dre_gemm_probe: products belong to gemm_batched");
        DRE_REQUIRE(!o.use_count || (o.per >= 1 && o.nmax >= 0), "dre_gemm_probe: count needs per >= 1, nmax >= 0");

        int M = 0, N = 0, K = 0;
        if (kind != DRE_PROBE_GEMM_BATCHED) {
            const int64_t sa = stacked ? o.stride_a : 0, sb = stacked ? o.stride_b : 0;
            const int64_t sc = kind == DRE_PROBE_GEMM_STRIDED ? o.stride_c : (kind == DRE_PROBE_GEMM_Z ? o.cz : 0);
            probe_check(A, "A", batch, sa);
            probe_check(B, "B", batch, sb);
            probe_check(C, "C", batch, sc);
            if (kind == DRE_PROBE_GEMM_SYM) {
                M = N = C->rows; K = A->cols;
                DRE_REQUIRE(C->cols == M && A->rows == M && B->rows == M && B->cols == K && !tA && !tB, "dre_gemm_probe: gemm_sym_update takes A, B of n x K and C of n x n");
            } else {
                M = tA ? A->cols : A->rows; K = tA ? A->rows : A->cols; N = tB ? B->rows : B->cols;
                DRE_REQUIRE((tB ? B->cols : B->rows) == K, "dre_gemm_probe: inner dimensions differ");
                DRE_REQUIRE(C->cols == N, "dre_gemm_probe: C has the wrong number of columns");
                const bool mapped = kind == DRE_PROBE_GEMM_ROWS || (kind == DRE_PROBE_GEMM_Z && o.rowmap);
                DRE_REQUIRE(mapped ? C->rows >= M : C->rows == M, "dre_gemm_probe: C has the wrong number of rows");
                DRE_REQUIRE(kind != DRE_PROBE_GEMM_ROWS || o.rowmap, "dre_gemm_probe: gemm_reduce_rows needs a rowmap");
                DRE_REQUIRE(kind != DRE_PROBE_GEMM_THIN || !tB, "dre_gemm_probe: gemm_thin has no transposed B");
            }
            if (o.rowmap) for (int i = 0; i < M; ++i) DRE_REQUIRE(o.rowmap[i] >= 0 && o.rowmap[i] < C->rows, "dre_gemm_probe: rowmap entry outside C");
        }

        // device-side control blocks
        DevArr<AdiState> st;
        const AdiState* stp = nullptr;
        if (o.use_done || o.use_count) {
            std::vector<AdiState> h(1);
            std::memset(h.data(), 0, sizeof(AdiState));
            h[0].done = o.use_done ? o.done : 0; h[0].iters = o.iters;
            st = DevArr<AdiState>(c, 1); st.upload(c, h);
            stp = st.p;
        }
        const AdiState* done_st = o.use_done ? stp : nullptr;
        DevCount dc;
        if (o.use_count) { dc.st = stp; dc.base = o.base; dc.nmax = o.nmax; dc.per = o.per; }
        DevArr<int> rowmap;
        if (o.rowmap && M > 0) { rowmap = DevArr<int>(c, (size_t)M); rowmap.upload(c, o.rowmap, (size_t)M); }
        int splits = 1;

        switch (kind) {
        case DRE_PROBE_GEMM: {
            double* ss = nullptr;
            if (o.tile_sumsq) {
                DRE_REQUIRE(probe_cap(o.tile_sumsq) >= (int64_t)gemm_num_tiles(M, N), "dre_gemm_probe: tile_sumsq is too small");
                ss = o.tile_sumsq->m.p;
            }
            if (M > 0 && N > 0 && !(ss && K > 64)) splits = gemm_split_plan(c, ceil_div(M, 64) * ceil_div(N, 64), K);
            gemm(c, tA, tB, M, N, K, alpha, probe_ptr(A), A->ld, probe_ptr(B), B->ld, beta, probe_ptr(C), C->ld, done_st, "gemm_probe", ss);
            break;
        }
        case DRE_PROBE_GEMM_THIN:
            gemm_thin(c, tA, M, N, K, alpha, probe_ptr(A), A->ld, probe_ptr(B), B->ld, beta, probe_ptr(C), C->ld, done_st, "gemm_probe");
            break;
        case DRE_PROBE_GEMM_STRIDED: {
            DevArr<BatchCtl> ctl;
            BatchMask mask;
            if (o.member_on) {
                std::vector<BatchCtl> h((size_t)batch);
                std::memset(h.data(), 0, h.size() * sizeof(BatchCtl));
                for (int b = 0; b < batch; ++b) h[(size_t)b].fail = o.member_on[b] ? 0 : DRE_ERR_SINGULAR;
                ctl = DevArr<BatchCtl>(c, (size_t)batch); ctl.upload(c, h);
                mask.ctl = ctl.p;
            }
            DevArr<double> coef;
            if (o.coef) {
                DRE_REQUIRE(o.coef_stride >= 2 && o.coef_stride <= 4096, "dre_gemm_probe: coef_stride");
                coef = DevArr<double>(c, (size_t)batch * (size_t)o.coef_stride);
                coef.upload(c, o.coef, (size_t)batch * (size_t)o.coef_stride);
            }
            gemm_strided(c, batch, tA, tB, M, N, K, alpha, probe_ptr(A), A->ld, (size_t)o.stride_a, probe_ptr(B), B->ld, (size_t)o.stride_b, beta, probe_ptr(C),
                         C->ld, (size_t)o.stride_c, mask, "gemm_probe", o.coef ? coef.p : nullptr, o.coef ? (size_t)o.coef_stride : 0);
            c->sync();          // (the uploaded blocks live until here)
            break;
        }
        case DRE_PROBE_GEMM_BATCHED: {
            DRE_REQUIRE(o.nprod >= 0 && o.nprod <= 65535 && (o.nprod == 0 || o.prod), "dre_gemm_probe: product list");
            std::vector<GemmBatchDesc> descs;
            for (int i = 0; i < o.nprod; ++i) {
                const dre_gemm_product& p = o.prod[i];
                probe_check(&p.A, "A of a product"); probe_check(&p.B, "B of a product"); probe_check(&p.C, "C of a product");
                DRE_REQUIRE(p.A.cols == p.B.rows && p.C.rows == p.A.rows && p.C.cols == p.B.cols, "dre_gemm_probe: shapes of a product");
                GemmBatchDesc d;
                d.A = probe_ptr(&p.A); d.B = probe_ptr(&p.B); d.C = probe_ptr(&p.C); d.copy_dst = nullptr; d.alpha = p.alpha;
                d.M = p.A.rows; d.N = p.B.cols; d.K = p.A.cols; d.lda = p.A.ld; d.ldb = p.B.ld; d.ldc = p.C.ld; d.ldcopy = 0;
                if (p.copy_dst.buf) {
                    probe_check(&p.copy_dst, "copy_dst of a product");
                    DRE_REQUIRE(p.copy_dst.rows == d.M && p.copy_dst.cols == d.K, "dre_gemm_probe: copy_dst has the shape of A");
                    d.copy_dst = probe_ptr(&p.copy_dst); d.ldcopy = p.copy_dst.ld;
                }
                descs.push_back(d);
            }
            gemm_batched(c, descs, "gemm_probe", dc);
            break;
        }
        case DRE_PROBE_GEMM_ROWS: {
            BufP pb = gemm_partials(c, tA, tB, M, N, K, probe_ptr(A), A->ld, probe_ptr(B), B->ld, &splits, done_st, "gemm_probe", dc);
            gemm_reduce_rows(c, M, N, splits, (const double*)pb->p, rowmap.p, probe_ptr(C), C->ld, done_st);
            break;
        }
        case DRE_PROBE_GEMM_Z: {
            GemmZ zb;
            for (int z = 0; z < MF_ZMAX; ++z) {       // (a batch beyond MF_ZMAX is for gemm_partials_z to refuse)
                const int zz = std::min(z, batch - 1);
                zb.A[z] = probe_ptr(A) + (size_t)zz * (size_t)o.stride_a; zb.B[z] = probe_ptr(B) + (size_t)zz * (size_t)o.stride_b;
            }
            BufP pb = gemm_partials_z(c, tA, tB, M, N, K, zb, batch, A->ld, B->ld, &splits, done_st, "gemm_probe");
            gemm_reduce_z(c, M, N, splits, batch, (const double*)pb->p, o.rowmap ? rowmap.p : nullptr, probe_ptr(C), C->ld, (long)o.cz, done_st);
            break;
        }
        case DRE_PROBE_GEMM_SYM: {
            Mat Am, Bm, Xm;
            probe_mat(A, Am); probe_mat(B, Bm); probe_mat(C, Xm);
            if (M > 0 && K > 0) splits = gemm_split_plan(c, ceil_div(M, 64) * ceil_div(M, 64), K);
            gemm_sym_update(c, Am, Bm, Xm, "gemm_probe", dc);
            break;
        }
        }
        c->sync();
        if (splits_out) *splits_out = splits;
    });
}
// ---- dre_sym_eig_probe: the stages of the Householder + QL solver one by one (test and diagnostic surface) --------------------------------
int dre_sym_eig_probe(dre_ctx* ctx, const dre_dense* S, double tolfac, int want_eig, double abs_tol, int floor_mode, double deflate, const int32_t* ids,
                      int nids, int64_t* ii, double* snorm, dre_dense** d, dre_dense** e, dre_dense** tau, dre_dense** V, dre_dense** w, dre_dense** Z,
                      dre_dense** B) {
    return guarded_out<dre_dense>(ctx, [&](DenseOut& o) {
        Ctx* c = &ctx->c;
        dre_dense** outs[7] = {d, e, tau, V, w, Z, B};
        for (dre_dense** o : outs) if (o) *o = nullptr;
        DRE_REQUIRE(S && ii, "dre_sym_eig_probe: null argument");
        DRE_REQUIRE(S->m.rows == S->m.cols, "dre_sym_eig_probe: square matrix expected");
        DRE_REQUIRE(S->m.rows <= 8192, "dre_sym_eig_probe: order above 8192 not supported by the single-workgroup reduction");
        DRE_REQUIRE(nids <= 0 || ids, "dre_sym_eig_probe: ids missing");
        DRE_REQUIRE(nids == 0 || B, "dre_sym_eig_probe: ids without a place for B");
        DRE_REQUIRE(tolfac > 0.0 && deflate >= 0.0, "dre_sym_eig_probe: tolfac must be positive, deflate not negative");
        const int q = S->m.rows;
        Mat A(c, q, q);
        copy_mat(c, S->m, A);
        struct Method0 { Ctx* c; int was; ~Method0() { c->sym_eig_method = was; } } method0{c, c->sym_eig_method};
        c->sym_eig_method = 0;
        SymEig r = sym_eig(c, A, tolfac, want_eig != 0, abs_tol, floor_mode != 0, deflate);
        std::vector<int> cols;
        if (nids < 0) { cols.resize((size_t)r.j); for (int i = 0; i < r.j; ++i) cols[(size_t)i] = i; }          // (every column)
        else cols.assign(ids, ids + nids);
        for (int id : cols) DRE_REQUIRE(id >= 0 && id < r.j, "dre_sym_eig_probe: an entry of ids lies outside [0, jdim)");
        ii[0] = r.j; ii[1] = r.nref; ii[2] = q;
        if (snorm) *snorm = r.snorm;
        auto column = [&](dre_dense** slot, const double* src, bool on_host, int n) {
            dre_dense* h = put(o, slot, Mat(c, n, 1));
            if (n) DRE_HIP(hipMemcpyAsync(h->m.p, src, (size_t)n * sizeof(double), on_host ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, c->stream));
        };
        const bool has_z = want_eig && r.j > 0;
        if (d) column(d, r.d.p, false, r.j);
        if (e) column(e, r.e.p, false, std::max(r.j - 1, 0));
        if (tau) column(tau, r.tau.p, false, q);
        if (V) put(o, V, q ? r.V : Mat(c, 0, 0));
        if (w && has_z) column(w, r.w.data(), true, r.j);
        if (Z && has_z) put(o, Z, r.Z);
        if (B && !cols.empty()) put(o, B, sym_eig_backtransform(c, r, cols));
        c->sync();          // (r.w is host memory of this scope)
    });
}
// ---- dre_warm_probe: the kernels of the warm-started compression (warm.hip) on caller-supplied operands (test and diagnostic surface) -------
// Every launch goes through warm_project, warm_z, warm_zapply, warm_small, warm_eig, warm_finish or warm_chain_jacobi, with the buffer shapes of
// their callers (dense_x.hip, compress_warm; ldlt.hip, warm_compress_eig).
int dre_warm_probe(dre_ctx* ctx, const dre_warm_probe_args* args) {
    return guarded(ctx, [&] {
        DRE_REQUIRE(args, "dre_warm_probe: null argument");
        const dre_warm_probe_args& p = *args;
        const int st = p.stage, n = p.n, q = p.q, m = p.m, kl = p.kl, qn = p.qn;
        DRE_REQUIRE(st >= DRE_WARM_PROBE_PROJECT && st <= DRE_WARM_PROBE_CHAIN, "dre_warm_probe: unknown stage");
        DRE_REQUIRE(p.ldpad >= 0 && p.ldpad <= 64, "dre_warm_probe: ldpad must lie in 0 .. 64");
        const bool rows_n = st != DRE_WARM_PROBE_SMALL && st != DRE_WARM_PROBE_EIG;
        if (rows_n) DRE_REQUIRE(n >= 1 && n <= 65536, "dre_warm_probe: n must lie in 1 .. 65536");
        if (st == DRE_WARM_PROBE_PROJECT || st == DRE_WARM_PROBE_Z || st == DRE_WARM_PROBE_ZAPPLY || st == DRE_WARM_PROBE_SMALL || st == DRE_WARM_PROBE_CHAIN)
            DRE_REQUIRE(q >= 1 && q <= 64, "dre_warm_probe: q must lie in 1 .. 64");
        if (st == DRE_WARM_PROBE_Z || st == DRE_WARM_PROBE_CHAIN) DRE_REQUIRE(n <= 1024, "dre_warm_probe: n above 1024 (warm_z keeps all of Z in LDS)");
        if (st == DRE_WARM_PROBE_PROJECT) DRE_REQUIRE(p.Q && p.Yf && p.Pf, "dre_warm_probe: Q, Yf or Pf missing");
        if (st == DRE_WARM_PROBE_Z) DRE_REQUIRE(p.Z1 && p.Cw && p.Res, "dre_warm_probe: Z1, Cw or Res missing");
        if (st == DRE_WARM_PROBE_ZAPPLY) DRE_REQUIRE(p.Z1 && p.Cw, "dre_warm_probe: Z1 or Cw missing");
        if (st == DRE_WARM_PROBE_SMALL || st == DRE_WARM_PROBE_CHAIN) {
            const int mm = st == DRE_WARM_PROBE_CHAIN ? q + 16 : m;
            DRE_REQUIRE(mm == q || mm == q + 16, "dre_warm_probe: m must be q or q + 16");
            DRE_REQUIRE(mm <= 80, "dre_warm_probe: m above 80");
            DRE_REQUIRE(qn >= 1 && qn <= mm && (st != DRE_WARM_PROBE_CHAIN || qn <= 64), "dre_warm_probe: qn must lie in 1 .. m (chain: at most 64)");
            DRE_REQUIRE(kl >= 1 && kl <= qn, "dre_warm_probe: kl must lie in 1 .. qn");
            DRE_REQUIRE(p.nparts >= 0 && p.nparts <= (1 << 24) && (p.nparts == 0 || p.parts), "dre_warm_probe: nparts without parts");
            DRE_REQUIRE(p.budget_frac >= 0.0 && p.budget_frac <= 1.0, "dre_warm_probe: budget_frac must lie in 0 .. 1");
        }
        if (st == DRE_WARM_PROBE_SMALL) {
            DRE_REQUIRE(p.mode == 0 || p.mode == 1, "dre_warm_probe: mode must be 0 or 1");
            DRE_REQUIRE(p.Cc, "dre_warm_probe: Cc missing");
        }
        if (st == DRE_WARM_PROBE_EIG) {
            DRE_REQUIRE(m >= 1 && m <= 80, "dre_warm_probe: m must lie in 1 .. 80");
            DRE_REQUIRE(p.S, "dre_warm_probe: S missing");
        }
        if (st == DRE_WARM_PROBE_FINISH) {
            DRE_REQUIRE(q >= 1 && q <= 80, "dre_warm_probe: q must lie in 1 .. 80");
            DRE_REQUIRE(kl >= 1 && kl <= 80, "dre_warm_probe: kl must lie in 1 .. 80");
            DRE_REQUIRE(p.Q && p.Wk && p.Yp && p.Pp && p.tols_in, "dre_warm_probe: B, Wk, Yp, Pp or tols_in missing");
        }
        if (st == DRE_WARM_PROBE_CHAIN) DRE_REQUIRE(p.Res && p.basis, "dre_warm_probe: Res or basis missing");
        // (the arguments are judged without a context, so that the refusals can be tested on a machine without a device)
        DRE_REQUIRE(ctx, "dre_warm_probe: arguments accepted, context missing");
        Ctx* c = &ctx->c;
        const int ldn = n + p.ldpad;
        // a matrix of `rows` rows prefilled with NaN (all bits set): the view has the rows the entry points expect, the allocation ld of them
        auto nan_mat = [&](int rows, int ld, int cols) {
            Mat full(c, ld, cols);
            DRE_HIP(hipMemsetAsync(full.p, 0xFF, (size_t)ld * cols * sizeof(double), c->stream));
            return full.view(0, 0, rows, cols);
        };
        auto put = [&](const double* h, const Mat& v, int c0, int rows, int cols) {
            DRE_HIP(hipMemcpy2DAsync(v.p + (size_t)c0 * v.ld, (size_t)v.ld * sizeof(double), h, (size_t)rows * sizeof(double), (size_t)rows * sizeof(double), (size_t)cols,
                                     hipMemcpyHostToDevice, c->stream));
        };
        auto get = [&](double* h, const Mat& v, int c0, int cols) {          // whole columns of the allocation, padding rows included
            if (h) DRE_HIP(hipMemcpyAsync(h, v.p + (size_t)c0 * v.ld, (size_t)v.ld * cols * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        };
        auto nan_arr = [&](size_t cnt) {
            DevArr<double> d(c, std::max<size_t>(cnt, 1));
            DRE_HIP(hipMemsetAsync(d.p, 0xFF, d.n * sizeof(double), c->stream));
            return d;
        };
        auto up = [&](double* d, const double* h, size_t cnt) { if (cnt) DRE_HIP(hipMemcpyAsync(d, h, cnt * sizeof(double), hipMemcpyHostToDevice, c->stream)); };
        auto down = [&](double* h, const double* d, size_t cnt) { if (h && cnt) DRE_HIP(hipMemcpyAsync(h, d, cnt * sizeof(double), hipMemcpyDeviceToHost, c->stream)); };
        if (!c->warm_tickets) {
            c->warm_tickets = std::make_shared<Buf>(c, 4 * sizeof(int));
            DRE_HIP(hipMemsetAsync(c->warm_tickets->p, 0, 4 * sizeof(int), c->stream));
        }
        int* const tickets = (int*)c->warm_tickets->p;
        auto finish = [&] {
            int ht[4] = {-1, -1, -1, -1};
            DRE_HIP(hipMemcpyAsync(ht, tickets, 4 * sizeof(int), hipMemcpyDeviceToHost, c->stream));
            c->sync();
            if (p.ticket) { p.ticket[0] = ht[0]; p.ticket[1] = ht[1]; }
        };
        const int nstrip = rows_n ? ceil_div(n, 16) : 0, nslab = rows_n ? warm_project_slabs(n) : 0;
        if (st == DRE_WARM_PROBE_PROJECT || st == DRE_WARM_PROBE_Z || st == DRE_WARM_PROBE_ZAPPLY) {
            // the buffers of the callers: the basis buffer [Om | Q | Z], the right-hand block [Y_p, Y_f, W, Z, W_2], the slab with C behind the shares
            Mat QO = nan_mat(n, ldn, 32 + q + 16), YB = nan_mat(n, ldn, 64 + q), Z1 = nan_mat(n, ldn, 16);
            DevArr<double> slab = nan_arr((size_t)nslab * 256 + nstrip + 256);
            double* const Cw = slab.p + (size_t)nslab * 256 + nstrip;
            if (st == DRE_WARM_PROBE_PROJECT) {
                Mat Qv = QO.colsview(32, q), Yf = YB.colsview(16, 16), Pf(c, q, 16);
                put(p.Q, QO, 32, n, q); put(p.Yf, YB, 16, n, 16); up(Pf.p, p.Pf, (size_t)q * 16);
                warm_project(c, n, q, Qv, Yf, Pf, Z1, slab.p, tickets, Cw);
                get(p.Z1_out, Z1, 0, 16); down(p.Cw_out, Cw, 256); down(p.slab, slab.p, (size_t)nslab * 256);
            } else {
                put(p.Z1, Z1, 0, n, 16); up(Cw, p.Cw, 256);
                Mat Zb = QO.colsview(32 + q, 16), Zy = YB.colsview(32 + q, 16), W2 = YB.colsview(48 + q, 16);
                if (st == DRE_WARM_PROBE_Z) {
                    Mat Res = nan_mat(n, ldn, n);
                    put(p.Res, Res, 0, n, n);
                    warm_z(c, n, Z1, Cw, Res, Zb, Zy, W2);
                    get(p.W2, YB, 48 + q, 16);
                } else {
                    warm_zapply(c, n, Z1, Cw, Zb, Zy);
                }
                get(p.Zb, QO, 32 + q, 16); get(p.Zy, YB, 32 + q, 16);
            }
            finish();
            return;
        }
        if (st == DRE_WARM_PROBE_SMALL) {
            Mat Cc(c, m, 64 + q), Uc = nan_mat(m, m, qn), T = nan_mat(kl, kl, kl), Cp = nan_mat(m, m, 16), Mo = nan_mat(m, m, m), LT = nan_mat(m, m, m);
            up(Cc.p, p.Cc, (size_t)m * (64 + q));
            DevArr<double> parts(c, std::max(p.nparts, 1)), tols = nan_arr(12);
            up(parts.p, p.parts, (size_t)p.nparts);
            warm_small(c, q, m, kl, qn, Cc, p.nparts ? parts.p : nullptr, p.nparts, p.reltol, p.abstol, p.frac, p.budget_frac, tols.p, Uc, T, Cp, tickets + 1,
                       p.mode == 1 ? &Mo : nullptr, p.mode == 1 ? &LT : nullptr);
            down(p.tols, tols.p, 12); get(p.Uc, Uc, 0, qn); get(p.T, T, 0, kl); get(p.Cp, Cp, 0, 16); get(p.Mout, Mo, 0, m); get(p.LTout, LT, 0, m);
            finish();
            return;
        }
        if (st == DRE_WARM_PROBE_EIG) {
            Mat S(c, m, m), U = nan_mat(m, m, m);
            up(S.p, p.S, (size_t)m * m);
            warm_eig(c, m, S, U);
            get(p.U, U, 0, m);
            finish();
            return;
        }
        if (st == DRE_WARM_PROBE_FINISH) {
            const int rc = 16 * ceil_div(kl, 16);
            Mat B = nan_mat(n, ldn, q), Wk(c, q, kl), Yp = nan_mat(n, ldn, 16), Pp(c, q, 16), R = nan_mat(n, ldn, rc);
            put(p.Q, B, 0, n, q); up(Wk.p, p.Wk, (size_t)q * kl); put(p.Yp, Yp, 0, n, 16); up(Pp.p, p.Pp, (size_t)q * 16);
            DevArr<double> slab = nan_arr((size_t)nstrip), tols(c, 12);
            up(tols.p, p.tols_in, 12);
            warm_finish(c, n, q, kl, B, Wk, Yp, Pp, R, slab.p, tickets + 1, tols.p);
            get(p.R, R, 0, rc); down(p.tols, tols.p, 12); down(p.slab, slab.p, (size_t)nstrip);
            finish();
            return;
        }
        // CHAIN: the Jacobi form of the dense-X time loop's compression
        WarmChain w;
        const int mb = q + 16;
        w.n = n; w.qb = q; w.kl = kl; w.qn = qn;
        w.Res = nan_mat(n, ldn, n); w.QOc = nan_mat(n, ldn, 32 + 64 + 16); w.QOn = nan_mat(n, ldn, 32 + 64 + 16);
        put(p.Res, w.Res, 0, n, n); put(p.basis, w.QOc, 0, n, 32 + q);
        w.YB = nan_mat(n, ldn, 64 + q); w.Z1 = nan_mat(n, ldn, 16); w.Cc = nan_mat(mb, mb, 64 + q); w.Uc = nan_mat(mb, mb, qn); w.Cp = nan_mat(mb, mb, 16);
        w.Pf = nan_mat(q, q, 16); w.Tm = nan_mat(kl, kl, kl);
        DevArr<double> slab = nan_arr((size_t)nstrip * 256 + nstrip + 256), parts(c, std::max(p.nparts, 1)), tols = nan_arr(12);
        up(parts.p, p.parts, (size_t)p.nparts);
        w.slab = slab.p; w.tickets = tickets; w.tols = tols.p;
        w.parts = p.nparts ? parts.p : nullptr; w.nparts = p.nparts; w.reltol = p.reltol; w.abstol = p.abstol; w.frac = p.frac; w.bf = p.budget_frac;
        warm_chain_jacobi(c, w);
        get(p.R, w.QOn, 32, qn); get(p.basis_out, w.QOc, 0, 32 + q + 16); get(p.T, w.Tm, 0, kl); get(p.Uc, w.Uc, 0, qn); get(p.Cp, w.Cp, 0, 16);
        down(p.tols, tols.p, 12);
        finish();
    });
}
// ---- dre_adi_chain_probe: the dense-inverse ADI chain on caller-supplied operands (test and diagnostic surface) ----------------------------
// Every launch goes through adi_fast_build, adi_fast_pack_r, adi_fast_iter, adi_group_pack or adi_group_iter; the loops are those of adi_advance
// (engine.hip, fast branch) and of the dense-X time loop (dense_x.hip, group branch).
int dre_adi_chain_probe(dre_ctx* ctx, const dre_adi_chain_probe_args* args) {
    return guarded(ctx, [&] {
        DRE_REQUIRE(args, "dre_adi_chain_probe: null argument");
        const dre_adi_chain_probe_args& p = *args;
        const bool group = p.kind == DRE_ADI_PROBE_GROUP, build_only = p.kind == DRE_ADI_PROBE_BUILD;
        DRE_REQUIRE(p.kind == DRE_ADI_PROBE_FAST || group || build_only, "dre_adi_chain_probe: unknown kind");
        const int n = p.n, k = p.k, m = group ? 0 : p.m, nit = p.nit, g = p.g;
        DRE_REQUIRE(n >= 1 && n <= 8192, "dre_adi_chain_probe: n must lie in 1 .. 8192");
        DRE_REQUIRE(p.nstack >= 1 && p.nstack <= 4096 && p.stacks, "dre_adi_chain_probe: stacks missing");
        DRE_REQUIRE(m >= 0 && m <= 4096 && (m == 0 || p.wks), "dre_adi_chain_probe: m must not be negative and needs wks");
        int mode = 0, nt = 1;
        if (!build_only) {
            DRE_REQUIRE(k >= 1, "dre_adi_chain_probe: k must be at least 1");
            DRE_REQUIRE(k <= (group ? ADI_GROUP_MAX_K : ADI_FAST_MAX_K), "dre_adi_chain_probe: residual too wide");
            DRE_REQUIRE(nit >= 1 && nit <= 480, "dre_adi_chain_probe: nit must lie in 1 .. 480 (ring of the norm history)");
            DRE_REQUIRE(p.ncyc >= 1 && p.mu && p.R0 && p.T, "dre_adi_chain_probe: cycle, R0 or T missing");
            DRE_REQUIRE(p.ld >= n + 2, "dre_adi_chain_probe: ld must be at least n + 2");
            DRE_REQUIRE(p.base_it >= 0 && p.base_it <= (1 << 30), "dre_adi_chain_probe: base_it");
            if (group) {
                DRE_REQUIRE(g >= 2 && g <= ADI_GROUP_MAX_G, "dre_adi_chain_probe: g must lie in 2 .. 6");
                DRE_REQUIRE(nit % g == 0, "dre_adi_chain_probe: nit must be a multiple of g");
                DRE_REQUIRE(p.ncyc % g == 0 && p.nstack == p.ncyc / g, "dre_adi_chain_probe: one group stack per start position of the cycle (ncyc / g)");
                const int ct = (k + 15) / 16;
                DRE_REQUIRE(g * ct * ((ct + 3) / 4) <= ADI_FAST_NWS - 1, "dre_adi_chain_probe: norm meeting point too small");
            } else {
                DRE_REQUIRE(p.cycle, "dre_adi_chain_probe: cycle missing");
                for (int i = 0; i < p.ncyc; ++i) DRE_REQUIRE(p.cycle[i] >= 0 && p.cycle[i] < p.nstack, "dre_adi_chain_probe: entry of cycle outside [0, nstack)");
                DRE_REQUIRE((p.mode == -1) == (p.nt == -1), "dre_adi_chain_probe: mode and nt are picked together");
                if (p.mode == -1) adi_fast_pick(n, k, &mode, &nt);
                else {
                    DRE_REQUIRE(p.mode == 0 || p.mode == 1, "dre_adi_chain_probe: mode must be 0 or 1");
                    DRE_REQUIRE(p.nt == 1 || p.nt == 2 || p.nt == 4, "dre_adi_chain_probe: nt must be 1, 2 or 4");
                    mode = p.mode; nt = p.nt;
                }
            }
        }
        // (the arguments are judged without a context, so that the refusals can be tested on a machine without a device)
        DRE_REQUIRE(ctx, "dre_adi_chain_probe: arguments accepted, context missing");
        Ctx* c = &ctx->c;
        const int nstrip = adi_fast_nstrip(n), kst = adi_fast_kst(n);
        const double nan = std::numeric_limits<double>::quiet_NaN();
        auto up = [&](const double* h, size_t cnt) {
            DevArr<double> d(c, std::max<size_t>(cnt, 1));
            if (cnt) DRE_HIP(hipMemcpyAsync(d.p, h, cnt * sizeof(double), hipMemcpyHostToDevice, c->stream));
            return d;
        };
        auto nan_arr = [&](size_t cnt) {          // (all bits set is a NaN)
            DevArr<double> d(c, std::max<size_t>(cnt, 1));
            DRE_HIP(hipMemsetAsync(d.p, 0xFF, d.n * sizeof(double), c->stream));
            return d;
        };
        auto down = [&](double* h, const double* d, size_t cnt) { if (h && cnt) DRE_HIP(hipMemcpyAsync(h, d, cnt * sizeof(double), hipMemcpyDeviceToHost, c->stream)); };
        // ---- the packed stacks ----
        const int srows = group ? 2 * g * n : 2 * n + m;
        const size_t pkd = group ? (size_t)2 * g * nstrip * kst * 64 : adi_fast_pack_doubles(n);
        DevArr<double> stacks_d = up(p.stacks, (size_t)p.nstack * srows * n);
        DevArr<double> wks_d = up(p.wks, m ? (size_t)p.nstack * 2 * n * m : 0);
        DevArr<double> packs_d = nan_arr((size_t)p.nstack * pkd);
        if (group) {
            for (int s = 0; s < p.nstack; ++s) adi_group_pack(c, n, 2 * g, stacks_d.p + (size_t)s * srows * n, srows, packs_d.p + (size_t)s * pkd);
        } else {
            std::vector<const double*> stacks, wks; std::vector<double*> outs;
            for (int s = 0; s < p.nstack; ++s) {
                stacks.push_back(stacks_d.p + (size_t)s * srows * n);
                wks.push_back(m && !(p.wks_null && p.wks_null[s]) ? wks_d.p + (size_t)s * 2 * n * m : nullptr);
                outs.push_back(packs_d.p + (size_t)s * pkd);
            }
            adi_fast_build(c, n, m, stacks, srows, wks, 2 * n, outs);
        }
        down(p.packs, packs_d.p, (size_t)p.nstack * pkd);
        if (build_only) { c->sync(); return; }
        // ---- control block, meeting point, buffers ----
        AdiState hst;
        std::memset(&hst, 0, sizeof(hst));
        hst.iters = p.base_it; hst.maxiters = p.maxiters; hst.abstol = p.abstol; hst.res_norm = nan;
        for (double& v : hst.norms) v = nan;
        DevArr<AdiState> st(c, 1);
        DRE_HIP(hipMemcpyAsync(st.p, &hst, sizeof(AdiState), hipMemcpyHostToDevice, c->stream));
        DevArr<double> nws(c, ADI_FAST_NWS);
        DRE_HIP(hipMemsetAsync(nws.p, 0, ADI_FAST_NWS * sizeof(double), c->stream));
        DevArr<double> R0 = up(p.R0, (size_t)n * k), Tm = up(p.T, (size_t)k * k);
        const int ld = p.ld;
        const size_t ring = (size_t)ld * k * (nit + 1);
        DevArr<double> Vall = nan_arr(ring), Rring = nan_arr(ring);
        const bool use_pk = group || mode == 0;
        const size_t rpd = adi_fast_rpack_doubles(n, k);
        DevArr<double> Rp0 = nan_arr(use_pk ? rpd : 1);                          // exactly one slot, like the time loop's
        DevArr<double> Rpk = nan_arr(use_pk ? rpd * (size_t)(nit + 1) : 1);
        DevArr<double> Gm = nan_arr((size_t)k * k * 2 * (group ? g : 1));
        if (use_pk) adi_fast_pack_r(c, n, k, R0.p, n, Rp0.p, st.p);
        const int base_it = p.base_it;
        if (group) {
            const int NG = nit / g;
            AdiGroupArgs ga;
            std::memset(&ga, 0, sizeof(ga));
            ga.n = n; ga.k = k; ga.nstrip = nstrip; ga.kst = kst; ga.g = g;
            ga.ldr = ld; ga.rpd = rpd; ga.ldv = ld;
            ga.T = Tm.p; ga.ldt = k; ga.alpha = p.alpha; ga.st = st.p; ga.nws = nws.p;
            for (int L = 0; L <= NG + 1; ++L) {
                ga.do_strips = L < NG ? 1 : 0;
                if (L < NG) {
                    ga.Gpack = packs_d.p + (size_t)(((L * g) % p.ncyc) / g) * pkd;
                    ga.Rpc = L == 0 ? Rp0.p : Rpk.p + (size_t)(L * g) * rpd;
                    ga.Rring = Rring.p + (size_t)(L * g) * k * ld;
                    ga.Rpk = Rpk.p + (size_t)(L * g + 1) * rpd;
                    ga.V = Vall.p + (size_t)(L * g * k) * ld;
                }
                // Gram matrices of the residuals launch L - 1 produced; norms + decisions for those of launch L - 2
                ga.n_prev = (L >= 1 && L <= NG) ? g : 0;
                ga.Rp_prev = ga.n_prev ? Rpk.p + (size_t)((L - 1) * g + 1) * rpd : nullptr;
                ga.G_prev = Gm.p + (size_t)(L & 1) * g * k * k;
                ga.n_prev2 = L >= 2 ? g : 0;
                ga.G_prev2 = Gm.p + (size_t)((L - 1) & 1) * g * k * k;
                ga.it0_prev2 = base_it + (L - 2) * g + 1;
                adi_group_iter(c, ga);
            }
        } else {
            AdiFastArgs a;
            std::memset(&a, 0, sizeof(a));
            a.n = n; a.k = k; a.nstrip = nstrip; a.kst = kst; a.mode = mode; a.nt = nt;
            a.T = Tm.p; a.ldt = k; a.tdiag = p.tdiag ? 1 : 0; a.alpha = p.alpha; a.st = st.p; a.nws = nws.p;
            for (int j = 1; j <= nit; ++j) {
                const int pos = (j - 1) % p.ncyc;
                a.Apack = packs_d.p + (size_t)p.cycle[pos] * pkd;
                if (j == 1) { a.Rcur = R0.p; a.ldr = n; } else { a.Rcur = Rring.p + (size_t)(j - 2) * k * ld; a.ldr = ld; }
                a.Rnext = Rring.p + (size_t)(j - 1) * k * ld; a.ldr_next = ld;
                a.Rpc = use_pk ? (j == 1 ? Rp0.p : Rpk.p + (size_t)(j - 1) * rpd) : nullptr;
                a.Rpn = use_pk ? Rpk.p + (size_t)j * rpd : nullptr;
                a.V = Vall.p + (size_t)(j - 1) * k * ld; a.ldv = ld;
                a.two_mu = 2.0 * p.mu[pos];
                const int it = base_it + j;                                 // shifts consumed after this iteration
                a.G_prev = j >= 2 ? Gm.p + (size_t)((it - 1) & 1) * k * k : nullptr;
                a.G_prev2 = j >= 3 ? Gm.p + (size_t)((it - 2) & 1) * k * k : nullptr;
                a.it_prev2 = it - 2; a.do_strips = 1;
                adi_fast_iter(c, a);
            }
            {   // drain the norm pipeline: Gram matrix of the last residual, decisions for the last two iterations
                const int it = base_it + nit;
                a.do_strips = 0; a.Apack = nullptr; a.Rnext = nullptr; a.V = nullptr;
                a.Rpc = use_pk ? Rpk.p + (size_t)nit * rpd : nullptr; a.Rpn = nullptr;
                a.Rcur = Rring.p + (size_t)(nit - 1) * k * ld; a.ldr = ld;
                a.G_prev = Gm.p + (size_t)(it & 1) * k * k;
                a.G_prev2 = nit >= 2 ? Gm.p + (size_t)((it - 1) & 1) * k * k : nullptr;
                a.it_prev2 = it - 1;
                adi_fast_iter(c, a);
                a.G_prev = nullptr;
                a.G_prev2 = Gm.p + (size_t)(it & 1) * k * k;
                a.it_prev2 = it;
                adi_fast_iter(c, a);
            }
        }
        DRE_HIP(hipMemcpyAsync(&hst, st.p, sizeof(AdiState), hipMemcpyDeviceToHost, c->stream));
        down(p.V, Vall.p, ring);
        down(p.R, Rring.p, ring);
        down(p.G, Gm.p, (size_t)k * k * 2 * (group ? g : 1));
        if (p.Rp) {
            if (use_pk) { down(p.Rp, Rp0.p, rpd); down(p.Rp + rpd, Rpk.p + rpd, rpd * (size_t)nit); }
            else for (size_t i = 0; i < rpd * (size_t)(nit + 1); ++i) p.Rp[i] = nan;
        }
        c->sync();
        if (p.state_i) { p.state_i[0] = hst.iters; p.state_i[1] = hst.done; p.state_i[2] = mode; p.state_i[3] = nt; }
        if (p.state_d) { p.state_d[0] = hst.res_norm; p.state_d[1] = hst.abstol; std::memcpy(p.state_d + 2, hst.norms, sizeof(hst.norms)); }
    });
}

}  // extern "C"
