// Dense GARE solver (GAREProblem + MatrixSign; in the place of the reference's riccati/newton.jl for dense data):
//   Z0 = H = [[A, -G], [-Q, -A']], K = diag(E, E')        the Hamiltonian pencil, 2n x 2n, assembled on the device from the factors of G and Q;
//   Z_{k+1} = struct((Z_k / c_k + c_k K Z_k^-1 K) / 2)     the generalized sign iteration with determinantal scaling, gj_invert on a copy of Z_k
//                                                         and eight n x n GEMMs for K W K; the update kernel keeps JZ symmetric (Byers);
//   (Z_inf + K)[I; XE] = 0                                extraction by the blocked Householder QR of the 2n x n operand [Z12; Z22 + E'];
//   (A - GXE)'DE + E'D(A - GXE) = -R(X), X <- X + D       Newton-Kleinman refinement with SignLyap on the closed loop.
// Every kernel indexes n x n blocks of the 2n x 2n operands in size_t (2n <= DENSE_MAX_N).  The host model of exactly this solver is
// tests/_hamiltonian_sign_model.py.
//
// dense_gare_solve_pair (host model tests/_lqg_model.py) returns, from the SAME sign iteration, also the filter solution Y of
//   G + A Y E' + E Y A' - E Y Q Y E' = 0:   its pencil is (H', K'), whose Z_inf is Z_inf', so
//   (Z_inf' + K')[I; Y E'] = 0              extraction from the transposed blocks, M_f = [Z21'; Z22' + E], rhs_f = -[Z11' + E'; Z12'] (k_are_extract_ops_t),
//   F_f D E' + E D F_f' = -R_f(Y)           Newton-Kleinman on the dual closed loop F_f = A - E Y Q with SignLyap::solve_t.
// The dual extraction runs first, in Zi, and leaves Z untouched; the regulator's extraction then runs exactly as in the single call.  Memory,
// checked before any kernel: the single call's 24 n^2 plus Y, 25 n^2; with refinement SignLyap's (maxiters + 10) n^2 and the step's two n x n
// (the regulator's and the filter's residual and step matrices are live one after the other and share the pool's blocks).
#include "dense_are.hpp"

#include <cmath>
#include <memory>

#include "dense.hpp"
#include "dense_are_body.hpp"
#include "profiling.hpp"

namespace dre {

// Device-side control words of the sign iteration and of the residual (read back once per step by the host).
struct AreCtl {
    double step;        // ||Z_{k+1} - Z_k||_F / ||Z_{k+1}||_F
    double best;        // smallest step so far
    double res;         // scaled residual ||R||_F / (||Q||_F + 2 ||A'XE||_F + ||E'XGXE||_F) of the last residual evaluation
    double resnorm;     // ||R||_F
    int since;          // unscaled iterations since the last new minimum of the step
    int scale;          // determinantal scaling still on
    int done;           // 0 running, 1 converged, 2 stagnated, 3 non-finite, 4 singular Z_k
    int pad;
};

__global__ void k_are_ctl_init(AreCtl* c) {
    c->step = 0.0; c->best = INFINITY; c->res = 0.0; c->resnorm = 0.0;
    c->since = 0; c->scale = 1; c->done = 0; c->pad = 0;
}

// The kernels' bodies are dense_are_body.hpp's, shared with the member-indexed kernels of dense_are_batch.hip.
__global__ __launch_bounds__(256) void k_are_assemble(int n, const double* __restrict__ A, const double* __restrict__ G, const double* __restrict__ Q,
                                                      double* __restrict__ Z, double* __restrict__ Zi) {
    are_assemble_body(KERNEL_GRID_STRIDE, n, A, G, Q, Z, Zi);
}

// c = (|det Z_k| / |det K|)^(1/2n) while ctl->scale, else 1
__global__ __launch_bounds__(256) void k_are_update(int n, double* __restrict__ Z, double* __restrict__ Zi, const GjCtl* ictl, const AreCtl* actl,
                                                    double logdetK, double* __restrict__ part) {
    if (ictl->singular) return;                     // (uniform: k_are_decide reports it)
    const double c = actl->scale ? exp((ictl->logdet - logdetK) / (2.0 * n)) : 1.0;
    are_update_body(KERNEL_GRID_STRIDE, n, Z, Zi, c, part);
}

// the stopping norm and the decision of the sign iteration
__global__ __launch_bounds__(256) void k_are_decide(int nparts, const double* __restrict__ part, double tol, const GjCtl* ictl, AreCtl* c) {
    double s[2];                                    // ||Z_{k+1} - Z_k||^2, ||Z_{k+1}||^2
    load_partials(nparts, part, s);
    if (threadIdx.x != 0) return;
    if (ictl->singular) { c->done = 4; return; }
    const double d = sqrt(s[0] / s[1]);
    c->step = d;
    const int done = are_step_rule(d, tol, c->best, c->since, c->scale);
    if (done) c->done = done;
}

__global__ __launch_bounds__(256) void k_are_extract_ops(int n, const double* __restrict__ Z, const double* __restrict__ E, double* __restrict__ Zi) {
    are_extract_ops_body(KERNEL_GRID_STRIDE, n, Z, E, Zi);
}

// one workgroup per 32 x 32 tile of the n x n blocks
__global__ __launch_bounds__(256) void k_are_extract_ops_t(int n, const double* __restrict__ Z, const double* __restrict__ E, double* __restrict__ Zi) {
    are_extract_ops_t_body(n, Z, E, Zi);
}

__global__ __launch_bounds__(256) void k_are_residual(int n, const double* __restrict__ Q, const double* __restrict__ AXE, const double* __restrict__ XGX,
                                                      double* __restrict__ Res, double* __restrict__ part) {
    are_residual_body(KERNEL_GRID_STRIDE, n, Q, AXE, XGX, Res, part);
}

__global__ __launch_bounds__(256) void k_are_residual_finish(int nparts, const double* __restrict__ part, AreCtl* c) {
    double s[4];
    load_partials(nparts, part, s);
    if (threadIdx.x == 0) c->res = are_scaled_residual(s, &c->resnorm);
}

// the "what" of a sign iteration that ended with done > 1 at iteration k (done 4: the singular Z_k), behind the caller's "dense GARE: "
std::string gare_sign_failure(int done, int k, double step, int maxiters) {
    if (done == 4) return "singular Z_" + std::to_string(k) + " in the sign iteration";
    if (done == 2)
        return "the sign iteration stagnated at a relative step " + std::to_string(step) +
               " (Hamiltonian eigenvalues on or near the imaginary axis: not stabilizable or not detectable?)";
    if (done == 3) return "the sign iteration produced non-finite values";
    return "the sign iteration did not converge in " + std::to_string(maxiters) + " iterations (relative step " + std::to_string(step) +
           "; Hamiltonian eigenvalues on or near the imaginary axis?)";
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
namespace {

// G = B Rinv B' (Rinv null: B B'), n x n
void form_gram(Ctx* ctx, const Mat& B, const Mat* Rinv, Mat& G) {
    if (B.cols == 0) { fill_mat(ctx, G, 0.0); return; }
    if (Rinv) {
        Mat BR(ctx, B.rows, B.cols);
        gemm(ctx, false, false, 1.0, B, *Rinv, 0.0, BR, nullptr, "dense_are");
        gemm(ctx, false, true, 1.0, BR, B, 0.0, G, nullptr, "dense_are");
    } else {
        gemm(ctx, false, true, 1.0, B, B, 0.0, G, nullptr, "dense_are");
    }
}

void check_operands(const Mat& E, const Mat& A, const Mat& B, const Mat* Rinv, const Mat& Ct, const Mat* S) {
    const int n = E.rows;
    DRE_REQUIRE(n >= 1 && 2 * n <= DENSE_MAX_N, "dense GARE: E must be square of order 1 .. " + std::to_string(DENSE_MAX_N / 2) +
                                                    " (the Hamiltonian of order 2n, the device's 32-bit index limit)");
    DRE_REQUIRE(E.cols == n && A.rows == n && A.cols == n && B.rows == n && Ct.rows == n, "dense GARE: E, A must be n x n, B n x m, Ct n x q");
    DRE_REQUIRE(E.ld == n && A.ld == n, "dense GARE: E and A must be stored with leading dimension n");
    DRE_REQUIRE(!Rinv || (Rinv->rows == B.cols && Rinv->cols == B.cols), "dense GARE: Rinv must be m x m");
    DRE_REQUIRE(!S || (S->rows == Ct.cols && S->cols == Ct.cols), "dense GARE: S must be q x q");
}

// The regulator's residual and, with dual = true and the roles of G and Q exchanged by the caller, the filter's: R_f(Y) = G + A Y E' + E Y A' - E Y Q Y E'
// is the same chain with the transposition flags of its first two GEMMs flipped (XE holds Y E', AXE holds A Y E', GXE holds Q Y E').
struct Residual {
    Ctx* c;
    const Mat &E, &A, &G, &Q;
    const bool tE, tA;          // X op(E) and op(A) (X op(E)): regulator (N, T), filter (T, N)
    Mat XE, AXE, GXE, XGX, Res;
    DevArr<double> part;
    DevArr<AreCtl> ctl;
    Residual(Ctx* ctx, const Mat& E_, const Mat& A_, const Mat& G_, const Mat& Q_, const DevArr<AreCtl>& ctl_, bool dual = false)
        : c(ctx), E(E_), A(A_), G(G_), Q(Q_), tE(dual), tA(!dual), part(ctx, 4 * NORM_PARTS), ctl(ctl_) {
        const int n = E.rows;
        XE = Mat(c, n, n); AXE = Mat(c, n, n); GXE = Mat(c, n, n); XGX = Mat(c, n, n); Res = Mat(c, n, n);
    }
    // Res = R(X); returns the scaled residual, *fro = ||R(X)||_F (synchronising)
    double eval(const Mat& X, double* fro = nullptr) {
        const int n = E.rows;
        gemm(c, false, tE, 1.0, X, E, 0.0, XE, nullptr, "are_residual");           // X E
        gemm(c, tA, false, 1.0, A, XE, 0.0, AXE, nullptr, "are_residual");         // A' X E
        gemm(c, false, false, 1.0, G, XE, 0.0, GXE, nullptr, "are_residual");      // G X E
        gemm(c, true, false, 1.0, XE, GXE, 0.0, XGX, nullptr, "are_residual");     // E' X G X E
        {
            TimedScope ts(c, "are_residual_sym", 48.0 * n * n, 0.0);
            hipLaunchKernelGGL(k_are_residual, dim3(NORM_PARTS), dim3(256), 0, c->stream, n, (const double*)Q.p, (const double*)AXE.p, (const double*)XGX.p,
                               Res.p, part.p);
            hipLaunchKernelGGL(k_are_residual_finish, dim3(1), dim3(256), 0, c->stream, NORM_PARTS, (const double*)part.p, ctl.p);
        }
        const AreCtl h = read_back(c, ctl.p);
        if (fro) *fro = h.resnorm;
        return h.res;
    }
};

}  // namespace

Mat dense_gare_residual(Ctx* ctx, const Mat& E, const Mat& A, const Mat& B, const Mat* Rinv, const Mat& Ct, const Mat* S, const Mat& X, double* fro) {
    check_operands(E, A, B, Rinv, Ct, S);
    const int n = E.rows;
    DRE_REQUIRE(X.rows == n && X.cols == n && X.ld == n, "dense GARE residual: X must be n x n");
    require_memory(ctx, 8 * (size_t)n * n);
    Mat G(ctx, n, n), Q(ctx, n, n);
    form_gram(ctx, B, Rinv, G);
    form_gram(ctx, Ct, S, Q);
    DevArr<AreCtl> ctl(ctx, 1);
    hipLaunchKernelGGL(k_are_ctl_init, dim3(1), dim3(1), 0, ctx->stream, ctl.p);
    Residual r(ctx, E, A, G, Q, ctl);
    r.eval(X, fro);
    return r.Res;
}

namespace {

// One solution's refinement: Newton-Kleinman steps on res (the regulator's Residual, or the filter's with dual = true) while the scaled residual
// exceeds the target and decreases.  who: empty in the single call, else the solution's name for the messages of the pair call.
void refine(Ctx* ctx, Residual& res, SignLyap* lyap, const Mat& A, int max_refine, bool dual, const char* who, DenseGareResult& out) {
    const int n = A.rows;
    out.res0 = out.res = res.eval(out.X);
    const double target = 100.0 * n * DBL_EPS;
    auto axpby = [&](Mat& o, double a0, const Mat& M0, double a1, const Mat& M1) { comb(ctx, o, a0, M0, a1, &M1, 0.0, nullptr, false, "are_axpby"); };
    if (lyap && out.res > target) {
        Mat F(ctx, n, n), D(ctx, n, n), Xn(ctx, n, n);
        while (out.res > target && out.refinements < max_refine) {
            try {
                if (dual) {
                    gemm(ctx, true, false, 1.0, res.XE, res.G, 0.0, D, nullptr, "are_residual");   // (Y E')' Q = E Y Q  (res.G is the filter's Q)
                    axpby(F, 1.0, A, -1.0, D);                                           // F_f = A - E Y Q
                    lyap->factor(F);
                    lyap->solve_t(res.Res, D);                                           // F_f D E' + E D F_f' = -R_f(Y)
                } else {
                    axpby(F, 1.0, A, -1.0, res.GXE);                                     // F = A - G X E
                    lyap->factor(F);                                                     // NOT_STABLE: X is not the stabilizing solution
                    lyap->solve(res.Res, D);                                             // F'DE + E'DF = -R(X)
                }
            } catch (const Error& e) {
                if (!*who) throw;
                throw Error(e.code, std::string("dense GARE pair, ") + who + " refinement: " + e.what());
            }
            axpby(Xn, 1.0, out.X, 1.0, D);
            const double rn = res.eval(Xn);
            ++out.refinements;
            if (!(rn < out.res)) break;                                                  // stopped decreasing: keep the better iterate
            std::swap(out.X, Xn);
            out.res = rn;
        }
    }
}

// dense_gare_solve (dual null) and dense_gare_solve_pair (dual: receives the filter solution)
DenseGareResult gare_solve(Ctx* ctx, const Mat& E, const Mat& A, const Mat& B, const Mat* Rinv, const Mat& Ct, const Mat* S, int maxiters, double tol,
                           int max_refine, DenseGareResult* dual) {
    check_operands(E, A, B, Rinv, Ct, S);
    const int n = E.rows, n2 = 2 * n;
    gj_check_order(ctx, n2, "dense GARE (the Hamiltonian of order 2n)");
    DRE_REQUIRE(maxiters >= 1 && maxiters <= 1000, "dense GARE: maxiters must be in 1 .. 1000");
    DRE_REQUIRE(max_refine >= 0, "dense GARE: max_refine must be >= 0");
    const double tol2 = tol > 0.0 ? tol : 10.0 * n2 * DBL_EPS;
    // Up-front memory check, before any kernel: Z, Zi (8 n^2), the extraction's QR (V, VT, grouped VT: 6 n^2; R: n^2), E^-1, G, Q, X and the
    // residual's five n x n work matrices (9 n^2): 24 n^2; with refinement also SignLyap's (maxiters + 10) n^2 and the step's two n x n.
    // The pair call adds Y: 25 n^2 (the dual extraction works in Zi, its residual and step matrices follow the regulator's in the same blocks).
    const size_t own = dual ? 25 : 24;
    std::unique_ptr<SignLyap> lyap;
    if (max_refine > 0) lyap.reset(new SignLyap(ctx, E, maxiters, tol, max_refine, own + 2));     // (its constructor checks the whole sum)
    else require_memory(ctx, own * (size_t)n * n);

    DenseGareResult out;
    Mat G(ctx, n, n), Q(ctx, n, n), Einv(ctx, n, n);
    form_gram(ctx, B, Rinv, G);
    form_gram(ctx, Ct, S, Q);
    DevArr<int> piv(ctx, n2);
    DevArr<GjCtl> ictl(ctx, 1);
    DevArr<AreCtl> actl(ctx, 1);
    DevArr<double> part(ctx, 2 * NORM_PARTS);
    DRE_HIP(hipMemsetAsync(ictl.p, 0, sizeof(GjCtl), ctx->stream));
    hipLaunchKernelGGL(k_are_ctl_init, dim3(1), dim3(1), 0, ctx->stream, actl.p);
    // E^-1 and log|det K| = 2 log|det E|
    copy_mat(ctx, E, Einv);
    gj_invert(ctx, Einv, piv.p, ictl.p);
    const GjCtl he = read_back(ctx, ictl.p);
    if (he.singular) throw Error(ERR_SINGULAR, "dense GARE: E is singular (zero pivot in the Gauss-Jordan inversion)");
    const double logdetK = 2.0 * he.logdet;

    // ---- sign iteration on the Hamiltonian pencil ----
    Mat Z(ctx, n2, n2), Zi(ctx, n2, n2), T(ctx, n, n);
    {
        TimedScope ts(ctx, "are_assemble", 8.0 * 12 * n * n, 0.0);
        hipLaunchKernelGGL(k_are_assemble, dim3(grid_for((size_t)n * n)), dim3(256), 0, ctx->stream, n, (const double*)A.p, (const double*)G.p,
                           (const double*)Q.p, Z.p, Zi.p);
    }
    AreCtl h{};
    bool converged = false;
    for (int k = 0; k < maxiters && !converged; ++k) {
        gj_invert(ctx, Zi, piv.p, ictl.p);
        // Zi <- K Zi K block by block: W_ab <- K_a W_ab K_b with K_0 = E, K_1 = E'
        for (int b = 0; b < 2; ++b) {
            for (int a = 0; a < 2; ++a) {
                Mat W = Zi.view(a * n, b * n, n, n);
                gemm(ctx, false, b == 1, 1.0, W, E, 0.0, T, nullptr, "are_kwk");
                gemm(ctx, a == 1, false, 1.0, E, T, 0.0, W, nullptr, "are_kwk");
            }
        }
        {
            TimedScope ts(ctx, "are_update", 8.0 * 4 * 4.0 * n * n, 0.0);
            hipLaunchKernelGGL(k_are_update, dim3(NORM_PARTS), dim3(256), 0, ctx->stream, n, Z.p, Zi.p, (const GjCtl*)ictl.p, (const AreCtl*)actl.p,
                               logdetK, part.p);
            hipLaunchKernelGGL(k_are_decide, dim3(1), dim3(256), 0, ctx->stream, NORM_PARTS, (const double*)part.p, tol2, (const GjCtl*)ictl.p, actl.p);
        }
        h = read_back(ctx, actl.p);
        out.iters = k + 1;
        if (h.done == 1) converged = true;
        else if (h.done) throw Error(h.done == 4 ? ERR_SINGULAR : ERR_NOT_STABLE, "dense GARE: " + gare_sign_failure(h.done, k, h.step, maxiters));
    }
    if (!converged) throw Error(ERR_NOT_STABLE, "dense GARE: " + gare_sign_failure(5, maxiters, h.step, maxiters));

    // ---- pair: the filter's extraction first, [Z21'; Z22' + E] Yr = -[Z11' + E'; Z12'], Y = sym(Yr E^-T); it works in Zi and leaves Z as it is ----
    if (dual) {
        dual->iters = out.iters;
        {
            TimedScope ts(ctx, "are_extract_ops", 8.0 * 10 * n * n, 0.0);
            const unsigned tiles = (unsigned)((n + 31) / 32);
            hipLaunchKernelGGL(k_are_extract_ops_t, dim3(tiles, tiles), dim3(256), 0, ctx->stream, n, (const double*)Z.p, (const double*)E.p, Zi.p);
        }
        Mat M = Zi.colsview(0, n), rhs = Zi.colsview(n, n);
        dual->X = Mat(ctx, n, n);
        QRFact f = qr_factor(ctx, M);
        qr_apply_q(ctx, f, rhs, true);
        gj_invert(ctx, f.R, piv.p, ictl.p);
        if (read_back(ctx, ictl.p).singular)
            throw Error(ERR_SINGULAR, "dense GARE pair, filter: [Z21'; Z22' + E] is rank deficient (no stable deflating subspace of dimension n)");
        const Mat top = rhs.view(0, 0, n, n);
        gemm(ctx, false, false, 1.0, f.R, top, 0.0, T, nullptr, "are_extract");      // Yr = R^-1 (Q' rhs)(0:n, :)
        Mat YEi = Zi.view(0, 0, n, n);                                               // (M and rhs are spent)
        gemm(ctx, false, true, 1.0, T, Einv, 0.0, YEi, nullptr, "are_extract");      // Yr E^-T
        comb(ctx, dual->X, 1.0, YEi, 0.0, nullptr, 0.0, nullptr, true, "are_sym", 3);
    }

    // ---- extraction: [Z12; Z22 + E'] Y = -[Z11 + E; Z21] by Householder QR, X = sym(Y E^-1) ----
    {
        TimedScope ts(ctx, "are_extract_ops", 8.0 * 10 * n * n, 0.0);
        hipLaunchKernelGGL(k_are_extract_ops, dim3(grid_for((size_t)n * n)), dim3(256), 0, ctx->stream, n, (const double*)Z.p, (const double*)E.p, Zi.p);
    }
    Mat M = Zi.colsview(0, n), rhs = Zi.colsview(n, n);
    out.X = Mat(ctx, n, n);
    {
        QRFact f = qr_factor(ctx, M);
        qr_apply_q(ctx, f, rhs, true);                                               // Q' rhs
        gj_invert(ctx, f.R, piv.p, ictl.p);                                          // R^-1
        if (read_back(ctx, ictl.p).singular)
            throw Error(ERR_SINGULAR, std::string(dual ? "dense GARE pair, regulator" : "dense GARE") +
                                          ": [Z12; Z22 + E'] is rank deficient (no stable deflating subspace of dimension n)");
        const Mat top = rhs.view(0, 0, n, n);
        gemm(ctx, false, false, 1.0, f.R, top, 0.0, T, nullptr, "are_extract");      // Y = R^-1 (Q' rhs)(0:n, :)
        Mat YEi = Z.view(0, 0, n, n);
        gemm(ctx, false, false, 1.0, T, Einv, 0.0, YEi, nullptr, "are_extract");     // Y E^-1
        comb(ctx, out.X, 1.0, YEi, 0.0, nullptr, 0.0, nullptr, true, "are_sym", 3);  // X = sym(Y E^-1), YEi with ld 2n; 3 words: YEi is read twice
    }
    Z = Mat(); Zi = Mat(); M = Mat(); rhs = Mat();      // (back to the pool for the refinement)

    // ---- Newton-Kleinman refinement ----
    {
        Residual res(ctx, E, A, G, Q, actl);
        refine(ctx, res, lyap.get(), A, max_refine, false, dual ? "regulator" : "", out);
    }
    if (dual) {          // the filter's equation is the regulator's with G and Q exchanged and the pencil transposed
        Residual res(ctx, E, A, Q, G, actl, true);
        refine(ctx, res, lyap.get(), A, max_refine, true, "filter", *dual);
    }
    ctx->sync();
    return out;
}

}  // namespace

DenseGareResult dense_gare_solve(Ctx* ctx, const Mat& E, const Mat& A, const Mat& B, const Mat* Rinv, const Mat& Ct, const Mat* S, int maxiters,
                                 double tol, int max_refine) {
    return gare_solve(ctx, E, A, B, Rinv, Ct, S, maxiters, tol, max_refine, nullptr);
}

DenseGarePair dense_gare_solve_pair(Ctx* ctx, const Mat& E, const Mat& A, const Mat& B, const Mat* Rinv, const Mat& Ct, const Mat* S, int maxiters,
                                    double tol, int max_refine) {
    DenseGarePair out;
    out.X = gare_solve(ctx, E, A, B, Rinv, Ct, S, maxiters, tol, max_refine, &out.Y);
    return out;
}

}  // namespace dre
