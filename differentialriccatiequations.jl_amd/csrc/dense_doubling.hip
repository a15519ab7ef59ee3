// Discrete-time dense solvers by doubling (GDALEProblem / GDAREProblem + Doubling); DESIGN.md §9.14, host model tests/_doubling_model.py.
//
// Stein, A'XA - E'XE = -Q (squared Smith):
//   M_0 = E^-1 A, H_0 = sym(Q)                             one gj_invert of E, one product
//   H_{k+1} = H_k + sym(M_k' H_k M_k),  M_{k+1} = M_k^2      three GEMMs, the fused update, the decision: no inversion in the loop
//   X = sym(E^-T H E^-1)
//   dual (A Y A' - E Y E' = -Q): the same loop on the transposed operands through the GEMM's flags, M_0 = A E^-1, H += sym(M H M'),
//   Y = sym(E^-1 H E^-T).
// DARE, Q + A'X(I + GX)^-1 A - E'XE = 0 (SDA of Chu, Fan, Lin and Wang) on A_0 = E^-1 A, G_0 = sym((E^-1 B) Rinv (E^-1 B)'), H_0 = sym(Ct S Ct'):
//   W = I + G_k H_k, inverted with one Newton-Schulz step   one GEMM, the add-identity kernel, gj_invert on a copy; two GEMMs (the sides, below)
//   [T1 T2] = W^-1 [A_k G_k]                                one GEMM on the n x 2n operand that keeps A_k and G_k side by side
//   A_{k+1} = A_k T1
//   G_{k+1} = G_k + sym(A_k T2 A_k')
//   H_{k+1} = H_k + sym(A_k' H_k T1)                        seven GEMMs and the correction's two, the fused update, the decision
//   X = sym(E^-T H_inf E^-1),  Y = G_inf (the filter's solution, no back-transformation)
//   refinement: Newton (Hewer) steps A_c' D A_c - E'DE = -R(X), X <- X + D on the closed loop A_c = (I + GX)^-1 A with the Stein solver above,
//   while the scaled residual exceeds 100 n eps and decreases; the filter's Y by the dual Stein solve on A (I + YQ)^-1.
// The decision rule is doubling_decide.hpp's; the host reads the control word back once per iteration.
//
// The sides of the inversion.  Gauss-Jordan inversion with row pivoting leaves a small LEFT residual V W - I but a RIGHT residual W V - I of the
// order cond(W)^2 eps (measured on W_6 of the n = 70 test system, cond 2.5e6: left 8e-11, right 3.5e-6; an LU-based inverse: 2e-10 and 4e-11).
// The doubling needs both sides: H_{k+1} wants T1 to solve W T1 = A_k with a small residual (W V - I small), and G_{k+1}, which is the H-sequence
// of the transposed problem, wants the same of W' (V W - I small).  With V straight from gj_invert the n = 70 system ended at a scaled
// residual of 7e-12 for X where the NumPy model reaches 2e-13; with the inverse of W' applied transposed X reached 6e-13 and Y fell to 1.6e-12.
// So one Newton-Schulz step V <- V + V (I - W V) follows the inversion (two GEMMs, the add-identity kernel and a copy): its residuals are
// the squares of the old ones on both sides, down to the rounding of I - W V, which is of the order cond(W) eps like an LU-based inverse's.
// The residual's A_c = (I + G X)^-1 A needs the one side only and gets it for free: (I + G X)' = I + X G' is inverted and applied through the
// GEMM's transposition flag.  The filter's A (I + Y Q)^-1 applies the inverse from the right and takes it straight.
//
// Memory, checked before any kernel (n^2 doubles; operands of size n x m, n x q and the partial sums not counted):
//   dense_stein_solve     7: E^-1, M_k, M_{k+1}, H, two products, X
//   dense_stein_residual  4: one product, A'XA, E'XE, the residual
//   dense_dare_solve     17: the doubling holds E^-1, G, Q, [A_k G_k] and its successor (4), H, W, V, [T1 T2] (2), three products and X: 17; it hands its
//                            work back to the pool, and the refinement holds X, G, Q, E^-1, the residual's six (W, A_c, a product, A'X A_c, E'XE, R),
//                            the Stein solver's five, the step and the candidate: 17.  The pair call adds Y: 18.
//   dense_dare_residual   8: G, Q and the residual's six
// Nothing is allocated inside a loop.
#include "dense_doubling.hpp"

#include <cmath>
#include <memory>

#include "dense.hpp"
#include "dense_device.hpp"
#include "profiling.hpp"

namespace dre {

// scaled residual and its Frobenius norm (read back by the host after a residual evaluation)
struct DoublingRes {
    double res;         // ||R||_F / (||Q||_F + ||A'X A_c||_F + ||E'XE||_F)
    double resnorm;     // ||R||_F
};

__global__ void k_dbl_ctl_init(DoublingCtl* c) {
    c->gj.logdet = 0.0; c->gj.singular = 0;
    c->done = 0; c->step = 0.0; c->normA = 0.0;
}

// W += I (n x n, ld n)
__global__ __launch_bounds__(256) void k_dbl_add_identity(int n, double* __restrict__ W) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < (size_t)n) W[i + i * (size_t)n] += 1.0;
}

// The fused update of one doubling iteration, in place: H += sym(dH) and, for the DARE, Gn = G + sym(dG) (G the right half of [A_k G_k], Gn that of
// its successor), with the partial sums of ||dH||^2, ||H_{k+1}||^2, ||A_{k+1}||^2, ||dG||^2, ||G_{k+1}||^2 per workgroup (Stein: the last two are 0).
// The thread of element idx = (i, j) with i <= j owns the unordered pair {i, j}: it forms ONE symmetrised increment and ONE sum and writes both
// entries, so H and G stay symmetric bit for bit; every thread adds its own element of A_{k+1} (An) to the third sum.  All operands n x n, ld n.
template <bool DARE>
__global__ __launch_bounds__(256) void k_dbl_update(int n, double* __restrict__ H, const double* __restrict__ dH, const double* __restrict__ An,
                                                    const double* __restrict__ G, const double* __restrict__ dG, double* __restrict__ Gn,
                                                    const DoublingCtl* ctl, double* __restrict__ part) {
    if (ctl->gj.singular) return;                   // (uniform: k_dbl_decide reports the singular W_k)
    const GridStride g = KERNEL_GRID_STRIDE;
    const size_t N = (size_t)n, tot = N * N;
    double sdh = 0.0, sh = 0.0, sa = 0.0, sdg = 0.0, sg = 0.0;
    for (size_t idx = g.first; idx < tot; idx += g.step) {
        const size_t i = idx % N, j = idx / N;
        const double a = An[idx];
        sa += a * a;
        if (i > j) continue;
        const size_t t = j + i * N;
        const double w = i < j ? 2.0 : 1.0;
        {
            const double d = 0.5 * (dH[idx] + dH[t]);
            const double h = H[idx] + d;
            sdh += w * d * d;
            sh += w * h * h;
            H[idx] = h; H[t] = h;
        }
        if (DARE) {
            const double d = 0.5 * (dG[idx] + dG[t]);
            const double v = G[idx] + d;
            sdg += w * d * d;
            sg += w * v * v;
            Gn[idx] = v; Gn[t] = v;
        }
    }
    store_partials(part, sdh, sh, sa, sdg, sg);
}

// the decision of one doubling iteration: one workgroup adds the partial sums in a fixed order and applies doubling_decide
__global__ __launch_bounds__(256) void k_dbl_decide(int nparts, const double* __restrict__ part, double tol, DoublingCtl* c) {
    double s[5];
    load_partials(nparts, part, s);
    if (threadIdx.x != 0) return;
    if (c->gj.singular) { c->done = DOUBLING_SINGULAR; return; }
    const DoublingDecision d = doubling_decide(s[0], s[1], s[2], s[3], s[4], tol);
    c->done = d.done; c->step = d.step; c->normA = d.normA;
}

// Res = sym(Q) + sym(AXA) - sym(EXE) and the partial sums of ||Res||^2, ||Q||^2, ||AXA||^2, ||EXE||^2 (all n x n, ld n)
__global__ __launch_bounds__(256) void k_dbl_residual(int n, const double* __restrict__ Q, const double* __restrict__ AXA, const double* __restrict__ EXE,
                                                      double* __restrict__ Res, double* __restrict__ part) {
    const GridStride g = KERNEL_GRID_STRIDE;
    const size_t N = (size_t)n, tot = N * N;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (size_t idx = g.first; idx < tot; idx += g.step) {
        const size_t i = idx % N, j = idx / N, t = j + i * N;
        const double v = 0.5 * (Q[idx] + Q[t]) + 0.5 * (AXA[idx] + AXA[t]) - 0.5 * (EXE[idx] + EXE[t]);      // (exactly symmetric)
        Res[idx] = v;
        s0 += v * v; s1 += Q[idx] * Q[idx]; s2 += AXA[idx] * AXA[idx]; s3 += EXE[idx] * EXE[idx];
    }
    store_partials(part, s0, s1, s2, s3);
}

__global__ __launch_bounds__(256) void k_dbl_residual_finish(int nparts, const double* __restrict__ part, DoublingRes* c) {
    double s[4];
    load_partials(nparts, part, s);
    if (threadIdx.x != 0) return;
    const double r = sqrt(s[0]), den = sqrt(s[1]) + sqrt(s[2]) + sqrt(s[3]);
    c->resnorm = r;
    c->res = den > 0.0 ? r / den : r;
}

// ---- host side --------------------------------------------------------------------------------------------------------------------
namespace {

// the "what" of a doubling iteration that ended at iteration k with done > 1 (doubling_decide.hpp), behind the caller's "dense Stein: " /
// "dense DARE: ", in the words of gare_sign_failure
std::string doubling_failure(bool dare, int done, int k, double step, int maxiters) {
    const char* why = dare ? "symplectic pencil has eigenvalues on or near the unit circle / not d-stabilizable"
                           : "E^-1 A has eigenvalues on or outside the unit circle";
    if (done == DOUBLING_SINGULAR) return "singular W_" + std::to_string(k) + " = I + G_k H_k in the doubling iteration";
    if (done == DOUBLING_NON_FINITE) return "the doubling iteration produced non-finite values at iteration " + std::to_string(k) + " (" + why + ")";
    return "the doubling iteration did not converge in " + std::to_string(maxiters) + " iterations (relative step " + std::to_string(step) + "; " + why +
           ")";
}

void check_iteration_args(const char* who, int maxiters) {
    DRE_REQUIRE(maxiters >= 1 && maxiters <= 1000, std::string(who) + ": maxiters must be in 1 .. 1000");
}

void check_pencil(Ctx* ctx, const char* who, const Mat& E, const Mat& A) {
    const int n = E.rows;
    DRE_REQUIRE(n >= 1 && n <= DENSE_MAX_N, std::string(who) + ": E must be square of order 1 .. " + std::to_string(DENSE_MAX_N) +
                                                " (the device's 32-bit index limit)");
    DRE_REQUIRE(E.cols == n && A.rows == n && A.cols == n, std::string(who) + ": E and A must be n x n");
    DRE_REQUIRE(E.ld == n && A.ld == n, std::string(who) + ": E and A must be stored with leading dimension n");
    gj_check_order(ctx, n, who);
}

void check_square(const char* who, const char* name, const Mat& M, int n) {
    DRE_REQUIRE(M.rows == n && M.cols == n && M.ld == n, std::string(who) + ": " + name + " must be n x n with leading dimension n");
}

// the control words, the pivots and the partial sums one call shares among its iterations
struct Ctl {
    DevArr<int> piv;
    DevArr<DoublingCtl> ctl;
    DevArr<DoublingRes> res;
    DevArr<double> part;
    Ctl(Ctx* ctx, int n) : piv(ctx, n), ctl(ctx, 1), res(ctx, 1), part(ctx, 5 * NORM_PARTS) {
        hipLaunchKernelGGL(k_dbl_ctl_init, dim3(1), dim3(1), 0, ctx->stream, ctl.p);
        DRE_HIP(hipMemsetAsync(res.p, 0, sizeof(DoublingRes), ctx->stream));
    }
    GjCtl* gj() { return &ctl.p->gj; }
};

// Einv = E^-1 (who: for the message of a singular E)
void invert_E(Ctx* ctx, const char* who, const Mat& E, Mat& Einv, Ctl& w) {
    copy_mat(ctx, E, Einv);
    gj_invert(ctx, Einv, w.piv.p, w.gj());
    if (read_back(ctx, w.ctl.p).gj.singular)
        throw Error(ERR_SINGULAR, std::string(who) + ": E is singular (zero pivot in the Gauss-Jordan inversion)");
}

// W += I
void add_identity(Ctx* ctx, Mat& W) {
    const int n = W.rows;
    TimedScope ts(ctx, "doubling_add_identity", 16.0 * n, 0.0);
    hipLaunchKernelGGL(k_dbl_add_identity, dim3(ceil_div(n, 256)), dim3(256), 0, ctx->stream, n, W.p);
}

void launch_decide(Ctx* ctx, Ctl& w, double tol) {
    hipLaunchKernelGGL(k_dbl_decide, dim3(1), dim3(256), 0, ctx->stream, NORM_PARTS, (const double*)w.part.p, tol, w.ctl.p);
}

// The Stein solver's work matrices (five n x n) and its loop, shared by dense_stein_solve and the DARE's refinement (which calls it once per
// Newton step on the same E^-1).
struct SteinWork {
    Mat M, Mn, H, T, D;
    SteinWork(Ctx* ctx, int n) : M(ctx, n, n), Mn(ctx, n, n), H(ctx, n, n), T(ctx, n, n), D(ctx, n, n) {}
};

// X = the solution of A'XA - E'XE = -Q (dual: A X A' - E X E' = -Q) given Einv = E^-1; returns the iteration count, *step the last relative step
long stein_run(Ctx* ctx, const char* who, SteinWork& s, Ctl& w, const Mat& Einv, const Mat& A, const Mat& Q, bool dual, int maxiters, double tol,
               Mat& X, double* step) {
    const int n = A.rows;
    const double tol1 = doubling_default_tol(n, tol);
    if (dual) gemm(ctx, false, false, 1.0, A, Einv, 0.0, s.M, nullptr, "stein_setup");     // M = A E^-1
    else gemm(ctx, false, false, 1.0, Einv, A, 0.0, s.M, nullptr, "stein_setup");          // M = E^-1 A
    comb(ctx, s.H, 1.0, Q, 0.0, nullptr, 0.0, nullptr, true, "stein_setup", 3);             // H_0 = sym(Q)
    DoublingCtl h{};
    bool converged = false;
    long iters = 0;
    for (int k = 0; k < maxiters && !converged; ++k) {
        gemm(ctx, !dual, false, 1.0, s.M, s.H, 0.0, s.T, nullptr, "stein_step");           // M' H      (dual: M H)
        gemm(ctx, false, dual, 1.0, s.T, s.M, 0.0, s.D, nullptr, "stein_step");            // M' H M    (dual: M H M')
        gemm(ctx, false, false, 1.0, s.M, s.M, 0.0, s.Mn, nullptr, "stein_step");          // M^2
        {
            TimedScope ts(ctx, "doubling_update", 8.0 * 4 * n * n, 0.0);
            hipLaunchKernelGGL(k_dbl_update<false>, dim3(NORM_PARTS), dim3(256), 0, ctx->stream, n, s.H.p, (const double*)s.D.p, (const double*)s.Mn.p,
                               (const double*)nullptr, (const double*)nullptr, (double*)nullptr, (const DoublingCtl*)w.ctl.p, w.part.p);
            launch_decide(ctx, w, tol1);
        }
        h = read_back(ctx, w.ctl.p);
        iters = k + 1;
        std::swap(s.M, s.Mn);
        if (h.done == DOUBLING_CONVERGED) converged = true;
        else if (h.done) throw Error(ERR_NOT_STABLE, std::string(who) + ": " + doubling_failure(false, h.done, k, h.step, maxiters));
    }
    if (!converged) throw Error(ERR_NOT_STABLE, std::string(who) + ": " + doubling_failure(false, DOUBLING_OUT_OF_ITERS, maxiters, h.step, maxiters));
    gemm(ctx, !dual, false, 1.0, Einv, s.H, 0.0, s.T, nullptr, "stein_finish");            // E^-T H        (dual: E^-1 H)
    gemm(ctx, false, dual, 1.0, s.T, Einv, 0.0, s.D, nullptr, "stein_finish");             // E^-T H E^-1   (dual: E^-1 H E^-T)
    comb(ctx, X, 1.0, s.D, 0.0, nullptr, 0.0, nullptr, true, "stein_finish", 3);
    if (step) *step = h.step;
    return iters;
}

// Res = sym(C0 + AXA - EXE) from the two products and the scaled norm (synchronising)
DoublingRes residual_finish(Ctx* ctx, Ctl& w, const Mat& C0, const Mat& AXA, const Mat& EXE, Mat& Res) {
    const int n = C0.rows;
    {
        TimedScope ts(ctx, "doubling_residual", 8.0 * 7 * n * n, 0.0);
        hipLaunchKernelGGL(k_dbl_residual, dim3(NORM_PARTS), dim3(256), 0, ctx->stream, n, (const double*)C0.p, (const double*)AXA.p, (const double*)EXE.p,
                           Res.p, w.part.p);
        hipLaunchKernelGGL(k_dbl_residual_finish, dim3(1), dim3(256), 0, ctx->stream, NORM_PARTS, (const double*)w.part.p, w.res.p);
    }
    return read_back(ctx, w.res.p);
}

// G = B Rinv B' (Rinv null: B B'), n x n
void form_gram(Ctx* ctx, const Mat& B, const Mat* Rinv, Mat& G) {
    if (B.cols == 0) { fill_mat(ctx, G, 0.0); return; }
    if (Rinv) {
        Mat BR(ctx, B.rows, B.cols);
        gemm(ctx, false, false, 1.0, B, *Rinv, 0.0, BR, nullptr, "dense_dare");
        gemm(ctx, false, true, 1.0, BR, B, 0.0, G, nullptr, "dense_dare");
    } else {
        gemm(ctx, false, true, 1.0, B, B, 0.0, G, nullptr, "dense_dare");
    }
}

void check_dare_operands(Ctx* ctx, const char* who, const Mat& E, const Mat& A, const Mat& B, const Mat* Rinv, const Mat& Ct, const Mat* S) {
    check_pencil(ctx, who, E, A);
    const int n = E.rows;
    DRE_REQUIRE(B.rows == n && Ct.rows == n, std::string(who) + ": B must be n x m, Ct n x q");
    DRE_REQUIRE(!Rinv || (Rinv->rows == B.cols && Rinv->cols == B.cols), std::string(who) + ": Rinv must be m x m");
    DRE_REQUIRE(!S || (S->rows == Ct.cols && S->cols == Ct.cols), std::string(who) + ": S must be q x q");
}

// The regulator's residual R(X) = sym(C0 + A'X(I + Gq X)^-1 A - E'XE) with C0 = Q, Gq = G and, with dual = true and the roles of G and Q
// exchanged by the caller, the filter's R_f(Y) = sym(C0 + A Y (I + Gq Y)^-1 A' - E Y E'), the same chain with its GEMMs' operands in the other
// order.  eval leaves the closed loop in Ac: (I + G X)^-1 A, dual A (I + Y Q)^-1.
struct DareResidual {
    Ctx* c;
    Ctl& w;
    const Mat &E, &A, &Gq, &C0;
    const bool dual;
    Mat W, Ac, T, AXA, EXE, Res;
    DareResidual(Ctx* ctx, Ctl& w_, const Mat& E_, const Mat& A_, const Mat& Gq_, const Mat& C0_, bool dual_)
        : c(ctx), w(w_), E(E_), A(A_), Gq(Gq_), C0(C0_), dual(dual_) {
        const int n = E.rows;
        W = Mat(c, n, n); Ac = Mat(c, n, n); T = Mat(c, n, n); AXA = Mat(c, n, n); EXE = Mat(c, n, n); Res = Mat(c, n, n);
    }
    // Res = R(X); returns the scaled residual and ||R(X)||_F (synchronising); who: for the message of a singular I + G X
    DoublingRes eval(const char* who, const Mat& X) {
        const int n = E.rows;
        if (dual) gemm(c, false, false, 1.0, X, Gq, 0.0, W, nullptr, "dare_residual");      // Y Q
        else gemm(c, false, true, 1.0, X, Gq, 0.0, W, nullptr, "dare_residual");            // X G' = (G X)'
        add_identity(c, W);
        gj_invert(c, W, w.piv.p, w.gj());
        if (dual) {
            gemm(c, false, false, 1.0, A, W, 0.0, Ac, nullptr, "dare_residual");            // A_c = A (I + Y Q)^-1
            gemm(c, false, false, 1.0, Ac, X, 0.0, T, nullptr, "dare_residual");            // A_c Y
            gemm(c, false, true, 1.0, T, A, 0.0, AXA, nullptr, "dare_residual");            // A_c Y A'
            gemm(c, false, true, 1.0, X, E, 0.0, T, nullptr, "dare_residual");              // Y E'
            gemm(c, false, false, 1.0, E, T, 0.0, EXE, nullptr, "dare_residual");           // E Y E'
        } else {
            gemm(c, true, false, 1.0, W, A, 0.0, Ac, nullptr, "dare_residual");             // A_c = (I + G X)^-1 A  (W holds (I + G X)^-T)
            gemm(c, false, false, 1.0, X, Ac, 0.0, T, nullptr, "dare_residual");            // X A_c
            gemm(c, true, false, 1.0, A, T, 0.0, AXA, nullptr, "dare_residual");            // A' X A_c
            gemm(c, false, false, 1.0, X, E, 0.0, T, nullptr, "dare_residual");             // X E
            gemm(c, true, false, 1.0, E, T, 0.0, EXE, nullptr, "dare_residual");            // E' X E
        }
        if (read_back(c, w.ctl.p).gj.singular)
            throw Error(ERR_SINGULAR, std::string(who) + ": " + (dual ? "I + Y Q" : "I + G X") + " is singular");
        return residual_finish(c, w, C0, AXA, EXE, Res);
    }
};

// One solution's refinement: Newton (Hewer) steps on res while the scaled residual exceeds the target and decreases (the rule of refine() in
// dense_are.hip).  who: "dense DARE" in the single call, else with the solution's name.
void refine(Ctx* ctx, const std::string& who, DareResidual& res, SteinWork* stein, Ctl& w, const Mat& Einv, int maxiters, double tol, int max_refine,
            DenseDareResult& out) {
    const int n = Einv.rows;
    out.res0 = out.res = res.eval(who.c_str(), out.X).res;
    const double target = doubling_refine_target(n);
    if (!stein || !(out.res > target)) return;
    Mat D(ctx, n, n), Xn(ctx, n, n);
    const std::string step_who = who + ", refinement (the closed loop is not d-stable: not the stabilizing solution?)";
    while (out.res > target && out.refinements < max_refine) {
        stein_run(ctx, step_who.c_str(), *stein, w, Einv, res.Ac, res.Res, res.dual, maxiters, tol, D, nullptr);      // A_c' D A_c - E'DE = -R(X)
        comb(ctx, Xn, 1.0, out.X, 1.0, &D, 0.0, nullptr, false, "dare_axpby");
        const double rn = res.eval(who.c_str(), Xn).res;
        ++out.refinements;
        if (!(rn < out.res)) break;                                                          // stopped decreasing: keep the better iterate
        std::swap(out.X, Xn);
        out.res = rn;
    }
}

// dense_dare_solve (dual null) and dense_dare_solve_pair (dual: receives the filter solution)
DenseDareResult dare_solve(Ctx* ctx, const Mat& E, const Mat& A, const Mat& B, const Mat* Rinv, const Mat& Ct, const Mat* S, int maxiters, double tol,
                           int max_refine, DenseDareResult* dual) {
    const char* who = dual ? "dense DARE pair" : "dense DARE";
    check_dare_operands(ctx, who, E, A, B, Rinv, Ct, S);
    check_iteration_args(who, maxiters);
    DRE_REQUIRE(max_refine >= 0, std::string(who) + ": max_refine must be >= 0");
    const int n = E.rows;
    const double tol1 = doubling_default_tol(n, tol);
    require_memory(ctx, (size_t)(dual ? 18 : 17) * n * n);      // (the count: the head of this file)

    DenseDareResult out;
    Ctl w(ctx, n);
    Mat Einv(ctx, n, n), G(ctx, n, n), Q(ctx, n, n);
    invert_E(ctx, who, E, Einv, w);
    form_gram(ctx, B, Rinv, G);
    form_gram(ctx, Ct, S, Q);

    // ---- the doubling ----
    {
        Mat AG(ctx, n, 2 * n), AGn(ctx, n, 2 * n), H(ctx, n, n), W(ctx, n, n), V(ctx, n, n), T12(ctx, n, 2 * n), U(ctx, n, n), dH(ctx, n, n), dG(ctx, n, n);
        {
            Mat Ak = AG.colsview(0, n), Gk = AG.colsview(n, n);
            gemm(ctx, false, false, 1.0, Einv, A, 0.0, Ak, nullptr, "dare_setup");            // A_0 = E^-1 A
            gemm(ctx, false, false, 1.0, Einv, G, 0.0, U, nullptr, "dare_setup");
            gemm(ctx, false, true, 1.0, U, Einv, 0.0, dG, nullptr, "dare_setup");             // E^-1 G E^-T = (E^-1 B) Rinv (E^-1 B)'
            comb(ctx, Gk, 1.0, dG, 0.0, nullptr, 0.0, nullptr, true, "dare_setup", 3);        // G_0
            comb(ctx, H, 1.0, Q, 0.0, nullptr, 0.0, nullptr, true, "dare_setup", 3);          // H_0
        }
        DoublingCtl h{};
        bool converged = false;
        for (int k = 0; k < maxiters && !converged; ++k) {
            Mat Ak = AG.colsview(0, n), Gk = AG.colsview(n, n), An = AGn.colsview(0, n), Gn = AGn.colsview(n, n);
            Mat T1 = T12.colsview(0, n), T2 = T12.colsview(n, n);
            gemm(ctx, false, false, 1.0, Gk, H, 0.0, W, nullptr, "dare_step");               // G_k H_k
            add_identity(ctx, W);
            copy_mat(ctx, W, V);
            gj_invert(ctx, V, w.piv.p, w.gj());                                              // V = W^-1, small residual on the left only
            gemm(ctx, false, false, -1.0, W, V, 0.0, U, nullptr, "dare_step");               // (the note on the inversion's sides above)
            add_identity(ctx, U);                                                            // I - W V
            copy_mat(ctx, V, dH);
            gemm(ctx, false, false, 1.0, V, U, 1.0, dH, nullptr, "dare_step");               // V + V (I - W V): small residuals on both sides
            gemm(ctx, false, false, 1.0, dH, AG, 0.0, T12, nullptr, "dare_step");            // [T1 T2] = W^-1 [A_k G_k]
            gemm(ctx, false, false, 1.0, Ak, T1, 0.0, An, nullptr, "dare_step");             // A_{k+1} = A_k T1
            gemm(ctx, false, false, 1.0, Ak, T2, 0.0, U, nullptr, "dare_step");              // A_k T2
            gemm(ctx, false, true, 1.0, U, Ak, 0.0, dG, nullptr, "dare_step");               // A_k T2 A_k'
            gemm(ctx, true, false, 1.0, Ak, H, 0.0, U, nullptr, "dare_step");                // A_k' H_k
            gemm(ctx, false, false, 1.0, U, T1, 0.0, dH, nullptr, "dare_step");              // A_k' H_k T1
            {
                TimedScope ts(ctx, "doubling_update", 8.0 * 8 * n * n, 0.0);
                hipLaunchKernelGGL(k_dbl_update<true>, dim3(NORM_PARTS), dim3(256), 0, ctx->stream, n, H.p, (const double*)dH.p, (const double*)An.p,
                                   (const double*)Gk.p, (const double*)dG.p, Gn.p, (const DoublingCtl*)w.ctl.p, w.part.p);
                launch_decide(ctx, w, tol1);
            }
            h = read_back(ctx, w.ctl.p);
            out.iters = k + 1;
            std::swap(AG, AGn);
            if (h.done == DOUBLING_CONVERGED) converged = true;
            else if (h.done)
                throw Error(h.done == DOUBLING_SINGULAR ? ERR_SINGULAR : ERR_NOT_STABLE, std::string(who) + ": " + doubling_failure(true, h.done, k, h.step, maxiters));
        }
        if (!converged) throw Error(ERR_NOT_STABLE, std::string(who) + ": " + doubling_failure(true, DOUBLING_OUT_OF_ITERS, maxiters, h.step, maxiters));
        out.X = Mat(ctx, n, n);
        gemm(ctx, true, false, 1.0, Einv, H, 0.0, U, nullptr, "dare_finish");                // E^-T H
        gemm(ctx, false, false, 1.0, U, Einv, 0.0, dH, nullptr, "dare_finish");              // E^-T H E^-1
        comb(ctx, out.X, 1.0, dH, 0.0, nullptr, 0.0, nullptr, true, "dare_finish", 3);
        if (dual) {
            dual->iters = out.iters;
            dual->X = Mat(ctx, n, n);
            Mat Ginf = AG.colsview(n, n);
            copy_mat(ctx, Ginf, dual->X);                                                    // Y = G_inf (symmetric bit for bit by the update)
        }
    }       // (the doubling's work goes back to the pool for the refinement)

    // ---- residual and Newton refinement ----
    std::unique_ptr<SteinWork> stein;
    if (max_refine > 0) stein.reset(new SteinWork(ctx, n));
    {
        DareResidual res(ctx, w, E, A, G, Q, false);
        refine(ctx, dual ? "dense DARE pair, regulator" : "dense DARE", res, stein.get(), w, Einv, maxiters, tol, max_refine, out);
    }
    if (dual) {          // the filter's equation is the regulator's with G and Q exchanged and the pencil transposed
        DareResidual res(ctx, w, E, A, Q, G, true);
        refine(ctx, "dense DARE pair, filter", res, stein.get(), w, Einv, maxiters, tol, max_refine, *dual);
    }
    ctx->sync();
    return out;
}

}  // namespace

DenseSteinResult dense_stein_solve(Ctx* ctx, const Mat& E, const Mat& A, const Mat& Q, bool dual, int maxiters, double tol) {
    const char* who = "dense Stein";
    check_pencil(ctx, who, E, A);
    const int n = E.rows;
    check_square(who, "Q", Q, n);
    check_iteration_args(who, maxiters);
    require_memory(ctx, 7 * (size_t)n * n);
    DenseSteinResult out;
    Ctl w(ctx, n);
    Mat Einv(ctx, n, n);
    invert_E(ctx, who, E, Einv, w);
    SteinWork s(ctx, n);
    out.X = Mat(ctx, n, n);
    out.iters = stein_run(ctx, who, s, w, Einv, A, Q, dual, maxiters, tol, out.X, &out.step);
    ctx->sync();
    return out;
}

Mat dense_stein_residual(Ctx* ctx, const Mat& E, const Mat& A, const Mat& Q, const Mat& X, bool dual, double* fro, double* scaled) {
    const char* who = "dense Stein residual";
    check_pencil(ctx, who, E, A);
    const int n = E.rows;
    check_square(who, "Q", Q, n);
    check_square(who, "X", X, n);
    require_memory(ctx, 4 * (size_t)n * n);
    Ctl w(ctx, n);
    Mat T(ctx, n, n), AXA(ctx, n, n), EXE(ctx, n, n), Res(ctx, n, n);
    gemm(ctx, false, dual, 1.0, X, A, 0.0, T, nullptr, "stein_residual");                   // X A      (dual: X A')
    gemm(ctx, !dual, false, 1.0, A, T, 0.0, AXA, nullptr, "stein_residual");                // A' X A   (dual: A X A')
    gemm(ctx, false, dual, 1.0, X, E, 0.0, T, nullptr, "stein_residual");
    gemm(ctx, !dual, false, 1.0, E, T, 0.0, EXE, nullptr, "stein_residual");
    const DoublingRes r = residual_finish(ctx, w, Q, AXA, EXE, Res);
    if (fro) *fro = r.resnorm;
    if (scaled) *scaled = r.res;
    return Res;
}

DenseDareResult dense_dare_solve(Ctx* ctx, const Mat& E, const Mat& A, const Mat& B, const Mat* Rinv, const Mat& Ct, const Mat* S, int maxiters,
                                 double tol, int max_refine) {
    return dare_solve(ctx, E, A, B, Rinv, Ct, S, maxiters, tol, max_refine, nullptr);
}

DenseDarePair dense_dare_solve_pair(Ctx* ctx, const Mat& E, const Mat& A, const Mat& B, const Mat* Rinv, const Mat& Ct, const Mat* S, int maxiters,
                                    double tol, int max_refine) {
    DenseDarePair out;
    out.X = dare_solve(ctx, E, A, B, Rinv, Ct, S, maxiters, tol, max_refine, &out.Y);
    return out;
}

Mat dense_dare_residual(Ctx* ctx, const Mat& E, const Mat& A, const Mat& B, const Mat* Rinv, const Mat& Ct, const Mat* S, const Mat& X, double* fro,
                        double* scaled) {
    const char* who = "dense DARE residual";
    check_dare_operands(ctx, who, E, A, B, Rinv, Ct, S);
    const int n = E.rows;
    check_square(who, "X", X, n);
    require_memory(ctx, 8 * (size_t)n * n);
    Ctl w(ctx, n);
    Mat G(ctx, n, n), Q(ctx, n, n);
    form_gram(ctx, B, Rinv, G);
    form_gram(ctx, Ct, S, Q);
    DareResidual res(ctx, w, E, A, G, Q, false);
    const DoublingRes r = res.eval(who, X);
    if (fro) *fro = r.resnorm;
    if (scaled) *scaled = r.res;
    return res.Res;
}

}  // namespace dre
