// Dense path with step-size control (GDREProblem{<:Matrix}, Ros2(MatrixSign()), adaptive = StepControl(...)):
//   k_step_error, k_step_decide   the new state, the weighted error of the embedded 2(1) pair and the controller's factor, in two launches;
//   dense_gdre_solve_adaptive     the Ros2 stages of dense_ros.hpp (the step of dense_gdre_solve) inside an accept / reject loop on the host.
// One trial costs one sign factorisation of gamma tau (A - BK) - E/2, exactly like a step of the fixed grid: both stages replay it, and the
// estimate D = Xnew - (X + tau K1) needs nothing beyond K1 and K2.  The host model of exactly this driver is tests/_adaptive_ros2_model.py.
#include "dense_adaptive.hpp"

#include <cmath>

#include "dense.hpp"
#include "dense_device.hpp"
#include "dense_ros.hpp"
#include "profiling.hpp"

namespace dre {

// Xnew = X + a2 K2 + a1 K1 (the combination that ends a Ros2 step of dense_gdre_solve: a2 = tau/2, a1 = (tau/2)(4 - 1/gamma)), written to its
// own buffer (X survives a rejection); partial sums of (D / sc)^2 with D = Xnew - (X + tau K1), sc = atol + rtol max(|X|, |Xnew|), and the
// number of non-finite quotients, per workgroup
__global__ __launch_bounds__(256) void k_step_error(int n, const double* __restrict__ X, const double* __restrict__ K1, const double* __restrict__ K2,
                                                    double* __restrict__ Xnew, double a2, double a1, double tau, double rtol, double atol,
                                                    double* __restrict__ part) {
    double s = 0.0, bad = 0.0;
    const size_t tot = (size_t)n * n;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < tot; idx += (size_t)gridDim.x * blockDim.x) {
        const double x = X[idx], k1 = K1[idx];
        const double xn = x + a2 * K2[idx] + a1 * k1;
        const double d = xn - (x + tau * k1);
        const double r = d / (atol + rtol * fmax(fabs(x), fabs(xn)));
        if (isfinite(r)) s += r * r; else bad += 1.0;
        Xnew[idx] = xn;
    }
    store_partials(part, s, bad);
}

// the error measure and the decision of one trial (tests/_adaptive_ros2_model.py: decide)
__global__ __launch_bounds__(256) void k_step_decide(int nparts, const double* __restrict__ part, double count, StepCtl* ctl) {
    double s[2];
    load_partials(nparts, part, s);
    if (threadIdx.x == 0) {
        const double err = sqrt(s[0] / count);
        const bool nonfinite = s[1] > 0.0 || !isfinite(err);
        ctl->err = nonfinite ? INFINITY : err;
        ctl->nonfinite = nonfinite ? 1 : 0;
        ctl->accept = !nonfinite && err <= 1.0 ? 1 : 0;
        ctl->fac = nonfinite ? 0.2 : (err == 0.0 ? 5.0 : fmin(5.0, fmax(0.2, 0.9 / sqrt(err))));
    }
}

static void check_control(double t0, double tf, double dt0, int order, const StepControl& sc) {
    DRE_REQUIRE(order == 2, "adaptive dense path: only Ros2 (order 2) has step-size control; order " + std::to_string(order) +
                                " runs on the fixed grid through dre_dense_gdre_solve");
    DRE_REQUIRE(std::isfinite(t0) && std::isfinite(tf) && tf != t0, "adaptive dense path: t0 and tf must be finite and different");
    DRE_REQUIRE(std::isfinite(dt0) && dt0 != 0.0 && (dt0 > 0.0) == (tf > t0), "adaptive dense path: dt0 must be finite, nonzero and of the sign of tf - t0");
    DRE_REQUIRE(sc.rtol > 0.0 && std::isfinite(sc.rtol), "adaptive dense path: rtol must be positive");
    DRE_REQUIRE(sc.atol > 0.0 && std::isfinite(sc.atol), "adaptive dense path: atol must be positive (with atol = 0 a zero entry of X has no error scale)");
    DRE_REQUIRE(sc.dt_min >= 0.0 && sc.dt_min <= sc.dt_max, "adaptive dense path: 0 <= dt_min <= dt_max expected");   // (false for a NaN too)
    DRE_REQUIRE(sc.max_steps >= 1, "adaptive dense path: max_steps must be >= 1");
    double prev = t0;
    for (size_t i = 0; i < sc.tstops.size(); ++i) {
        const double s = sc.tstops[i];
        DRE_REQUIRE(std::isfinite(s) && (tf > t0 ? (s > prev && s < tf) : (s < prev && s > tf)),
                    "adaptive dense path: tstops must lie strictly between t0 and tf and be strictly monotone in the direction of integration (tstops[" +
                        std::to_string(i) + "])");
        prev = s;
    }
}

DenseAdaptiveResult dense_gdre_solve_adaptive(Ctx* ctx, const Mat& E, const Mat& A, const Mat& B, const Mat& C, const Mat& X0, double t0, double tf,
                                              double dt0, int order, const StepControl& sc, bool save_state, int maxiters, double tol, int max_refine) {
    const int n = E.rows, m = B.cols;
    check_control(t0, tf, dt0, order, sc);
    dense_check_shapes("adaptive dense path", E, A, B, C, X0);
    DenseAdaptiveResult res;
    DenseGdreResult& out = res.r;
    // the fixed part: dense_gdre_solve's count with one state (the sign solver's (maxiters + 10) n^2, 16 n^2 of driver matrices, one state)
    // and Xnew; K(t) and the saved states grow in chunks
    SignLyap lyap(ctx, E, maxiters, tol, max_refine, 16 + 1 + 1);
    DenseRosOps ops{ctx, lyap, out.solves};
    auto sq = [&] { return Mat(ctx, n, n); };
    Mat X = sq(), Xnew = sq(), CtC = sq();
    RosWork<Mat> w{sq(), sq(), sq(), sq(), sq(), sq(), sq(), sq(), Mat(), Mat(), Mat(ctx, n, m), Mat(ctx, n, m), Mat()};    // (Ros2: no K3, K4, V2)
    const RosOperands<Mat> p{E, A, B, CtC};
    DevArr<double> part(ctx, 2 * NORM_PARTS);
    DevArr<StepCtl> ctl(ctx, 1);
    copy_mat(ctx, X0, X);
    ops.gemm(true, false, 1.0, C, C, 0.0, CtC);
    // the result grows by chunks: a failed growth names the step
    Mat Kchunk, Xchunk;
    int kfill = ADAPT_K_CHUNK, xfill = ADAPT_X_CHUNK;
    auto grow = [&](Mat& chunk, int& fill, int cols, int count, const char* what) {
        if (fill < count) return;
        try {
            require_memory(ctx, (size_t)n * cols * count);
            chunk = Mat(ctx, n, cols * count);
        } catch (const Error& e) {
            if (e.code != ERR_ALLOC) throw;
            throw Error(ERR_ALLOC, std::string("adaptive dense path: no device memory for ") + what + " of accepted step " + std::to_string(res.accepted) +
                                       " (" + e.what() + ")");
        }
        fill = 0;
    };
    auto save = [&](const Mat& Xs) {
        grow(Xchunk, xfill, n, save_state ? ADAPT_X_CHUNK : 1, "the state");
        Mat c = Xchunk.colsview(xfill++ * n, n);
        copy_mat(ctx, Xs, c);
        out.X.push_back(c);
    };
    // Kt = (B'XE)' = E'XB
    auto feedback = [&](const Mat& Xs) {
        grow(Kchunk, kfill, m, ADAPT_K_CHUNK, "K(t)");
        Mat Kt = Kchunk.colsview(kfill++ * m, m);
        ros_EtKB(ops, p, w, Xs, Kt);
        return Kt;
    };
    save(X);
    Mat Kt = feedback(X);
    out.Kt.push_back(Kt);
    out.t.push_back(t0);
    const double dirn = tf > t0 ? 1.0 : -1.0;
    auto clamp_h = [&](double h) { return std::min(std::max(h, sc.dt_min), sc.dt_max); };
    std::vector<double> stops = sc.tstops;
    stops.push_back(tf);
    double t = t0, h = clamp_h(std::fabs(dt0));
    size_t next = 0;
    bool after_reject = false;
    long trials = 0;
    while (next < stops.size()) {
        // the must-hit rule: land on the next stop when it is within 1.1 h, halve the distance when it is within 2 h
        const double d = std::fabs(stops[next] - t);
        double tau = h;
        bool hit = false;
        if (d <= 1.1 * h) { tau = d; hit = true; }
        else if (d < 2.0 * h) tau = 0.5 * d;
        if (++trials > sc.max_steps)
            throw Error(ERR_STEP, "adaptive dense path: more than max_steps = " + std::to_string(sc.max_steps) + " trial steps (t = " + std::to_string(t) +
                                      ", " + std::to_string(res.accepted) + " accepted, " + std::to_string(res.rejected) + " rejected)");
        // one Ros2 step of dense_gdre_solve from (X, Kt) with step tau, up to its last combination
        ros_stages(ops, order, tau, p, X, Kt, w);
        {
            TimedScope ts(ctx, "dense_step_error", 32.0 * n * n, 0.0);
            hipLaunchKernelGGL(k_step_error, dim3(NORM_PARTS), dim3(256), 0, ctx->stream, n, (const double*)X.p, (const double*)w.K1.p, (const double*)w.K2.p,
                               Xnew.p, ros2_weight_k2(tau), ros2_weight_k1(tau), tau, sc.rtol, sc.atol, part.p);
            hipLaunchKernelGGL(k_step_decide, dim3(1), dim3(256), 0, ctx->stream, NORM_PARTS, (const double*)part.p, (double)n * n, ctl.p);
        }
        const StepCtl c = read_back(ctx, ctl.p);
        const double fac = after_reject ? std::min(c.fac, 1.0) : c.fac;      // no growth on the trial right after a rejection
        if (c.accept) {
            t = hit ? stops[next] : t + dirn * tau;                          // (a must-hit time is reached as that value itself)
            if (hit) ++next;
            std::swap(X, Xnew);
            ++res.accepted;
            res.err.push_back(c.err);
            out.t.push_back(t);
            if (save_state) save(X);
            Kt = feedback(X);
            out.Kt.push_back(Kt);
            after_reject = false;
        } else {
            if (tau <= sc.dt_min)
                throw Error(ERR_STEP, "adaptive dense path: step rejected at dt_min = " + std::to_string(sc.dt_min) + " (t = " + std::to_string(t) +
                                          ", err = " + std::to_string(c.err) + (c.nonfinite ? ", non-finite values" : "") + ")");
            ++res.rejected;
            after_reject = true;
        }
        h = clamp_h(tau * fac);
    }
    if (!save_state) save(X);
    ctx->sync();
    return res;
}

}  // namespace dre
