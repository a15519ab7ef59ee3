// Dense path with step-size control: Ros2 with its embedded first-order solution X + tau K1 as the error estimator (dense_adaptive.hip).
// The host model of exactly this driver is tests/_adaptive_ros2_model.py.  See DESIGN.md, "Adaptive Ros2".
#pragma once
#include "dense_sign.hpp"

namespace dre {

enum : int { ERR_STEP = -8 };          // = DRE_ERR_STEP of include/dre_hip.h

// Device-side control words of one trial step (read back once per trial by the host).
struct StepCtl {
    double err;         // sqrt(mean_ij (D_ij / sc_ij)^2), D = Xnew - (X + tau K1), sc = atol + rtol max(|X|, |Xnew|)
    double fac;         // clamp(0.9 err^(-1/2), 0.2, 5); 5 when err == 0, 0.2 when non-finite
    int accept;         // err <= 1 (0 when non-finite)
    int nonfinite;      // a non-finite D / sc was met
};

struct StepControl {
    double rtol = 1e-3, atol = 1e-6, dt_min = 0.0, dt_max = std::numeric_limits<double>::infinity();
    long max_steps = 10000;                 // trial steps, rejected ones included
    std::vector<double> tstops;             // must-hit times strictly between t0 and tf, strictly monotone in the direction of integration
};

struct DenseAdaptiveResult {
    DenseGdreResult r;                      // over the accepted steps (solves: of every trial)
    long accepted = 0, rejected = 0;
    std::vector<double> err;                // per accepted step
};

// Growth of the result while the number of steps is unknown: K(t_i)' in chunks of ADAPT_K_CHUNK steps, the states under save_state in chunks
// of ADAPT_X_CHUNK
constexpr int ADAPT_K_CHUNK = 64, ADAPT_X_CHUNK = 8;

// Ros2 (order must be 2) from t0 to tf with first step dt0 (the sign of tf - t0) and the controller of tests/_adaptive_ros2_model.py.
// Throws Error(ERR_INVALID) on argument errors, Error(ERR_ALLOC) from the up-front check of the fixed part ((maxiters + 28) n^2 doubles) or
// from a failed growth of the result, Error(ERR_STEP) on a rejection at dt_min or more than max_steps trials; ERR_NOT_STABLE and
// ERR_SINGULAR of a factorisation pass through.
DenseAdaptiveResult dense_gdre_solve_adaptive(Ctx* ctx, const Mat& E, const Mat& A, const Mat& B, const Mat& C, const Mat& X0, double t0, double tf,
                                              double dt0, int order, const StepControl& sc, bool save_state, int maxiters, double tol, int max_refine);

}  // namespace dre
