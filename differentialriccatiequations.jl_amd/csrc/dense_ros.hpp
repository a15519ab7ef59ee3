// The stage program of the dense Rosenbrock methods Ros1..Ros4 (dense_ros{1,2,3,4}.jl of the reference), written once for the single, the
// adaptive and the batched driver (dense_sign.hip, dense_adaptive.hip, dense_batch.hip) and for a host back end (tests/test_dense_ros_host.py).
// Nothing of the project and no HIP header is included: the program speaks to its matrices only through a back end Ops with
//   Ops::M                                      the matrix type (a handle; the program never copies one)
//   gemm(tA, tB, alpha, A, B, beta, C)          C = alpha op(A) op(B) + beta C
//   comb(out, a0, M0, a1, M1, a2, M2, sym)      out = sym?(a0 M0 + a1 M1 + a2 M2); M1, M2 are pointers and may be null; out may alias unless sym
//   copy(src, dst)
//   factor(F)                                   the stage pencil (F, E) of the following solves
//   solve(R, X)                                 F'XE + E'XF = -R, R symmetric
// The order of the calls is part of the contract: every driver issues exactly these launches in exactly this order.
#pragma once
#include <cmath>

namespace dre {

// the operands of a run: E, A n x n, B n x m, C'C n x n
template <class M> struct RosOperands { const M &E, &A, &B, &CtC; };

// the work matrices of a step (n x n; XB, V1, V2 n x m).  Ros1 and Ros2 leave K3, K4 and V2 untouched (they may stay empty), Ros1 also K1, V1
template <class M> struct RosWork { M Acl, gF, T, AXE, Racc, Rs, K1, K2, K3, K4, XB, V1, V2; };

// ---- the constants of the four methods ------------------------------------------------------------------------------------------
inline double ros2_gamma() { return 1.0 + 1.0 / std::sqrt(2.0); }
// the weights of K2 and K1 in the Ros2 update X + tau/2 (K2 + (4 - 1/gamma) K1): ros_combine's, and k_step_error's of the adaptive driver
inline double ros2_weight_k2(double tau) { return tau / 2.0; }
inline double ros2_weight_k1(double tau) { return (tau / 2.0) * (4.0 - 1.0 / ros2_gamma()); }
struct Ros3Coef {
    static constexpr double g = 7.886751345948129e-1, a21 = 1.267949192431123;
    static constexpr double c21 = -1.607695154586736, c31 = -3.464101615137755, c32 = -1.732050807568877;
    static constexpr double m1 = 2.0, m2 = 5.773502691896258e-1, m3 = 4.226497308103742e-1;
};

// ---- products every driver needs ------------------------------------------------------------------------------------------------
// V = E'(K B) = (B'KE)'  (K symmetric); with K = X this is the feedback K(t)' = E'XB
template <class Ops> void ros_EtKB(Ops& ops, const RosOperands<typename Ops::M>& p, RosWork<typename Ops::M>& w, const typename Ops::M& K, typename Ops::M& V) {
    ops.gemm(false, false, 1.0, K, p.B, 0.0, w.XB);
    ops.gemm(true, false, 1.0, p.E, w.XB, 0.0, V);
}

// Y = E' S E
template <class Ops> void ros_EtSE(Ops& ops, const RosOperands<typename Ops::M>& p, RosWork<typename Ops::M>& w, const typename Ops::M& S, typename Ops::M& Y) {
    ops.gemm(false, false, 1.0, S, p.E, 0.0, w.T);
    ops.gemm(true, false, 1.0, p.E, w.T, 0.0, Y);
}

// ---- one step from (X, Kt) with step tau: from the closed loop through the last stage solve --------------------------------------
// Ros1 has no combination: its solve writes X.  Ros2..Ros4 leave K1.. in w for ros_combine (or for the caller's own combination).
template <class Ops>
void ros_stages(Ops& ops, int order, double tau, const RosOperands<typename Ops::M>& p, typename Ops::M& X, const typename Ops::M& Kt,
                RosWork<typename Ops::M>& w) {
    using M = typename Ops::M;
    const M* const none = nullptr;
    auto comb = [&](M& out, double a0, const M& M0, double a1 = 0.0, const M* M1 = nullptr, double a2 = 0.0, const M* M2 = nullptr, bool sym = false) {
        ops.comb(out, a0, M0, a1, M1, a2, M2, sym);
    };
    auto sym_rhs = [&] { comb(w.Rs, 1.0, w.Racc, 0.0, none, 0.0, none, true); };             // Rs = sym(Racc)
    // R of the first stage (Ros2..4): C'C + A'XE + E'XA - K'K
    auto first_rhs = [&] {
        ops.gemm(false, false, 1.0, X, p.E, 0.0, w.T);
        ops.gemm(true, false, 1.0, p.A, w.T, 0.0, w.AXE);
        ops.copy(p.CtC, w.Racc);
        ops.gemm(false, true, -1.0, Kt, Kt, 1.0, w.Racc);
        comb(w.Racc, 1.0, w.Racc, 2.0, &w.AXE);                                              // sym(R + 2 A'XE) = C'C + A'XE + E'XA - K'K
        sym_rhs();
    };
    ops.copy(p.A, w.Acl);                                                                    // Acl = A - B K
    ops.gemm(false, true, -1.0, p.B, Kt, 1.0, w.Acl);
    if (order == 1) {
        comb(w.gF, 1.0, w.Acl, -1.0 / (2.0 * tau), &p.E);                                    // F = (A - BK) - E/(2 tau)
        ops.factor(w.gF);
        ops.copy(p.CtC, w.Racc);                                                             // R = C'C + K'K + E'XE / tau
        ops.gemm(false, true, 1.0, Kt, Kt, 1.0, w.Racc);
        ros_EtSE(ops, p, w, X, w.K2);
        comb(w.Rs, 1.0, w.Racc, 1.0 / tau, &w.K2, 0.0, none, true);
        ops.solve(w.Rs, X);
    } else if (order == 2) {
        const double gamma = ros2_gamma();
        comb(w.gF, gamma * tau, w.Acl, -0.5, &p.E);                                          // gF = gamma tau (A - BK) - E/2
        ops.factor(w.gF);
        first_rhs();
        ops.solve(w.Rs, w.K1);
        ros_EtKB(ops, p, w, w.K1, w.V1);                                                     // V1 = E'(K1 B), then E' K1 E
        ros_EtSE(ops, p, w, w.K1, w.Racc);
        comb(w.Racc, -(2.0 - 1.0 / gamma), w.Racc);
        ops.gemm(false, true, -tau * tau, w.V1, w.V1, 1.0, w.Racc);
        sym_rhs();
        ops.solve(w.Rs, w.K2);
    } else if (order == 3) {
        using c = Ros3Coef;
        comb(w.gF, 1.0, w.Acl, -1.0 / (2.0 * c::g * tau), &p.E);                             // gF = (A - BK) - E/(2 gamma tau)
        ops.factor(w.gF);
        first_rhs();
        ops.solve(w.Rs, w.K1);
        ops.gemm(false, false, 1.0, w.K1, p.E, 0.0, w.T);                                    // RX = (A - BK)' K1 E
        ops.gemm(true, false, 1.0, w.Acl, w.T, 0.0, w.AXE);
        ros_EtSE(ops, p, w, w.K1, w.Racc);
        comb(w.Rs, 2.0 * c::a21, w.AXE, c::c21 / tau, &w.Racc, 0.0, none, true);             // sym(a21 (RX + RX') + c21/tau E'K1E)
        ops.solve(w.Rs, w.K2);                                                               // K21
        comb(w.K3, (c::c31 + c::c32) / tau, w.K1, c::c32 / tau, &w.K2);
        ros_EtSE(ops, p, w, w.K3, w.Racc);
        comb(w.Rs, 2.0 * c::a21, w.AXE, 1.0, &w.Racc, 0.0, none, true);
        ops.solve(w.Rs, w.K3);                                                               // K31
    } else {
        comb(w.gF, tau / 2.0, w.Acl, -0.5, &p.E);                                            // gF = (tau (A - BK) - E)/2
        ops.factor(w.gF);
        first_rhs();
        ops.solve(w.Rs, w.K1);
        M& EK1E = w.AXE;                                                                     // (A'XE is dead from here on)
        ros_EtSE(ops, p, w, w.K1, EK1E);                                                     // E' K1 E first, then V1
        ros_EtKB(ops, p, w, w.K1, w.V1);
        comb(w.Racc, -2.0, EK1E);
        ops.gemm(false, true, -tau * tau, w.V1, w.V1, 1.0, w.Racc);
        sym_rhs();
        ops.solve(w.Rs, w.K2);                                                               // K21
        comb(w.K2, 1.0, w.K2, -1.0, &w.K1);                                                  // K2 = K21 - K1
        const double al = (24.0 / 25.0) * tau, be = (3.0 / 25.0) * tau;
        ros_EtSE(ops, p, w, w.K2, w.K4);                                                     // EK2E (in K4 until K4 is formed)
        ros_EtKB(ops, p, w, w.K2, w.V2);
        comb(w.Racc, 245.0 / 25.0, EK1E, 36.0 / 25.0, &w.K4);
        ops.gemm(false, true, -(426.0 / 625.0) * tau * tau, w.V1, w.V1, 1.0, w.Racc);
        ops.gemm(false, true, -be * be, w.V2, w.V2, 1.0, w.Racc);
        ops.gemm(false, true, -2.0 * al * be, w.V2, w.V1, 1.0, w.Racc);                      // -al be (TMP + TMP') under sym
        sym_rhs();
        ops.solve(w.Rs, w.K3);                                                               // K31
        comb(w.K3, 1.0, w.K3, -17.0 / 25.0, &w.K1);                                          // K3 = K31 - 17/25 K1
        comb(w.Racc, -981.0 / 125.0, EK1E, -177.0 / 125.0, &w.K4);
        ros_EtSE(ops, p, w, w.K3, w.Rs);                                                     // (the last E'K3E goes through Rs)
        comb(w.Racc, 1.0, w.Racc, -0.2, &w.Rs);
        sym_rhs();
        ops.solve(w.Rs, w.K4);                                                               // K41
        comb(w.K4, 1.0, w.K4, 1.0, &w.K3);                                                   // K4 = K41 + K3
    }
}

// ---- the update of X from the stages ros_stages left in w --------------------------------------------------------------------------
template <class Ops> void ros_combine(Ops& ops, int order, double tau, typename Ops::M& X, RosWork<typename Ops::M>& w) {
    using M = typename Ops::M;
    const M* const none = nullptr;
    if (order == 2) {
        ops.comb(X, 1.0, X, ros2_weight_k2(tau), &w.K2, ros2_weight_k1(tau), &w.K1, false);  // X + tau/2 (Kt2 + (4 - 1/gamma) K1)
    } else if (order == 3) {
        using c = Ros3Coef;
        ops.comb(X, 1.0, X, c::m1 + c::m2 + c::m3, &w.K1, c::m2, &w.K2, false);
        ops.comb(X, 1.0, X, c::m3, &w.K3, 0.0, none, false);
    } else if (order == 4) {
        ops.comb(X, 1.0, X, tau * 19.0 / 18.0, &w.K1, tau * 0.25, &w.K2, false);
        ops.comb(X, 1.0, X, tau * 25.0 / 216.0, &w.K3, tau * 125.0 / 216.0, &w.K4, false);
    }
}

}  // namespace dre
