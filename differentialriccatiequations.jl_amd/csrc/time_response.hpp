// Time response of dense descriptor systems (time_response.hip):  E x' = A x + B u,  y = C x (+ D u on the host)  on the
// uniform grid t_k = k dt, k = 0 .. K: step response, impulse response, and the output for S given input signals ("scenarios").
//
// Two one-step schemes, both of the form  x_{k+1} = M x_k + N w_k:
//   TR_TUSTIN (order 2, A-stable):          P = E - (dt/2) A,  M = 2 P^-1 E - I,  N = (dt/2) P^-1 B,  w_k = u_k + u_{k+1}
//   TR_BACKWARD_EULER (order 1, L-stable):  P = E - dt A,      M = P^-1 E,        N = dt P^-1 B,      w_k = u_{k+1}
// With  G_j = C M^j  (q x n) and  h_j = G_j N  (q x m):   y_k = G_k x_0 + sum_{j < k} h_j w_{k-1-j}.
//   step (unit step on channel c, x_0 = 0):   y_k[:, c] = beta sum_{j < k} h_j[:, c],  beta = 2 (tustin) or 1 (backward Euler)
//   impulse:  the free response from x(0+) = E^-1 B:  y_k = G_k E^-1 B  (needs a regular E)
//   simulate: the full formula for S scenarios at once.
//
// Method: the outputs need only the Markov sequence G_j, and no state.  The straightforward recurrence is one thin n x n product per time
// step, K dependent launches that are bound by latency (n = 371) or by reading M from HBM (n = 4096).  Here the stack
// O = [G_0; G_1; ...; G_K] ((K+1) q x n) is built from full-size GEMMs instead:
//   1. k_tr_pencil writes P = E - theta A; gj_invert inverts it in place (the panel gj_invert picks for n);
//   2. M and N from gemm() (the -I of tustin through beta = -1 on C = I);
//   3. doubling:  O_{2J} = [O_J; O_J M^J],  M^{2J} = (M^J)^2,  until J = L, the block length (a power of two);
//   4. block marching:  block_{b+1} = block_b M^L, an (L q x n)(n x n) GEMM each, until (K+1) q rows exist;
//   5. h = O N (one thin GEMM; impulse: O (E^-1 B) after a second gj_invert, of E; simulate with x_0: also O X_0);
//   6. k_tr_scan_* (step: exclusive prefix sum over j, three phases), k_tr_layout (impulse), k_tr_conv (simulate: causal convolution).
// That is log2 L + ceil((K+1)/L) + O(1) GEMMs in place of K.  L = 1 is the plain sequential recurrence on the same code.
// The price is accuracy where M is far from normal: M^J is formed explicitly, so an error of eps |M^J| enters rows J .. 2J - 1, where
// the sequential recurrence has eps |G_j| |M| per step.  For a power-bounded M (a stable pencil under either scheme) both stay at
// O(j eps); the measured distances are in DESIGN.md §9.13.
//
// The pencil need not be stable: a growing response is a valid result.  E may be singular for step and simulate.  Under tustin the
// algebraic part of a singular E has the eigenvalue -1 in M (it neither decays nor grows: an inconsistent start rings for ever), under
// backward Euler it has the eigenvalue 0: backward Euler is the method for singular E.
// Every kernel is an ordinary launch, nothing is accumulated with atomics, and every summation order follows from the shapes alone: a call
// is bit for bit repeatable.  Memory: the stack of ceil((K+1)/L) L q n doubles, 4 n^2 and thin operands, checked before any launch
// (require_memory); there is no chunking over time.
#pragma once
#include <vector>

#include "common.hpp"

namespace dre {

enum : int { TR_TUSTIN = 0, TR_BACKWARD_EULER = 1 };
enum : int { TR_STEP = 0, TR_IMPULSE = 1, TR_SIMULATE = 2 };

// limits of k_tr_conv (its LDS staging): outputs and outputs x inputs of a simulate call
#define TR_CONV_MAX_Q 256
#define TR_CONV_MAX_QM 2048

struct TimeResponse {
    std::vector<double> Y;   // step, impulse: sample k at k q m, q x m column-major;  simulate: scenario s at s (K+1) q, sample k at k q
    int block = 0;           // L in force
    int blocks = 0;          // ceil((K+1) / L)
    int squarings = 0;       // products M^J M^J
    long launches = 0;       // kernels, GEMM calls and inversions enqueued (a GEMM and an inversion count as one each)
};

// default block length: the smallest power of two L at which the marching GEMM's ceil(L q / 64) ceil(n / 64) output tiles fill the 256
// compute units once (a fixed number, not the device's: the bits of a result depend on L), at most the power of two >= K + 1, halved while
// the stack rounded up to whole blocks would hold over 5/4 (K + 1) sample rows.  Measured against L q >= 256 in DESIGN.md §9.13.
#define TR_FILL_TILES 256
int tr_default_block(int q, int K, int n);

// U (host, kind TR_SIMULATE only): (K+1) m x S column-major, u_k of scenario s at s (K+1) m + k m.  X0 (host, TR_SIMULATE only, may be
// null): n x S column-major.  block: 0 = tr_default_block, else a power of two (one beyond the power of two >= K + 1 is cut to it).
// ERR_INVALID before any launch: K < 1, dt not finite or <= 0, unknown method or kind, mismatched shapes, U null or S < 1 under
// TR_SIMULATE, block not a power of two, a stack whose element count does not fit an int index ((K+1 rounded up to L) q n >= 2^31),
// q > TR_CONV_MAX_Q or q m > TR_CONV_MAX_QM under TR_SIMULATE.  ERR_ALLOC before any launch.  ERR_SINGULAR: singular P (or a
// NaN in E or A), or singular E under TR_IMPULSE.
TimeResponse time_response(Ctx* ctx, const Mat& E, const Mat& A, const Mat& B, const Mat& C, int method, double dt, int K, int kind,
                           const double* U, int S, const double* X0, int block);

}  // namespace dre
