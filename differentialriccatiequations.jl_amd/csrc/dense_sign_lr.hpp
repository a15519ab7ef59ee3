// Factored replay of a kept sign iteration (SignLyap::solve_lr, and solve_lr_t for the dual equation): LDL' right-hand side in, LDL' solution
// out, no shifts.
// See DESIGN.md §9.2.
#pragma once
#include "dense_sign.hpp"

namespace dre {

// Largest accepted width cap: the compression diagonalises a matrix of order <= 2 max_width with the single-workgroup reduction of sym_eig
// (order <= 8192).
#define SIGN_LR_MAX_WIDTH 4096

struct SignLrStats {
    long iters = 0;          // sign iterations replayed (= SignLyap::iters())
    long rank = 0;           // columns of the returned L
    long peak_width = 0;     // widest factor the recursion held (before a compression)
    long compressions = 0;   // rank-revealing compressions (replays, residual factors and the append of a correction)
    long refinements = 0;
    double res0 = 0.0, res = 0.0;   // ||G S G' + F'XE + E'XF||_F / ||G S G'||_F before / after refinement
};

// doubles that solve_lr checks with require_memory before its first kernel: the n x 2 max_width factor buffer, the QR's copy of it and the QR's
// three reflector stores (V, V T, grouped V T), plus the small matrices of order 2 max_width
inline size_t sign_lr_doubles(int n, int max_width) {
    const size_t w2 = 2 * (size_t)max_width;
    return 5 * (size_t)n * w2 + 6 * w2 * w2;
}

// what solve_lr_t checks on top of that: the entry block E^-1 G (n x r) and the residual's F L_Y and E L_Y blocks (n x max_width each; the
// dual has no exit transform, so these are the only products with F, E and E^-1 outside the recursion)
inline size_t sign_lr_t_doubles(int n, int r, int max_width) { return sign_lr_doubles(n, max_width) + (size_t)n * ((size_t)r + 2 * (size_t)max_width); }

}  // namespace dre
