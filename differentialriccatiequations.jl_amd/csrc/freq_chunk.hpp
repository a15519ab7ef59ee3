// Chunking of a frequency sweep (freq_sweep.hpp: the driver of freq_response.hip and transfer_eval.hip) as plain host arithmetic:
// no HIP, no other header of the library, so that a host compiler takes it alone (tests/test_freq_response_host.py compiles it and checks it against brute force).
#pragma once

namespace dre {

// width of the register panel of the batched Gauss-Jordan inversion at order N (the table of gj_batch_nb, dense_batch.hip; freq_response
// checks at run time that the two agree)
inline int fr_panel_nb(long long N) {
    const long long R = (N + 511) / 512;
    return R <= 3 ? 32 : (R <= 5 ? 16 : 8);
}

// doubles of device memory that one member (one frequency of one system) holds while its chunk is in flight, N = 2n:
//   N^2          the real form of i w E - A, inverted in place
//   2 N nb       the panel's work stacks Pn and W
//   2 N m        Y = M^-1[:, 0:n] B and the residual [B; 0] - M Y of its refinement step
//   2 q m        Re H and Im H
//   N / 2 + 1    N interchanges (int)
//   20           the member's control block (BatchCtl, 128 bytes at most) and the four coefficients of its residual
// 0 when an argument is out of range or the count does not fit 63 bits.
inline unsigned long long fr_member_doubles(int n, int m, int q) {
    if (n < 1 || m < 1 || q < 1) return 0;
    typedef unsigned __int128 u128;
    const u128 N = (u128)2 * (u128)n;
    const u128 per = N * N + (u128)2 * N * (u128)fr_panel_nb((long long)2 * n) + (u128)2 * N * (u128)m + (u128)2 * (u128)q * (u128)m + N / 2 + 1 + 20;
    return per >> 63 ? 0ull : (unsigned long long)per;
}

enum : int { FR_PLAN_OK = 0, FR_PLAN_INVALID = 1, FR_PLAN_MEMORY = 2 };
struct FrChunkPlan { int chunk; long long chunks; int err; };

constexpr int FR_MAX_CHUNK = 65535;       // the member sits on a grid axis of every launch

// Members per chunk and number of chunks of a sweep of `members` members when `free_doubles` doubles of device memory are free.
// forced_chunk = 0: the largest chunk that fits, at most FR_MAX_CHUNK and at most `members`.  forced_chunk > 0: that many members per chunk
// (cut to `members`); FR_PLAN_MEMORY when they do not fit.  FR_PLAN_MEMORY also when not even one member fits; FR_PLAN_INVALID for
// n, m, q or members < 1, forced_chunk < 0 or > FR_MAX_CHUNK, or a member whose size does not fit 63 bits.
inline FrChunkPlan fr_chunk_plan_of(unsigned long long free_doubles, unsigned long long per, long long members, int forced_chunk) {
    FrChunkPlan p = {0, 0, FR_PLAN_INVALID};
    if (!per || members < 1 || forced_chunk < 0 || forced_chunk > FR_MAX_CHUNK) return p;
    const unsigned long long fit = free_doubles / per;
    long long chunk;
    if (forced_chunk > 0) {
        chunk = forced_chunk < members ? forced_chunk : members;
        if ((unsigned long long)chunk > fit) { p.err = FR_PLAN_MEMORY; return p; }
    } else {
        if (fit < 1) { p.err = FR_PLAN_MEMORY; return p; }
        chunk = members < FR_MAX_CHUNK ? members : FR_MAX_CHUNK;
        if ((unsigned long long)chunk > fit) chunk = (long long)fit;
    }
    p.chunk = (int)chunk;
    p.chunks = (members - 1) / chunk + 1;
    p.err = FR_PLAN_OK;
    return p;
}
inline FrChunkPlan fr_chunk_plan(unsigned long long free_doubles, int n, int m, int q, long long members, int forced_chunk) {
    return fr_chunk_plan_of(free_doubles, fr_member_doubles(n, m, q), members, forced_chunk);
}

// ---- the complex path (transfer_eval.hip) -------------------------------------------------------------------------
// width of the complex register panel at order n (the table of cgj_batch_nb, dense_cgj.hip; transfer_eval checks at run time that the two
// agree)
inline int fr_panel_nb_c(long long n) {
    const long long R = (n + 511) / 512;
    return R <= 1 ? 32 : (R <= 3 ? 16 : (R <= 5 ? 8 : 4));
}

// doubles of device memory that one member (one point s of one system) holds while its chunk is in flight on the complex path:
//   2 n^2        the planes of s E - A, inverted in place
//   6 n nb       the panel's work stacks Ptilde (n x 2nb) and Wtilde (2nb x 2n)
//   2 n m        the planes of Y = X B
//   4 n m        the residual of its refinement step in the block form [[Rr, Ri], [-Ri, Rr]] (2n x 2m)
//   2 q m        Re H and Im H
//   n / 2 + 1    n interchanges (int)
//   22           the member's control block (BatchCtl, 128 bytes at most) and the six coefficients of its residual
// 0 when an argument is out of range or the count does not fit 63 bits.
inline unsigned long long fr_member_doubles_c(int n, int m, int q) {
    if (n < 1 || m < 1 || q < 1) return 0;
    typedef unsigned __int128 u128;
    const u128 N = (u128)n, M = (u128)m;
    const u128 per = 2 * N * N + (u128)6 * N * (u128)fr_panel_nb_c(n) + 6 * N * M + (u128)2 * (u128)q * M + N / 2 + 1 + 22;
    return per >> 63 ? 0ull : (unsigned long long)per;
}

// fr_chunk_plan with the complex path's member size: the same rules and the same error codes
inline FrChunkPlan fr_chunk_plan_c(unsigned long long free_doubles, int n, int m, int q, long long members, int forced_chunk) {
    return fr_chunk_plan_of(free_doubles, fr_member_doubles_c(n, m, q), members, forced_chunk);
}

}  // namespace dre
