// Workgroup -> output tile of the split-K GEMM (gemm.hip, k_gemm) as plain arithmetic, for the device and for the host (the host side is what
// tests/test_gemm_tilemap_host.py compiles and checks on every small grid).
#pragma once

#if defined(__HIPCC__)
#define DRE_TILEMAP_FN __host__ __device__ __forceinline__
#else
#define DRE_TILEMAP_FN inline
#endif

namespace dre {

// Workgroups are dealt round-robin over the 8 XCDs (blocks b and b + 8 share one; observed, a speed matter only), each with its own L2: in
// launch order the tiles that share an operand panel sit on DIFFERENT L2s and every XCD streams the large operand for itself (the 5 row tiles
// of a 304 x 6400 x 20209 sketch product: the 1 GB factor crosses the fabric five times).  swz != 0: every XCD takes a CONTIGUOUS chunk of the
// tile list (bijective remap for any grid size), and the list runs fastest along the dimension with FEWER tiles, so the tiles that are
// resident together on one XCD share the panels of the large operand; splits slowest (they share nothing).  swz == 0: launch order.
// (gx, gy, gz): the grid; (ix, iy, iz): the workgroup's index in it; (bx, by, bz): the tile (row tile, column tile, split) it computes.
DRE_TILEMAP_FN void gemm_tile_map(int swz, unsigned gx, unsigned gy, unsigned gz, unsigned ix, unsigned iy, unsigned iz, int& bx, int& by, int& bz) {
    if (!swz) { bx = (int)ix; by = (int)iy; bz = (int)iz; return; }
    const unsigned per = gx * gy, T = per * gz;
    unsigned L = ix + gx * (iy + gy * iz);
    const unsigned xcd = L & 7u, slot = L >> 3, q = T >> 3, r = T & 7u;
    L = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + slot;
    const unsigned z = L / per, rem = L - z * per;
    bz = (int)z;
    if (gx <= gy) { const unsigned y = rem / gx; by = (int)y; bx = (int)(rem - y * gx); }
    else { const unsigned x = rem / gy; bx = (int)x; by = (int)(rem - x * gy); }
}

}  // namespace dre
