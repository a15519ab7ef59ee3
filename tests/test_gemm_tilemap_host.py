"""Host checks of two small headers of the GEMM family, compiled with g++ into stand-alone programs (no GPU, no HIP):

* csrc/gemm_tilemap.hpp — the workgroup -> tile map of k_gemm, on every grid with gx, gy in 1..9 and gz in 1..5 (tile counts of every residue
  mod 8, counts below 8): identity without the swizzle; with it a bijection of the grid onto itself in which the workgroups of one XCD
  (launch index b = x mod 8) take one contiguous run of the tile list, the runs follow each other in XCD order, and the list runs fastest
  along the dimension with fewer tiles, splits slowest.
* csrc/gemm_probe_check.hpp — the bounds check in front of every launch of dre_gemm_probe, against a brute-force statement of the same
  condition on all small arguments, and on arguments near the integer limits (compiled with -ftrapv: an overflow aborts).
"""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "differentialriccatiequations.jl_amd", "csrc")

TILEMAP_SRC = r"""
#include <cstdio>
#include <vector>
#include "gemm_tilemap.hpp"

// position of tile (bx, by, bz) in the documented tile list: fastest along the dimension with fewer tiles, splits slowest
static unsigned list_pos(unsigned gx, unsigned gy, int bx, int by, int bz) {
    const unsigned in_plane = gx <= gy ? (unsigned)by * gx + (unsigned)bx : (unsigned)bx * gy + (unsigned)by;
    return (unsigned)bz * gx * gy + in_plane;
}

int main() {
    long bad = 0, grids = 0;
    for (unsigned gx = 1; gx <= 9; ++gx)
        for (unsigned gy = 1; gy <= 9; ++gy)
            for (unsigned gz = 1; gz <= 5; ++gz) {
                ++grids;
                const unsigned T = gx * gy * gz;
                std::vector<int> hit(T, 0);
                std::vector<unsigned> pos_of_block(T);
                for (unsigned iz = 0; iz < gz; ++iz)
                    for (unsigned iy = 0; iy < gy; ++iy)
                        for (unsigned ix = 0; ix < gx; ++ix) {
                            int bx = -1, by = -1, bz = -1;
                            dre::gemm_tile_map(0, gx, gy, gz, ix, iy, iz, bx, by, bz);
                            if (bx != (int)ix || by != (int)iy || bz != (int)iz) { ++bad; std::printf("identity broken on %u %u %u\n", gx, gy, gz); }
                            bx = by = bz = -1;
                            dre::gemm_tile_map(1, gx, gy, gz, ix, iy, iz, bx, by, bz);
                            if (bx < 0 || by < 0 || bz < 0 || bx >= (int)gx || by >= (int)gy || bz >= (int)gz) {
                                ++bad; std::printf("tile outside the grid on %u %u %u\n", gx, gy, gz); continue;
                            }
                            hit[(size_t)bx + gx * ((size_t)by + gy * (size_t)bz)] += 1;
                            pos_of_block[ix + gx * (iy + gy * iz)] = list_pos(gx, gy, bx, by, bz);
                        }
                for (unsigned t = 0; t < T; ++t) if (hit[t] != 1) { ++bad; std::printf("not a bijection on %u %u %u\n", gx, gy, gz); break; }
                // XCD x owns blocks x, x + 8, x + 16, ...: their tiles are list positions start, start + 1, ... and the runs of XCD 0, 1, ... 7
                // follow each other without a gap
                unsigned next = 0;
                for (unsigned x = 0; x < 8; ++x)
                    for (unsigned b = x; b < T; b += 8) {
                        if (pos_of_block[b] != next) { ++bad; std::printf("XCD %u does not hold a contiguous run on %u %u %u\n", x, gx, gy, gz); b = T; x = 8; break; }
                        ++next;
                    }
            }
    std::printf("%ld grids, %ld failures\n", grids, bad);
    return bad ? 1 : 0;
}
"""

CHECK_SRC = r"""
#include <cstdint>
#include <cstdio>
#include "gemm_probe_check.hpp"

// the same condition, stated through the largest element index any member touches
static bool brute(int64_t cap, int64_t off, int64_t ld, int64_t rows, int64_t cols, int64_t count, int64_t stride) {
    if (ld < (rows > 1 ? rows : 1)) return false;
    int64_t end = off + (count - 1) * stride;          // first element of the last member
    if (rows > 0 && cols > 0) end += (cols - 1) * ld + rows;
    return end <= cap;
}

int main() {
    long bad = 0, n = 0;
    for (int64_t cap = 0; cap <= 40; ++cap)
        for (int64_t off = 0; off <= 6; ++off)
            for (int64_t ld = 0; ld <= 5; ++ld)
                for (int64_t rows = 0; rows <= 4; ++rows)
                    for (int64_t cols = 0; cols <= 4; ++cols)
                        for (int64_t count = 1; count <= 3; ++count)
                            for (int64_t stride = 0; stride <= 12; ++stride) {
                                ++n;
                                if (dre::probe_view_fits(cap, off, ld, rows, cols, count, stride) != brute(cap, off, ld, rows, cols, count, stride)) {
                                    if (++bad < 10) std::printf("mismatch cap %ld off %ld ld %ld %ld x %ld count %ld stride %ld\n", (long)cap, (long)off, (long)ld, (long)rows, (long)cols, (long)count, (long)stride);
                                }
                            }
    struct { int64_t cap, off, ld, rows, cols, count, stride; bool want; } edge[] = {
        {100, 0, 10, 10, 10, 1, 0, true},                       // the whole buffer
        {100, 1, 10, 10, 10, 1, 0, false},                      // one element too far
        {100, 0, 10, 10, 10, 2, 0, true},                       // overlapping members are not this check's business
        {100, 0, 10, 10, 10, 2, 1, false},
        {100, -1, 10, 1, 1, 1, 0, false},                       // negative anything
        {100, 0, 10, -1, 1, 1, 0, false},
        {100, 0, 10, 1, -1, 1, 0, false},
        {100, 0, 10, 1, 1, 0, 0, false},
        {100, 0, 10, 1, 1, 2, -1, false},
        {-1, 0, 1, 0, 0, 1, 0, false},                          // a missing buffer
        {100, 100, 1, 0, 0, 1, 0, true},                        // an empty view may sit at the very end
        {100, 101, 1, 0, 0, 1, 0, false},
        {100, 0, 9, 10, 1, 1, 0, false},                        // ld below the row count
        {100, 0, 0, 0, 0, 1, 0, false},                         // ld below 1
        {INT64_MAX, INT64_MAX - 1, 1, 1, 1, 1, 0, true},        // near the limits: answered without overflow (-ftrapv)
        {INT64_MAX, INT64_MAX, 1, 1, 1, 1, 0, false},
        {INT64_MAX, 0, INT32_MAX, INT32_MAX, INT32_MAX, 65535, INT64_MAX, false},
        {INT64_MAX, 0, INT32_MAX, INT32_MAX, INT32_MAX, 1, 0, true},
        {INT64_MAX, 0, (int64_t)INT32_MAX + 1, 1, 1, 1, 0, false},
        {INT64_MAX, 0, 1, 1, 1, 65536, 0, false},
        {1000, 0, 1, 1, 1, 65535, INT64_MAX, false},
    };
    for (auto& e : edge) {
        ++n;
        if (dre::probe_view_fits(e.cap, e.off, e.ld, e.rows, e.cols, e.count, e.stride) != e.want) {
            ++bad; std::printf("edge case cap %ld off %ld ld %ld %ld x %ld count %ld stride %ld: expected %d\n", (long)e.cap, (long)e.off, (long)e.ld, (long)e.rows, (long)e.cols, (long)e.count, (long)e.stride, (int)e.want);
        }
    }
    std::printf("%ld cases, %ld failures\n", n, bad);
    return bad ? 1 : 0;
}
"""


def _compile_and_run(tmp_path, name, src, flags=()):
    cpp = tmp_path / (name + ".cpp")
    cpp.write_text(src)
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", CSRC, str(cpp), "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True)


def test_tile_map_is_identity_or_contiguous_bijection_on_every_small_grid(tmp_path):
    r = _compile_and_run(tmp_path, "tilemap", TILEMAP_SRC)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("405 grids, 0 failures"), r.stdout


def test_probe_view_check_matches_brute_force_and_survives_the_integer_limits(tmp_path):
    r = _compile_and_run(tmp_path, "viewcheck", CHECK_SRC, flags=("-ftrapv",))
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 failures"), r.stdout
