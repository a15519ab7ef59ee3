// Bounds check of dre_gemm_probe's operand views (api_probe.hip).  Plain host C++ without any HIP type, so that a stand-alone program can test it on
// a machine without a GPU (tests/test_gemm_tilemap_host.py): this check is what keeps a wrong probe call from reading or writing outside a buffer.
#pragma once
#include <cstdint>

namespace dre {

// True when `count` column-major members of rows x cols with leading dimension ld, member m beginning at element offset + m * stride, lie
// inside a buffer of `cap` elements.  An empty member (rows or cols zero) takes no room, but its offset must still lie inside the buffer.
// Every comparison is arranged so that no intermediate value can overflow an int64_t.
inline bool probe_view_fits(int64_t cap, int64_t offset, int64_t ld, int64_t rows, int64_t cols, int64_t count, int64_t stride) {
    const int64_t lim = INT32_MAX;
    if (cap < 0 || offset < 0 || rows < 0 || cols < 0 || count < 1 || stride < 0) return false;
    if (rows > lim || cols > lim || ld > lim || count > 65535) return false;
    if (ld < (rows > 1 ? rows : 1)) return false;
    if (offset > cap) return false;
    const int64_t room = cap - offset;
    const int64_t extent = (rows == 0 || cols == 0) ? 0 : (cols - 1) * ld + rows;          // < 2^62
    if (extent > room) return false;
    if (count > 1 && stride > (room - extent) / (count - 1)) return false;
    return true;
}

}  // namespace dre
