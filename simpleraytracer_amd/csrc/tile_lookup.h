// The cull tile whose analytic box contains an image position: the point queries' lookup
// (query.hip QueryKernel; DESIGN.md section 5 "Point queries"). Host and device share it (the
// host self-test rtqTileHost).
//
// Tile column c of a W-wide frame has the analytic box [fl(64 c / W), fl((64 c + 64) / W)] in fx,
// tile row r of an H-high one [fl(16 r / H), fl((16 r + 16) / H)] in fy -- render.hip
// AnalyticTileBound's expressions: float(first) / float(extent), one correctly rounded division.
// Consecutive boxes share their boundary value, the first starts at 0 and the last ends at
// fl(step n / extent) >= 1 (n = ceil(extent / step) tiles), so every position in [0, 1] lies in at
// least one box, partial last tiles included. The float guess floor(f extent / step) can miss by
// one at a boundary (two roundings against the bound's one), so it is corrected by comparing
// against the bounds themselves: the result is a tile whose box contains f, bit for bit.
#pragma once

#include <hip/hip_runtime.h>

namespace srt {

// i in [0, n) with fl(step i / extent) <= f <= fl(step (i + 1) / extent). Needs f in [0, 1],
// n >= 1, step n >= extent (as a float) and step n < 2^24.
__host__ __device__ inline int TileAxisIndex(float f, float extent, int step, int n) {
    int i = static_cast<int>(f * extent / static_cast<float>(step));  // f >= 0: truncation is floor
    i = i < n - 1 ? i : n - 1;
    while (i > 0 && f < static_cast<float>(i * step) / extent) {
        --i;  // f < lo(i) = hi(i - 1)
    }
    while (i < n - 1 && f > static_cast<float>((i + 1) * step) / extent) {
        ++i;  // f > hi(i) = lo(i + 1)
    }
    return i;
}

// The tile (col, row) of position (fx, fy) in a frame of nx x ny tiles of cols x rows pixels;
// false when the position is not in [0, 1]^2 (NaN included): it has no tile.
__host__ __device__ inline bool TileOfPosition(float fx, float fy, float wf, float hf, int cols, int rows, int nx,
                                               int ny, int& col, int& row) {
    if (!(fx >= 0.f && fx <= 1.f && fy >= 0.f && fy <= 1.f)) {
        return false;
    }
    col = TileAxisIndex(fx, wf, cols, nx);
    row = TileAxisIndex(fy, hf, rows, ny);
    return true;
}

}  // namespace srt
