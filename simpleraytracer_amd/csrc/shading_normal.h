// Row 0 of the shading table, shared by the render kernels (render.hip), the motion kernels
// (spatial.hip) and their host twin (rtmOrderHost): one definition, so a table row rewritten after a
// move has the bits of a fresh table's.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace srt {

// Shading normal of the triangle with vertex coordinates v[0..9): the exact expressions the
// shading epilogue used to evaluate per hit. (x, y, z) = cross(v1 - v0, v2 - v0), separate multiplies
// and subtracts (-ffp-contract=off); w = its length, the dot product in explicit fmaf.
__host__ __device__ __forceinline__ float4 ShadingNormal(const float* __restrict__ v) {
    const float e1x = v[3] - v[0], e1y = v[4] - v[1], e1z = v[5] - v[2];
    const float e2x = v[6] - v[0], e2y = v[7] - v[1], e2z = v[8] - v[2];
    const float nx = e1y * e2z - e1z * e2y;
    const float ny = e1z * e2x - e1x * e2z;
    const float nz = e1x * e2y - e1y * e2x;
    return make_float4(nx, ny, nz, sqrtf(fmaf(nz, nz, fmaf(ny, ny, nx * nx))));
}

}  // namespace srt
