// Sampled visibility of one element: the arithmetic of the rta family (include/srt_visibility.h;
// DESIGN.md section 2 "Visibility"). The kernels (visibility.hip) and the host answers
// (rtaRaysHost, rtaVisibilityHost) share it, so both evaluate the same float expressions.
//
// Every operation this header adds follows shadow_math.h's convention: float32 with separate multiply
// and add -- no fma, no contraction (-ffp-contract=off) --, in the order written, IEEE divide and
// square root, so that a numpy float32 restatement reproduces the bits. dotp is ShadowDot. The depth
// alone is the traces' (VisibilityDepth: the edge record's explicit fmaf, as the G-buffer's).
//
// An element (fx, fy, id) with id in [0, n):
//   t = ShadowDepth of the triangle's record at (fx, fy); d, P = LightingPoint
//   N = the shading-table normal (shading_normal.h); nn = dotp(N, N), nd = dotp(N, d)
//   valid iff RayFinite(t) and RayFinite(nn) and nn > 0; else every ray is eight zeros
//   r = sqrt(nn), n_k = N_k / r; nd > 0: n = -n
//   hemisphere: sg = n.z < 0 ? -1 : 1, a = -1 / (sg + n.z), b = (n.x n.y) a      (|sg + n.z| >= 1)
//     T = (1 + ((sg n.x) n.x) a, sg b, (-sg) n.x), B = (b, sg + (n.y n.y) a, -n.y)
//     lx' = lx c - ly s, ly' = lx s + ly c  (no rotation: lx' = lx, ly' = ly)
//     dir_k = (lx' T_k + ly' B_k) + lz n_k
//   area: L_k = (corner_k + a eu_k) + b ev_k, dir_k = L_k - P_k
//   mirror: dn = dotp(d, n), dir_k = d_k - (2 dn) n_k
//   the ray is (P, tmin, dir, tmax)
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "lighting_math.h"
#include "ray_math.h"
#include "shading_normal.h"

namespace srt {

constexpr int kVisibilityHemisphere = 0;  // include/srt_visibility.h RTA_HEMISPHERE
constexpr int kVisibilityArea = 1;        // RTA_AREA
constexpr int kVisibilityMirror = 2;      // RTA_MIRROR
constexpr unsigned kVisibilityMaxSamples = 64;
constexpr unsigned kVisibilityRotations = 16;

__host__ __device__ inline float VisibilityDot3(float ax, float ay, float az, float bx, float by, float bz) {
    return fmaf(az, bz, fmaf(ay, by, ax * bx));
}

// ShadowDepth of the triangle with vertex coordinates v[0..9) at (fx, fy) under the frame (origin,
// base, du, dv): the edge record's expressions (trace_device.h ComputeEdges, cpu_render.cpp MakeRecord),
// so the traces' t. NaN for a disabled record (vol zero or not finite).
__host__ __device__ inline float VisibilityDepth(const float origin[3], const float base[3], const float du[3],
                                                 const float dv[3], const float v[9], float fx, float fy) {
    const float ax = v[0] - origin[0], ay = v[1] - origin[1], az = v[2] - origin[2];
    const float bx = v[3] - origin[0], by = v[4] - origin[1], bz = v[5] - origin[2];
    const float cx = v[6] - origin[0], cy = v[7] - origin[1], cz = v[8] - origin[2];
    float n[9];
    n[0] = by * cz - bz * cy, n[1] = bz * cx - bx * cz, n[2] = bx * cy - by * cx;
    n[3] = cy * az - cz * ay, n[4] = cz * ax - cx * az, n[5] = cx * ay - cy * ax;
    n[6] = ay * bz - az * by, n[7] = az * bx - ax * bz, n[8] = ax * by - ay * bx;
    float vol = VisibilityDot3(ax, ay, az, n[0], n[1], n[2]);
    if (!(RayFinite(vol) && vol != 0.f)) {
        return __builtin_nanf("");
    }
    if (vol < 0.f) {
        for (int k = 0; k < 9; ++k) {
            n[k] = -n[k];
        }
        vol = -vol;
    }
    float c[9];
    for (int e = 0; e < 3; ++e) {
        const float nx = n[3 * e], ny = n[3 * e + 1], nz = n[3 * e + 2];
        c[3 * e + 0] = VisibilityDot3(nx, ny, nz, base[0], base[1], base[2]);
        c[3 * e + 1] = VisibilityDot3(nx, ny, nz, du[0], du[1], du[2]);
        c[3 * e + 2] = VisibilityDot3(nx, ny, nz, dv[0], dv[1], dv[2]);
    }
    return ShadowDepth(c, vol, fx, fy);
}

// Steps 2 to 4: the surface point, the direction and the unit normal towards the eye.
struct VisibilitySurface {
    bool valid;
    float p[3], d[3], n[3];
};

__host__ __device__ inline VisibilitySurface VisibilitySurfaceAt(const float origin[3], const float base[3],
                                                                 const float du[3], const float dv[3],
                                                                 const float v[9], float fx, float fy) {
    VisibilitySurface s;
    const float t = VisibilityDepth(origin, base, du, dv, v, fx, fy);
    LightingPoint(origin, base, du, dv, fx, fy, t, s.d, s.p);
    const float4 nr = ShadingNormal(v);
    const float N[3] = {nr.x, nr.y, nr.z};
    const float nn = ShadowDot(N, N), nd = ShadowDot(N, s.d);
    s.valid = RayFinite(t) && RayFinite(nn) && nn > 0.f;
    const float r = sqrtf(nn);
    for (int k = 0; k < 3; ++k) {
        const float u = N[k] / r;
        s.n[k] = nd > 0.f ? -u : u;
    }
    return s;
}

// The hemisphere's basis around the unit normal n.
__host__ __device__ inline void VisibilityBasis(const float n[3], float T[3], float B[3]) {
    const float sg = n[2] < 0.f ? -1.f : 1.f;
    const float a = -1.f / (sg + n[2]);
    const float b = (n[0] * n[1]) * a;
    T[0] = 1.f + ((sg * n[0]) * n[0]) * a;
    T[1] = sg * b;
    T[2] = (-sg) * n[0];
    B[0] = b;
    B[1] = sg + (n[1] * n[1]) * a;
    B[2] = -n[1];
}

// (c, s) = the element's rotation; rotate == false: none.
__host__ __device__ inline void VisibilityHemisphereDir(const float n[3], const float T[3], const float B[3], float lx,
                                                        float ly, float lz, bool rotate, float c, float s,
                                                        float dir[3]) {
    const float rx = rotate ? lx * c - ly * s : lx;
    const float ry = rotate ? lx * s + ly * c : ly;
    for (int k = 0; k < 3; ++k) {
        dir[k] = (rx * T[k] + ry * B[k]) + lz * n[k];
    }
}

__host__ __device__ inline void VisibilityAreaDir(const float corner[3], const float eu[3], const float ev[3], float a,
                                                  float b, const float p[3], float dir[3]) {
    for (int k = 0; k < 3; ++k) {
        const float l = (corner[k] + a * eu[k]) + b * ev[k];
        dir[k] = l - p[k];
    }
}

__host__ __device__ inline void VisibilityMirrorDir(const float d[3], const float n[3], float dir[3]) {
    const float dn = ShadowDot(d, n);
    for (int k = 0; k < 3; ++k) {
        dir[k] = d[k] - (2.f * dn) * n[k];
    }
}

}  // namespace srt
