// The surface attributes of one (image position, triangle) pair: the G-buffer's per-pair arithmetic
// (outputs.hip GBufferKernel; DESIGN.md section 2 "Surface attributes"). Host and device share it
// (cpu_render.cpp HostGBuffer, the host answer rtgPointsHost), so both evaluate the same float
// expressions: explicit fma, no contraction, IEEE divide and square root.
//
// Inputs: the triangle's edge record under the prepared frame (c, vol: ComputeEdges' values, the
// bits the traces test with), the ray frame (base, du, dv), the position (fx, fy), the triangle's
// shading table row (N, |N|; albedo) and its id. With E_k = fma(fy, cy_k, fma(fx, cx_k, c0_k)) and
// det = (E_A + E_B) + E_C:
//   depth   t = vol / det           (the traces' t; planar depth, since d . f = 1 for every primary ray)
//   bary    (E_B / det, E_C / det)  (the weights of v1 and v2; w0 = E_A / det is not stored)
//   normal  (s N / |N|, cos)        (s = -1 if N . d > 0 else +1: turned towards the eye; cos is
//                                    the shading cosine, ShadeRecord's expression)
//   albedo  (r, g, b, float(id))
// so albedo.rgb * normal.w and albedo.a are the pixel the traces store. No hit test is run: for a
// pair that does not hit, the values are simply the formulas'.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace srt {

struct GBufferTexel {
    float depth;
    float w1, w2;
    float nx, ny, nz, cosv;
    float r, g, b, a;
};

__host__ __device__ inline float GBufferDot3(float ax, float ay, float az, float bx, float by, float bz) {
    return fmaf(az, bz, fmaf(ay, by, ax * bx));
}

// An id outside the scene (a miss, or any sentinel).
__host__ __device__ inline GBufferTexel GBufferMiss(const float bg[3]) {
    return GBufferTexel{__builtin_inff(), 0.f, 0.f, 0.f, 0.f, 0.f, 1.f, bg[0], bg[1], bg[2], -1.f};
}

// nr = (N, |N|) and al = the albedo: the triangle's shading table row.
__host__ __device__ inline GBufferTexel GBufferHit(const float c[9], float vol, const float base[3], const float du[3],
                                                   const float dv[3], float fx, float fy, int id, float nrx, float nry,
                                                   float nrz, float nrw, float alr, float alg, float alb) {
    GBufferTexel o;
    const float eA = fmaf(fy, c[2], fmaf(fx, c[1], c[0]));
    const float eB = fmaf(fy, c[5], fmaf(fx, c[4], c[3]));
    const float eC = fmaf(fy, c[8], fmaf(fx, c[7], c[6]));
    const float det = (eA + eB) + eC;
    o.depth = vol / det;
    o.w1 = eB / det;
    o.w2 = eC / det;
    const float dx = fmaf(fy, dv[0], fmaf(fx, du[0], base[0]));
    const float dy = fmaf(fy, dv[1], fmaf(fx, du[1], base[1]));
    const float dz = fmaf(fy, dv[2], fmaf(fx, du[2], base[2]));
    const float nd = GBufferDot3(nrx, nry, nrz, dx, dy, dz);
    const float dd = GBufferDot3(dx, dy, dz, dx, dy, dz);
    o.cosv = fminf(fabsf(nd) / (nrw * sqrtf(dd)), 1.f);
    const float ux = nrx / nrw, uy = nry / nrw, uz = nrz / nrw;
    const bool flip = nd > 0.f;
    o.nx = flip ? -ux : ux;
    o.ny = flip ? -uy : uy;
    o.nz = flip ? -uz : uz;
    o.r = alr;
    o.g = alg;
    o.b = alb;
    o.a = static_cast<float>(id);
    return o;
}

}  // namespace srt
