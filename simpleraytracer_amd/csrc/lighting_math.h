// Direct lighting of one pixel: the per-light arithmetic of the lit frame (render.hip LightingKernel;
// DESIGN.md section 2 "Lighting"). Host and device share it (cpu_render.cpp HostLighting, the host
// answer rtdLightHost), so both evaluate the same float expressions.
//
// Every operation this header adds follows shadow_math.h's convention: float32 with separate multiply
// and add -- no fma, no contraction (-ffp-contract=off), in the order written, IEEE divide and square
// root -- so that a numpy float32 restatement reproduces the bits. dotp is ShadowDot.
//
// A pixel with image position (fx, fy), hit id `id` and that hit's depth t (shadow_math.h ShadowDepth):
//   d = (base + fx du) + fy dv,  P = eye + t d                       (per component; LightingPoint)
//   N = the triangle's shading-table normal (e1 x e2, unnormalised); nn = dotp(N, N), nd = dotp(N, d)
//   E = ambient
//   for every light, in ascending order:
//     q = P - origin; cls = the light's shadow class of the pixel (shadow_math.h, omni_math.h)
//     nl = dotp(N, q); facing = (nl < 0 and nd < 0) or (nl > 0 and nd > 0)   (NaN fails)
//     if cls == 1 and facing:
//       qq = dotp(q, q); c = |nl| / (sqrt(nn) sqrt(qq)); cosl = c < 1 ? c : 1   (a NaN c gives 1)
//       w = falloff > 0 ? cosl (falloff / qq) : cosl;  E_c = E_c + color_c w
//   rgb_c = albedo_c E_c (not clamped), alpha = float(id)
// q is ShadowOffset's q bit for bit: the same three expressions, P computed once for all lights.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "shadow_math.h"

namespace srt {

constexpr int kLightingMaxLights = 8;   // include/srt_lighting.h RTD_MAX_LIGHTS
constexpr int kLightingMaxFrames = 16;  // include/srt_lighting.h RTD_MAX_FRAMES: 1 per spot, 6 per point light

// d and P of the pixel: ShadowOffset's first two expressions.
__host__ __device__ inline void LightingPoint(const float eye[3], const float base[3], const float du[3],
                                              const float dv[3], float fx, float fy, float t, float d[3], float p[3]) {
    for (int k = 0; k < 3; ++k) {
        d[k] = (base[k] + fx * du[k]) + fy * dv[k];
        p[k] = eye[k] + t * d[k];
    }
}

// The light and the eye lie on the same side of the triangle's plane.
__host__ __device__ inline bool LightingFacing(float nl, float nd) {
    return (nl < 0.f && nd < 0.f) || (nl > 0.f && nd > 0.f);
}

// The weight of a contributing light: its cosine, times falloff / |q|^2 where falloff > 0.
__host__ __device__ inline float LightingWeight(float nl, float nn, float qq, float falloff) {
    const float c = fabsf(nl) / (sqrtf(nn) * sqrtf(qq));
    const float cosl = c < 1.f ? c : 1.f;
    return falloff > 0.f ? cosl * (falloff / qq) : cosl;
}

}  // namespace srt
