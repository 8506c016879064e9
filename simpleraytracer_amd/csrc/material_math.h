// Lit surfaces: the per-light arithmetic of a pixel whose surface comes from the vertex-attribute
// tables (render.hip LitSurfaceKernel; DESIGN.md section 2 "Lit surfaces"). Host and device share it
// (cpu_render.cpp HostLitSurface, the host answer rtpLightSurfaceHost), so both evaluate the same
// float expressions.
//
// Every operation this header adds follows shadow_math.h's convention: float32 with separate multiply
// and add -- no fma, no contraction (-ffp-contract=off), in the order written, IEEE divide and square
// root -- so that a numpy float32 restatement reproduces the bits. dotp is ShadowDot.
//
// The pixel's d, P, N, nn, nd and, per light, q, cls, nl and facing are "Lighting"'s (lighting_math.h):
// which lights contribute is a matter of geometry alone. u is the unit normal of the pixel's normal
// plane ("Vertex attributes"), A its albedo plane. For a contributing light (cls == 1 and facing):
//   qq = dotp(q, q)
//   diffuse   without a normals table: w = LightingWeight(nl, nn, qq, falloff)
//             with one: c = (0 - dotp(u, q)) / sqrt(qq); cosl = c > 0 ? (c < 1 ? c : 1) : 0  (NaN: 0)
//                       w = falloff > 0 ? cosl (falloff / qq) : cosl
//             E_c = E_c + color_c w
//   specular  (with a material, and only where w > 0) dd = dotp(d, d);
//             g_k = q_k / sqrt(qq) + d_k / sqrt(dd)          (the negated half vector)
//             s = (0 - dotp(u, g)) / sqrt(dotp(g, g)), clamped as cosl; then shininess_log2 times s = s s
//             ws = falloff > 0 ? s (falloff / qq) : s;  S_c = S_c + color_c ws
//   rgb_c = A_c E_c (+ specular_c S_c with a material), alpha = float(id)
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

#include "shadow_math.h"

namespace srt {

constexpr int kMaterialMaxShininessLog2 = 12;  // include/srt_material.h RTP_MAX_SHININESS_LOG2

// Into [0, 1]; NaN becomes 0.
__host__ __device__ inline float MaterialClamp(float c) { return c > 0.f ? (c < 1.f ? c : 1.f) : 0.f; }

__host__ __device__ inline float MaterialFalloff(float c, float qq, float falloff) {
    return falloff > 0.f ? c * (falloff / qq) : c;
}

// The diffuse weight of a contributing light under the unit normal u of a normals table.
__host__ __device__ inline float MaterialDiffuse(const float u[3], const float q[3], float qq, float falloff) {
    const float c = (0.f - ShadowDot(u, q)) / sqrtf(qq);
    return MaterialFalloff(MaterialClamp(c), qq, falloff);
}

// The Blinn-Phong weight of a contributing light: exponent 2^k by k exact squarings.
__host__ __device__ inline float MaterialSpecular(const float u[3], const float q[3], float qq, const float d[3], int k,
                                                  float falloff) {
    const float lq = sqrtf(qq), ld = sqrtf(ShadowDot(d, d));
    float g[3];
    for (int j = 0; j < 3; ++j) {
        g[j] = q[j] / lq + d[j] / ld;
    }
    float s = MaterialClamp((0.f - ShadowDot(u, g)) / sqrtf(ShadowDot(g, g)));
    for (int j = 0; j < k; ++j) {
        s = s * s;
    }
    return MaterialFalloff(s, qq, falloff);
}

}  // namespace srt
