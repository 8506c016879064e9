// Lit ray hits: what an element (ray, id, t) is and how its colour is stored (render.hip
// LightHitsKernel; DESIGN.md section 2 "Hits"). Host and device share it (cpu_render.cpp
// HostLightHits, the host answer rthLightHitsHost), so both evaluate the same float expressions.
//
// shadow_math.h's convention: float32 with separate multiply and add -- no fma, no contraction
// (-ffp-contract=off), in the order written. Everything after the surface point is lighting_math.h's.
//
// An element with the ray (o, d), the id and the t:
//   absent  = dx == 0 and dy == 0 and dz == 0             (-0.0 counts: the comparison is IEEE's)
//   surface = not absent and 0 <= id < n and t finite and the six floats of o, d finite
//   P_k = o_k + t d_k                                     (per component; HitPoint)
//   the colour c and alpha a: lighting_math.h's with this P and d; (background, -1) without a
//   surface; (0, 0, 0, -1) absent
//   stored: (c, a); with a blend (base, weight): absent -> base's four floats unchanged,
//   else (base_c + weight_c c_c, base_a)                  (HitBlend)
#pragma once

#include <hip/hip_runtime.h>

namespace srt {

// (false for NaN and for either infinity)
__host__ __device__ inline bool HitFinite(float x) { return fabsf(x) < __builtin_inff(); }

__host__ __device__ inline bool HitAbsent(const float d[3]) { return d[0] == 0.f && d[1] == 0.f && d[2] == 0.f; }

// Whether the element has a surface: then, and only then, the tables are read through id.
__host__ __device__ inline bool HitSurface(const float o[3], const float d[3], int id, float t, unsigned n) {
    return !HitAbsent(d) && static_cast<unsigned>(id) < n && HitFinite(t) && HitFinite(o[0]) && HitFinite(o[1]) &&
           HitFinite(o[2]) && HitFinite(d[0]) && HitFinite(d[1]) && HitFinite(d[2]);
}

__host__ __device__ inline void HitPoint(const float o[3], const float d[3], float t, float p[3]) {
    for (int k = 0; k < 3; ++k) {
        p[k] = o[k] + t * d[k];
    }
}

// The stored element of a blend: out = (c, a) on entry.
__host__ __device__ inline void HitBlend(bool absent, const float base[4], const float weight[3], float out[4]) {
    for (int k = 0; k < 3; ++k) {
        out[k] = absent ? base[k] : base[k] + weight[k] * out[k];
    }
    out[3] = base[3];
}

}  // namespace srt
