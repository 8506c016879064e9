// The spot-light shadow test of one pixel: the per-pixel arithmetic of the shadow mask (render.hip
// ShadowKernel; DESIGN.md section 2 "Shadow"). Host and device share it (cpu_render.cpp HostShadow,
// the host answer rtlShadowHost), so both evaluate the same float expressions.
//
// Every operation this header adds is float32 with separate multiply and add -- no fma, no
// contraction (-ffp-contract=off), in the order written, IEEE divide -- so that a numpy float32
// restatement reproduces the bits. dotp(a, b) = (a.x b.x + a.y b.y) + a.z b.z.
//
// The light is a second prepared frame (origin, base, du, dv at WL x HL). Its projection rows, from
// those 12 floats in double, each component rounded once to float32:
//   f  = (base + 0.5 du) + 0.5 dv         (the frame's centre direction)
//   px = du / dot(du, du) + 0.5 f,  py = dv / dot(dv, dv) + 0.5 f,  pz = f
// so that a world point X, q = X - origin, lies at the light-frame position (px.q / pz.q, py.q / pz.q)
// and pz.q is its planar depth, the quantity a light-frame t measures.
//
// A pixel with image position (fx, fy) on the view frame, hit id `id` and that hit's depth t
// (ShadowDepth: the G-buffer's depth, the traces' t):
//   d = (base + fx du) + fy dv,  P = eye + t d,  q = P - light origin           (per component)
//   z = dotp(q, pz);  not 0 < z < +inf: class 2 (outside the light's frustum)
//   gx = dotp(q, px) / z,  gy = dotp(q, py) / z;  not both in [0, 1] (NaN fails): class 2
//   (id', t') = the light frame's canonical closest hit at (gx, gy)  (miss: (-1, +inf))
//   thr = z - b z  (bias b >= 0, two roundings);  class 1 (lit) iff id' == id or t' >= thr, else 0.
// An id outside [0, n) is class 3 (no surface); nothing is read through it.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace srt {

constexpr unsigned char kShadowShadowed = 0;
constexpr unsigned char kShadowLit = 1;
constexpr unsigned char kShadowOutside = 2;    // not in the light's frustum
constexpr unsigned char kShadowNoSurface = 3;  // the pixel's id is no triangle of the scene

__host__ __device__ inline float ShadowDot(const float a[3], const float b[3]) {
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

// rows = (px, py, pz) of a light frame. Host only: double, + - x / in this order.
inline void ShadowProjectionRows(const float base[3], const float du[3], const float dv[3], float rows[9]) {
    double f[3], u[3], v[3];
    for (int k = 0; k < 3; ++k) {
        u[k] = du[k];
        v[k] = dv[k];
        f[k] = (static_cast<double>(base[k]) + 0.5 * u[k]) + 0.5 * v[k];
    }
    const double uu = (u[0] * u[0] + u[1] * u[1]) + u[2] * u[2];
    const double vv = (v[0] * v[0] + v[1] * v[1]) + v[2] * v[2];
    for (int k = 0; k < 3; ++k) {
        rows[k] = static_cast<float>(u[k] / uu + 0.5 * f[k]);
        rows[3 + k] = static_cast<float>(v[k] / vv + 0.5 * f[k]);
        rows[6 + k] = static_cast<float>(f[k]);
    }
}

// The depth of triangle record (c, vol: ComputeEdges' values under the view frame) at (fx, fy): the
// traces' t = vol / det, gbuffer_math.h's depth (the same expressions, so the same bits).
__host__ __device__ inline float ShadowDepth(const float c[9], float vol, float fx, float fy) {
    const float eA = fmaf(fy, c[2], fmaf(fx, c[1], c[0]));
    const float eB = fmaf(fy, c[5], fmaf(fx, c[4], c[3]));
    const float eC = fmaf(fy, c[8], fmaf(fx, c[7], c[6]));
    const float det = (eA + eB) + eC;
    return vol / det;
}

// Where the pixel's surface point lies in the light frame. inside == false: class 2, the rest unset.
struct ShadowPoint {
    bool inside;
    float gx, gy;  // light-frame position
    float thr;     // an occluder's t is below this
};

__host__ __device__ inline ShadowPoint ShadowProject(const float eye[3], const float base[3], const float du[3],
                                                     const float dv[3], float fx, float fy, float t,
                                                     const float light_origin[3], const float rows[9], float bias) {
    float q[3];
    for (int k = 0; k < 3; ++k) {
        const float d = (base[k] + fx * du[k]) + fy * dv[k];
        const float p = eye[k] + t * d;
        q[k] = p - light_origin[k];
    }
    ShadowPoint o{false, 0.f, 0.f, 0.f};
    const float z = ShadowDot(q, rows + 6);
    if (!(z > 0.f && z < __builtin_inff())) {
        return o;
    }
    o.gx = ShadowDot(q, rows) / z;
    o.gy = ShadowDot(q, rows + 3) / z;
    if (!(o.gx >= 0.f && o.gx <= 1.f && o.gy >= 0.f && o.gy <= 1.f)) {
        return o;
    }
    o.inside = true;
    o.thr = z - bias * z;
    return o;
}

// ShadowProject in two steps, for a caller that chooses its light frame from q (omni_math.h): the
// same expressions in the same order, so ShadowProjectOffset(ShadowOffset(...)) has ShadowProject's bits.
__host__ __device__ inline void ShadowOffset(const float eye[3], const float base[3], const float du[3],
                                             const float dv[3], float fx, float fy, float t,
                                             const float light_origin[3], float q[3]) {
    for (int k = 0; k < 3; ++k) {
        const float d = (base[k] + fx * du[k]) + fy * dv[k];
        const float p = eye[k] + t * d;
        q[k] = p - light_origin[k];
    }
}

__host__ __device__ inline ShadowPoint ShadowProjectOffset(const float q[3], const float rows[9], float bias) {
    ShadowPoint o{false, 0.f, 0.f, 0.f};
    const float z = ShadowDot(q, rows + 6);
    if (!(z > 0.f && z < __builtin_inff())) {
        return o;
    }
    o.gx = ShadowDot(q, rows) / z;
    o.gy = ShadowDot(q, rows + 3) / z;
    if (!(o.gx >= 0.f && o.gx <= 1.f && o.gy >= 0.f && o.gy <= 1.f)) {
        return o;
    }
    o.inside = true;
    o.thr = z - bias * z;
    return o;
}

// The class of a pixel inside the light's frustum from the light frame's closest hit (id', t').
__host__ __device__ inline unsigned char ShadowClass(int id, int light_id, float light_t, float thr) {
    return light_id == id || light_t >= thr ? kShadowLit : kShadowShadowed;
}

// The RGBA scale of a class: 1 for a lit pixel, `dim` for a shadowed one and one outside the frustum.
__host__ __device__ inline float ShadowScale(unsigned char cls, float dim) { return cls == kShadowLit ? 1.f : dim; }

}  // namespace srt
