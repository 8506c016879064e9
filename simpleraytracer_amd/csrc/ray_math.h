// The test of one caller-supplied ray against one triangle (DESIGN.md section 2 "Rays"): the
// arithmetic of the rtr family (include/srt_rays.h). The kernels (rays.hip) and the host answer
// (rtrClosestHost, rtrOccludedHost) share it, so both evaluate the same float expressions.
//
// Shadow's convention (shadow_math.h): float32, separate multiply and add -- no fma, no contraction
// (-ffp-contract=off) -- in the order written, IEEE divide, so that a numpy float32 restatement
// reproduces the bits. dotp(a, b) = (a.x b.x + a.y b.y) + a.z b.z;
// cross(a, b) = (a.y b.z - a.z b.y, a.z b.x - a.x b.z, a.x b.y - a.y b.x).
//
// A ray is 8 floats (ox, oy, oz, tmin, dx, dy, dz, tmax); d is not normalised, t is in units of d.
//
// Edge test:  A = v0 - o, B = v1 - o, C = v2 - o;  nA = cross(B, C), nB = cross(C, A), nC = cross(A, B);
//   vol = dotp(A, nA); vol 0 or not finite: no hit;  s = vol < 0 ? -1 : +1;  E_k = s dotp(n_k, d);
//   det = (E_A + E_B) + E_C;  pass iff E_A >= 0 and E_B >= 0 and E_C >= 0 and det > 0;
//   t = |vol| / det, w1 = E_B / det, w2 = E_C / det;  the hit counts iff tmin <= t <= tmax.
// Box clause (part of the definition: it is what lets a hierarchy be exact):
//   lo_k, hi_k = min / max of the three vertices;  m = max_k max(|lo_k|, |hi_k|);  m not finite: the
//   triangle is never hit;  pad = m 2^-12;  plo_k = lo_k - pad, phi_k = hi_k + pad;
//   inv_k = 1 / d_k;  a = (plo_k - o_k) inv_k, b = (phi_k - o_k) inv_k;  a or b NaN: near_k = -inf,
//   far_k = +inf, else near_k = min(a, b), far_k = max(a, b);  tn = max_k near_k, tf = min_k far_k;
//   pass iff tn <= tf and tn <= tmax and tf >= tmin.
// A box with plo_x > phi_x is empty (RayBoxClause fails on it): the mark of a never-hit triangle
// and of a node with none below it.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace srt {

constexpr float kRayPadScale = 1.f / 4096.f;  // 2^-12

struct Ray {
    float o[3];
    float tmin;
    float d[3];
    float tmax;
};

__host__ __device__ inline bool RayFinite(float x) { return x - x == 0.f; }  // false for NaN and +-inf

// A ray that can hit nothing: a non-finite origin or direction component, d = 0, a NaN range, tmin > tmax.
__host__ __device__ inline bool RayDegenerate(const Ray& r) {
    for (int k = 0; k < 3; ++k) {
        if (!RayFinite(r.o[k]) || !RayFinite(r.d[k])) {
            return true;
        }
    }
    if (r.d[0] == 0.f && r.d[1] == 0.f && r.d[2] == 0.f) {
        return true;
    }
    return !(r.tmin <= r.tmax);  // (false when either is NaN)
}

__host__ __device__ inline void RayInverse(const Ray& r, float inv[3]) {
    for (int k = 0; k < 3; ++k) {
        inv[k] = 1.f / r.d[k];
    }
}

// The padded box of a triangle; false (and the empty box) when a vertex is not finite.
__host__ __device__ inline bool RayTriangleBox(const float v[9], float plo[3], float phi[3]) {
    float m = 0.f;
    float lo[3], hi[3];
    for (int k = 0; k < 3; ++k) {
        lo[k] = fminf(fminf(v[k], v[3 + k]), v[6 + k]);
        hi[k] = fmaxf(fmaxf(v[k], v[3 + k]), v[6 + k]);
    }
    bool finite = true;
    for (int k = 0; k < 9; ++k) {
        finite = finite && RayFinite(v[k]);
    }
    for (int k = 0; k < 3; ++k) {
        m = fmaxf(m, fmaxf(fabsf(lo[k]), fabsf(hi[k])));
    }
    if (!finite) {
        for (int k = 0; k < 3; ++k) {
            plo[k] = __builtin_inff();
            phi[k] = -__builtin_inff();
        }
        return false;
    }
    const float pad = m * kRayPadScale;
    for (int k = 0; k < 3; ++k) {
        plo[k] = lo[k] - pad;
        phi[k] = hi[k] + pad;
    }
    return true;
}

// The box clause against any box (a triangle's padded box, a node's union of them).
__host__ __device__ inline bool RayBoxClause(const Ray& r, const float inv[3], const float plo[3], const float phi[3]) {
    if (!(plo[0] <= phi[0])) {
        return false;
    }
    float tn = -__builtin_inff(), tf = __builtin_inff();
    for (int k = 0; k < 3; ++k) {
        const float a = (plo[k] - r.o[k]) * inv[k];
        const float b = (phi[k] - r.o[k]) * inv[k];
        if (a != a || b != b) {
            continue;
        }
        const float near = a < b ? a : b;
        const float far = a < b ? b : a;
        tn = near > tn ? near : tn;
        tf = far < tf ? far : tf;
    }
    return tn <= tf && tn <= r.tmax && tf >= r.tmin;
}

struct RayHit {
    bool hit;
    float t, w1, w2;
};

// The edge test and the range (no box clause).
__host__ __device__ inline RayHit RayEdgeTest(const Ray& r, const float v[9]) {
    RayHit h{false, 0.f, 0.f, 0.f};
    float a[3], b[3], c[3];
    for (int k = 0; k < 3; ++k) {
        a[k] = v[k] - r.o[k];
        b[k] = v[3 + k] - r.o[k];
        c[k] = v[6 + k] - r.o[k];
    }
    const float na[3] = {b[1] * c[2] - b[2] * c[1], b[2] * c[0] - b[0] * c[2], b[0] * c[1] - b[1] * c[0]};
    const float nb[3] = {c[1] * a[2] - c[2] * a[1], c[2] * a[0] - c[0] * a[2], c[0] * a[1] - c[1] * a[0]};
    const float nc[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    const float vol = (a[0] * na[0] + a[1] * na[1]) + a[2] * na[2];
    if (vol == 0.f || !RayFinite(vol)) {
        return h;
    }
    const float s = vol < 0.f ? -1.f : 1.f;
    const float ea = s * ((na[0] * r.d[0] + na[1] * r.d[1]) + na[2] * r.d[2]);
    const float eb = s * ((nb[0] * r.d[0] + nb[1] * r.d[1]) + nb[2] * r.d[2]);
    const float ec = s * ((nc[0] * r.d[0] + nc[1] * r.d[1]) + nc[2] * r.d[2]);
    const float det = (ea + eb) + ec;
    if (!(ea >= 0.f && eb >= 0.f && ec >= 0.f && det > 0.f)) {
        return h;
    }
    const float t = fabsf(vol) / det;
    if (!(r.tmin <= t && t <= r.tmax)) {
        return h;
    }
    h.hit = true;
    h.t = t;
    h.w1 = eb / det;
    h.w2 = ec / det;
    return h;
}

// (t, id) below the best so far, lexicographically; best_id < 0: no hit yet.
__host__ __device__ inline bool RayCloser(float t, int id, float best_t, int best_id) {
    return best_id < 0 || t < best_t || (t == best_t && id < best_id);
}

}  // namespace srt
