// Vertex attributes of one (image position, triangle) pair: perspective-correct weights, the
// interpolation of per-corner tables, the smooth normal and the texture lookup (outputs.hip
// SurfaceKernel / InterpolateKernel; DESIGN.md section 2 "Vertex attributes"). Host and device
// share it (cpu_render.cpp HostSurface / HostInterpolate, the host answers rtvSurfaceHost and
// rtvInterpolateHost), so both evaluate the same float expressions.
//
// Every operation this header adds is float32 with separate multiply and add -- no fma, no
// contraction (-ffp-contract=off), in the order written, IEEE divide and square root -- so that a
// numpy float32 restatement reproduces the bits (shadow_math.h's convention). The one exception is
// inherited: E_A, E_B, E_C are "Surface attributes"' fma edge functions (gbuffer_math.h), the
// traces' own bits.
//
//   weights   w_k = E_k / det, det = (E_A + E_B) + E_C: (w1, w2) are the G-buffer's bary bits. The
//             E_k come from planes through the eye, so these are object-space barycentrics of the
//             hit point: perspective-correct by construction.
//   mix       out = (w0 a0 + w1 a1) + w2 a2 of a corner table's three values.
//   normal    Ns = mix of the corner normals (any length), d = (base + fx du) + fy dv,
//             c = |Ns.d| / (sqrt(Ns.Ns) sqrt(d.d)), cos = c < 1 ? c : 1, u = Ns / sqrt(Ns.Ns),
//             negated iff Ns.d > 0; dotp(a, b) = (a.x b.x + a.y b.y) + a.z b.z.
//   texture   per axis: wrap (repeat: r = u - floor(u), outside [0, 1] or NaN -> 0; clamp:
//             u > 0 ? (u < 1 ? u : 1) : 0), then bilinear (x = r size - 0.5, x0 = floor(x),
//             a = x - x0, taps int(x0) and int(x0) + 1 wrapped or clamped into [0, size)) or nearest
//             (min(int(floor(r size)), size - 1)); texel = top + b (bot - top) with
//             top = T[j0][i0] + a (T[j0][i1] - T[j0][i0]) and bot the same on row j1.
// r lies in [0, 1] whatever u is, so every tap is in range by construction, also at size 1.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace srt {

constexpr unsigned kSurfaceWrapClamp = 1u;      // include/srt_surface.h RTV_WRAP_CLAMP
constexpr unsigned kSurfaceFilterNearest = 2u;  // RTV_FILTER_NEAREST
constexpr unsigned kSurfaceModulate = 4u;       // RTV_MODULATE
constexpr unsigned kSurfaceFlags = 7u;
constexpr unsigned kSurfaceMaxTexture = 16384u;  // RTV_MAX_TEXTURE: texels per side
constexpr int kSurfaceMaxChannels = 4;           // RTV_MAX_CHANNELS: floats per corner

struct SurfaceWeights {
    float w0, w1, w2;
};

// c = the triangle's edge record under the prepared frame (ComputeEdges' values).
__host__ __device__ inline SurfaceWeights SurfaceBary(const float c[9], float fx, float fy) {
    const float eA = fmaf(fy, c[2], fmaf(fx, c[1], c[0]));
    const float eB = fmaf(fy, c[5], fmaf(fx, c[4], c[3]));
    const float eC = fmaf(fy, c[8], fmaf(fx, c[7], c[6]));
    const float det = (eA + eB) + eC;
    return SurfaceWeights{eA / det, eB / det, eC / det};
}

__host__ __device__ inline float SurfaceMix(const SurfaceWeights& w, float a0, float a1, float a2) {
    return (w.w0 * a0 + w.w1 * a1) + w.w2 * a2;
}

__host__ __device__ inline float SurfaceDot(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}

// The normal plane of an interpolated normal Ns: (unit normal towards the eye, shading cosine).
struct SurfaceNormal {
    float x, y, z, cosv;
};

__host__ __device__ inline SurfaceNormal SurfaceSmoothNormal(float nsx, float nsy, float nsz, const float base[3],
                                                             const float du[3], const float dv[3], float fx, float fy) {
    const float dx = (base[0] + fx * du[0]) + fy * dv[0];
    const float dy = (base[1] + fx * du[1]) + fy * dv[1];
    const float dz = (base[2] + fx * du[2]) + fy * dv[2];
    const float nn = SurfaceDot(nsx, nsy, nsz, nsx, nsy, nsz);
    const float nd = SurfaceDot(nsx, nsy, nsz, dx, dy, dz);
    const float dd = SurfaceDot(dx, dy, dz, dx, dy, dz);
    const float len = sqrtf(nn);
    const float c = fabsf(nd) / (len * sqrtf(dd));
    const float ux = nsx / len, uy = nsy / len, uz = nsz / len;
    const bool flip = nd > 0.f;
    return SurfaceNormal{flip ? -ux : ux, flip ? -uy : uy, flip ? -uz : uz, c < 1.f ? c : 1.f};
}

// A texture coordinate into [0, 1]; NaN and +-inf become 0.
__host__ __device__ inline float SurfaceWrap(float u, bool clamp) {
    if (clamp) {
        return u > 0.f ? (u < 1.f ? u : 1.f) : 0.f;
    }
    const float r = u - floorf(u);
    return (r >= 0.f && r <= 1.f) ? r : 0.f;
}

// The two taps of one axis and the weight of the second. r in [0, 1], 1 <= size <= kSurfaceMaxTexture.
struct SurfaceTaps {
    int i0, i1;
    float a;
};

__host__ __device__ inline SurfaceTaps SurfaceBilinear(float r, int size, bool clamp) {
    const float x = r * static_cast<float>(size) - 0.5f;  // in [-0.5, size - 0.5]
    const float x0 = floorf(x);
    SurfaceTaps t;
    t.a = x - x0;
    t.i0 = static_cast<int>(x0);
    t.i1 = t.i0 + 1;
    if (clamp) {
        t.i0 = t.i0 > 0 ? t.i0 : 0;
        t.i1 = t.i1 < size - 1 ? t.i1 : size - 1;
    } else {
        t.i0 = t.i0 < 0 ? t.i0 + size : t.i0;
        t.i1 = t.i1 >= size ? t.i1 - size : t.i1;
    }
    return t;
}

__host__ __device__ inline int SurfaceNearest(float r, int size) {
    const int i = static_cast<int>(floorf(r * static_cast<float>(size)));
    return i < size - 1 ? i : size - 1;
}

__host__ __device__ inline float SurfaceLerp(float p, float q, float a) { return p + a * (q - p); }

}  // namespace srt
