// The resolve of a multi-sample pixel: the shade of one (image position, hit id) sample and the
// accumulate / divide step (outputs.hip ResolveKernel; DESIGN.md section 2 "Resolve"). Host and
// device share it (cpu_render.cpp HostResolve, the host answer rtsResolveHost), so both evaluate
// the same float expressions: explicit fma, no contraction, IEEE divide and square root.
//
// For a pixel with samples s = 0 .. S-1, each an image position (fx_s, fy_s) -- ray generation's
// expression of the pixel under sample offset o_s -- and a hit id:
//   c_s    the shaded rgb of the sample: albedo * min(|N . d| / (|N| |d|), 1) with
//          d = base + fx du + fy dv for a hit (ShadeRecord's expressions, so ShadeRecord's bits),
//          the background for a miss (an id outside the scene)
//   acc    c_0, then acc + c_s for s = 1 .. S-1: float32, ascending s, one rounding per add
//   rgb    acc / float(S), one correctly rounded division per channel
//   alpha  float(hits) / float(S), hits = the samples that are hits: the pixel's coverage
// S = 1, and S = 2 or 4 equal samples, give a sample's own rgb bit for bit (8 and 16 do not: 5c, 6c
// and 7c each round).
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace srt {

struct ResolveRgb {
    float r, g, b;
};

// The running sum of a pixel's samples and the number of hits among them.
struct ResolveAcc {
    float r, g, b;
    unsigned hits;
};

struct ResolveTexel {
    float r, g, b, a;
};

__host__ __device__ inline float ResolveDot3(float ax, float ay, float az, float bx, float by, float bz) {
    return fmaf(az, bz, fmaf(ay, by, ax * bx));
}

// The image position of pixel (x, y) of the w x h frame under sample offset (ox, oy): ray
// generation's expression (wf = float(w), hf = float(h)).
__host__ __device__ inline void ResolvePosition(unsigned x, unsigned y, float ox, float oy, float wf, float hf,
                                                float& fx, float& fy) {
    fx = (static_cast<float>(x) + ox) / wf;
    fy = (static_cast<float>(y) + oy) / hf;
}

// A hit's rgb. nr = (N, |N|) and al = the albedo: the triangle's shading table row.
__host__ __device__ inline ResolveRgb ResolveShadeHit(const float base[3], const float du[3], const float dv[3],
                                                      float fx, float fy, float nrx, float nry, float nrz, float nrw,
                                                      float alr, float alg, float alb) {
    const float dx = fmaf(fy, dv[0], fmaf(fx, du[0], base[0]));
    const float dy = fmaf(fy, dv[1], fmaf(fx, du[1], base[1]));
    const float dz = fmaf(fy, dv[2], fmaf(fx, du[2], base[2]));
    const float nd = ResolveDot3(nrx, nry, nrz, dx, dy, dz);
    const float dd = ResolveDot3(dx, dy, dz, dx, dy, dz);
    const float cosv = fminf(fabsf(nd) / (nrw * sqrtf(dd)), 1.f);
    return ResolveRgb{alr * cosv, alg * cosv, alb * cosv};
}

// Sample s of the pixel joins the sum: the first one starts it (no 0 + c_0).
__host__ __device__ inline void ResolveAdd(ResolveAcc& acc, unsigned s, const ResolveRgb& c, bool hit) {
    if (s == 0) {
        acc = ResolveAcc{c.r, c.g, c.b, 0u};
    } else {
        acc.r = acc.r + c.r;
        acc.g = acc.g + c.g;
        acc.b = acc.b + c.b;
    }
    acc.hits += hit ? 1u : 0u;
}

__host__ __device__ inline ResolveTexel ResolveFinish(const ResolveAcc& acc, unsigned samples) {
    const float sf = static_cast<float>(samples);
    return ResolveTexel{acc.r / sf, acc.g / sf, acc.b / sf, static_cast<float>(acc.hits) / sf};
}

}  // namespace srt
