// The over-composite of a pixel's depth layers: the per-pixel arithmetic of CompositeKernel
// (query.hip; DESIGN.md section 2 "Composite"). Host and device share it (cpu_render.cpp
// HostComposite, the host answer rtkCompositeHost), so both evaluate the same float expressions.
//
// Every operation this header adds is float32 with separate multiply and add -- no fma, no
// contraction (-ffp-contract=off), in the order written -- shadow_math.h's convention, so that a
// numpy float32 restatement reproduces the bits. A layer's rgb c_k is samples_math.h's
// ResolveShadeHit (ShadeRecord's expressions, explicit fma), as the resolve's samples are.
//
// For a pixel with layer ids id_0 .. id_{K-1} (front to back) and a per-triangle opacity table:
//   T = 1, acc = (0, 0, 0)
//   for k = 0 .. K-1, stopping at the first id_k outside [0, n):
//     a = opacity[id_k];  w = T a;  acc_c = acc_c + w c_k,c;  T = T - w
//   rgb_c = acc_c + T background_c;  alpha = 1 - T
// Opacity values are not range-checked; NaN propagates.
#pragma once

#include <hip/hip_runtime.h>

#include "samples_math.h"

namespace srt {

// The running composite of a pixel: the colour gathered so far and the transmittance left.
struct CompositeAcc {
    float r, g, b;
    float T;
};

__host__ __device__ inline CompositeAcc CompositeStart() { return CompositeAcc{0.f, 0.f, 0.f, 1.f}; }

// The next layer (front to back) of opacity a and rgb c joins the composite.
__host__ __device__ inline void CompositeAdd(CompositeAcc& acc, float a, const ResolveRgb& c) {
    const float w = acc.T * a;
    acc.r = acc.r + w * c.r;
    acc.g = acc.g + w * c.g;
    acc.b = acc.b + w * c.b;
    acc.T = acc.T - w;
}

__host__ __device__ inline ResolveTexel CompositeFinish(const CompositeAcc& acc, const float bg[3]) {
    return ResolveTexel{acc.r + acc.T * bg[0], acc.g + acc.T * bg[1], acc.b + acc.T * bg[2], 1.f - acc.T};
}

}  // namespace srt
