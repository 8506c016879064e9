// Sampled radiance (include/srt_radiance.h, DESIGN.md sections 2 "Radiance" and 5): for every
// element of a prepared frame a generator's S rays from the surface point, each walked to its
// closest hit, the hit shaded under the lights, and the S colours summed in ascending s -- one
// launch, a ray's life in registers and LDS. The answer is defined as the composition's
// (LaunchVisibilityRays -> LaunchRayClosest -> LaunchLightHits -> the ordered sum), bit for bit.
// render.hip holds the kernel (beside LightHitsKernel, whose light scan it calls); radiance.cpp the
// host answer, which is that composition of the host answers.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "cpu_render.h"
#include "render.h"
#include "visibility.h"

namespace srt {

// What is stored (step 6). modulate: the mean is multiplied by the albedo of the element's own
// triangle. base (elements x 4, 16-byte aligned on the device; null: store; may be rgba) with weight[3]
// (finite): an element on a surface stores (base.rgb + weight . m, base.a), any other the base element.
struct RadianceStore {
    bool modulate;
    const float* base;
    float weight[3];
    float* rgba;  // elements x 4, 16-byte aligned on the device
};

// The fused launch over the elements `e` of the scene (d_vertices, d_shade, n, frame, background)
// under `count` lights. gen.kind is kVisibilityHemisphere or kVisibilityMirror. tree == nullptr: brute
// force over d_vertices. One launch whatever count and S; no elements: none.
hipError_t LaunchRadiance(const RayTree* tree, const float* d_vertices, const float* d_shade, std::uint64_t n,
                          const Frame& frame, const float background[3], const LightingLight* lights, std::size_t count,
                          const float ambient[3], const VisibilityElements& e, const VisibilityGen& gen,
                          const RadianceStore& store, hipStream_t stream);

// The host answer for `elements` points elements on the scene's width x height frame: the
// composition HostVisibilityRays -> HostRayClosest -> HostLightHits, then steps 4 to 6.
void HostRadiance(const Scene& scene, std::size_t width, std::size_t height, const HostLight* lights, std::size_t count,
                  const float ambient[3], const float* positions, const int* ids, std::size_t elements,
                  const VisibilityGen& gen, const RadianceStore& store);

}  // namespace srt
