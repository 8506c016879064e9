// Sampled visibility (include/srt_visibility.h, DESIGN.md sections 2 "Visibility" and 5): for every
// element of a prepared frame a generator's S rays from the surface point, exported in the ray
// queries' format or traced in the same launch and counted. visibility.hip holds the kernels and
// the host answer; visibility_math.h the arithmetic they share; ray_walk.h the walk they share with
// the ray queries.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "rays.h"
#include "scene.h"

namespace srt {

// include/srt_visibility.h rta_generator, checked. samples / rotations: device pointers for the
// launches, host pointers for the host answer.
struct VisibilityGen {
    int kind;
    unsigned count;  // S
    const float* samples;
    const float* rotations;  // null: none
    float corner[3], eu[3], ev[3];
    float tmin, tmax;
};

// The elements of a call. points: `count` positions `where` (count x 2) with ids; else the band rows
// [row_begin, row_begin + rows) of the width-wide frame, `where` its sample offsets, band-local.
struct VisibilityElements {
    bool points;
    const float* where;
    const int* ids;
    std::size_t width;   // elements per row (points: count)
    std::size_t rows;    // (points: 1)
    std::size_t row_begin;
    std::size_t frame_width, frame_height;
};

// The fused launch: visible (uint8) and fraction (float), either may be null, one per element.
// tree == nullptr: brute force over d_vertices.
void LaunchVisibility(const RayTree* tree, const float* d_vertices, std::uint64_t n, const Frame& frame,
                      const VisibilityElements& e, const VisibilityGen& gen, unsigned char* d_visible,
                      float* d_fraction, hipStream_t stream);
// The export launch: d_rays, S x elements x 8 floats, sample-major.
void LaunchVisibilityRays(const float* d_vertices, std::uint64_t n, const Frame& frame, const VisibilityElements& e,
                          const VisibilityGen& gen, float* d_rays, hipStream_t stream);

// The host answers for `count` points elements on the scene's width x height frame. rays: S x count x
// 8 floats, sample-major. visible / fraction: either may be null.
void HostVisibilityRays(const Scene& scene, std::size_t width, std::size_t height, const float* positions,
                        const int* ids, std::size_t count, const VisibilityGen& gen, float* rays);
void HostVisibility(const Scene& scene, std::size_t width, std::size_t height, const float* positions, const int* ids,
                    std::size_t count, const VisibilityGen& gen, unsigned char* visible, float* fraction);

}  // namespace srt
