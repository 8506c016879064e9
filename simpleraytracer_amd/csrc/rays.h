// Ray queries (include/srt_rays.h, DESIGN.md sections 2 "Rays", 4 and 5): closest hit and occlusion
// for caller-supplied rays, each with an origin, a direction and a range of its own. rays.hip holds
// the world-space tree of a device scene, its build, the two traversal kernels, the brute-force
// kernels beside them and the host answer; ray_math.h the arithmetic all of them share.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "render.h"  // BvhLayout
#include "scene.h"

namespace srt {

constexpr int kRayRecordFloats = 16;   // a triangle of the tree: 9 vertex floats, padded box (6), id
constexpr unsigned kRayBoundBlocks = 256;  // partial results of the centroid bounds reduction

// The world-space tree of one device scene: an implicit, complete 8-wide tree (BvhLayout: level 0
// node i = records [8 i, 8 i + 8), level L node i = level L - 1 nodes [8 i, 8 i + 8)) over the
// triangles in the order of the 30-bit 3-D Morton keys of their centroids. Every buffer's size
// depends on the triangle count only: allocated once, rebuilt in place.
struct RayTree {
    BvhLayout layout;
    float4* records = nullptr;  // layout.count[0] * 8 records of 4 float4 (padding: never hit)
    float4* nodes = nullptr;    // layout.nodes x (lo, hi)
    unsigned* keys = nullptr;
    unsigned* keys_sorted = nullptr;
    unsigned* ids = nullptr;
    unsigned* order = nullptr;
    float* bounds = nullptr;    // kRayBoundBlocks x 6 partials, then the 6 bounds
    void* temp = nullptr;       // rocPRIM's
    std::size_t temp_bytes = 0;
};

// Bytes of the standing structure per triangle, scratch of the build included.
std::size_t RayTreeBytes(std::uint64_t n);
// Allocates every buffer (n > 0); throws, with nothing left allocated, on failure.
void AllocRayTree(RayTree& tree, std::uint64_t n, hipStream_t stream);
void FreeRayTree(RayTree& tree) noexcept;
// The whole build on `stream`: bounds, keys, sort, gather, leaf boxes, upper levels. No allocation,
// no host synchronisation: the bounds stay on the device.
void EnqueueRayTreeBuild(const RayTree& tree, const float* d_vertices, std::uint64_t n, hipStream_t stream);

// `count` rays (count x 8 floats, device) against the scene. tree == nullptr: brute force over
// d_vertices (n x 9) in ascending id. closest: d_ids, d_t and (may be null) d_bary (count x 2);
// else d_out, one byte per ray. n == 0 stores misses; count == 0 enqueues nothing.
void LaunchRayClosest(const RayTree* tree, const float* d_vertices, std::uint64_t n, const float* d_rays,
                      std::size_t count, int* d_ids, float* d_t, float* d_bary, hipStream_t stream);
void LaunchRayOccluded(const RayTree* tree, const float* d_vertices, std::uint64_t n, const float* d_rays,
                       std::size_t count, unsigned char* d_out, hipStream_t stream);

// The host answer: brute force over every triangle in ascending id, no tree. box_clause == false
// leaves the box clause out of the definition (what it costs: tests/test_rays_host.py).
void HostRayClosest(const Scene& scene, const float* rays, std::size_t count, int* ids, float* t, float* bary,
                    bool box_clause);
void HostRayOccluded(const Scene& scene, const float* rays, std::size_t count, unsigned char* out, bool box_clause);

}  // namespace srt
