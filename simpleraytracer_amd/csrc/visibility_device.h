// Sampled visibility on the device: a call's parameters, a lane's element and a surface's ray, as the
// visibility kernels (visibility.hip) and the radiance kernel (render.hip RadianceKernel) share
// them, so a ray has the same bits whichever kernel generates it. The arithmetic is
// visibility_math.h's; DESIGN.md section 2 "Visibility" defines it.
#pragma once

#include <hip/hip_runtime.h>

#include "ray_math.h"
#include "visibility.h"
#include "visibility_math.h"

namespace srt {

// The pixel footprint of a frame call's block: kVisibilityTileW x (256 / kVisibilityTileW) pixels, a
// lane's pixel at (tid % W, tid / W). Measured (profiles/visibility/): a compact tile keeps a block's
// origins close together; 8 x 32 is the fastest tried, 256 pixels of one row 2.6 times slower.
// SRT_VISIBILITY_TILE_W, SRT_VISIBILITY_THREADS: measurement builds.
#ifndef SRT_VISIBILITY_TILE_W
#define SRT_VISIBILITY_TILE_W 8
#endif
#ifndef SRT_VISIBILITY_THREADS
#define SRT_VISIBILITY_THREADS 256
#endif
constexpr unsigned kVisibilityThreads = SRT_VISIBILITY_THREADS;
static_assert(kVisibilityThreads == 64 || kVisibilityThreads == 128 || kVisibilityThreads == 256,
              "a block is one, two or four waves (the sample table is loaded by the first 192 lanes or in passes)");
constexpr unsigned kVisibilityTileW = SRT_VISIBILITY_TILE_W;
constexpr unsigned kVisibilityTileH = kVisibilityThreads / kVisibilityTileW;  // rows of one pass of the block
static_assert(kVisibilityTileW >= 1 && kVisibilityTileW <= kVisibilityThreads &&
                  (kVisibilityTileW & (kVisibilityTileW - 1)) == 0,
              "the tile width is a power of two up to the block");

struct VisibilityParams {
    const float* __restrict__ vertices;  // the scene's, by id
    const float2* __restrict__ where;    // positions (POINTS) or sample offsets
    const int* __restrict__ ids;
    const float4* __restrict__ nodes;    // tree
    const float4* __restrict__ records;
    const float* __restrict__ samples;
    const float2* __restrict__ rotations;  // may be null
    unsigned char* __restrict__ visible;   // may be null
    float* __restrict__ fraction;          // may be null
    float4* __restrict__ rays;             // export
    unsigned long long count;  // elements of the call
    unsigned n;
    unsigned width;    // elements per row
    unsigned rows;
    unsigned row_begin;
    unsigned tiles_x;  // blocks per tile row
    unsigned samples_count;
    float wf, hf;
    float eye[3], base[3], du[3], dv[3];
    float corner[3], eu[3], ev[3];
    float tmin, tmax;
};

// A lane's element: where it is, its rotation index and its surface (steps 1 to 4). in == false: the
// lane is past the call's elements.
struct VisibilityElement {
    bool in;
    unsigned long long e;
    unsigned turn;
    VisibilitySurface sf;
};

// The block takes EPT passes of 256 elements: pass k of a points call the k-th 256 consecutive ones of
// its 256 EPT, of a frame call the k-th kVisibilityTileH rows of its tile.
template <bool POINTS, unsigned EPT = 1>
__device__ __forceinline__ VisibilityElement ElementOf(const VisibilityParams& p, unsigned tid, unsigned k = 0) {
    VisibilityElement el{};
    unsigned x = 0, y = 0;
    if constexpr (POINTS) {
        el.e = (blockIdx.x * static_cast<unsigned long long>(EPT) + k) * kVisibilityThreads + tid;
        el.in = el.e < p.count;
        el.turn = static_cast<unsigned>(el.e) & (kVisibilityRotations - 1);
    } else {
        const unsigned tile_y = blockIdx.x / p.tiles_x, tile_x = blockIdx.x - tile_y * p.tiles_x;
        x = tile_x * kVisibilityTileW + (tid & (kVisibilityTileW - 1));
        y = (tile_y * EPT + k) * kVisibilityTileH + tid / kVisibilityTileW;
        el.in = x < p.width && y < p.rows;
        el.e = static_cast<unsigned long long>(y) * p.width + x;
        el.turn = (((p.row_begin + y) & 3u) << 2) | (x & 3u);
    }
    if (!el.in) {
        return el;
    }
    const int id = p.ids[el.e];
    const float2 w = p.where[el.e];
    float fx = w.x, fy = w.y;
    if constexpr (!POINTS) {
        fx = (static_cast<float>(x) + w.x) / p.wf;
        fy = (static_cast<float>(p.row_begin + y) + w.y) / p.hf;
    }
    if (static_cast<unsigned>(id) < p.n) {
        const float* __restrict__ at = p.vertices + 9ull * static_cast<unsigned>(id);
        float v[9];
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            v[j] = at[j];
        }
        el.sf = VisibilitySurfaceAt(p.eye, p.base, p.du, p.dv, v, fx, fy);
    }
    return el;
}

// Sample s of a surface's rays (step 5). T, B: the hemisphere's basis; (rc, rs): its rotation.
template <int KIND>
__device__ __forceinline__ Ray RayOf(const VisibilityParams& p, const float* s_samples, unsigned s, const float pt[3],
                                     const float d[3], const float n[3], const float T[3], const float B[3],
                                     bool rotate, float rc, float rs) {
    Ray r;
    if constexpr (KIND == kVisibilityHemisphere) {
        VisibilityHemisphereDir(n, T, B, s_samples[3 * s], s_samples[3 * s + 1], s_samples[3 * s + 2], rotate, rc, rs, r.d);
    } else if constexpr (KIND == kVisibilityArea) {
        VisibilityAreaDir(p.corner, p.eu, p.ev, s_samples[2 * s], s_samples[2 * s + 1], pt, r.d);
    } else {
        VisibilityMirrorDir(d, n, r.d);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        r.o[k] = pt[k];
    }
    r.tmin = p.tmin;
    r.tmax = p.tmax;
    return r;
}

// What a launch fills of p from the frame, the elements (at least one) and the generator -- the scene,
// the tree and the outputs are the caller's -- and its grid, a block taking `passes` passes of
// kVisibilityThreads elements (visibility.hip). Throws on more elements than one call takes.
dim3 FillVisibility(VisibilityParams& p, const Frame& frame, const VisibilityElements& e, const VisibilityGen& gen,
                    unsigned passes);

}  // namespace srt
