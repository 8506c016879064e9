// One ray's walk through the world-space tree of a device scene (rays.h RayTree), and the brute-force
// scan beside it: the device functions the ray-query kernels (rays.hip) and the sampled-visibility
// kernels (visibility.hip) share, so a ray answers with the same bits whichever kernel carries it.
// DESIGN.md section 2 "Rays" proves the walk exact; section 5 describes it.
#pragma once

#include <hip/hip_runtime.h>

#include "ray_math.h"
#include "render.h"  // kBvhWidth, kBvhMaxLevels

namespace srt {

struct RayBest {
    int id = -1;
    float t = __builtin_inff(), w1 = 0.f, w2 = 0.f;
};

// The per-level node counts and offsets of the implicit tree over n triangles, recomputed by one
// thread into LDS (a lane indexes them by its level). The caller's barrier follows.
__device__ __forceinline__ void RayLevelsInit(unsigned n, unsigned* s_count, unsigned* s_offset, unsigned* s_levels) {
    unsigned below = n, offset = 0, levels = 0;
    do {
        const unsigned c = (below + kBvhWidth - 1) / kBvhWidth;
        s_count[levels] = c;
        s_offset[levels] = offset;
        offset += c;
        ++levels;
        below = c;
    } while (below > 1 && levels < kBvhMaxLevels);
    *s_levels = levels;
}

// The tree is implicit and complete, so the walk keeps (level, idx) and no stack: a node that passes
// is entered at its first child, idx 8; after a node is done the walk moves to idx + 1, climbing
// first while idx is the last child of its parent. kClosest: the lexicographic (t, id) minimum of
// the triangles that count; else the walk leaves at its first counted hit (id >= 0). The ray comes by
// value and the answer goes back by value: the form whose code in RayTreeKernel is the code the walk
// had as that kernel's own body.
template <bool kClosest>
__device__ __forceinline__ RayBest RayWalk(const Ray r, const float4* nodes, const float4* records,
                                           const unsigned* s_count, const unsigned* s_offset,
                                           const unsigned* s_levels) {
    RayBest best;
    if (RayDegenerate(r)) {
        return best;
    }
    float inv[3];
    RayInverse(r, inv);
    const unsigned top = *s_levels - 1;
    unsigned level = top, idx = 0;
    for (;;) {
        const float4 nlo = nodes[2ull * (s_offset[level] + idx)];
        const float4 nhi = nodes[2ull * (s_offset[level] + idx) + 1];
        const float lo[3] = {nlo.x, nlo.y, nlo.z}, hi[3] = {nhi.x, nhi.y, nhi.z};
        bool pass = RayBoxClause(r, inv, lo, hi);
        if (pass && level == 0) {
            const float4* __restrict__ rec = records + 4ull * (static_cast<unsigned long long>(idx) * kBvhWidth);
            bool done = false;
            for (int c = 0; c < kBvhWidth; ++c) {
                const float4 q2 = rec[4 * c + 2], q3 = rec[4 * c + 3];
                const float plo[3] = {q2.y, q2.z, q2.w}, phi[3] = {q3.x, q3.y, q3.z};
                if (!RayBoxClause(r, inv, plo, phi)) {
                    continue;
                }
                const float4 q0 = rec[4 * c], q1 = rec[4 * c + 1];
                const float v[9] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x};
                const RayHit h = RayEdgeTest(r, v);
                const int id = __float_as_int(q3.w);
                if (h.hit && RayCloser(h.t, id, best.t, best.id)) {
                    best.id = id;
                    best.t = h.t;
                    best.w1 = h.w1;
                    best.w2 = h.w2;
                    if (!kClosest) {
                        done = true;
                        break;
                    }
                }
            }
            if (done) {
                break;
            }
            pass = false;
        }
        if (pass) {
            --level;
            idx *= kBvhWidth;
            continue;
        }
        bool end = false;
        for (;;) {
            if (level == top) {
                end = true;
                break;
            }
            if ((idx & (kBvhWidth - 1)) != kBvhWidth - 1 && idx + 1 < s_count[level]) {
                ++idx;
                break;
            }
            idx /= kBvhWidth;
            ++level;
        }
        if (end) {
            break;
        }
    }
    return best;
}

// Brute force over the scene's own vertices (n x 9) in ascending id: no structure. Lanes that scan
// together read the same triangle, so the loads are wave-uniform.
template <bool kClosest>
__device__ __forceinline__ RayBest RayScan(const Ray r, const float* vertices, unsigned n) {
    RayBest best;
    if (RayDegenerate(r)) {
        return best;
    }
    float inv[3];
    RayInverse(r, inv);
    for (unsigned k = 0; k < n; ++k) {
        const float* __restrict__ src = vertices + 9ull * k;
        float v[9], plo[3], phi[3];
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            v[j] = src[j];
        }
        if (!RayTriangleBox(v, plo, phi) || !RayBoxClause(r, inv, plo, phi)) {
            continue;
        }
        const RayHit h = RayEdgeTest(r, v);
        if (h.hit && RayCloser(h.t, static_cast<int>(k), best.t, best.id)) {
            best.id = static_cast<int>(k);
            best.t = h.t;
            best.w1 = h.w1;
            best.w2 = h.w2;
            if (!kClosest) {
                break;
            }
        }
    }
    return best;
}

}  // namespace srt
