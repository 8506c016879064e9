// Ray queries (include/srt_rays.h): the world-space tree of a device scene and the kernels that
// answer caller-supplied rays from it. DESIGN.md section 2 "Rays" defines the answer and proves the
// traversal exact; section 4 has the structure's layout, section 5 the kernels.
//
// The answer does not depend on the tree: a triangle is hit iff its own padded box passes the box
// clause and the edge test passes (ray_math.h), and a node's box -- the union of the padded boxes
// below it -- passes the same clause whenever one of them does. So a node that fails is skipped
// with everything below it, in any visiting order, and the closest hit is the lexicographic
// (t, id) minimum over the triangles that count. No node is skipped on the best t so far.
#include <rocprim/device/device_radix_sort.hpp>

#include <cstring>
#include <stdexcept>
#include <string>

#include "ray_math.h"
#include "ray_walk.h"
#include "rays.h"

namespace srt {
namespace {

void Check(hipError_t e, const char* what) {
    if (e != hipSuccess) {
        throw std::runtime_error(std::string("HIP error: ") + what + ": " + hipGetErrorString(e));
    }
}

// ---------------------------------------------------------------------------------------------
// Build
// ---------------------------------------------------------------------------------------------

// The centroid the keys are made from: ((v0 + v1) + v2) / 3 per axis. Only the order depends on it.
__device__ __forceinline__ bool Centroid(const float* __restrict__ v, float c[3]) {
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        c[k] = ((v[k] + v[3 + k]) + v[6 + k]) / 3.f;
        finite = finite && RayFinite(c[k]);
    }
    return finite;
}

// Bounds of the finite centroids, step 1: one partial (lo.xyz, hi.xyz) per block, grid-stride.
__global__ __launch_bounds__(256) void RayBoundsKernel(const float* __restrict__ vertices, unsigned n,
                                                       float* __restrict__ partial) {
    __shared__ float s[6][256];
    const unsigned tid = threadIdx.x;
    float lo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float hi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    for (unsigned i = blockIdx.x * 256 + tid; i < n; i += gridDim.x * 256) {
        float c[3];
        if (Centroid(vertices + 9ull * i, c)) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                lo[k] = fminf(lo[k], c[k]);
                hi[k] = fmaxf(hi[k], c[k]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        s[k][tid] = lo[k];
        s[3 + k][tid] = hi[k];
    }
    __syncthreads();
    for (unsigned w = 128; w > 0; w >>= 1) {
        if (tid < w) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                s[k][tid] = fminf(s[k][tid], s[k][tid + w]);
                s[3 + k][tid] = fmaxf(s[3 + k][tid], s[3 + k][tid + w]);
            }
        }
        __syncthreads();
    }
    if (tid < 6) {
        partial[6 * blockIdx.x + tid] = s[tid][0];
    }
}

// Step 2: one block folds the `blocks` (<= 256) partials into bounds[0..6).
__global__ __launch_bounds__(256) void RayBoundsFoldKernel(const float* __restrict__ partial, unsigned blocks,
                                                           float* __restrict__ bounds) {
    __shared__ float s[6][256];
    const unsigned tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        s[k][tid] = tid < blocks ? partial[6 * tid + k] : __builtin_inff();
        s[3 + k][tid] = tid < blocks ? partial[6 * tid + 3 + k] : -__builtin_inff();
    }
    __syncthreads();
    for (unsigned w = 128; w > 0; w >>= 1) {
        if (tid < w) {
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                s[k][tid] = fminf(s[k][tid], s[k][tid + w]);
                s[3 + k][tid] = fmaxf(s[3 + k][tid], s[3 + k][tid + w]);
            }
        }
        __syncthreads();
    }
    if (tid < 6) {
        bounds[tid] = s[tid][0];
    }
}

__device__ __forceinline__ unsigned Spread10(unsigned x) {  // bit b of x (b < 10) to bit 3 b
    x &= 0x3FFu;
    x = (x | (x << 16)) & 0x030000FFu;
    x = (x | (x << 8)) & 0x0300F00Fu;
    x = (x | (x << 4)) & 0x030C30C3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

// 30-bit 3-D Morton key of each centroid inside the bounds (read from device memory: the host never
// sees them); a non-finite centroid sorts last (bit 30).
__global__ __launch_bounds__(256) void RayKeysKernel(const float* __restrict__ vertices, unsigned n,
                                                     const float* __restrict__ bounds, unsigned* __restrict__ keys,
                                                     unsigned* __restrict__ ids) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) {
        return;
    }
    float c[3];
    unsigned key = 0x40000000u;
    if (Centroid(vertices + 9ull * i, c)) {
        unsigned q[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float lo = bounds[k], ext = bounds[3 + k] - lo;
            float f = ext > 0.f ? (c[k] - lo) / ext * 1023.f : 0.f;
            f = f >= 0.f ? f : 0.f;  // (NaN too)
            f = f <= 1023.f ? f : 1023.f;
            q[k] = static_cast<unsigned>(f);
        }
        key = (Spread10(q[2]) << 2) | (Spread10(q[1]) << 1) | Spread10(q[0]);
    }
    keys[i] = key;
    ids[i] = i;
}

// Position i of the order takes triangle order[i]: its vertices, its padded box and its id, 64
// bytes. Positions [n, padded) are padding: the empty box, never hit.
__global__ __launch_bounds__(256) void RayGatherKernel(const float* __restrict__ vertices, unsigned n,
                                                       unsigned padded, const unsigned* __restrict__ order,
                                                       float4* __restrict__ records) {
    const unsigned i = blockIdx.x * 256 + threadIdx.x;
    if (i >= padded) {
        return;
    }
    float v[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float plo[3] = {__builtin_inff(), __builtin_inff(), __builtin_inff()};
    float phi[3] = {-__builtin_inff(), -__builtin_inff(), -__builtin_inff()};
    unsigned id = 0xFFFFFFFFu;
    if (i < n) {
        id = order[i];
        const float* __restrict__ src = vertices + 9ull * id;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            v[k] = src[k];
        }
        RayTriangleBox(v, plo, phi);
    }
    float4* r = records + 4ull * i;
    r[0] = make_float4(v[0], v[1], v[2], v[3]);
    r[1] = make_float4(v[4], v[5], v[6], v[7]);
    r[2] = make_float4(v[8], plo[0], plo[1], plo[2]);
    r[3] = make_float4(phi[0], phi[1], phi[2], __uint_as_float(id));
}

struct RayNodeParams {
    const float4* records;
    float4* nodes;  // (lo, hi) per node, all levels
    BvhLayout layout;
};

// Leaves (one thread each) and level 1 (the first 32 threads of each block), as the screen-space
// tree's refit (render.hip BvhLeafKernel). The empty box (+inf, -inf) is the union's identity.
__global__ __launch_bounds__(256) void RayLeafKernel(RayNodeParams p) {
    __shared__ float4 slo[256], shi[256];
    const unsigned tid = threadIdx.x;
    const unsigned leaf = blockIdx.x * 256 + tid;
    float4 lo = make_float4(__builtin_inff(), __builtin_inff(), __builtin_inff(), 0.f);
    float4 hi = make_float4(-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), 0.f);
    if (leaf < p.layout.count[0]) {
#pragma unroll
        for (int c = 0; c < kBvhWidth; ++c) {
            const float4* r = p.records + 4ull * (static_cast<unsigned long long>(leaf) * kBvhWidth + c);
            const float4 a = r[2], b = r[3];
            lo = make_float4(fminf(lo.x, a.y), fminf(lo.y, a.z), fminf(lo.z, a.w), 0.f);
            hi = make_float4(fmaxf(hi.x, b.x), fmaxf(hi.y, b.y), fmaxf(hi.z, b.z), 0.f);
        }
        p.nodes[2ull * (p.layout.offset[0] + leaf)] = lo;
        p.nodes[2ull * (p.layout.offset[0] + leaf) + 1] = hi;
    }
    slo[tid] = lo;
    shi[tid] = hi;
    __syncthreads();
    if (p.layout.levels > 1 && tid < 256 / kBvhWidth) {
        const unsigned node = blockIdx.x * (256 / kBvhWidth) + tid;
        if (node < p.layout.count[1]) {
            float4 l = slo[tid * kBvhWidth], h = shi[tid * kBvhWidth];
#pragma unroll
            for (int c = 1; c < kBvhWidth; ++c) {
                const float4 a = slo[tid * kBvhWidth + c], b = shi[tid * kBvhWidth + c];
                l = make_float4(fminf(l.x, a.x), fminf(l.y, a.y), fminf(l.z, a.z), 0.f);
                h = make_float4(fmaxf(h.x, b.x), fmaxf(h.y, b.y), fmaxf(h.z, b.z), 0.f);
            }
            p.nodes[2ull * (p.layout.offset[1] + node)] = l;
            p.nodes[2ull * (p.layout.offset[1] + node) + 1] = h;
        }
    }
}

// Levels 2.. in one block, level by level (one workgroup: the barrier orders a level's writes
// before the next level's reads).
__global__ __launch_bounds__(1024) void RayUpperKernel(RayNodeParams p) {
    for (unsigned L = 2; L < p.layout.levels; ++L) {
        const unsigned below = p.layout.offset[L - 1], nb = p.layout.count[L - 1];
        for (unsigned i = threadIdx.x; i < p.layout.count[L]; i += blockDim.x) {
            float4 l = make_float4(__builtin_inff(), __builtin_inff(), __builtin_inff(), 0.f);
            float4 h = make_float4(-__builtin_inff(), -__builtin_inff(), -__builtin_inff(), 0.f);
            const unsigned c1 = min(nb, (i + 1) * kBvhWidth);
            for (unsigned c = i * kBvhWidth; c < c1; ++c) {
                const float4 a = p.nodes[2ull * (below + c)], b = p.nodes[2ull * (below + c) + 1];
                l = make_float4(fminf(l.x, a.x), fminf(l.y, a.y), fminf(l.z, a.z), 0.f);
                h = make_float4(fmaxf(h.x, b.x), fmaxf(h.y, b.y), fmaxf(h.z, b.z), 0.f);
            }
            p.nodes[2ull * (p.layout.offset[L] + i)] = l;
            p.nodes[2ull * (p.layout.offset[L] + i) + 1] = h;
        }
        __threadfence_block();
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// Queries
// ---------------------------------------------------------------------------------------------

struct RayQueryParams {
    const float4* __restrict__ rays;     // 2 per ray
    unsigned long long count;
    const float4* __restrict__ records;  // tree
    const float4* __restrict__ nodes;
    const float* __restrict__ vertices;  // brute force
    unsigned n;
    int* __restrict__ ids;
    float* __restrict__ t;
    float2* __restrict__ bary;           // may be null
    unsigned char* __restrict__ out;     // occlusion
};

__device__ __forceinline__ Ray LoadRay(const float4* __restrict__ rays, unsigned long long i) {
    const float4 a = rays[2 * i], b = rays[2 * i + 1];
    Ray r;
    r.o[0] = a.x;
    r.o[1] = a.y;
    r.o[2] = a.z;
    r.tmin = a.w;
    r.d[0] = b.x;
    r.d[1] = b.y;
    r.d[2] = b.z;
    r.tmax = b.w;
    return r;
}

template <bool kClosest>
__device__ __forceinline__ void StoreAnswer(const RayQueryParams& p, unsigned long long i, const RayBest& best) {
    if (kClosest) {
        p.ids[i] = best.id;
        p.t[i] = best.t;
        if (p.bary != nullptr) {
            p.bary[i] = make_float2(best.w1, best.w2);
        }
    } else {
        p.out[i] = best.id >= 0 ? 1 : 0;
    }
}

// One ray per lane, walked by RayWalk (ray_walk.h): (level, idx) and no stack. Rays of a wave diverge
// freely. The per-level counts and offsets are recomputed from n into LDS.
template <bool kClosest>
__global__ __launch_bounds__(256) void RayTreeKernel(RayQueryParams p) {
    __shared__ unsigned s_count[kBvhMaxLevels], s_offset[kBvhMaxLevels];
    __shared__ unsigned s_levels;
    if (threadIdx.x == 0) {
        RayLevelsInit(p.n, s_count, s_offset, &s_levels);
    }
    __syncthreads();
    const unsigned long long i = blockIdx.x * 256ull + threadIdx.x;
    if (i >= p.count) {
        return;
    }
    const Ray r = LoadRay(p.rays, i);
    const RayBest best = RayWalk<kClosest>(r, p.nodes, p.records, s_count, s_offset, &s_levels);
    StoreAnswer<kClosest>(p, i, best);
}

// Brute force over the scene's own vertices in ascending id (ray_walk.h RayScan): no structure.
template <bool kClosest>
__global__ __launch_bounds__(256) void RayBruteKernel(RayQueryParams p) {
    const unsigned long long i = blockIdx.x * 256ull + threadIdx.x;
    if (i >= p.count) {
        return;
    }
    const Ray r = LoadRay(p.rays, i);
    const RayBest best = RayScan<kClosest>(r, p.vertices, p.n);
    StoreAnswer<kClosest>(p, i, best);
}

template <bool kClosest>
void LaunchRays(const RayTree* tree, const float* d_vertices, std::uint64_t n, const float* d_rays, std::size_t count,
                int* d_ids, float* d_t, float* d_bary, unsigned char* d_out, hipStream_t stream) {
    if (count == 0) {
        return;
    }
    if (count > 0x7FFFFFFFull * 256ull) {
        throw std::runtime_error("Bad argument: too many rays for one call");
    }
    RayQueryParams p{};
    p.rays = reinterpret_cast<const float4*>(d_rays);
    p.count = count;
    p.records = tree != nullptr ? tree->records : nullptr;
    p.nodes = tree != nullptr ? tree->nodes : nullptr;
    p.vertices = d_vertices;
    p.n = static_cast<unsigned>(n);
    p.ids = d_ids;
    p.t = d_t;
    p.bary = reinterpret_cast<float2*>(d_bary);
    p.out = d_out;
    const dim3 grid(static_cast<unsigned>((count + 255) / 256));
    if (tree != nullptr && n != 0) {
        hipLaunchKernelGGL(RayTreeKernel<kClosest>, grid, dim3(256), 0, stream, p);
    } else {
        hipLaunchKernelGGL(RayBruteKernel<kClosest>, grid, dim3(256), 0, stream, p);  // (n == 0: misses)
    }
    Check(hipGetLastError(), "ray query launch");
}

}  // namespace

std::size_t RayTreeBytes(std::uint64_t n) {
    const BvhLayout l = MakeBvhLayout(n);
    return static_cast<std::size_t>(l.count[0]) * kBvhWidth * kRayRecordFloats * 4 +
           static_cast<std::size_t>(l.nodes) * 32 + static_cast<std::size_t>(n) * 16 + (kRayBoundBlocks + 1) * 6 * 4;
}

void FreeRayTree(RayTree& t) noexcept {
    (void)hipFree(t.records);
    (void)hipFree(t.nodes);
    (void)hipFree(t.keys);
    (void)hipFree(t.keys_sorted);
    (void)hipFree(t.ids);
    (void)hipFree(t.order);
    (void)hipFree(t.bounds);
    (void)hipFree(t.temp);
    t = RayTree{};
}

void AllocRayTree(RayTree& tree, std::uint64_t n, hipStream_t stream) {
    if (n == 0 || n > 0x7FFFFFFFull) {
        throw std::runtime_error("Ray tree: bad triangle count");
    }
    RayTree a;
    a.layout = MakeBvhLayout(n);
    try {
        Check(hipMalloc(&a.records, static_cast<std::size_t>(a.layout.count[0]) * kBvhWidth * kRayRecordFloats * 4),
              "hipMalloc(ray records)");
        Check(hipMalloc(&a.nodes, static_cast<std::size_t>(a.layout.nodes) * 32), "hipMalloc(ray nodes)");
        Check(hipMalloc(&a.keys, n * 4), "hipMalloc(ray keys)");
        Check(hipMalloc(&a.keys_sorted, n * 4), "hipMalloc(ray sorted keys)");
        Check(hipMalloc(&a.ids, n * 4), "hipMalloc(ray ids)");
        Check(hipMalloc(&a.order, n * 4), "hipMalloc(ray order)");
        Check(hipMalloc(&a.bounds, (kRayBoundBlocks + 1) * 6 * sizeof(float)), "hipMalloc(ray bounds)");
        Check(rocprim::radix_sort_pairs(nullptr, a.temp_bytes, a.keys, a.keys_sorted, a.ids, a.order,
                                        static_cast<unsigned>(n), 0, 31, stream),
              "rocprim::radix_sort_pairs (size query)");
        Check(hipMalloc(&a.temp, a.temp_bytes == 0 ? 4 : a.temp_bytes), "hipMalloc(ray sort temporary)");
    } catch (...) {
        FreeRayTree(a);
        throw;
    }
    tree = a;
}

void EnqueueRayTreeBuild(const RayTree& t, const float* d_vertices, std::uint64_t n, hipStream_t stream) {
    const unsigned un = static_cast<unsigned>(n);
    const unsigned blocks = (un + 255) / 256;
    const unsigned bound_blocks = blocks < kRayBoundBlocks ? blocks : kRayBoundBlocks;
    float* bounds = t.bounds + 6 * kRayBoundBlocks;
    hipLaunchKernelGGL(RayBoundsKernel, dim3(bound_blocks), dim3(256), 0, stream, d_vertices, un, t.bounds);
    Check(hipGetLastError(), "RayBoundsKernel launch");
    hipLaunchKernelGGL(RayBoundsFoldKernel, dim3(1), dim3(256), 0, stream, t.bounds, bound_blocks, bounds);
    Check(hipGetLastError(), "RayBoundsFoldKernel launch");
    hipLaunchKernelGGL(RayKeysKernel, dim3(blocks), dim3(256), 0, stream, d_vertices, un, bounds, t.keys, t.ids);
    Check(hipGetLastError(), "RayKeysKernel launch");
    // stable LSD radix sort: equal keys keep id order, so the order is a function of the vertices
    std::size_t temp_bytes = t.temp_bytes;
    Check(rocprim::radix_sort_pairs(t.temp, temp_bytes, t.keys, t.keys_sorted, t.ids, t.order, un, 0, 31, stream),
          "rocprim::radix_sort_pairs");
    const unsigned padded = t.layout.count[0] * kBvhWidth;
    hipLaunchKernelGGL(RayGatherKernel, dim3((padded + 255) / 256), dim3(256), 0, stream, d_vertices, un, padded, t.order,
                       t.records);
    Check(hipGetLastError(), "RayGatherKernel launch");
    RayNodeParams np{t.records, t.nodes, t.layout};
    hipLaunchKernelGGL(RayLeafKernel, dim3((t.layout.count[0] + 255) / 256), dim3(256), 0, stream, np);
    Check(hipGetLastError(), "RayLeafKernel launch");
    if (t.layout.levels > 2) {
        hipLaunchKernelGGL(RayUpperKernel, dim3(1), dim3(1024), 0, stream, np);
        Check(hipGetLastError(), "RayUpperKernel launch");
    }
}

void LaunchRayClosest(const RayTree* tree, const float* d_vertices, std::uint64_t n, const float* d_rays,
                      std::size_t count, int* d_ids, float* d_t, float* d_bary, hipStream_t stream) {
    LaunchRays<true>(tree, d_vertices, n, d_rays, count, d_ids, d_t, d_bary, nullptr, stream);
}

void LaunchRayOccluded(const RayTree* tree, const float* d_vertices, std::uint64_t n, const float* d_rays,
                       std::size_t count, unsigned char* d_out, hipStream_t stream) {
    LaunchRays<false>(tree, d_vertices, n, d_rays, count, nullptr, nullptr, nullptr, d_out, stream);
}

namespace {

// One ray against every triangle in ascending id: the definition, restated nowhere else.
RayBest HostRay(const Scene& scene, const float* ray8, bool box_clause, bool first_hit) {
    Ray r;
    std::memcpy(&r, ray8, sizeof(Ray));
    RayBest best;
    if (RayDegenerate(r)) {
        return best;
    }
    float inv[3];
    RayInverse(r, inv);
    const std::uint64_t n = scene.triangle_count();
    for (std::uint64_t k = 0; k < n; ++k) {
        const float* v = scene.vertices.data() + 9 * k;
        float plo[3], phi[3];
        if (!RayTriangleBox(v, plo, phi) || (box_clause && !RayBoxClause(r, inv, plo, phi))) {
            continue;
        }
        const RayHit h = RayEdgeTest(r, v);
        if (h.hit && RayCloser(h.t, static_cast<int>(k), best.t, best.id)) {
            best.id = static_cast<int>(k);
            best.t = h.t;
            best.w1 = h.w1;
            best.w2 = h.w2;
            if (first_hit) {
                break;
            }
        }
    }
    return best;
}

}  // namespace

static_assert(sizeof(Ray) == 32, "a ray is 8 floats");

void HostRayClosest(const Scene& scene, const float* rays, std::size_t count, int* ids, float* t, float* bary,
                    bool box_clause) {
    for (std::size_t i = 0; i < count; ++i) {
        const RayBest b = HostRay(scene, rays + 8 * i, box_clause, false);
        ids[i] = b.id;
        t[i] = b.t;
        if (bary != nullptr) {
            bary[2 * i] = b.w1;
            bary[2 * i + 1] = b.w2;
        }
    }
}

void HostRayOccluded(const Scene& scene, const float* rays, std::size_t count, unsigned char* out, bool box_clause) {
    for (std::size_t i = 0; i < count; ++i) {
        out[i] = HostRay(scene, rays + 8 * i, box_clause, true).id >= 0 ? 1 : 0;
    }
}

}  // namespace srt
