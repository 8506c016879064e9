// Sampled visibility (include/srt_visibility.h): the kernels that generate an element's S rays from
// its surface point and either export them or walk them through the scene's world-space tree and
// count the unoccluded ones, and the host answer. DESIGN.md section 2 "Visibility" defines the
// answer; section 5 describes the kernels.
//
// Every ray a kernel counts is the ray the export kernel stores, walked by the ray queries' own walk
// (ray_walk.h): the fused answer is the composition's, and tree-independent as the ray queries' is.
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "ray_walk.h"
#include "visibility.h"
#include "visibility_device.h"
#include "visibility_math.h"

namespace srt {
namespace {

void Check(hipError_t e, const char* what) {
    if (e != hipSuccess) {
        throw std::runtime_error(std::string("HIP error: ") + what + ": " + hipGetErrorString(e));
    }
}

constexpr int kModeExport = 0;  // store the rays
constexpr int kModeTree = 1;    // walk them through the tree and count
constexpr int kModeBrute = 2;   // scan the vertices for each and count

// How the fused kernels hand rays to lanes (profiles/visibility/ has the measurement):
//   0  one element per lane, its S rays one after the other (the count stays in the lane's register)
//   1  packed, element-major: the block's elements on a surface are compacted in LDS and the
//      (element, sample) pairs dealt to the 256 lanes, a lane's neighbours carrying the other samples of
//      its element
//   2  packed, sample-major: the same, a lane's neighbours carrying the same sample of the next
//      elements on a surface
// SRT_VISIBILITY_MAPPING: measurement builds.
#ifndef SRT_VISIBILITY_MAPPING
#define SRT_VISIBILITY_MAPPING 2
#endif
constexpr int kVisibilityMapping = SRT_VISIBILITY_MAPPING;
static_assert(kVisibilityMapping >= 0 && kVisibilityMapping <= 2, "SRT_VISIBILITY_MAPPING is 0, 1 or 2");

template <int MODE>
__device__ __forceinline__ bool Occluded(const VisibilityParams& p, const Ray& r, const unsigned* s_count,
                                         const unsigned* s_offset, const unsigned* s_levels) {
    if constexpr (MODE == kModeTree) {
        return RayWalk<false>(r, p.nodes, p.records, s_count, s_offset, s_levels).id >= 0;
    } else {
        return RayScan<false>(r, p.vertices, p.n).id >= 0;
    }
}

// One element per lane, its S rays one after the other. POINTS: element e = the block's 256
// consecutive ones; else the block's tile of the band. The sample table sits in LDS and is indexed by
// the loop counter, the same for every lane: without a rotation table the lanes of a wave carry one
// local direction per iteration from neighbouring surface points, and they meet again at every
// sample. The count stays in the lane's register: no cross-lane step. An element off a surface
// (steps 1 and 3) walks nothing. The export kernels (MODE == kModeExport) are this kernel: plain,
// store-bound.
template <bool POINTS, int KIND, int MODE>
__global__ __launch_bounds__(kVisibilityThreads) void VisibilityKernel(const VisibilityParams p) {
    constexpr unsigned kPer = KIND == kVisibilityHemisphere ? 3u : 2u;
    __shared__ float s_samples[kVisibilityMaxSamples * 3];
    __shared__ unsigned s_count[kBvhMaxLevels], s_offset[kBvhMaxLevels];
    __shared__ unsigned s_levels;
    const unsigned tid = threadIdx.x;
    const unsigned S = p.samples_count;
    if (KIND != kVisibilityMirror) {
        for (unsigned i = tid; i < S * kPer; i += kVisibilityThreads) {  // (S <= 64: at most 192 floats)
            s_samples[i] = p.samples[i];
        }
    }
    if (MODE == kModeTree && tid == 0) {
        RayLevelsInit(p.n, s_count, s_offset, &s_levels);
    }
    __syncthreads();
    const VisibilityElement el = ElementOf<POINTS>(p, tid);
    if (!el.in) {
        return;
    }
    const VisibilitySurface& sf = el.sf;
    float T[3] = {0.f, 0.f, 0.f}, B[3] = {0.f, 0.f, 0.f};
    float rc = 1.f, rs = 0.f;
    const bool rotate = KIND == kVisibilityHemisphere && p.rotations != nullptr;
    if (KIND == kVisibilityHemisphere && sf.valid) {
        VisibilityBasis(sf.n, T, B);
        if (rotate) {
            const float2 r = p.rotations[el.turn];
            rc = r.x;
            rs = r.y;
        }
    }
    unsigned visible = S;
    for (unsigned s = 0; s < S; ++s) {
        Ray r{};
        if (sf.valid) {
            r = RayOf<KIND>(p, s_samples, s, sf.p, sf.d, sf.n, T, B, rotate, rc, rs);
        }
        if constexpr (MODE == kModeExport) {
            float4* out = p.rays + 2ull * (s * p.count + el.e);
            out[0] = make_float4(r.o[0], r.o[1], r.o[2], r.tmin);
            out[1] = make_float4(r.d[0], r.d[1], r.d[2], r.tmax);
        } else if (sf.valid && Occluded<MODE>(p, r, s_count, s_offset, &s_levels)) {  // (a zero ray misses)
            --visible;
        }
    }
    if constexpr (MODE != kModeExport) {
        if (p.visible != nullptr) {
            p.visible[el.e] = static_cast<unsigned char>(visible);
        }
        if (p.fraction != nullptr) {
            p.fraction[el.e] = static_cast<float>(visible) / static_cast<float>(S);
        }
    }
}

// The packed mappings. Elements off a surface cost a lane nothing after their load, but with one
// element per lane they leave that lane idle through every walk of its wave. So the block first
// compacts its 256 EPT elements on a surface: each writes its point, its normal and its rotation index
// to the slot its rank among them gives it (a ballot and a popcount per wave and pass, the counts
// summed through LDS). The slots x S rays are then dealt to the 256 lanes in rounds, ray `item` to lane
// item mod 256, so every round but the last is full; EPT > 1 would make the last round a smaller share
// but measured 1.6 times slower at 2 and 2.5 times at 4 (profiles/visibility/), so the default is 1. An
// occluded ray takes one off its slot's count in LDS (an LDS atomic: S of them per slot at the most);
// after the last round every lane stores its own elements' counts. The basis is recomputed per ray
// from the slot's normal -- the same expressions, so the same bits. SAMPLE_MAJOR: item = s slots +
// slot, else item = slot S + s. SRT_VISIBILITY_ELEMENTS: measurement builds.
#ifndef SRT_VISIBILITY_ELEMENTS
#define SRT_VISIBILITY_ELEMENTS 1
#endif
constexpr unsigned kVisibilityElements = SRT_VISIBILITY_ELEMENTS;  // per thread of a packed kernel
static_assert(kVisibilityElements >= 1 && kVisibilityElements <= 4, "SRT_VISIBILITY_ELEMENTS is 1 to 4");

template <bool POINTS, int KIND, int MODE, bool SAMPLE_MAJOR>
__global__ __launch_bounds__(kVisibilityThreads) void VisibilityPackedKernel(const VisibilityParams p) {
    constexpr unsigned kPer = KIND == kVisibilityHemisphere ? 3u : 2u;
    constexpr unsigned kWaves = kVisibilityThreads / 64;
    constexpr unsigned EPT = kVisibilityElements;
    constexpr unsigned kSlots = kVisibilityThreads * EPT;
    __shared__ float s_samples[kVisibilityMaxSamples * 3];
    __shared__ float2 s_turns[kVisibilityRotations];
    __shared__ unsigned s_count[kBvhMaxLevels], s_offset[kBvhMaxLevels];
    __shared__ unsigned s_levels;
    __shared__ float s_surface[6][kSlots];  // p.xyz, n.xyz by slot
    __shared__ unsigned s_left[kSlots];     // the slot's count, its rotation index above bit 8
    __shared__ unsigned s_wave[EPT][kWaves];
    const unsigned tid = threadIdx.x;
    const unsigned S = p.samples_count;
    const bool rotate = KIND == kVisibilityHemisphere && p.rotations != nullptr;
    for (unsigned i = tid; i < S * kPer; i += kVisibilityThreads) {
        s_samples[i] = p.samples[i];
    }
    if (rotate && tid < kVisibilityRotations) {
        s_turns[tid] = p.rotations[tid];
    }
    if (MODE == kModeTree && tid == 0) {
        RayLevelsInit(p.n, s_count, s_offset, &s_levels);
    }
    const unsigned wave = tid / 64, lane = tid & 63u;
    VisibilityElement el[EPT];
    unsigned rank[EPT];
#pragma unroll
    for (unsigned k = 0; k < EPT; ++k) {
        el[k] = ElementOf<POINTS, EPT>(p, tid, k);
        const unsigned long long ballot = __ballot(el[k].in && el[k].sf.valid);
        rank[k] = static_cast<unsigned>(__popcll(ballot & ((1ull << lane) - 1ull)));
        if (lane == 0) {
            s_wave[k][wave] = static_cast<unsigned>(__popcll(ballot));
        }
    }
    __syncthreads();
    unsigned slots = 0;
#pragma unroll
    for (unsigned k = 0; k < EPT; ++k) {
#pragma unroll
        for (unsigned w = 0; w < kWaves; ++w) {
            if (w == wave) {
                rank[k] += slots;  // (the elements on a surface before this wave's of pass k)
            }
            slots += s_wave[k][w];
        }
    }
#pragma unroll
    for (unsigned k = 0; k < EPT; ++k) {
        if (el[k].in && el[k].sf.valid) {
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                s_surface[j][rank[k]] = el[k].sf.p[j];
                s_surface[3 + j][rank[k]] = el[k].sf.n[j];
            }
            s_left[rank[k]] = S | (el[k].turn << 8);
        }
    }
    __syncthreads();
    const unsigned items = slots * S;  // (<= 1024 x 64)
    for (unsigned item = tid; item < items; item += kVisibilityThreads) {
        const unsigned hi = item / (SAMPLE_MAJOR ? slots : S);
        const unsigned lo = item - hi * (SAMPLE_MAJOR ? slots : S);
        const unsigned at = SAMPLE_MAJOR ? lo : hi, s = SAMPLE_MAJOR ? hi : lo;
        const float pt[3] = {s_surface[0][at], s_surface[1][at], s_surface[2][at]};
        const float n[3] = {s_surface[3][at], s_surface[4][at], s_surface[5][at]};
        float T[3] = {0.f, 0.f, 0.f}, B[3] = {0.f, 0.f, 0.f};
        float2 turn = make_float2(1.f, 0.f);
        if constexpr (KIND == kVisibilityHemisphere) {
            VisibilityBasis(n, T, B);
            if (rotate) {
                turn = s_turns[(s_left[at] >> 8) & (kVisibilityRotations - 1)];
            }
        }
        const Ray r = RayOf<KIND>(p, s_samples, s, pt, pt, n, T, B, rotate, turn.x, turn.y);
        if (Occluded<MODE>(p, r, s_count, s_offset, &s_levels)) {
            atomicSub(&s_left[at], 1u);
        }
    }
    __syncthreads();
#pragma unroll
    for (unsigned k = 0; k < EPT; ++k) {
        if (!el[k].in) {
            continue;
        }
        const unsigned visible = el[k].sf.valid ? (s_left[rank[k]] & 0xFFu) : S;
        if (p.visible != nullptr) {
            p.visible[el[k].e] = static_cast<unsigned char>(visible);
        }
        if (p.fraction != nullptr) {
            p.fraction[el[k].e] = static_cast<float>(visible) / static_cast<float>(S);
        }
    }
}

template <bool POINTS, int MODE>
void LaunchKind(const VisibilityParams& p, int kind, dim3 grid, hipStream_t stream) {
    const dim3 block(kVisibilityThreads);
    if constexpr (MODE != kModeExport && kVisibilityMapping != 0) {
        constexpr bool kSampleMajor = kVisibilityMapping == 2;
        if (kind == kVisibilityHemisphere) {
            hipLaunchKernelGGL((VisibilityPackedKernel<POINTS, kVisibilityHemisphere, MODE, kSampleMajor>), grid, block, 0,
                               stream, p);
        } else if (kind == kVisibilityArea) {
            hipLaunchKernelGGL((VisibilityPackedKernel<POINTS, kVisibilityArea, MODE, kSampleMajor>), grid, block, 0,
                               stream, p);
        } else {
            throw std::runtime_error("Visibility: the mirror generator is export only");
        }
    } else if (kind == kVisibilityHemisphere) {
        hipLaunchKernelGGL((VisibilityKernel<POINTS, kVisibilityHemisphere, MODE>), grid, block, 0, stream, p);
    } else if (kind == kVisibilityArea) {
        hipLaunchKernelGGL((VisibilityKernel<POINTS, kVisibilityArea, MODE>), grid, block, 0, stream, p);
    } else if constexpr (MODE == kModeExport) {
        hipLaunchKernelGGL((VisibilityKernel<POINTS, kVisibilityMirror, MODE>), grid, block, 0, stream, p);
    } else {
        throw std::runtime_error("Visibility: the mirror generator is export only");
    }
}

template <int MODE>
void Launch(VisibilityParams p, const Frame& frame, const VisibilityElements& e, const VisibilityGen& gen,
            hipStream_t stream) {
    if (static_cast<unsigned long long>(e.width) * e.rows == 0) {
        return;
    }
    // (a packed kernel's block takes kVisibilityElements passes of 256 elements)
    constexpr unsigned kPasses = MODE != kModeExport && kVisibilityMapping != 0 ? kVisibilityElements : 1u;
    const dim3 grid = FillVisibility(p, frame, e, gen, kPasses);
    if (e.points) {
        LaunchKind<true, MODE>(p, gen.kind, grid, stream);
    } else {
        LaunchKind<false, MODE>(p, gen.kind, grid, stream);
    }
    Check(hipGetLastError(), "visibility launch");
}

}  // namespace

dim3 FillVisibility(VisibilityParams& p, const Frame& frame, const VisibilityElements& e, const VisibilityGen& gen,
                    unsigned passes) {
    const unsigned long long count = static_cast<unsigned long long>(e.width) * e.rows;
    if (e.width > 0x7FFFFFFFull * kVisibilityThreads || (!e.points && e.width > 0x7FFFFFFFull) || e.rows > 0x7FFFFFFFull) {
        throw std::runtime_error("Bad argument: too many elements for one call");
    }
    p.where = reinterpret_cast<const float2*>(e.where);
    p.ids = e.ids;
    p.samples = gen.samples;
    p.rotations = reinterpret_cast<const float2*>(gen.rotations);
    p.count = count;
    p.rows = static_cast<unsigned>(e.rows);
    p.row_begin = static_cast<unsigned>(e.row_begin);
    p.samples_count = gen.count;
    p.wf = static_cast<float>(e.frame_width);
    p.hf = static_cast<float>(e.frame_height);
    std::memcpy(p.eye, frame.origin, sizeof p.eye);
    std::memcpy(p.base, frame.base, sizeof p.base);
    std::memcpy(p.du, frame.du, sizeof p.du);
    std::memcpy(p.dv, frame.dv, sizeof p.dv);
    std::memcpy(p.corner, gen.corner, sizeof p.corner);
    std::memcpy(p.eu, gen.eu, sizeof p.eu);
    std::memcpy(p.ev, gen.ev, sizeof p.ev);
    p.tmin = gen.tmin;
    p.tmax = gen.tmax;
    if (e.points) {
        p.width = 0;  // (unused)
        p.tiles_x = 1;
        const unsigned long long per_block = static_cast<unsigned long long>(kVisibilityThreads) * passes;
        return dim3(static_cast<unsigned>((count + per_block - 1) / per_block));
    }
    p.width = static_cast<unsigned>(e.width);
    p.tiles_x = (p.width + kVisibilityTileW - 1) / kVisibilityTileW;
    const unsigned tile_rows = kVisibilityTileH * passes;
    const unsigned long long tiles = static_cast<unsigned long long>(p.tiles_x) * ((p.rows + tile_rows - 1) / tile_rows);
    if (tiles > 0x7FFFFFFFull) {
        throw std::runtime_error("Bad argument: too many elements for one call");
    }
    return dim3(static_cast<unsigned>(tiles));
}

void LaunchVisibility(const RayTree* tree, const float* d_vertices, std::uint64_t n, const Frame& frame,
                      const VisibilityElements& e, const VisibilityGen& gen, unsigned char* d_visible,
                      float* d_fraction, hipStream_t stream) {
    VisibilityParams p{};
    p.vertices = d_vertices;
    p.n = static_cast<unsigned>(n);
    p.visible = d_visible;
    p.fraction = d_fraction;
    if (tree != nullptr && n != 0) {
        p.nodes = tree->nodes;
        p.records = tree->records;
        Launch<kModeTree>(p, frame, e, gen, stream);
    } else {
        Launch<kModeBrute>(p, frame, e, gen, stream);  // (n == 0: every element is off a surface)
    }
}

void LaunchVisibilityRays(const float* d_vertices, std::uint64_t n, const Frame& frame, const VisibilityElements& e,
                          const VisibilityGen& gen, float* d_rays, hipStream_t stream) {
    VisibilityParams p{};
    p.vertices = d_vertices;
    p.n = static_cast<unsigned>(n);
    p.rays = reinterpret_cast<float4*>(d_rays);
    Launch<kModeExport>(p, frame, e, gen, stream);
}

void HostVisibilityRays(const Scene& scene, std::size_t width, std::size_t height, const float* positions,
                        const int* ids, std::size_t count, const VisibilityGen& gen, float* rays) {
    if (width == 0 || height == 0) {
        throw std::runtime_error("Host visibility: frame dimensions must be non-zero");
    }
    const Frame f = MakeFrame(scene.camera, width, height);
    const std::size_t n = scene.triangle_count();
    for (std::size_t q = 0; q < count; ++q) {
        const int id = ids[q];
        VisibilitySurface sf{};
        if (id >= 0 && static_cast<std::size_t>(id) < n) {
            sf = VisibilitySurfaceAt(f.origin, f.base, f.du, f.dv, scene.vertices.data() + 9 * static_cast<std::size_t>(id),
                                     positions[2 * q], positions[2 * q + 1]);
        }
        float T[3] = {0.f, 0.f, 0.f}, B[3] = {0.f, 0.f, 0.f};
        float rc = 1.f, rs = 0.f;
        const bool rotate = gen.kind == kVisibilityHemisphere && gen.rotations != nullptr;
        if (gen.kind == kVisibilityHemisphere && sf.valid) {
            VisibilityBasis(sf.n, T, B);
            if (rotate) {
                const std::size_t turn = q & (kVisibilityRotations - 1);
                rc = gen.rotations[2 * turn];
                rs = gen.rotations[2 * turn + 1];
            }
        }
        for (unsigned s = 0; s < gen.count; ++s) {
            Ray r{};
            if (sf.valid) {
                if (gen.kind == kVisibilityHemisphere) {
                    const float* l = gen.samples + 3 * s;
                    VisibilityHemisphereDir(sf.n, T, B, l[0], l[1], l[2], rotate, rc, rs, r.d);
                } else if (gen.kind == kVisibilityArea) {
                    VisibilityAreaDir(gen.corner, gen.eu, gen.ev, gen.samples[2 * s], gen.samples[2 * s + 1], sf.p, r.d);
                } else {
                    VisibilityMirrorDir(sf.d, sf.n, r.d);
                }
                for (int k = 0; k < 3; ++k) {
                    r.o[k] = sf.p[k];
                }
                r.tmin = gen.tmin;
                r.tmax = gen.tmax;
            }
            std::memcpy(rays + 8 * (static_cast<std::size_t>(s) * count + q), &r, sizeof r);
        }
    }
}

void HostVisibility(const Scene& scene, std::size_t width, std::size_t height, const float* positions, const int* ids,
                    std::size_t count, const VisibilityGen& gen, unsigned char* visible, float* fraction) {
    if (visible == nullptr && fraction == nullptr) {
        return;  // (no plane: nothing is read either)
    }
    std::vector<float> rays(static_cast<std::size_t>(gen.count) * count * 8);
    HostVisibilityRays(scene, width, height, positions, ids, count, gen, rays.data());
    std::vector<unsigned char> occluded(static_cast<std::size_t>(gen.count) * count);
    HostRayOccluded(scene, rays.data(), occluded.size(), occluded.data(), true);
    for (std::size_t q = 0; q < count; ++q) {
        unsigned v = 0;
        for (unsigned s = 0; s < gen.count; ++s) {
            v += occluded[static_cast<std::size_t>(s) * count + q] == 0 ? 1u : 0u;
        }
        if (visible != nullptr) {
            visible[q] = static_cast<unsigned char>(v);
        }
        if (fraction != nullptr) {
            fraction[q] = static_cast<float>(v) / static_cast<float>(gen.count);
        }
    }
}

}  // namespace srt
