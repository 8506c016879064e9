// MI355X (gfx950) per-element output kernels: the G-buffer, surface, interpolate and resolve passes,
// which read hit ids and walk nothing (render.h LaunchGBuffer .. LaunchResolve). Built as render.hip is:
// -ffp-contract=off, every fused multiply-add an explicit fmaf.
#include "render.h"
#include "gbuffer_math.h"
#include "samples_math.h"
#include "surface_math.h"
#include "trace_device.h"

namespace srt {

namespace {

// ---------------------------------------------------------------------------------------
// G-buffer (render.h LaunchGBuffer; DESIGN.md section 5 "G-buffer"): the surface attributes of
// (position, hit id) pairs -- ShadeIdsKernel's deferred pass with more outputs. POINTS: element k's
// position is read from `where`; else element (x, y) is pixel (x, row_begin + y) of the frame and its
// position is ray generation's expression of its sample offset (as ShadeIdsKernel). The elements
// form rows of `width` (points: one row of count); a block takes kGBufferThreads * PPT consecutive
// elements of one row, a thread PPT of them kGBufferThreads apart, so every wave instruction loads
// and stores consecutive elements. Three phases with no control flow that depends on loaded data
// between the loads: (1) every element's id and position, (2) every element's gather -- the
// triangle's 9 vertex floats (skipped when neither depth nor bary is asked for) and its shading
// table row (skipped without normal and albedo), an id outside the scene gathers triangle 0's,
// unused --, (3) the arithmetic (ComputeEdges + gbuffer_math.h) and the nontemporal stores of the
// planes asked for (uniform branches). No LDS, no atomics, no scratch.
// Elements per thread, measured at C3 (1 / 2 / 4 / 8: DESIGN.md; profiles/gbuffer/): a launch that
// needs one of the two gathers is fastest with 4 (depth only 23.1 / 18.9 / 15.4 / 17.7 us), one that
// needs both with 8 (all planes 35.8 / 35.0 / 33.3 / 28.8 us: 184 VGPRs, two waves per SIMD, and
// twice the loads in flight per wave). SRT_GBUFFER_PIXELS, SRT_GBUFFER_PIXELS_BOTH: measurement builds.
// ---------------------------------------------------------------------------------------
#ifndef SRT_GBUFFER_PIXELS
#define SRT_GBUFFER_PIXELS 4
#endif
#ifndef SRT_GBUFFER_PIXELS_BOTH
#define SRT_GBUFFER_PIXELS_BOTH 8
#endif
constexpr int kGBufferPixels = SRT_GBUFFER_PIXELS;           // elements per thread, one gather
constexpr int kGBufferPixelsBoth = SRT_GBUFFER_PIXELS_BOTH;  // ... both gathers
constexpr int kGBufferThreads = 256;
typedef float F2 __attribute__((ext_vector_type(2)));
struct GBufferParams {
    const float* __restrict__ vertices;
    const float4* __restrict__ shade;
    const float2* __restrict__ where;  // positions (POINTS) or sample offsets
    const int* __restrict__ ids;
    float* __restrict__ depth;
    F2* __restrict__ bary;
    F4* __restrict__ normal;
    F4* __restrict__ albedo;
    unsigned n;
    unsigned width;   // elements per row
    unsigned chunks;  // blocks per row
    unsigned row_begin;
    float wf, hf;
    float eye[3], base[3], du[3], dv[3], bg[3];
};

template <bool POINTS, int PPT>
__global__ __launch_bounds__(kGBufferThreads) void GBufferKernel(const GBufferParams q) {
    const unsigned row = POINTS ? 0u : blockIdx.x / q.chunks;  // (uniform: scalar)
    const unsigned chunk = blockIdx.x - row * q.chunks;
    const unsigned x0 = chunk * (kGBufferThreads * PPT) + threadIdx.x;
    const size_t row_at = static_cast<size_t>(row) * q.width;
    const bool edges = q.depth != nullptr || q.bary != nullptr;
    const bool table = q.normal != nullptr || q.albedo != nullptr;
    // (1) An element past the row loads the row's last one and is not stored.
    int code[PPT];
    float2 w[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const unsigned x = min(x0 + k * kGBufferThreads, q.width - 1u);
        code[k] = __builtin_nontemporal_load(q.ids + row_at + x);
        w[k] = q.where[row_at + x];
    }
    // (2)
    int hit[PPT];
    float v[PPT][9];
    float4 nr[PPT], al[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        hit[k] = static_cast<unsigned>(code[k]) < q.n ? code[k] : -1;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            v[k][j] = 0.f;
        }
        nr[k] = al[k] = float4{};
    }
    if (q.n != 0u) {  // (an empty scene has no triangle 0)
        if (edges) {
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                const float* at = q.vertices + 9ull * static_cast<unsigned>(max(hit[k], 0));
#pragma unroll
                for (int j = 0; j < 9; ++j) {
                    v[k][j] = at[j];
                }
            }
        }
        if (table) {
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                const float4* sr = q.shade + 2ull * static_cast<unsigned>(max(hit[k], 0));
                nr[k] = sr[0];
                al[k] = sr[1];
            }
        }
    }
    // (3)
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const unsigned x = x0 + k * kGBufferThreads;
        if (x >= q.width) {
            continue;
        }
        float fx = w[k].x, fy = w[k].y;
        if constexpr (!POINTS) {
            fx = (static_cast<float>(x) + w[k].x) / q.wf;
            fy = (static_cast<float>(q.row_begin + row) + w[k].y) / q.hf;
        }
        GBufferTexel o = GBufferMiss(q.bg);
        if (hit[k] >= 0) {
            float c[9], vol;
            ComputeEdges(q.eye, q.base, q.du, q.dv, v[k], true, c, vol);
            o = GBufferHit(c, vol, q.base, q.du, q.dv, fx, fy, hit[k], nr[k].x, nr[k].y, nr[k].z, nr[k].w, al[k].x,
                           al[k].y, al[k].z);
        }
        const size_t at = row_at + x;
        if (q.depth != nullptr) {
            __builtin_nontemporal_store(o.depth, q.depth + at);
        }
        if (q.bary != nullptr) {
            __builtin_nontemporal_store(F2{o.w1, o.w2}, q.bary + at);
        }
        if (q.normal != nullptr) {
            StoreNontemporal(q.normal + at, F4{o.nx, o.ny, o.nz, o.cosv});
        }
        if (q.albedo != nullptr) {
            StoreNontemporal(q.albedo + at, F4{o.r, o.g, o.b, o.a});
        }
    }
}

// ---------------------------------------------------------------------------------------
// Vertex attributes (render.h LaunchSurface / LaunchInterpolate; DESIGN.md section 5 "Vertex
// attributes"): what the surface looks like at (position, hit id) pairs -- GBufferKernel's deferred
// pass with the caller's per-triangle corner tables interpolated at the hit point and a texture
// looked up there. Element mapping as GBufferKernel's: a block takes kSurfaceThreads * PPT
// consecutive elements of one row, a thread PPT of them kSurfaceThreads apart. Four phases with no
// control flow that depends on loaded data between a phase's loads: (1) every element's id and
// position, (2) every element's by-id gathers, each behind a uniform branch on what the call
// needs -- the vertex row (36 B: the weights), the shading table row (32 B: the geometric normal
// and the scene's albedo), the normals row (36 B), the uvs row (24 B); an id outside the scene
// gathers triangle 0's, unused --, (3) the weights (ComputeEdges + surface_math.h), the uv and the
// texel gathers (four float4 taps, one with the nearest filter: the second dependent chain; the
// taps are in range whatever the uv, surface_math.h), (4) the arithmetic and the nontemporal
// stores of the planes asked for. No LDS, no atomics, no scratch.
// Elements per thread, measured at C3 with random tables (1 / 2 / 4: DESIGN.md; profiles/surface/):
// normal + albedo 50.3 / 49.4 / 50.0 us with a 64 KB texture, 93.1 / 98.9 / 96.2 us with a 16 MB one --
// the pass is bound by its two dependent round trips, not by chains per wave or waves; 2 keeps 5 waves
// per SIMD at 94 VGPRs. SRT_SURFACE_PIXELS: measurement builds.
// ---------------------------------------------------------------------------------------
#ifndef SRT_SURFACE_PIXELS
#define SRT_SURFACE_PIXELS 2
#endif
constexpr int kSurfacePixels = SRT_SURFACE_PIXELS;
constexpr int kSurfaceThreads = 256;
constexpr int kInterpolatePixels = 4;  // (GBufferKernel's figure for one 36 B gather plus one more row)
struct SurfaceParams {
    const float* __restrict__ vertices;
    const float4* __restrict__ shade;
    const float2* __restrict__ where;  // positions (POINTS) or sample offsets
    const int* __restrict__ ids;
    const float* __restrict__ normals;
    const float* __restrict__ uvs;
    const float4* __restrict__ texture;
    F4* __restrict__ normal;
    F4* __restrict__ albedo;
    F4* __restrict__ rgba;
    F2* __restrict__ uv;
    unsigned n;
    unsigned width;   // elements per row
    unsigned chunks;  // blocks per row
    unsigned row_begin;
    int tw, th;
    unsigned flags;
    float wf, hf;
    float eye[3], base[3], du[3], dv[3], bg[3];
};

template <bool POINTS, int PPT>
__global__ __launch_bounds__(kSurfaceThreads) void SurfaceKernel(const SurfaceParams q) {
    const unsigned row = POINTS ? 0u : blockIdx.x / q.chunks;  // (uniform: scalar)
    const unsigned chunk = blockIdx.x - row * q.chunks;
    const unsigned x0 = chunk * (kSurfaceThreads * PPT) + threadIdx.x;
    const size_t row_at = static_cast<size_t>(row) * q.width;
    // What the call needs (uniform).
    const bool out_n = q.normal != nullptr || q.rgba != nullptr;
    const bool out_a = q.albedo != nullptr || q.rgba != nullptr;
    const bool smooth = q.normals != nullptr && out_n;
    const bool textured = q.texture != nullptr && out_a;
    const bool modulate = (q.flags & kSurfaceModulate) != 0u;
    const bool clamp = (q.flags & kSurfaceWrapClamp) != 0u;
    const bool nearest = (q.flags & kSurfaceFilterNearest) != 0u;
    const bool coords = q.uvs != nullptr && (q.uv != nullptr || textured);
    const bool weights = smooth || coords;
    const bool table = (out_n && !smooth) || (out_a && (!textured || modulate));
    // (1) An element past the row loads the row's last one and is not stored.
    int code[PPT];
    float2 w[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const unsigned x = min(x0 + k * kSurfaceThreads, q.width - 1u);
        code[k] = __builtin_nontemporal_load(q.ids + row_at + x);
        w[k] = q.where[row_at + x];
    }
    // (2)
    int hit[PPT];
    float v[PPT][9], cn[PPT][9], ct[PPT][6];
    float4 nr[PPT], al[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        hit[k] = static_cast<unsigned>(code[k]) < q.n ? code[k] : -1;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            v[k][j] = cn[k][j] = 0.f;
        }
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            ct[k][j] = 0.f;
        }
        nr[k] = al[k] = float4{};
    }
    if (q.n != 0u) {  // (an empty scene has no triangle 0)
        if (weights) {
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                const float* at = q.vertices + 9ull * static_cast<unsigned>(max(hit[k], 0));
#pragma unroll
                for (int j = 0; j < 9; ++j) {
                    v[k][j] = at[j];
                }
            }
        }
        if (table) {
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                const float4* sr = q.shade + 2ull * static_cast<unsigned>(max(hit[k], 0));
                nr[k] = sr[0];
                al[k] = sr[1];
            }
        }
        if (smooth) {
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                const float* at = q.normals + 9ull * static_cast<unsigned>(max(hit[k], 0));
#pragma unroll
                for (int j = 0; j < 9; ++j) {
                    cn[k][j] = at[j];
                }
            }
        }
        if (coords) {
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                const float* at = q.uvs + 6ull * static_cast<unsigned>(max(hit[k], 0));
#pragma unroll
                for (int j = 0; j < 6; ++j) {
                    ct[k][j] = at[j];
                }
            }
        }
    }
    // (3)
    float fx[PPT], fy[PPT];
    SurfaceWeights bw[PPT];
    float tu[PPT], tv[PPT], ta[PPT], tb[PPT];
    float4 t00[PPT], t01[PPT], t10[PPT], t11[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        fx[k] = w[k].x;
        fy[k] = w[k].y;
        if constexpr (!POINTS) {
            const unsigned x = min(x0 + k * kSurfaceThreads, q.width - 1u);
            fx[k] = (static_cast<float>(x) + w[k].x) / q.wf;
            fy[k] = (static_cast<float>(q.row_begin + row) + w[k].y) / q.hf;
        }
        bw[k] = SurfaceWeights{0.f, 0.f, 0.f};
        if (weights) {
            float c[9], vol;
            ComputeEdges(q.eye, q.base, q.du, q.dv, v[k], true, c, vol);
            bw[k] = SurfaceBary(c, fx[k], fy[k]);
        }
        tu[k] = tv[k] = 0.f;  // (without a uvs table: (0, 0))
        if (coords) {
            tu[k] = SurfaceMix(bw[k], ct[k][0], ct[k][2], ct[k][4]);
            tv[k] = SurfaceMix(bw[k], ct[k][1], ct[k][3], ct[k][5]);
        }
        ta[k] = tb[k] = 0.f;
        t00[k] = t01[k] = t10[k] = t11[k] = float4{};
    }
    if (textured) {
        if (nearest) {
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                const int i = SurfaceNearest(SurfaceWrap(tu[k], clamp), q.tw);
                const int j = SurfaceNearest(SurfaceWrap(tv[k], clamp), q.th);
                t00[k] = q.texture[static_cast<size_t>(j) * static_cast<unsigned>(q.tw) + static_cast<unsigned>(i)];
            }
        } else {
#pragma unroll
            for (int k = 0; k < PPT; ++k) {
                const SurfaceTaps sx = SurfaceBilinear(SurfaceWrap(tu[k], clamp), q.tw, clamp);
                const SurfaceTaps sy = SurfaceBilinear(SurfaceWrap(tv[k], clamp), q.th, clamp);
                const float4* top = q.texture + static_cast<size_t>(sy.i0) * static_cast<unsigned>(q.tw);
                const float4* bot = q.texture + static_cast<size_t>(sy.i1) * static_cast<unsigned>(q.tw);
                t00[k] = top[sx.i0];
                t01[k] = top[sx.i1];
                t10[k] = bot[sx.i0];
                t11[k] = bot[sx.i1];
                ta[k] = sx.a;
                tb[k] = sy.a;
            }
        }
    }
    // (4)
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const unsigned x = x0 + k * kSurfaceThreads;
        if (x >= q.width) {
            continue;
        }
        F4 on{0.f, 0.f, 0.f, 1.f}, oa{q.bg[0], q.bg[1], q.bg[2], -1.f};
        F2 ouv{0.f, 0.f};
        if (hit[k] >= 0) {
            if (smooth) {
                const SurfaceNormal s = SurfaceSmoothNormal(
                    SurfaceMix(bw[k], cn[k][0], cn[k][3], cn[k][6]), SurfaceMix(bw[k], cn[k][1], cn[k][4], cn[k][7]),
                    SurfaceMix(bw[k], cn[k][2], cn[k][5], cn[k][8]), q.base, q.du, q.dv, fx[k], fy[k]);
                on = F4{s.x, s.y, s.z, s.cosv};
            } else {
                const float none[9] = {};  // (the geometric normal needs no edge record)
                const GBufferTexel g = GBufferHit(none, 0.f, q.base, q.du, q.dv, fx[k], fy[k], hit[k], nr[k].x, nr[k].y,
                                                  nr[k].z, nr[k].w, al[k].x, al[k].y, al[k].z);
                on = F4{g.nx, g.ny, g.nz, g.cosv};
            }
            float r = al[k].x, g = al[k].y, b = al[k].z;
            if (textured) {
                float tr = t00[k].x, tg = t00[k].y, tbl = t00[k].z;
                if (!nearest) {
                    tr = SurfaceLerp(SurfaceLerp(t00[k].x, t01[k].x, ta[k]), SurfaceLerp(t10[k].x, t11[k].x, ta[k]), tb[k]);
                    tg = SurfaceLerp(SurfaceLerp(t00[k].y, t01[k].y, ta[k]), SurfaceLerp(t10[k].y, t11[k].y, ta[k]), tb[k]);
                    tbl = SurfaceLerp(SurfaceLerp(t00[k].z, t01[k].z, ta[k]), SurfaceLerp(t10[k].z, t11[k].z, ta[k]), tb[k]);
                }
                r = modulate ? tr * r : tr;
                g = modulate ? tg * g : tg;
                b = modulate ? tbl * b : tbl;
            }
            oa = F4{r, g, b, static_cast<float>(hit[k])};
            ouv = F2{tu[k], tv[k]};
        }
        const size_t at = row_at + x;
        if (q.normal != nullptr) {
            StoreNontemporal(q.normal + at, on);
        }
        if (q.albedo != nullptr) {
            StoreNontemporal(q.albedo + at, oa);
        }
        if (q.rgba != nullptr) {
            StoreNontemporal(q.rgba + at, F4{oa.x * on.w, oa.y * on.w, oa.z * on.w, oa.w});
        }
        if (q.uv != nullptr) {
            __builtin_nontemporal_store(ouv, q.uv + at);
        }
    }
}

// The interpolation of one corner table of C floats per corner: SurfaceKernel's phases (1), (2)
// with the vertex row and the table's row (12 C bytes), and the weights and the mix.
struct InterpolateParams {
    const float* __restrict__ vertices;
    const float2* __restrict__ where;
    const int* __restrict__ ids;
    const float* __restrict__ table;
    float* __restrict__ out;
    unsigned n;
    unsigned width;
    unsigned chunks;
    unsigned row_begin;
    float wf, hf;
    float eye[3], base[3], du[3], dv[3];
};

template <bool POINTS, int C>
__global__ __launch_bounds__(kSurfaceThreads) void InterpolateKernel(const InterpolateParams q) {
    constexpr int PPT = kInterpolatePixels;
    const unsigned row = POINTS ? 0u : blockIdx.x / q.chunks;  // (uniform: scalar)
    const unsigned chunk = blockIdx.x - row * q.chunks;
    const unsigned x0 = chunk * (kSurfaceThreads * PPT) + threadIdx.x;
    const size_t row_at = static_cast<size_t>(row) * q.width;
    int code[PPT];
    float2 w[PPT];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const unsigned x = min(x0 + k * kSurfaceThreads, q.width - 1u);
        code[k] = __builtin_nontemporal_load(q.ids + row_at + x);
        w[k] = q.where[row_at + x];
    }
    int hit[PPT];
    float v[PPT][9], a[PPT][3 * C];
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        hit[k] = static_cast<unsigned>(code[k]) < q.n ? code[k] : -1;
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            v[k][j] = 0.f;
        }
#pragma unroll
        for (int j = 0; j < 3 * C; ++j) {
            a[k][j] = 0.f;
        }
    }
    if (q.n != 0u) {
#pragma unroll
        for (int k = 0; k < PPT; ++k) {
            const float* at = q.vertices + 9ull * static_cast<unsigned>(max(hit[k], 0));
            const float* ta = q.table + static_cast<size_t>(3 * C) * static_cast<unsigned>(max(hit[k], 0));
#pragma unroll
            for (int j = 0; j < 9; ++j) {
                v[k][j] = at[j];
            }
#pragma unroll
            for (int j = 0; j < 3 * C; ++j) {
                a[k][j] = ta[j];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < PPT; ++k) {
        const unsigned x = x0 + k * kSurfaceThreads;
        if (x >= q.width) {
            continue;
        }
        float fx = w[k].x, fy = w[k].y;
        if constexpr (!POINTS) {
            fx = (static_cast<float>(x) + w[k].x) / q.wf;
            fy = (static_cast<float>(q.row_begin + row) + w[k].y) / q.hf;
        }
        float o[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            o[c] = 0.f;
        }
        if (hit[k] >= 0) {
            float e[9], vol;
            ComputeEdges(q.eye, q.base, q.du, q.dv, v[k], true, e, vol);
            const SurfaceWeights bw = SurfaceBary(e, fx, fy);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                o[c] = SurfaceMix(bw, a[k][c], a[k][C + c], a[k][2 * C + c]);
            }
        }
        float* at = q.out + (row_at + x) * C;
        if constexpr (C == 4) {
            StoreNontemporal(reinterpret_cast<F4*>(at), F4{o[0], o[1], o[2], o[3]});
        } else if constexpr (C == 2) {
            __builtin_nontemporal_store(F2{o[0], o[1]}, reinterpret_cast<F2*>(at));
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                __builtin_nontemporal_store(o[c], at + c);
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// Resolve (render.h LaunchResolve; DESIGN.md section 5 "Multi-sample frames"): one RGBA pixel from
// S sample planes -- S hit ids and S sample offsets per pixel in, the mean of the S shaded samples
// and the coverage out (samples_math.h), instead of S RGBA frames written, read back and averaged.
// The 2 x kMaxSamples plane pointers are kernel arguments. Element mapping as GBufferKernel's: a
// block takes kResolveThreads consecutive pixels of one band row, a thread one pixel, so every wave
// instruction loads consecutive ids and offsets and stores consecutive pixels. The samples are
// taken in groups of G, each group in three phases with no control flow that depends on loaded data
// between its loads: (1) the group's ids and offsets, (2) the group's shading table rows (an id
// outside the scene gathers row 0, unused), (3) the arithmetic, strictly in ascending s. A thread
// has G dependent chains (id -> table row) in flight. The samples that do not fill a group of G are
// taken in groups of G / 2, G / 4, ... 1 (S = 9, G = 8: a group of 8 and one of 1; loading a padded
// last group's planes twice cost S = 1 at G = 4 27.0 us against 19.4 at G = 1). No LDS, no atomics,
// no scratch.
// G, measured at C3 (1 / 2 / 4 / 8: DESIGN.md; profiles/samples/): 8 is fastest from S = 8 on (S = 8
// 68.5 / 59.2 / 55.9 / 52.8 us, S = 16 128.0 / 106.9 / 103.2 / 99.4 us: 106 VGPRs, four waves per SIMD,
// twice the loads in flight per wave), 4 below it (S = 4 40.7 / 35.9 / 33.4 / 36.5 us: 62 VGPRs, eight
// waves, and no group of 8 to fill). SRT_RESOLVE_GROUP, SRT_RESOLVE_GROUP_LONG: measurement builds.
// ---------------------------------------------------------------------------------------
#ifndef SRT_RESOLVE_GROUP
#define SRT_RESOLVE_GROUP 4
#endif
#ifndef SRT_RESOLVE_GROUP_LONG
#define SRT_RESOLVE_GROUP_LONG 8
#endif
constexpr int kResolveGroup = SRT_RESOLVE_GROUP;           // samples per group, S < kResolveLong
constexpr int kResolveGroupLong = SRT_RESOLVE_GROUP_LONG;  // ... S >= kResolveLong
constexpr unsigned kResolveLong = 8;
constexpr int kResolveThreads = 256;
static_assert(kResolveGroup >= 1 && (kResolveGroup & (kResolveGroup - 1)) == 0 && kResolveGroupLong >= 1 &&
                  (kResolveGroupLong & (kResolveGroupLong - 1)) == 0,
              "groups halve down to 1");
struct ResolveParams {
    const float2* offsets[kMaxSamples];
    const int* ids[kMaxSamples];
    const float4* __restrict__ shade;
    F4* __restrict__ out;
    unsigned n;
    unsigned samples;
    unsigned width;
    unsigned chunks;  // blocks per row
    unsigned row_begin;
    float wf, hf;
    float base[3], du[3], dv[3], bg[3];
};

// The samples [s0, ...) of pixel (x, y) (its planes' element `at`) join acc in groups of G while G
// of them are left, then in groups of G / 2, ... 1; s0 ends at q.samples.
template <int G>
__device__ __forceinline__ void ResolveGroups(const ResolveParams& q, size_t at, unsigned x, unsigned y, unsigned& s0,
                                              ResolveAcc& acc) {
    for (; s0 + G <= q.samples; s0 += G) {  // (uniform)
        // (1)
        int code[G];
        float2 o[G];
#pragma unroll
        for (int k = 0; k < G; ++k) {
            code[k] = __builtin_nontemporal_load(q.ids[s0 + k] + at);
            o[k] = q.offsets[s0 + k][at];
        }
        // (2)
        int hit[G];
        float4 nr[G], al[G];
#pragma unroll
        for (int k = 0; k < G; ++k) {
            hit[k] = static_cast<unsigned>(code[k]) < q.n ? code[k] : -1;
            nr[k] = al[k] = float4{};
        }
        if (q.n != 0u) {  // (an empty scene has no row 0)
#pragma unroll
            for (int k = 0; k < G; ++k) {
                const float4* sr = q.shade + 2ull * static_cast<unsigned>(max(hit[k], 0));
                nr[k] = sr[0];
                al[k] = sr[1];
            }
        }
        // (3)
#pragma unroll
        for (int k = 0; k < G; ++k) {
            ResolveRgb c{q.bg[0], q.bg[1], q.bg[2]};
            if (hit[k] >= 0) {
                float fx, fy;
                ResolvePosition(x, y, o[k].x, o[k].y, q.wf, q.hf, fx, fy);
                c = ResolveShadeHit(q.base, q.du, q.dv, fx, fy, nr[k].x, nr[k].y, nr[k].z, nr[k].w, al[k].x, al[k].y,
                                    al[k].z);
            }
            ResolveAdd(acc, s0 + k, c, hit[k] >= 0);
        }
    }
    if constexpr (G > 1) {
        ResolveGroups<G / 2>(q, at, x, y, s0, acc);
    }
}

template <int G>
__global__ __launch_bounds__(kResolveThreads) void ResolveKernel(const ResolveParams q) {
    const unsigned row = blockIdx.x / q.chunks;  // (uniform: scalar)
    const unsigned chunk = blockIdx.x - row * q.chunks;
    const unsigned x = chunk * kResolveThreads + threadIdx.x;
    // A pixel past the row loads the row's last one and is not stored.
    const size_t at = static_cast<size_t>(row) * q.width + min(x, q.width - 1u);
    ResolveAcc acc{};
    unsigned s0 = 0;
    ResolveGroups<G>(q, at, x, q.row_begin + row, s0, acc);
    if (x < q.width) {
        const ResolveTexel t = ResolveFinish(acc, q.samples);
        __builtin_nontemporal_store(F4{t.r, t.g, t.b, t.a}, q.out + at);
    }
}

}  // namespace

hipError_t LaunchGBuffer(const float* d_vertices, const float* d_shade, std::uint64_t n, const Frame& frame,
                         const float background[3], const GBufferArgs& args, hipStream_t stream) {
    const bool planes = args.depth != nullptr || args.bary != nullptr || args.normal != nullptr || args.albedo != nullptr;
    if (args.width == 0 || args.row_count == 0 || !planes) {
        return hipSuccess;
    }
    // Both gathers (the vertices for depth / bary, the shading table row for normal / albedo)?
    const bool both = (args.depth != nullptr || args.bary != nullptr) && (args.normal != nullptr || args.albedo != nullptr);
    const std::size_t block = static_cast<std::size_t>(kGBufferThreads) * (both ? kGBufferPixelsBoth : kGBufferPixels);
    const std::size_t chunks = (args.width + block - 1) / block;
    if (args.where == nullptr || args.ids == nullptr || d_shade == nullptr || (n != 0 && d_vertices == nullptr) ||
        n > 0xFFFFFFFFull || args.width > 0xFFFFFFFFull - block || (args.points && args.row_count != 1) ||
        (!args.points && (args.height == 0 || args.row_begin + args.row_count > args.height)) ||
        args.row_count > 0x7FFFFFFFull / chunks) {
        return hipErrorInvalidValue;
    }
    GBufferParams q{};
    q.vertices = d_vertices;
    q.shade = reinterpret_cast<const float4*>(d_shade);
    q.where = reinterpret_cast<const float2*>(args.where);
    q.ids = args.ids;
    q.depth = args.depth;
    q.bary = reinterpret_cast<F2*>(args.bary);
    q.normal = reinterpret_cast<F4*>(args.normal);
    q.albedo = reinterpret_cast<F4*>(args.albedo);
    q.n = static_cast<unsigned>(n);
    q.width = static_cast<unsigned>(args.width);
    q.chunks = static_cast<unsigned>(chunks);
    q.row_begin = static_cast<unsigned>(args.row_begin);
    q.wf = static_cast<float>(args.width);
    q.hf = static_cast<float>(args.height);
    for (int k = 0; k < 3; ++k) {
        q.eye[k] = frame.origin[k];
        q.base[k] = frame.base[k];
        q.du[k] = frame.du[k];
        q.dv[k] = frame.dv[k];
        q.bg[k] = background[k];
    }
    const dim3 grid(static_cast<unsigned>(chunks * args.row_count));
    const auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(kGBufferThreads), 0, stream, q); };
    if (args.points) {
        both ? launch(GBufferKernel<true, kGBufferPixelsBoth>) : launch(GBufferKernel<true, kGBufferPixels>);
    } else {
        both ? launch(GBufferKernel<false, kGBufferPixelsBoth>) : launch(GBufferKernel<false, kGBufferPixels>);
    }
    return hipGetLastError();
}

hipError_t LaunchSurface(const float* d_vertices, const float* d_shade, std::uint64_t n, const Frame& frame,
                         const float background[3], const SurfaceArgs& args, hipStream_t stream) {
    const bool planes = args.normal != nullptr || args.albedo != nullptr || args.rgba != nullptr || args.uv != nullptr;
    if (args.width == 0 || args.row_count == 0 || !planes) {
        return hipSuccess;
    }
    const std::size_t block = static_cast<std::size_t>(kSurfaceThreads) * kSurfacePixels;
    const std::size_t chunks = (args.width + block - 1) / block;
    const bool texture_ok = args.texture == nullptr ||
                            (args.uvs != nullptr && args.tex_width >= 1 && args.tex_width <= kSurfaceMaxTexture &&
                             args.tex_height >= 1 && args.tex_height <= kSurfaceMaxTexture);
    if (args.where == nullptr || args.ids == nullptr || d_shade == nullptr || (n != 0 && d_vertices == nullptr) ||
        n > 0xFFFFFFFFull || args.width > 0xFFFFFFFFull - block || (args.points && args.row_count != 1) ||
        (!args.points && (args.height == 0 || args.row_begin + args.row_count > args.height)) ||
        args.row_count > 0x7FFFFFFFull / chunks || !texture_ok || (args.flags & ~kSurfaceFlags) != 0u) {
        return hipErrorInvalidValue;
    }
    SurfaceParams q{};
    q.vertices = d_vertices;
    q.shade = reinterpret_cast<const float4*>(d_shade);
    q.where = reinterpret_cast<const float2*>(args.where);
    q.ids = args.ids;
    q.normals = args.normals;
    q.uvs = args.uvs;
    q.texture = reinterpret_cast<const float4*>(args.texture);
    q.normal = reinterpret_cast<F4*>(args.normal);
    q.albedo = reinterpret_cast<F4*>(args.albedo);
    q.rgba = reinterpret_cast<F4*>(args.rgba);
    q.uv = reinterpret_cast<F2*>(args.uv);
    q.n = static_cast<unsigned>(n);
    q.width = static_cast<unsigned>(args.width);
    q.chunks = static_cast<unsigned>(chunks);
    q.row_begin = static_cast<unsigned>(args.row_begin);
    q.tw = args.texture != nullptr ? static_cast<int>(args.tex_width) : 1;
    q.th = args.texture != nullptr ? static_cast<int>(args.tex_height) : 1;
    q.flags = args.flags;
    q.wf = static_cast<float>(args.width);
    q.hf = static_cast<float>(args.height);
    for (int k = 0; k < 3; ++k) {
        q.eye[k] = frame.origin[k];
        q.base[k] = frame.base[k];
        q.du[k] = frame.du[k];
        q.dv[k] = frame.dv[k];
        q.bg[k] = background[k];
    }
    const dim3 grid(static_cast<unsigned>(chunks * args.row_count));
    if (args.points) {
        hipLaunchKernelGGL((SurfaceKernel<true, kSurfacePixels>), grid, dim3(kSurfaceThreads), 0, stream, q);
    } else {
        hipLaunchKernelGGL((SurfaceKernel<false, kSurfacePixels>), grid, dim3(kSurfaceThreads), 0, stream, q);
    }
    return hipGetLastError();
}

hipError_t LaunchInterpolate(const float* d_vertices, std::uint64_t n, const Frame& frame, const InterpolateArgs& args,
                             hipStream_t stream) {
    if (args.width == 0 || args.row_count == 0) {
        return hipSuccess;
    }
    const std::size_t block = static_cast<std::size_t>(kSurfaceThreads) * kInterpolatePixels;
    const std::size_t chunks = (args.width + block - 1) / block;
    if (args.where == nullptr || args.ids == nullptr || args.out == nullptr || (n != 0 && d_vertices == nullptr) ||
        (n != 0 && args.table == nullptr) || args.channels < 1 ||
        args.channels > static_cast<std::size_t>(kSurfaceMaxChannels) || n > 0xFFFFFFFFull ||
        args.width > 0xFFFFFFFFull - block || (args.points && args.row_count != 1) ||
        (!args.points && (args.height == 0 || args.row_begin + args.row_count > args.height)) ||
        args.row_count > 0x7FFFFFFFull / chunks) {
        return hipErrorInvalidValue;
    }
    InterpolateParams q{};
    q.vertices = d_vertices;
    q.where = reinterpret_cast<const float2*>(args.where);
    q.ids = args.ids;
    q.table = args.table;
    q.out = args.out;
    q.n = static_cast<unsigned>(n);
    q.width = static_cast<unsigned>(args.width);
    q.chunks = static_cast<unsigned>(chunks);
    q.row_begin = static_cast<unsigned>(args.row_begin);
    q.wf = static_cast<float>(args.width);
    q.hf = static_cast<float>(args.height);
    for (int k = 0; k < 3; ++k) {
        q.eye[k] = frame.origin[k];
        q.base[k] = frame.base[k];
        q.du[k] = frame.du[k];
        q.dv[k] = frame.dv[k];
    }
    const dim3 grid(static_cast<unsigned>(chunks * args.row_count));
    const auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(kSurfaceThreads), 0, stream, q); };
    switch (args.channels * 2 + (args.points ? 1 : 0)) {
        case 2: launch(InterpolateKernel<false, 1>); break;
        case 3: launch(InterpolateKernel<true, 1>); break;
        case 4: launch(InterpolateKernel<false, 2>); break;
        case 5: launch(InterpolateKernel<true, 2>); break;
        case 6: launch(InterpolateKernel<false, 3>); break;
        case 7: launch(InterpolateKernel<true, 3>); break;
        case 8: launch(InterpolateKernel<false, 4>); break;
        default: launch(InterpolateKernel<true, 4>); break;
    }
    return hipGetLastError();
}

hipError_t LaunchResolve(const float* d_shade, std::uint64_t n, const Frame& frame, const float background[3],
                         const ResolveArgs& args, hipStream_t stream) {
    if (args.width == 0 || args.row_count == 0) {
        return hipSuccess;
    }
    const std::size_t chunks = (args.width + kResolveThreads - 1) / kResolveThreads;
    if (args.offsets == nullptr || args.ids == nullptr || args.rgba == nullptr || d_shade == nullptr ||
        args.samples == 0 || args.samples > static_cast<std::size_t>(kMaxSamples) || n > 0xFFFFFFFFull ||
        args.width > 0xFFFFFFFFull - kResolveThreads || args.height == 0 || args.row_begin > args.height ||
        args.row_count > args.height - args.row_begin || args.height > 0x7FFFFFFFull ||
        args.row_count > 0x7FFFFFFFull / chunks) {
        return hipErrorInvalidValue;
    }
    ResolveParams q{};
    for (std::size_t s = 0; s < args.samples; ++s) {
        if (args.offsets[s] == nullptr || args.ids[s] == nullptr) {
            return hipErrorInvalidValue;
        }
        q.offsets[s] = reinterpret_cast<const float2*>(args.offsets[s]);
        q.ids[s] = args.ids[s];
    }
    q.shade = reinterpret_cast<const float4*>(d_shade);
    q.out = reinterpret_cast<F4*>(args.rgba);
    q.n = static_cast<unsigned>(n);
    q.samples = static_cast<unsigned>(args.samples);
    q.width = static_cast<unsigned>(args.width);
    q.chunks = static_cast<unsigned>(chunks);
    q.row_begin = static_cast<unsigned>(args.row_begin);
    q.wf = static_cast<float>(args.width);
    q.hf = static_cast<float>(args.height);
    for (int k = 0; k < 3; ++k) {
        q.base[k] = frame.base[k];
        q.du[k] = frame.du[k];
        q.dv[k] = frame.dv[k];
        q.bg[k] = background[k];
    }
    const dim3 grid(static_cast<unsigned>(chunks * args.row_count));
    if (q.samples >= kResolveLong) {
        hipLaunchKernelGGL(ResolveKernel<kResolveGroupLong>, grid, dim3(kResolveThreads), 0, stream, q);
    } else {
        hipLaunchKernelGGL(ResolveKernel<kResolveGroup>, grid, dim3(kResolveThreads), 0, stream, q);
    }
    return hipGetLastError();
}

}  // namespace srt
