// What the render kernel units share (render.hip, outputs.hip, query.hip): the cull
// record and the trace parameters, the record source of a walk (TraceRecords), the exact test and the
// edge math under them, and the host carve-up of the record buffers. Each definition here is used by
// at least two of those units; what one unit uses alone stays in that unit.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "render.h"

namespace srt {

constexpr int kWave = 64;

// Cull record (the binned cull path's copy of one edge record, 64 B, stored at the record's
// rank in the scene's spatial order): a = (c0A, cxA, cyA, c0B), b = (cxB, cyB, c0C, cxC),
// x = (cyC, vol, id bits, 0), sb = screen box.
struct CullRecord {
    float4 a, b, x, sb;
};
static_assert(sizeof(CullRecord) == kCullRecordBytes, "render.h kCullRecordBytes");

// Per-tile facts the cull trace and the bin kernel share (TileInfoKernel), 32 B.
struct TileInfo {
    float4 box;         // (xlo, xhi, ylo, yhi) of the tile's ray positions (NaN positions drop out)
    float ox, oy;       // sample offset of the tile's first ray
    unsigned regular;   // every ray of the tile has offset (ox, oy), bit for bit
    unsigned usable;    // box within the screen-box range (else the tile streams every record)
};

// Per-tile facts of one frame on the shared setup (render.h CullSetup; TileFactsKernel),
// 16 B: what a trace block still needs from its own frame's offsets. The tile box is not among
// them: the shared lists were binned against the analytic box, which contains the tile's rays
// exactly when every offset of the tile lies in [0, 1] (kFactInRange).
constexpr unsigned kFactRegular = 1u;  // every ray of the tile has offset (ox, oy), bit for bit
constexpr unsigned kFactUsable = 2u;   // the tile's ray box lies within the screen-box range
constexpr unsigned kFactInRange = 4u;  // every offset of the tile lies in [0, 1] (NaN: outside)
struct TileFacts {
    float ox, oy;  // sample offset of the tile's first ray
    unsigned flags;
    unsigned pad;
};

struct TraceParams {
    const float4* __restrict__ edges;
    const float4* __restrict__ screen_boxes;
    const uint2* __restrict__ qboxes;
    const float* __restrict__ vertices;
    const float4* __restrict__ shade;  // per triangle: (shading normal, |normal|), (albedo, 0) -- ShadeTableKernel
    const float2* __restrict__ offsets;
    float4* __restrict__ out;
    int* __restrict__ out_ids;  // non-null: store the hit id per pixel (-1 = miss) instead of RGBA
    unsigned char* __restrict__ out_packed;  // non-null: store packed ids (render.h PackedIds) instead
    int id_planes;             // packed ids: bit planes above the low 16 bits
    unsigned id_words;         // packed ids: 64-bit words per row and plane
    unsigned id_low_row_bytes; // packed ids: the row's u16 values (padded to 8 B), then its plane words
    unsigned id_row_bytes;     // packed ids: bytes per row
    unsigned id_tile_row_bytes;  // packed ids: bytes per tile row (its rows, then its tiles' offsets)
    int out_frame_rows;  // RGBA out is a whole frame: band row y stores at its frame row (render.h BandArgs)
    unsigned n_pad;   // records in the edge buffer (multiple of kPadTriangles)
    unsigned n;       // records in the scene
    int tiles_x;         // cull tiles per tile row of the band
    unsigned tiles;      // cull tiles of the band
    unsigned n_tiles; // tiles holding at least one real record (>= 1)
    int width;
    int row_count;
    int row_begin;
    int row_interleave;  // band = frame tile rows row_begin / kTileRows + k * row_interleave (1: contiguous rows)
    // Cull variant with bins (render.h CullBins); tile_info == null: no bins, every tile
    // computes its own ray box and streams every record.
    const TileInfo* __restrict__ tile_info;   // per tile: ray box, uniform offset (TileInfoKernel)
    const TileFacts* __restrict__ tile_facts; // shared setup: this frame's per-tile facts (work, lists: the setup's)
    const CullRecord* __restrict__ cull;     // cull records in spatial order (the lists hold positions)
    const unsigned* __restrict__ order;       // spatial-order position -> record id
    const float* __restrict__ svertices;      // vertices by spatial-order position (binned trace: records recomputed)
    const uint4* __restrict__ work;           // tile parts (2 x uint4 each), most work first (BuildWorkOrder)
    const unsigned* __restrict__ work_count;  // [0]: tile parts listed
    unsigned long long* __restrict__ split_keys;  // key slices of split parts: one per split slot, kBlockRows x 64 each
    unsigned* __restrict__ arrive;            // per split part (its first slot): chunks finished (self-resetting)
    const unsigned* __restrict__ bin_lists;   // per tile: candidate positions (PrepareBinKernel)
    const unsigned* __restrict__ bin_counts;  // per tile: list length; [tiles]: large-list length (this frame's)
    unsigned* __restrict__ bin_counts_next;   // the slot's other count buffer: reset by the trace for its next frame
    const unsigned* __restrict__ large_list;  // ids of records binned to every tile
    const unsigned* __restrict__ range_tag;   // = gen: some sample offset of this frame lies outside [0, 1]
    const CullRecord* __restrict__ stream;    // shared setup's record stream (render.h; TraceCullKernel<.., STREAM>)
    const unsigned* __restrict__ empty_map;   // shared setup: per tile, non-zero = statically empty (render.h CullSetup)
    unsigned gen;                              // frame number of the scene (never 0)
    unsigned fused;                            // bins from the analytic tile bounds (BinParams::fused)
    unsigned plan_only;  // the work list is the slot's plan (no order launch for this frame): read the bins
    unsigned bin_capacity;
    unsigned list_descs;   // shared setup: the plan's descriptors that are not statically empty (they come first)
    unsigned empty_descs;  // shared setup: its statically empty descriptors (they follow)
    unsigned empty_group;  // shared setup: empty descriptors per sweep block (TraceCullKernel); 0: one block each
    unsigned facts_fill;   // shared setup, sweep on: the facts launch stores the valid empty tiles' misses (TileFactsKernel)
    unsigned exp;                                // diagnostic build: experiment bits (env SRT_EXP), 0 in the product
    float wf;
    float hf;
    float base[3];
    float du[3];
    float dv[3];
    float bg[3];
    float eye[3];  // ray origin (the 16-bit id decode recomputes candidate records)
};

// One edge record as the trace kernels consume it.
struct Record {
    float c0A, cxA, cyA, c0B, cxB, cyB, c0C, cxC, cyC;
};

__device__ __forceinline__ float Dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return fmaf(az, bz, fmaf(ay, by, ax * bx));
}

__device__ __forceinline__ void Cross3(float ax, float ay, float az, float bx, float by, float bz, float& cx,
                                       float& cy, float& cz) {
    cx = ay * bz - az * by;
    cy = az * bx - ax * bz;
    cz = ax * by - ay * bx;
}

// The edge coefficients and vol alone (ComputeRecord without the screen box), under the frame
// (origin, base, du, dv); returns false for a disabled record (c, vol NaN). One definition for the
// record pass and the 16-bit id decode, so both see the same bits.
__device__ __forceinline__ bool ComputeEdges(const float* origin, const float* base, const float* du, const float* dv,
                                             const float* __restrict__ v, bool real, float c[9], float& vol) {
    const float qnan = __builtin_nanf("");
    bool disabled = !real;
    vol = qnan;
    if (!disabled) {
        const float ax = v[0] - origin[0], ay = v[1] - origin[1], az = v[2] - origin[2];
        const float bx = v[3] - origin[0], by = v[4] - origin[1], bz = v[5] - origin[2];
        const float cx = v[6] - origin[0], cy = v[7] - origin[1], cz = v[8] - origin[2];
        float n[9];
        Cross3(bx, by, bz, cx, cy, cz, n[0], n[1], n[2]);
        Cross3(cx, cy, cz, ax, ay, az, n[3], n[4], n[5]);
        Cross3(ax, ay, az, bx, by, bz, n[6], n[7], n[8]);
        vol = Dot3(ax, ay, az, n[0], n[1], n[2]);
        disabled = !(std::isfinite(vol) && vol != 0.f);
        if (!disabled) {
            if (vol < 0.f) {
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    n[k] = -n[k];
                }
                vol = -vol;
            }
#pragma unroll
            for (int e = 0; e < 3; ++e) {
                const float nx = n[3 * e], ny = n[3 * e + 1], nz = n[3 * e + 2];
                c[3 * e + 0] = Dot3(nx, ny, nz, base[0], base[1], base[2]);
                c[3 * e + 1] = Dot3(nx, ny, nz, du[0], du[1], du[2]);
                c[3 * e + 2] = Dot3(nx, ny, nz, dv[0], dv[1], dv[2]);
            }
        }
    }
    if (disabled) {
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            c[k] = qnan;
        }
        vol = qnan;
    }
    return !disabled;
}

// Per-lane ray state: R rays sharing one image column.
template <int R>
struct Rays {
    float fx[R];
    float fy[R];
    float bt[R];  // closest t so far (+inf = none)
    int bi[R];    // closest triangle id (-1 = miss)
};

typedef float F4 __attribute__((ext_vector_type(4)));
// A nontemporal float4 store the compiler cannot merge: after ShadeIdsKernel's grid was compacted
// (its store no longer behind a row test), clang sank the two stores of ShadeRecord's hit / miss
// paths into one and dropped `nt` on the way (97 -> 112 us per 8-frame launch of a P = 8
// compositor; a branch-free ShadeRecord kept `nt` but shaded every miss: 104 us).
__device__ __forceinline__ void StoreNontemporal(F4* at, F4 v) {
    asm volatile("global_store_dwordx4 %0, %1, off nt" ::"v"(at), "v"(v) : "memory");
}

// (t, id) packed so that unsigned order is lexicographic order: t >= 0 here (vol > 0,
// det > 0), so its bit pattern orders like the value.
__device__ __forceinline__ unsigned long long HitKey(float t, int id) {
    return (static_cast<unsigned long long>(__float_as_uint(t)) << 32) | static_cast<unsigned>(id);
}

// Exact test of one record against every ray of the lane (records in any order): the
// lexicographic minimum of (t, id) equals the ascending-id strict-< result of TestTriangle
// (smallest t; among equal t the lowest id).
template <int R, bool SHARED>
__device__ __forceinline__ void ExactTestAnyOrder(Rays<R>& s, const Record& q, float vol, int id) {
    float gA[R], gB[R], gC[R];
    if constexpr (SHARED) {
        const float a = fmaf(s.fx[0], q.cxA, q.c0A), b = fmaf(s.fx[0], q.cxB, q.c0B),
                    c = fmaf(s.fx[0], q.cxC, q.c0C);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            gA[r] = a;
            gB[r] = b;
            gC[r] = c;
        }
    } else {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            gA[r] = fmaf(s.fx[r], q.cxA, q.c0A);
            gB[r] = fmaf(s.fx[r], q.cxB, q.c0B);
            gC[r] = fmaf(s.fx[r], q.cxC, q.c0C);
        }
    }
    float e[R][3];
    float m[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        e[r][0] = fmaf(s.fy[r], q.cyA, gA[r]);
        e[r][1] = fmaf(s.fy[r], q.cyB, gB[r]);
        e[r][2] = fmaf(s.fy[r], q.cyC, gC[r]);
        m[r] = fminf(fminf(e[r][0], e[r][1]), e[r][2]);
    }
    float mm = m[0];
#pragma unroll
    for (int r = 1; r < R; ++r) {
        mm = fmaxf(mm, m[r]);
    }
    if (mm >= 0.f) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (e[r][0] >= 0.f && e[r][1] >= 0.f && e[r][2] >= 0.f) {
                const float det = (e[r][0] + e[r][1]) + e[r][2];
                if (det > 0.f) {
                    const float t = vol / det;
                    if (t < s.bt[r] || (t == s.bt[r] && id < s.bi[r])) {
                        s.bt[r] = t;
                        s.bi[r] = id;
                    }
                }
            }
        }
    }
}

constexpr int kTileRows = kCullTileRows;

// Where a trace block's candidate records come from. RC = false: the 64-B cull record by position
// (written by the record pass: LaunchPrepare, or the bin kernel of a stored-record launch).
// RC = true (a binned launch with CullBins::recompute): the bin kernel writes only the screen box
// by position, and the trace recomputes the edge coefficients and vol from the vertices by position
// with the record pass's own ComputeEdges under the same frame vectors -- the same bits -- and
// takes the id from the spatial order (a padding position is its own id, >= n: a disabled record).
struct RawRecord {
    float v[9];
    unsigned id;
    float4 sb;
};
template <bool RC>
struct TraceRecords {
    using Raw = CullRecord;
    static __device__ __forceinline__ Raw Load(const TraceParams& p, unsigned pos) { return p.cull[pos]; }
    static __device__ __forceinline__ CullRecord Make(const TraceParams&, const Raw& r) { return r; }
};
template <>
struct TraceRecords<true> {
    using Raw = RawRecord;
    static __device__ __forceinline__ Raw Load(const TraceParams& p, unsigned pos) {
        Raw r;
        const bool real = pos < p.n;
        const float4* v = reinterpret_cast<const float4*>(p.svertices + static_cast<size_t>(kSpatialStride) * (real ? pos : 0u));
        const float4 v0 = v[0], v1 = v[1], v2 = v[2];
        r.v[0] = v0.x, r.v[1] = v0.y, r.v[2] = v0.z, r.v[3] = v0.w;
        r.v[4] = v1.x, r.v[5] = v1.y, r.v[6] = v1.z, r.v[7] = v1.w;
        r.v[8] = v2.x;
        r.id = real ? __float_as_uint(v2.y) : pos;
        r.sb = p.screen_boxes[pos];
        return r;
    }
    static __device__ __forceinline__ CullRecord Make(const TraceParams& p, const Raw& r) {
        float c[9], vol;
        ComputeEdges(p.eye, p.base, p.du, p.dv, r.v, r.id < p.n, c, vol);
        CullRecord cr;
        cr.a = make_float4(c[0], c[1], c[2], c[3]);
        cr.b = make_float4(c[4], c[5], c[6], c[7]);
        cr.x = make_float4(c[8], vol, __uint_as_float(r.id), 0.f);
        cr.sb = r.sb;
        return cr;
    }
};

// Carve-up of a scene's edge allocation (render.h kEdgeFloatsPerTriangle): tile-planar edge
// records, screen boxes, quantized boxes, cull records, shading normals.
struct EdgeLayout {
    float4* tiles;
    float4* screen_boxes;
    uint2* qboxes;
    CullRecord* cull;
};
inline EdgeLayout EdgeBuffers(const float* d_edges, std::uint64_t n) {
    EdgeLayout e;
    const std::uint64_t n_pad = PaddedTriangleCount(n);
    e.tiles = reinterpret_cast<float4*>(const_cast<float*>(d_edges));
    e.screen_boxes = e.tiles + n_pad / kTileTriangles * kTileFloat4;
    e.qboxes = reinterpret_cast<uint2*>(e.screen_boxes + n_pad);
    e.cull = reinterpret_cast<CullRecord*>(e.qboxes + n_pad);
    return e;
}

inline EdgeLayout SetupRecords(const CullSetup& s) {
    EdgeLayout e{};
    e.tiles = nullptr;  // the tile-planar records belong to the lds / scalar variants (edge slot 0)
    e.screen_boxes = static_cast<float4*>(s.screen_boxes);
    e.qboxes = static_cast<uint2*>(s.qboxes);
    e.cull = static_cast<CullRecord*>(s.cull);
    return e;
}

}  // namespace srt
