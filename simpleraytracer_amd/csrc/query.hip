// MI355X (gfx950) point-query kernels: the closest hit and the K nearest hits at arbitrary positions of
// a prepared frame, and the over-composite of depth layers (render.h LaunchQuery, LaunchLayers,
// LaunchComposite). Built as render.hip is: -ffp-contract=off, every fused multiply-add an explicit fmaf.
#include "render.h"
#include "candidate_walk.h"
#include "layers_math.h"
#include "samples_math.h"

#include <type_traits>

namespace srt {

namespace {

// The exact test of one record at one position as "passes, t" (the id is the caller's): the test
// ExactTestAnyOrder<1, false> makes before it compares with its running minimum -- the same fmaf
// chain, conditions and division, so the same bits -- for a kernel that keeps more than a minimum
// (LayersKernel). A hit with t = +inf or NaN does not pass: the traces' strict < from +inf never
// takes one either. Stated beside ExactTestAnyOrder rather than inside it, on measurement (DESIGN.md
// section 5 "Depth layers"): calling a shared "passes, t" piece from ExactTestAnyOrder's loop body
// changed the scalar register allocation of QueryKernel and ShadowKernel, and running
// ExactTestAnyOrder from an empty state here cost LayersKernel 8 to 20 %.
__device__ __forceinline__ bool ExactTestOne(float fx, float fy, const Record& q, float vol, float& t) {
    const float e0 = fmaf(fy, q.cyA, fmaf(fx, q.cxA, q.c0A));
    const float e1 = fmaf(fy, q.cyB, fmaf(fx, q.cxB, q.c0B));
    const float e2 = fmaf(fy, q.cyC, fmaf(fx, q.cxC, q.c0C));
    if (e0 >= 0.f && e1 >= 0.f && e2 >= 0.f) {
        const float det = (e0 + e1) + e2;
        if (det > 0.f) {
            t = vol / det;
            return t < __builtin_inff();
        }
    }
    return false;
}

// ---------------------------------------------------------------------------------------
// Point queries (render.h LaunchQuery; DESIGN.md section 5 "Point queries"): the closest hit at
// arbitrary image positions of the prepared frame, answered from the shared setup's lists by the
// candidate walk above.
// A group of kQueryLanes lanes per query runs the trace kernels' exact test on the candidates
// (ExactTestAnyOrder, one ray) and reduces the (t, id) key with shuffles -- no LDS, no atomics, no
// cross-block traffic; a repeated last candidate changes no minimum. The kernel is bound by the
// latency of its chain of dependent loads (position -> tile counts -> list entries -> records), not
// by bandwidth or VALU, so fewer, fuller waves win: 16 lanes x 2 candidates measured best of
// 64 / 32 / 16 / 8 lanes and 1 / 2 / 4 candidates at C3 (profiles/query/).
// SRT_QUERY_LANES, SRT_QUERY_AHEAD: measurement builds.
// ---------------------------------------------------------------------------------------
#ifndef SRT_QUERY_LANES
#define SRT_QUERY_LANES 16
#endif
constexpr int kQueryLanes = SRT_QUERY_LANES;  // lanes per query (a divisor of the wave)
#ifndef SRT_QUERY_AHEAD
#define SRT_QUERY_AHEAD 2
#endif
constexpr int kQueryAhead = SRT_QUERY_AHEAD;  // candidates per lane and round
constexpr int kQueryThreads = 256;
constexpr int kQueryBlock = kQueryThreads / kQueryLanes;  // queries per block
static_assert(kQueryLanes >= 2 && kWave % kQueryLanes == 0, "a query's lanes share a wave");
struct QueryParams {
    TraceParams rec;  // the records (TraceRecords), the frame vectors, the setup's tiles, lists and counts
    const float2* __restrict__ positions;
    int* __restrict__ ids;
    float* __restrict__ t;
    unsigned char* __restrict__ how;  // null: not stored
    unsigned count;
    unsigned stream_end;  // records of a streamed query: positions [0, stream_end)
    int tiles_y;
};

template <bool RC>
__global__ __launch_bounds__(kQueryThreads) void QueryKernel(const QueryParams q) {
    const TraceParams& p = q.rec;
    using Recs = TraceRecords<RC>;
    const unsigned lane = threadIdx.x & (kQueryLanes - 1);
    unsigned group = threadIdx.x / kQueryLanes;
    if constexpr (kQueryLanes == kWave) {  // wave-uniform: the query's facts load through the scalar cache
        group = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(group)));
    }
    const unsigned query = blockIdx.x * kQueryBlock + group;
    if (query >= q.count) {
        return;
    }
    const float2 f = q.positions[query];
    Rays<1> s;
    s.fx[0] = f.x;
    s.fy[0] = f.y;
    s.bt[0] = __builtin_inff();
    s.bi[0] = -1;
    const Candidates cand = FindCandidates(p, q.tiles_y, q.stream_end, f.x, f.y);
    auto test = [&](const typename Recs::Raw& raw) {
        const CullRecord r = Recs::Make(p, raw);
        const Record rec{r.a.x, r.a.y, r.a.z, r.a.w, r.b.x, r.b.y, r.b.z, r.b.w, r.x.x};
        ExactTestAnyOrder<1, false>(s, rec, r.x.y, static_cast<int>(__float_as_uint(r.x.z)));
    };
    WalkCandidates<kQueryLanes, kQueryAhead, typename Recs::Raw>(
        cand, lane, [&](unsigned pos) { return Recs::Load(p, pos); }, test, [] { return false; });
    // The lanes' (t, id) minimum; a miss is (+inf, -1), above every hit's key (a hit's t < +inf).
    unsigned long long key = HitKey(s.bt[0], s.bi[0]);
#pragma unroll
    for (int o = 1; o < kQueryLanes; o <<= 1) {
        const unsigned lo = static_cast<unsigned>(__shfl_xor(static_cast<int>(key), o));
        const unsigned hi = static_cast<unsigned>(__shfl_xor(static_cast<int>(key >> 32), o));
        const unsigned long long other = static_cast<unsigned long long>(hi) << 32 | lo;
        key = other < key ? other : key;
    }
    if (lane == 0u) {
        q.ids[query] = static_cast<int>(static_cast<unsigned>(key));
        q.t[query] = __uint_as_float(static_cast<unsigned>(key >> 32));
        if (q.how != nullptr) {
            q.how[query] = cand.listed ? 0 : 1;
        }
    }
}

// ---------------------------------------------------------------------------------------
// Depth layers (render.h LaunchLayers; DESIGN.md section 5 "Depth layers"): the K lexicographically
// smallest (t, id) keys among the records that pass the exact test at an image position, K <=
// kMaxLayers -- QueryKernel keeping K keys instead of one: the candidate walk visits every record
// that can pass at the position, so the K smallest keys over it are the K smallest over all records.
// The mapping is QueryKernel's (a group of kLayersLanes lanes per position). POINTS: position i is read
// from `where`; else element (x, y) is pixel (x, row_begin + y) of the frame and its position ray
// generation's expression of its sample offset (GBufferKernel's convention, buffers band-local).
// Each lane keeps its CAP smallest keys sorted in registers (KeyList: compile-time indices only, no
// scratch); an insertion drops a key that is not below the lane's CAP-th and one that the lane holds
// already, so a repeated candidate changes nothing. (A record cannot arrive twice by way of the
// lists: PrepareBinKernel puts a record whose tile range exceeds kLargeTiles on the large list and
// any other on tile lists, never both, and on a tile's list once.) The group then merges in K
// rounds: a shuffle-reduced minimum of the lanes' heads, stored by lane 0 as layer k, and every lane
// whose head equals it pops it -- a key held by two lanes (the repeated last candidate) leaves both.
// An empty slot is the all-ones key, above every hit's, and stored as (-1, +inf). No LDS, no
// atomics; the setup is read, never written.
// CAP is 2, 4 or 8 (K rounded up): the list costs 2 CAP VGPRs and the insertion ~3 CAP VALU
// instructions per passing candidate, so K <= 2 does not pay for 8 slots.
// Lanes per position, measured at C3 (8 / 16 / 32 lanes x 1 / 2 / 4 candidates: DESIGN.md;
// profiles/layers/): as for the query, 8 lanes win on coherent positions (K = 8: 609 us against 796)
// and lose on shuffled ones (K = 1: 1 265 us against 1 138). A frame's pixels are coherent by
// construction, arbitrary positions are not: frame mode takes 8 lanes, point mode 16.
// SRT_LAYERS_LANES, SRT_LAYERS_FRAME_LANES, SRT_LAYERS_AHEAD: measurement builds.
// ---------------------------------------------------------------------------------------
#ifndef SRT_LAYERS_LANES
#define SRT_LAYERS_LANES 16
#endif
#ifndef SRT_LAYERS_FRAME_LANES
#define SRT_LAYERS_FRAME_LANES 8
#endif
constexpr int kLayersLanes = SRT_LAYERS_LANES;             // lanes per position (a divisor of the wave), point mode
constexpr int kLayersFrameLanes = SRT_LAYERS_FRAME_LANES;  // ... frame mode
#ifndef SRT_LAYERS_AHEAD
#define SRT_LAYERS_AHEAD 2
#endif
constexpr int kLayersAhead = SRT_LAYERS_AHEAD;  // candidates per lane and round
constexpr int kLayersThreads = 256;
constexpr int LayersLanes(bool points) { return points ? kLayersLanes : kLayersFrameLanes; }
static_assert(kLayersLanes >= 2 && kWave % kLayersLanes == 0 && kLayersFrameLanes >= 2 && kWave % kLayersFrameLanes == 0,
              "a position's lanes share a wave");
constexpr unsigned long long kNoKey = ~0ull;  // an empty slot: above every HitKey (t < +inf)
struct LayersParams {
    TraceParams rec;  // as QueryParams::rec
    const float2* __restrict__ where;  // positions (POINTS) or the band's sample offsets
    int* __restrict__ ids;             // layers x (rows x width), layer-major
    float* __restrict__ t;             // the same shape, or null: not stored
    unsigned char* __restrict__ how;   // rows x width, or null: not stored
    unsigned layers;
    unsigned width;   // elements per row (POINTS: the count, one row)
    unsigned chunks;  // blocks per row
    unsigned row_begin;
    size_t plane;  // elements per layer plane
    float wf, hf;
    unsigned stream_end;
    int tiles_y;
};

// A lane's CAP smallest keys, ascending; empty slots hold kNoKey.
template <int CAP>
struct KeyList {
    unsigned long long k[CAP];
    __device__ __forceinline__ void Clear() {
#pragma unroll
        for (int j = 0; j < CAP; ++j) {
            k[j] = kNoKey;
        }
    }
    // Idempotent: a key the list holds, and one not below its last, change nothing.
    __device__ __forceinline__ void Insert(unsigned long long key) {
        bool held = false;
#pragma unroll
        for (int j = 0; j < CAP; ++j) {
            held |= k[j] == key;
        }
        key = held ? kNoKey : key;  // (kNoKey is below no slot)
#pragma unroll
        for (int j = CAP - 1; j >= 1; --j) {
            k[j] = key < k[j - 1] ? k[j - 1] : (key < k[j] ? key : k[j]);
        }
        k[0] = key < k[0] ? key : k[0];
    }
    __device__ __forceinline__ void Pop() {
#pragma unroll
        for (int j = 0; j + 1 < CAP; ++j) {
            k[j] = k[j + 1];
        }
        k[CAP - 1] = kNoKey;
    }
};

template <bool RC, bool POINTS, int CAP>
__global__ __launch_bounds__(kLayersThreads) void LayersKernel(const LayersParams q) {
    const TraceParams& p = q.rec;
    using Recs = TraceRecords<RC>;
    constexpr int kLanes = LayersLanes(POINTS);
    constexpr int kBlock = kLayersThreads / kLanes;  // positions per block
    const unsigned lane = threadIdx.x & (kLanes - 1);
    unsigned group = threadIdx.x / kLanes;
    if constexpr (kLanes == kWave) {
        group = static_cast<unsigned>(__builtin_amdgcn_readfirstlane(static_cast<int>(group)));
    }
    const unsigned row = POINTS ? 0u : blockIdx.x / q.chunks;  // (uniform: scalar)
    const unsigned chunk = blockIdx.x - row * q.chunks;
    const unsigned x = chunk * kBlock + group;
    if (x >= q.width) {
        return;
    }
    const size_t at = static_cast<size_t>(row) * q.width + x;
    float2 f = q.where[at];
    if constexpr (!POINTS) {
        f.x = (static_cast<float>(x) + f.x) / q.wf;
        f.y = (static_cast<float>(q.row_begin + row) + f.y) / q.hf;
    }
    const Candidates cand = FindCandidates(p, q.tiles_y, q.stream_end, f.x, f.y);
    KeyList<CAP> keys;
    keys.Clear();
    auto test = [&](const typename Recs::Raw& raw) {
        const CullRecord r = Recs::Make(p, raw);
        const Record rec{r.a.x, r.a.y, r.a.z, r.a.w, r.b.x, r.b.y, r.b.z, r.b.w, r.x.x};
        float t;
        if (ExactTestOne(f.x, f.y, rec, r.x.y, t)) {
            keys.Insert(HitKey(t, static_cast<int>(__float_as_uint(r.x.z))));
        }
    };
    WalkCandidates<kLanes, kLayersAhead, typename Recs::Raw>(
        cand, lane, [&](unsigned pos) { return Recs::Load(p, pos); }, test, [] { return false; });
    if (lane == 0u && q.how != nullptr) {
        q.how[at] = cand.listed ? 0 : 1;
    }
#pragma unroll
    for (int k = 0; k < CAP; ++k) {
        if (static_cast<unsigned>(k) >= q.layers) {  // (uniform)
            break;
        }
        unsigned long long key = keys.k[0];
#pragma unroll
        for (int o = 1; o < kLanes; o <<= 1) {
            const unsigned lo = static_cast<unsigned>(__shfl_xor(static_cast<int>(key), o));
            const unsigned hi = static_cast<unsigned>(__shfl_xor(static_cast<int>(key >> 32), o));
            const unsigned long long other = static_cast<unsigned long long>(hi) << 32 | lo;
            key = other < key ? other : key;
        }
        if (keys.k[0] == key) {  // (every holder; kNoKey: nothing is left, the pop changes nothing)
            keys.Pop();
        }
        if (lane == 0u) {
            const bool hit = key != kNoKey;
            const size_t out = static_cast<size_t>(k) * q.plane + at;
            q.ids[out] = hit ? static_cast<int>(static_cast<unsigned>(key)) : -1;
            if (q.t != nullptr) {
                q.t[out] = hit ? __uint_as_float(static_cast<unsigned>(key >> 32)) : __builtin_inff();
            }
        }
    }
}

// ---------------------------------------------------------------------------------------
// Composite (render.h LaunchComposite; DESIGN.md section 5 "Depth layers"): one RGBA pixel from K
// layer id planes -- the front-to-back over-composite of the layers' shades under a per-triangle
// opacity table (layers_math.h), a deferred pass shaped like ResolveKernel: a block takes
// kCompositeThreads consecutive pixels of one band row, a thread one pixel. Two phases with no
// control flow that depends on loaded data between the loads: (1) the pixel's offset and its K ids
// (plane stride `plane`), (2) every layer's shading table row and opacity (an id outside the scene
// gathers row 0 and opacity[0], unused); then the arithmetic, front to back, stopping at the first
// id outside the scene. Neither reads nor builds a cull setup. No LDS, no atomics, no scratch.
// ---------------------------------------------------------------------------------------
constexpr int kCompositeThreads = 256;
struct CompositeParams {
    const float2* __restrict__ offsets;
    const int* __restrict__ ids;  // layers planes of `plane` elements
    const float* __restrict__ opacity;
    const float4* __restrict__ shade;
    F4* __restrict__ out;
    size_t plane;
    unsigned n;
    unsigned width;
    unsigned chunks;  // blocks per row
    unsigned row_begin;
    float wf, hf;
    float base[3], du[3], dv[3], bg[3];
};

template <int K>
__global__ __launch_bounds__(kCompositeThreads) void CompositeKernel(const CompositeParams q) {
    const unsigned row = blockIdx.x / q.chunks;  // (uniform: scalar)
    const unsigned chunk = blockIdx.x - row * q.chunks;
    const unsigned x = chunk * kCompositeThreads + threadIdx.x;
    // A pixel past the row loads the row's last one and is not stored.
    const size_t at = static_cast<size_t>(row) * q.width + min(x, q.width - 1u);
    // (1)
    const float2 o = q.offsets[at];
    int code[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        code[k] = __builtin_nontemporal_load(q.ids + static_cast<size_t>(k) * q.plane + at);
    }
    // (2)
    int hit[K];
    float4 nr[K], al[K];
    float a[K];
#pragma unroll
    for (int k = 0; k < K; ++k) {
        hit[k] = static_cast<unsigned>(code[k]) < q.n ? code[k] : -1;
        nr[k] = al[k] = float4{};
        a[k] = 0.f;
    }
    if (q.n != 0u) {  // (an empty scene has no row 0)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const unsigned id = static_cast<unsigned>(max(hit[k], 0));
            const float4* sr = q.shade + 2ull * id;
            nr[k] = sr[0];
            al[k] = sr[1];
            a[k] = q.opacity[id];
        }
    }
    float fx, fy;
    ResolvePosition(x, q.row_begin + row, o.x, o.y, q.wf, q.hf, fx, fy);
    CompositeAcc acc = CompositeStart();
    bool open = true;  // no id outside the scene so far
#pragma unroll
    for (int k = 0; k < K; ++k) {
        open = open && hit[k] >= 0;
        if (open) {
            const ResolveRgb c = ResolveShadeHit(q.base, q.du, q.dv, fx, fy, nr[k].x, nr[k].y, nr[k].z, nr[k].w, al[k].x,
                                                 al[k].y, al[k].z);
            CompositeAdd(acc, a[k], c);
        }
    }
    if (x < q.width) {
        const ResolveTexel t = CompositeFinish(acc, q.bg);
        __builtin_nontemporal_store(F4{t.r, t.g, t.b, t.a}, q.out + at);
    }
}

}  // namespace

hipError_t LaunchQuery(const CullSetup* setup, std::uint64_t n, const Frame& frame, std::size_t width,
                       std::size_t height, const float* d_svertices, const float* d_edges, const QueryArgs& args,
                       hipStream_t stream) {
    if (args.count == 0) {
        return hipSuccess;
    }
    if (args.positions == nullptr || args.ids == nullptr || args.t == nullptr || d_svertices == nullptr ||
        d_edges == nullptr || args.count > 0xFFFFFFFFull - kQueryBlock ||
        (setup != nullptr && (width == 0 || height == 0 || !CullBinnable(width, height) ||
                              setup->tiles != CullTiles(width, height)))) {
        return hipErrorInvalidValue;
    }
    QueryParams q{};
    const bool recompute = QueryRecords(q.rec, q.tiles_y, setup, n, frame, width, height, d_svertices, d_edges);
    const TraceParams& p = q.rec;
    q.positions = reinterpret_cast<const float2*>(args.positions);
    q.ids = args.ids;
    q.t = args.t;
    q.how = args.how;
    q.count = static_cast<unsigned>(args.count);
    q.stream_end = n == 0 ? 0u : p.n_pad;  // (an empty scene: every query misses)
    const dim3 grid(static_cast<unsigned>((args.count + kQueryBlock - 1) / kQueryBlock));
    return LaunchBySource(recompute, QueryKernel<true>, QueryKernel<false>, grid, kQueryThreads, stream, q);
}

hipError_t LaunchLayers(const CullSetup* setup, std::uint64_t n, const Frame& frame, std::size_t width,
                        std::size_t height, const float* d_svertices, const float* d_edges, const LayersArgs& args,
                        hipStream_t stream) {
    // The elements: one row of `count` positions, or row_count rows of the frame's width.
    const std::size_t row_width = args.points ? args.count : width;
    const std::size_t rows = args.points ? 1 : args.row_count;
    if (row_width == 0 || rows == 0) {
        return hipSuccess;
    }
    const std::size_t block = static_cast<std::size_t>(kLayersThreads / LayersLanes(args.points));  // positions per block
    const std::size_t chunks = (row_width + block - 1) / block;
    if (args.where == nullptr || args.ids == nullptr || d_svertices == nullptr || d_edges == nullptr ||
        args.layers == 0 || args.layers > static_cast<std::size_t>(kMaxLayers) || row_width > 0xFFFFFFFFull - block ||
        rows > 0x7FFFFFFFull / chunks ||
        (!args.points && (height == 0 || height > 0x7FFFFFFFull || args.row_begin > height ||
                          args.row_count > height - args.row_begin)) ||
        (setup != nullptr && (width == 0 || height == 0 || !CullBinnable(width, height) ||
                              setup->tiles != CullTiles(width, height)))) {
        return hipErrorInvalidValue;
    }
    LayersParams q{};
    const bool recompute = QueryRecords(q.rec, q.tiles_y, setup, n, frame, width, height, d_svertices, d_edges);
    q.where = reinterpret_cast<const float2*>(args.where);
    q.ids = args.ids;
    q.t = args.t;
    q.how = args.how;
    q.layers = static_cast<unsigned>(args.layers);
    q.width = static_cast<unsigned>(row_width);
    q.chunks = static_cast<unsigned>(chunks);
    q.row_begin = static_cast<unsigned>(args.points ? 0 : args.row_begin);
    q.plane = row_width * rows;
    q.wf = static_cast<float>(width);
    q.hf = static_cast<float>(height);
    q.stream_end = n == 0 ? 0u : q.rec.n_pad;  // (an empty scene: every position has no layers)
    const dim3 grid(static_cast<unsigned>(chunks * rows));
    const auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, grid, dim3(kLayersThreads), 0, stream, q); };
    const auto source = [&](auto points, auto cap) {
        constexpr bool kPoints = decltype(points)::value;
        constexpr int kCap = decltype(cap)::value;
        recompute ? launch(LayersKernel<true, kPoints, kCap>) : launch(LayersKernel<false, kPoints, kCap>);
    };
    const auto capacity = [&](auto points) {
        if (args.layers <= 2) {
            source(points, std::integral_constant<int, 2>{});
        } else if (args.layers <= 4) {
            source(points, std::integral_constant<int, 4>{});
        } else {
            source(points, std::integral_constant<int, 8>{});
        }
    };
    args.points ? capacity(std::true_type{}) : capacity(std::false_type{});
    return hipGetLastError();
}

template <int K>
static void LaunchCompositeLayers(unsigned layers, dim3 grid, hipStream_t stream, const CompositeParams& q) {
    if (layers == static_cast<unsigned>(K)) {
        hipLaunchKernelGGL(CompositeKernel<K>, grid, dim3(kCompositeThreads), 0, stream, q);
    } else if constexpr (K > 1) {
        LaunchCompositeLayers<K - 1>(layers, grid, stream, q);
    }
}

hipError_t LaunchComposite(const float* d_shade, std::uint64_t n, const Frame& frame, const float background[3],
                           const CompositeArgs& args, hipStream_t stream) {
    if (args.width == 0 || args.row_count == 0) {
        return hipSuccess;
    }
    const std::size_t chunks = (args.width + kCompositeThreads - 1) / kCompositeThreads;
    if (args.offsets == nullptr || args.ids == nullptr || args.rgba == nullptr || d_shade == nullptr ||
        (n != 0 && args.opacity == nullptr) || args.layers == 0 || args.layers > static_cast<std::size_t>(kMaxLayers) ||
        n > 0xFFFFFFFFull || args.width > 0xFFFFFFFFull - kCompositeThreads || args.height == 0 ||
        args.row_begin > args.height || args.row_count > args.height - args.row_begin ||
        args.height > 0x7FFFFFFFull || args.row_count > 0x7FFFFFFFull / chunks) {
        return hipErrorInvalidValue;
    }
    CompositeParams q{};
    q.offsets = reinterpret_cast<const float2*>(args.offsets);
    q.ids = args.ids;
    q.opacity = args.opacity;
    q.shade = reinterpret_cast<const float4*>(d_shade);
    q.out = reinterpret_cast<F4*>(args.rgba);
    q.plane = args.width * args.row_count;
    q.n = static_cast<unsigned>(n);
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
    LaunchCompositeLayers<kMaxLayers>(static_cast<unsigned>(args.layers), dim3(static_cast<unsigned>(chunks * args.row_count)),
                                      stream, q);
    return hipGetLastError();
}

}  // namespace srt
