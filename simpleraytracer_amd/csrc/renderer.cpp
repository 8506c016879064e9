#include "renderer.h"

#include <rccl/rccl.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <type_traits>

#include "comm.h"
#include "engine.h"
#include "lighting_math.h"
#include "radiance.h"
#include "rays.h"
#include "render.h"
#include "visibility.h"

namespace srt {
namespace {

template <class T>
T* DeviceAlloc(std::size_t count, const char* what) {
    void* p = nullptr;
    HipCheck(hipMalloc(&p, count * sizeof(T)), what);
    return static_cast<T*>(p);
}

bool CullBinningEnabled() {
    const char* v = std::getenv("SRT_CULL_BIN");
    return v == nullptr || std::strcmp(v, "0") != 0;
}

GatherMode GatherModeFor(const std::vector<int>& devices) {
    const char* v = std::getenv("SRT_GATHER");
    if (v != nullptr && std::strcmp(v, "direct") == 0) {
        return GatherMode::kDirect;
    }
    if (v != nullptr && std::strcmp(v, "copy") == 0) {
        return GatherMode::kCopy;
    }
    if (v != nullptr && std::strcmp(v, "rccl") == 0) {
        return GatherMode::kRccl;
    }
    for (std::size_t i = 0; i < devices.size(); ++i) {
        for (std::size_t j = 0; j < i; ++j) {
            if (devices[i] == devices[j]) {
                return GatherMode::kCopy;  // one device twice: no RCCL communicator
            }
        }
    }
    return GatherMode::kRccl;
}

}  // namespace

void HipCheck(hipError_t err, const char* what) {
    if (err != hipSuccess) {
        throw std::runtime_error(std::string("HIP error: ") + what + ": " + hipGetErrorString(err));
    }
}

std::vector<int> VisibleDevices() {
    int count = 0;
    hipError_t err = hipGetDeviceCount(&count);
    if (err != hipSuccess || count <= 0) {
        throw std::runtime_error(std::string("HIP error: no HIP device available (") +
                                 (err != hipSuccess ? hipGetErrorString(err) : "device count 0") +
                                 "); set ML_VISIBLE_DEVICES=cpu to render on the CPU backend");
    }
    std::vector<int> devices;
    const char* env = std::getenv("ML_VISIBLE_DEVICES");
    if (env == nullptr || *env == '\0') {
        devices.push_back(0);
        return devices;
    }
    std::stringstream ss(env);
    std::string item;
    while (std::getline(ss, item, ',')) {
        char* end = nullptr;
        long v = std::strtol(item.c_str(), &end, 10);
        if (item.empty() || *end != '\0' || v < 0 || v >= count) {
            throw std::runtime_error("Bad ML_VISIBLE_DEVICES entry '" + item + "' (" + std::to_string(count) +
                                     " HIP devices present)");
        }
        devices.push_back(static_cast<int>(v));
    }
    if (devices.empty()) {
        devices.push_back(0);
    }
    return devices;
}

int TraceVariantFromEnv() {
    const char* v = std::getenv("SRT_TRACE_VARIANT");
    if (v != nullptr && (std::strcmp(v, "scalar") == 0 || std::strcmp(v, "1") == 0)) {
        return kTraceScalar;
    }
    if (v != nullptr && (std::strcmp(v, "lds") == 0 || std::strcmp(v, "0") == 0)) {
        return kTraceLds;
    }
    if (v != nullptr && (std::strcmp(v, "bvh") == 0 || std::strcmp(v, "3") == 0)) {
        return kTraceBvh;
    }
    return kTraceCull;
}

DeviceScene::DeviceScene(const Scene& scene, int device)
    : m_device(device), m_n(scene.triangle_count()), m_camera(scene.camera) {
    std::memcpy(m_background, scene.background, sizeof(m_background));
    DeviceGuard guard(device);
    try {
        m_vertices = DeviceAlloc<float>(m_n * 9, "hipMalloc(vertices)");
        m_shade = DeviceAlloc<float>(m_n == 0 ? 8 : m_n * 8, "hipMalloc(shading table)");
        m_edges = DeviceAlloc<float>(PaddedTriangleCount(m_n) * kEdgeFloatsPerTriangle, "hipMalloc(edges)");
        m_order = DeviceAlloc<unsigned>(m_n == 0 ? 1 : m_n, "hipMalloc(order)");
        m_rank = DeviceAlloc<unsigned>(m_n == 0 ? 1 : m_n, "hipMalloc(rank)");
        m_svertices = DeviceAlloc<float>((m_n == 0 ? 1 : m_n) * kSpatialStride, "hipMalloc(spatial vertices)");
        HipCheck(hipMemcpy(m_vertices, scene.vertices.data(), m_n * 9 * sizeof(float), hipMemcpyHostToDevice),
                 "hipMemcpy(vertices)");
        // The records' spatial order, built on the device (spatial.hip), timed.
        hipEvent_t b0 = nullptr, b1 = nullptr;
        HipCheck(hipEventCreate(&b0), "hipEventCreate(order build)");
        if (hipEventCreate(&b1) != hipSuccess) {
            (void)hipEventDestroy(b0);
            throw std::runtime_error("HIP error: hipEventCreate(order build)");
        }
        try {
            BuildSpatialOrder(m_vertices, m_n, m_camera, m_order, m_rank, m_svertices, nullptr, b0, b1);
            float ms = 0.f;
            if (m_n != 0 && hipEventElapsedTime(&ms, b0, b1) == hipSuccess) {
                m_build_ms = ms;
            }
        } catch (...) {
            (void)hipEventDestroy(b0);
            (void)hipEventDestroy(b1);
            throw;
        }
        (void)hipEventDestroy(b0);
        (void)hipEventDestroy(b1);
        if (m_n != 0) {  // the shading table from the vertices and the albedo (staged, then freed)
            float* albedo = DeviceAlloc<float>(m_n * 3, "hipMalloc(albedo)");
            hipError_t e = hipMemcpy(albedo, scene.albedo.data(), m_n * 3 * sizeof(float), hipMemcpyHostToDevice);
            if (e == hipSuccess) {
                e = LaunchShadeTable(m_vertices, albedo, m_n, m_shade, nullptr);
            }
            if (e == hipSuccess) {
                e = hipStreamSynchronize(nullptr);
            }
            (void)hipFree(albedo);
            HipCheck(e, "shading table");
        }
    } catch (...) {
        (void)hipFree(m_vertices);
        (void)hipFree(m_shade);
        (void)hipFree(m_edges);
        (void)hipFree(m_order);
        (void)hipFree(m_rank);
        (void)hipFree(m_svertices);
        throw;
    }
}

DeviceScene::~DeviceScene() {
    int prev = -1;
    (void)hipGetDevice(&prev);
    (void)hipSetDevice(m_device);
    (void)hipFree(m_vertices);
    (void)hipFree(m_shade);
    (void)hipFree(m_edges);
    (void)hipFree(m_order);
    (void)hipFree(m_rank);
    (void)hipFree(m_svertices);
    if (m_scratch != nullptr) {
        FreeOrderScratch(*m_scratch);
        delete m_scratch;
    }
    if (m_rays != nullptr) {
        FreeRayTree(*m_rays);
        delete m_rays;
    }
    (void)hipFree(m_block_ext);
    (void)hipFree(m_setup);
    (void)hipFree(m_stream);
    m_pins.Clear();
    for (const PinTable::Buffers& b : m_pins.TakeRetired()) {
        ReleasePinBuffers(b);
    }
    for (void* e : m_free_pin_events) {
        (void)hipEventDestroy(static_cast<hipEvent_t>(e));
    }
    for (void* chunk : m_pin_word_chunks) {
        (void)hipHostFree(chunk);
    }
    for (CullArena& a : m_arenas) {
        (void)hipFree(a.work);
    }
    (void)hipFree(m_bvh);
    for (hipEvent_t e : m_events) {
        (void)hipEventDestroy(e);
    }
    for (hipEvent_t e : m_prep_events) {
        (void)hipEventDestroy(e);
    }
    for (hipEvent_t e : m_order_events) {
        if (e != nullptr) {
            (void)hipEventDestroy(e);
        }
    }
    for (ParamTable& t : m_tables) {
        if (t.uploaded != nullptr) {
            (void)hipEventSynchronize(t.uploaded);
            (void)hipEventDestroy(t.uploaded);
        }
        (void)hipFree(t.device);
        (void)hipHostFree(t.host);
    }
    if (prev >= 0) {
        (void)hipSetDevice(prev);
    }
}

void DeviceScene::Prepare(std::size_t width, std::size_t height, hipStream_t stream) {
    if (width == 0 || height == 0) {
        throw std::runtime_error("Prepare: frame dimensions must be non-zero");
    }
    if (width != m_width || height != m_height) {
        DropPlans(~std::size_t{0});  // (a plan is scheduling only; a new shape deserves a new one)
        if (!m_pins.empty()) {  // pinned facts are of the old tile grid: the caller pins again if it wants
            m_pins.Clear();
            ReleaseRetiredPins();
        }
    }
    const Frame frame = MakeFrame(m_camera, width, height);
    if (width != m_width || height != m_height || std::memcmp(&frame, &m_frame, sizeof(Frame)) != 0) {
        m_setup_pending = true;  // the shared cull setup is a function of this frame (EnsureSetup's key: the rest)
    }
    m_frame = frame;
    m_width = width;
    m_height = height;
    // Deferred: the next Trace enqueues the record setup on its stream (the binned cull path
    // computes the records inside its bin kernel on every call, render.hip PrepareBinKernel).
    (void)stream;
    m_prepare_pending = true;
    m_ext_pending = true;
}

// What a pose shapes, and how each piece comes back (DESIGN.md section 5 "Motion"):
//   m_frame                      recomputed here, as Prepare(W, H) would (a prepared scene stays prepared);
//   edge slot 0, the BVH boxes   the next unbinned trace's record pass (m_prepare_pending; the bvh
//                                trace rebuilds its boxes from the records on every call);
//   m_block_ext                  the next binned trace (m_ext_pending);
//   the shared setup, its record stream and plan counts (m_stream_on, m_stream_records,
//   m_list_descs, m_empty_descs) the next whole-frame trace or query (m_setup_pending, set here
//                                explicitly: Prepare sets it only when the frame's bytes changed, and
//                                moved vertices leave the frame identical);
//   every arena's per-slot plans DropPlans: scheduling only, but built from the old pose's bins.
// The per-slot counters reset themselves at the end of the launches that use them, and an update is
// stream-ordered after those, so they are left alone, as are the count parity (CullSlotState::uses),
// m_cull_gen and the parameter tables (rewritten per call). Nothing else is keyed on the pose:
// m_vertices, m_shade, m_order, m_rank and m_svertices are rewritten by the update itself.
void DeviceScene::PoseChanged(bool vertices) {
    (void)vertices;  // (a camera move invalidates all a vertex move does: every cache reads both)
    if (m_width != 0) {
        m_frame = MakeFrame(m_camera, m_width, m_height);
    }
    m_prepare_pending = true;
    m_ext_pending = true;
    m_setup_pending = true;
    m_stream_on = false;
    m_stream_records = 0;
    m_list_descs = 0;
    m_empty_descs = 0;
    DropPlans(~std::size_t{0});
}

void DeviceScene::SetCamera(const Camera& camera, bool reorder, hipStream_t stream) {
    if (reorder && m_n != 0) {
        if (m_scratch == nullptr) {
            m_scratch = new OrderScratch{};
        }
        AllocOrderScratch(*m_scratch, m_n, stream);  // (first use only)
        OrderAfterPrevious(stream);
        EnqueueMotion(m_vertices, m_n, camera, nullptr, m_scratch, m_order, m_rank, m_svertices, stream);
        RecordOrder(stream);
    }
    m_camera = camera;
    PoseChanged(false);
}

void DeviceScene::SetVertices(const float* d_vertices, bool reorder, hipStream_t stream) {
    if (m_n == 0) {
        return;
    }
    if (reorder) {
        if (m_scratch == nullptr) {
            m_scratch = new OrderScratch{};
        }
        AllocOrderScratch(*m_scratch, m_n, stream);  // (first use only)
    }
    OrderAfterPrevious(stream);
    m_rays_stale = true;  // the world-space tree is a function of the vertices alone (rays.h)
    HipCheck(hipMemcpyAsync(m_vertices, d_vertices, m_n * 9 * sizeof(float), hipMemcpyDeviceToDevice, stream),
             "hipMemcpyAsync(vertices)");
    // (a failed enqueue below leaves the copy queued: the pose counts as changed either way)
    try {
        EnqueueMotion(m_vertices, m_n, m_camera, m_shade, reorder ? m_scratch : nullptr, m_order, m_rank, m_svertices,
                      stream);
    } catch (...) {
        PoseChanged(true);
        throw;
    }
    RecordOrder(stream);
    PoseChanged(true);
}

// Ray queries (rays.h). The tree is keyed on the vertices only, so PoseChanged leaves it alone and
// SetVertices marks it stale itself.
const RayTree* DeviceScene::EnsureRayTree(hipStream_t stream) const {
    const char* mode = std::getenv("SRT_RAYS");
    if (m_n == 0 || (mode != nullptr && std::strcmp(mode, "brute") == 0)) {
        return nullptr;
    }
    if (m_rays == nullptr) {
        RayTree* tree = new RayTree{};
        try {
            AllocRayTree(*tree, m_n, stream);
        } catch (...) {
            delete tree;
            throw;
        }
        m_rays = tree;
        m_rays_stale = true;
        ++m_ray_stats.allocations;
    }
    if (m_rays_stale) {
        EnqueueRayTreeBuild(*m_rays, m_vertices, m_n, stream);
        m_rays_stale = false;
        ++m_ray_stats.builds;
    }
    return m_rays;
}

void DeviceScene::LogRayStats() const {
    const char* e = std::getenv("SRT_SETUP_LOG");
    if (e == nullptr || *e == '\0' || std::strcmp(e, "0") == 0) {
        return;
    }
    std::fprintf(stderr, "srt rays: scene %p builds %llu allocations %llu\n", static_cast<const void*>(this),
                 m_ray_stats.builds, m_ray_stats.allocations);
    std::fflush(stderr);
}

void DeviceScene::BuildRays(hipStream_t stream) const {
    OrderAfterPrevious(stream);
    try {
        (void)EnsureRayTree(stream);
    } catch (...) {
        m_rays_stale = true;
        RecordOrder(stream);
        throw;
    }
    RecordOrder(stream);
    LogRayStats();
}

void DeviceScene::Closest(const float* d_rays, std::size_t count, int* d_ids, float* d_t, float* d_bary,
                          hipStream_t stream) const {
    if (count == 0) {
        return;
    }
    OrderAfterPrevious(stream);
    try {
        const RayTree* tree = EnsureRayTree(stream);
        LaunchRayClosest(tree, m_vertices, m_n, d_rays, count, d_ids, d_t, d_bary, stream);
    } catch (...) {
        RecordOrder(stream);
        throw;
    }
    RecordOrder(stream);
    LogRayStats();
}

void DeviceScene::Occluded(const float* d_rays, std::size_t count, unsigned char* d_out, hipStream_t stream) const {
    if (count == 0) {
        return;
    }
    OrderAfterPrevious(stream);
    try {
        const RayTree* tree = EnsureRayTree(stream);
        LaunchRayOccluded(tree, m_vertices, m_n, d_rays, count, d_out, stream);
    } catch (...) {
        RecordOrder(stream);
        throw;
    }
    RecordOrder(stream);
    LogRayStats();
}

// Sampled visibility (visibility.h): elements as GBuffer's, the tree as Closest's.
namespace {

VisibilityElements ElementsOf(bool points, const float* d_where, const int* d_ids, std::size_t row_begin,
                              std::size_t count, std::size_t width, std::size_t height) {
    return VisibilityElements{points, d_where, d_ids, points ? count : width, points ? 1 : count,
                              points ? 0 : row_begin, width, height};
}

}  // namespace

void DeviceScene::Visibility(bool points, const float* d_where, const int* d_ids, std::size_t row_begin,
                             std::size_t count, const VisibilityGen& gen, unsigned char* d_visible, float* d_fraction,
                             hipStream_t stream) const {
    if (m_width == 0) {
        throw std::runtime_error("Visibility: Prepare() has not been called");
    }
    if (!points && (row_begin > m_height || count > m_height - row_begin)) {
        throw std::runtime_error("Visibility: row band outside the frame");
    }
    if (count == 0 || (d_visible == nullptr && d_fraction == nullptr)) {
        return;
    }
    OrderAfterPrevious(stream);
    try {
        const RayTree* tree = EnsureRayTree(stream);
        LaunchVisibility(tree, m_vertices, m_n, m_frame, ElementsOf(points, d_where, d_ids, row_begin, count, m_width, m_height),
                         gen, d_visible, d_fraction, stream);
    } catch (...) {
        RecordOrder(stream);
        throw;
    }
    RecordOrder(stream);
    LogRayStats();
}

void DeviceScene::VisibilityRays(bool points, const float* d_where, const int* d_ids, std::size_t row_begin,
                                 std::size_t count, const VisibilityGen& gen, float* d_rays, hipStream_t stream) const {
    if (m_width == 0) {
        throw std::runtime_error("Visibility rays: Prepare() has not been called");
    }
    if (!points && (row_begin > m_height || count > m_height - row_begin)) {
        throw std::runtime_error("Visibility rays: row band outside the frame");
    }
    if (count == 0) {
        return;
    }
    OrderAfterPrevious(stream);
    try {
        LaunchVisibilityRays(m_vertices, m_n, m_frame, ElementsOf(points, d_where, d_ids, row_begin, count, m_width, m_height),
                             gen, d_rays, stream);
    } catch (...) {
        RecordOrder(stream);
        throw;
    }
    RecordOrder(stream);
}

// The block extents of the prepared frame, once per Prepare (on the first binned trace's stream,
// before its launches). They depend on the scene, its camera and W x H only, like the spatial order.
void DeviceScene::EnsureBlockExtents(hipStream_t stream) const {
    static const bool enabled = [] {
        const char* v = std::getenv("SRT_BLOCK_SKIP");
        return v == nullptr || std::strcmp(v, "0") != 0;
    }();
    if (!enabled || !m_ext_pending || m_n == 0) {
        return;
    }
    if (m_block_ext == nullptr) {
        m_block_ext = DeviceAlloc<float2>(BlockExtentCount(m_n), "hipMalloc(block extents)");
    }
    HipCheck(LaunchBlockExtents(m_svertices, m_n, m_frame, m_block_ext, stream), "block extents launch");
    m_ext_pending = false;
}

void DeviceScene::OrderAfterPrevious(hipStream_t stream) const {
    if (m_used && stream != m_last_stream) {
#if SRT_ORDER_EVENTS == 0
        HipCheck(hipEventRecord(m_order_events[0], m_last_stream), "hipEventRecord(scene order)");
#endif
        HipCheck(hipStreamWaitEvent(stream, m_order_events[m_order_next], 0), "hipStreamWaitEvent(scene order)");
    }
#if SRT_ORDER_EVENTS == 0
    if (m_order_events[0] == nullptr) {
        HipCheck(hipEventCreateWithFlags(&m_order_events[0], hipEventDisableTiming), "hipEventCreate(scene order)");
    }
    m_used = true;
    m_last_stream = stream;
#endif
}

// Marks the end of this call's work on `stream`: the next call on another stream waits for it. The
// event is recorded on the call's own stream, so the library never touches a stream after the call
// that was given it has returned (the caller may destroy it). A ring of events: recording an
// event whose previous record is still pending can stall the host, so consecutive calls use
// different events and only the newest is waited on.
void DeviceScene::RecordOrder(hipStream_t stream) const {
#if SRT_ORDER_EVENTS > 0
    const std::size_t k = (m_order_next + 1) % kOrderEvents;
    if (m_order_events[k] == nullptr) {
        HipCheck(hipEventCreateWithFlags(&m_order_events[k], hipEventDisableTiming), "hipEventCreate(scene order)");
    }
    HipCheck(hipEventRecord(m_order_events[k], stream), "hipEventRecord(scene order)");
    m_order_next = k;
    m_used = true;
    m_last_stream = stream;
#else
    (void)stream;
#endif
}

void DeviceScene::Shade(const float* d_offsets, const int* d_ids, float* d_rgba, std::size_t row_begin,
                        std::size_t row_count, hipStream_t stream, std::size_t frames, std::size_t band_rows,
                        std::size_t interleaved, std::size_t offsets_stride, int id_planes, long skip_band,
                        std::size_t own_bands, std::size_t first_rows) const {
    if (id_planes >= 0 && id_planes != IdPlanes(m_n)) {
        throw std::runtime_error("Shade: packed ids of this scene have " + std::to_string(IdPlanes(m_n)) + " bit planes");
    }
    if (m_width == 0) {
        throw std::runtime_error("Shade: Prepare() has not been called");
    }
    if (interleaved > 0) {  // every band the ids hold (from own_bands on) fits a band_rows-row buffer
        bool fits = row_begin == 0;
        for (std::size_t j = own_bands; j < interleaved && fits; ++j) {
            fits = band_rows >= InterleavedBandRows(m_height, interleaved, j);
        }
        if (!fits) {
            throw std::runtime_error("Shade: interleaved bands cover the whole frame in band_rows-row buffers");
        }
    }
    if (row_begin + row_count > m_height) {
        throw std::runtime_error("Shade: row band outside the frame");
    }
    if (band_rows > row_count || frames > 65535) {
        throw std::runtime_error("Shade: band_rows exceeds the rows shaded, or more than 65535 frames");
    }
    if (first_rows > row_count || (first_rows != 0 && interleaved > 0)) {
        throw std::runtime_error("Shade: first_rows exceeds the rows shaded, or with interleaved bands");
    }
    if (row_count == 0 || frames == 0) {
        return;
    }
    OrderAfterPrevious(stream);
    BandArgs band{d_offsets, d_rgba, m_width, m_height, row_begin, row_count, const_cast<int*>(d_ids)};
    band.id_planes = id_planes;
    HipCheck(LaunchShade(m_vertices, m_shade, m_edges, m_n, m_frame, m_background, band, stream, frames, band_rows,
                         interleaved, offsets_stride, skip_band, own_bands, first_rows),
             "shade kernel launch");
    RecordOrder(stream);
}

void DeviceScene::GBuffer(bool points, const float* d_where, const int* d_ids, std::size_t row_begin,
                          std::size_t count, float* d_depth, float* d_bary, float* d_normal, float* d_albedo,
                          hipStream_t stream) const {
    if (m_width == 0) {
        throw std::runtime_error("GBuffer: Prepare() has not been called");
    }
    if (!points && (row_begin > m_height || count > m_height - row_begin)) {
        throw std::runtime_error("GBuffer: row band outside the frame");
    }
    if (count == 0 || (d_depth == nullptr && d_bary == nullptr && d_normal == nullptr && d_albedo == nullptr)) {
        return;
    }
    OrderAfterPrevious(stream);
    // (points: one row of `count` elements)
    const GBufferArgs args{points, d_where, d_ids, points ? count : m_width, m_height, points ? 0 : row_begin,
                           points ? 1 : count, d_depth, d_bary, d_normal, d_albedo};
    HipCheck(LaunchGBuffer(m_vertices, m_shade, m_n, m_frame, m_background, args, stream), "G-buffer launch");
    LogSetupStats();  // (the counters as they stand: this call builds nothing)
    RecordOrder(stream);
}

void DeviceScene::Surface(bool points, const float* d_where, const int* d_ids, std::size_t row_begin, std::size_t count,
                          const SurfaceArgs& planes, hipStream_t stream) const {
    if (m_width == 0) {
        throw std::runtime_error("Surface: Prepare() has not been called");
    }
    if (!points && (row_begin > m_height || count > m_height - row_begin)) {
        throw std::runtime_error("Surface: row band outside the frame");
    }
    if (count == 0 ||
        (planes.normal == nullptr && planes.albedo == nullptr && planes.rgba == nullptr && planes.uv == nullptr)) {
        return;
    }
    OrderAfterPrevious(stream);
    SurfaceArgs args = planes;
    args.points = points;
    args.where = d_where;
    args.ids = d_ids;
    args.width = points ? count : m_width;  // (points: one row of `count` elements)
    args.height = m_height;
    args.row_begin = points ? 0 : row_begin;
    args.row_count = points ? 1 : count;
    HipCheck(LaunchSurface(m_vertices, m_shade, m_n, m_frame, m_background, args, stream), "surface launch");
    LogSetupStats();  // (the counters as they stand: this call builds nothing)
    RecordOrder(stream);
}

void DeviceScene::Interpolate(bool points, const float* d_where, const int* d_ids, std::size_t row_begin,
                              std::size_t count, const float* d_table, std::size_t channels, float* d_out,
                              hipStream_t stream) const {
    if (m_width == 0) {
        throw std::runtime_error("Interpolate: Prepare() has not been called");
    }
    if (!points && (row_begin > m_height || count > m_height - row_begin)) {
        throw std::runtime_error("Interpolate: row band outside the frame");
    }
    if (count == 0) {
        return;
    }
    OrderAfterPrevious(stream);
    const InterpolateArgs args{points, d_where, d_ids, points ? count : m_width, m_height, points ? 0 : row_begin,
                               points ? 1 : count, d_table, channels, d_out};
    HipCheck(LaunchInterpolate(m_vertices, m_n, m_frame, args, stream), "interpolation launch");
    LogSetupStats();
    RecordOrder(stream);
}

void DeviceScene::Resolve(const float* const* d_offsets, const int* const* d_ids, std::size_t samples,
                          std::size_t row_begin, std::size_t row_count, float* d_rgba, hipStream_t stream) const {
    if (m_width == 0) {
        throw std::runtime_error("Resolve: Prepare() has not been called");
    }
    if (samples == 0 || samples > static_cast<std::size_t>(kMaxSamples)) {
        throw std::runtime_error("Resolve: samples must be 1 to " + std::to_string(kMaxSamples) + ", got " +
                                 std::to_string(samples));
    }
    if (row_begin > m_height || row_count > m_height - row_begin) {
        throw std::runtime_error("Resolve: row band outside the frame");
    }
    if (row_count == 0) {
        return;
    }
    OrderAfterPrevious(stream);
    const ResolveArgs args{d_offsets, d_ids, samples, m_width, m_height, row_begin, row_count, d_rgba};
    HipCheck(LaunchResolve(m_shade, m_n, m_frame, m_background, args, stream), "resolve launch");
    LogSetupStats();  // (the counters as they stand: this call builds nothing)
    RecordOrder(stream);
}

void DeviceScene::RenderSamples(const float* const* d_offsets, int* const* d_ids, std::size_t samples, float* d_rgba,
                                int variant, hipStream_t stream) const {
    if (m_width == 0) {
        throw std::runtime_error("RenderSamples: Prepare() has not been called");
    }
    if (samples == 0 || samples > static_cast<std::size_t>(kMaxSamples)) {
        throw std::runtime_error("RenderSamples: samples must be 1 to " + std::to_string(kMaxSamples) + ", got " +
                                 std::to_string(samples));
    }
    // Every chunk on the trace grid of the largest one: the shared setup is keyed by it, so a
    // remainder chunk with a grid of its own would build the setup again.
    const std::size_t chunk = std::min(samples, static_cast<std::size_t>(kMaxBatch));
    for (std::size_t s = 0; s < samples; s += chunk) {
        TraceBatch(d_offsets + s, nullptr, d_ids + s, std::min(chunk, samples - s), 0, m_height, variant, stream, 1, -1,
                   false, nullptr, chunk);
    }
    Resolve(d_offsets, d_ids, samples, 0, m_height, d_rgba, stream);
}

// Grow-only cull work for `slots` frame slots of one carve-up (render.h CullBins; counters reset
// themselves, so a slot's counters are zero-filled only on its first use with this carve-up), in the
// arena of this band shape.
void DeviceScene::EnsureCullWork(std::size_t slots, std::size_t row_count, hipStream_t stream) const {
    const std::size_t bytes = CullBinBytes(m_n, m_width, row_count);
    const std::uint64_t shape = (static_cast<std::uint64_t>(m_width) << 32) | row_count;
    std::size_t pick = m_arenas.size();
    for (std::size_t i = 0; i < m_arenas.size(); ++i) {
        if (m_arenas[i].shape == shape && m_arenas[i].layout == bytes) {
            pick = i;
        }
    }
    if (pick == m_arenas.size()) {  // a new shape: a new arena, or the least recently used one re-carved
        if (m_arenas.size() < kCullArenas) {
            m_arenas.emplace_back();
        } else {
            pick = 0;
            for (std::size_t i = 1; i < m_arenas.size(); ++i) {
                pick = m_arenas[i].used < m_arenas[pick].used ? i : pick;
            }
        }
        CullArena& a = m_arenas[pick];
        a.shape = shape;
        a.layout = bytes;
        a.zeroed = 0;  // (stream order: earlier launches on this arena ran before its counters are reset)
    }
    CullArena& a = m_arenas[pick];
    if (slots * bytes > a.bytes) {
        HipCheck(hipStreamSynchronize(stream), "hipStreamSynchronize(cull work)");
        (void)hipFree(a.work);
        a.work = nullptr;
        a.bytes = 0;
        a.work = DeviceAlloc<unsigned char>(slots * bytes, "hipMalloc(cull work)");
        a.bytes = slots * bytes;
        a.zeroed = 0;
    }
    if (slots > a.zeroed) {
        // Only each slot's leading counters (render.h CullBins): zeroing whole slots (~30 MB each,
        // mostly split-key slices) cost 0.4-0.5 ms per 64-frame batch whenever a shape was re-carved.
        HipCheck(hipMemset2DAsync(a.work + a.zeroed * bytes, bytes, 0, CullBinCounterBytes(m_n, m_width, row_count),
                                  slots - a.zeroed, stream),
                 "hipMemset2DAsync(cull work)");
        a.state.resize(std::max(a.state.size(), slots));
        for (std::size_t k = a.zeroed; k < slots; ++k) {
            a.state[k] = CullSlotState{};  // zeroed: no plan
        }
        a.zeroed = slots;
    }
    a.used = ++m_cull_clock;
    m_arena = pick;
}

void DeviceScene::DropPlans(std::size_t slots) const {
    for (CullArena& a : m_arenas) {
        for (std::size_t k = 0; k < slots && k < a.state.size(); ++k) {
            a.state[k].plan_descs = 0;
        }
    }
}


CullBins DeviceScene::CullSlot(std::size_t slot, std::size_t row_count, unsigned descs) const {
    CullArena& a = m_arenas.at(m_arena);  // (EnsureCullWork picked and sized it)
    CullSlotState& st = a.state.at(slot);
    CullBins bins = CullBinLayout(a.work + slot * a.layout, m_n, m_width, row_count, st.uses & 1u);
    bins.descs = std::min(bins.descs, descs);
    bins.plan = st.plan_descs != bins.descs;  // (render.hip WorkPlan: the launch may order anyway)
    st.plan_descs = bins.descs;
    ++st.uses;
    bins.order = m_order;
    bins.svertices = m_svertices;
    bins.block_ext = m_ext_pending ? nullptr : m_block_ext;
    m_cull_gen = m_cull_gen + 1u == 0u ? 1u : m_cull_gen + 1u;
    bins.gen = m_cull_gen;
    return bins;
}

// Edge records for `slots` frame slots (slot 0 is the one Prepare / Trace / Shade use). Growing
// drops the prepared records, so the next trace recomputes them.
void DeviceScene::EnsureEdgeSlots(std::size_t slots, hipStream_t stream) const {
    if (slots <= m_edge_slots) {
        return;
    }
    HipCheck(hipStreamSynchronize(stream), "hipStreamSynchronize(edges)");
    const std::size_t floats = PaddedTriangleCount(m_n) * kEdgeFloatsPerTriangle;
    float* grown = DeviceAlloc<float>(slots * floats, "hipMalloc(edges)");
    (void)hipFree(m_edges);
    m_edges = grown;
    m_edge_slots = slots;
    m_prepare_pending = true;
}

DeviceScene::ParamTable& DeviceScene::AcquireTable(std::size_t frames, hipStream_t stream) const {
    ParamTable& t = m_tables[m_table_next];
    m_table_next = (m_table_next + 1) % kParamTables;
    if (t.pending) {
        HipCheck(hipEventSynchronize(t.uploaded), "hipEventSynchronize(parameter table)");
        t.pending = false;
    }
    if (t.frames < frames) {
        // Every table of the ring grows at once (one stall, on the first large call, instead of one at
        // the first use of each). Launches queued earlier may still read an old device table. They all
        // run before `stream`'s current end (calls on one scene are stream-ordered: OrderAfterPrevious
        // ran first), so draining this stream suffices -- never a device-wide sync from an engine worker
        // (other workers' queues and RCCL kernels waiting on peers would be waited for too).
        HipCheck(hipStreamSynchronize(stream), "hipStreamSynchronize(parameter table)");
        const std::size_t bytes = CullTableBytes(frames);
        for (ParamTable& r : m_tables) {
            if (r.frames >= frames) {
                continue;
            }
            r.pending = false;  // (its uploads ran: the stream is drained)
            (void)hipFree(r.device);
            (void)hipHostFree(r.host);
            r.device = nullptr;
            r.host = nullptr;
            r.host_device = nullptr;
            r.frames = 0;
            HipCheck(hipMalloc(&r.device, bytes), "hipMalloc(parameter table)");
            // Mapped and fine-grained (coherent): the upload kernel reads it over the bus, uncached,
            // so a table rewritten for a later launch is never read stale from the L2.
            HipCheck(hipHostMalloc(&r.host, bytes, hipHostMallocMapped | hipHostMallocCoherent),
                     "hipHostMalloc(parameter table)");
            HipCheck(hipHostGetDevicePointer(&r.host_device, r.host, 0), "hipHostGetDevicePointer(parameter table)");
            r.frames = frames;
        }
    }
    if (t.uploaded == nullptr) {
        HipCheck(hipEventCreateWithFlags(&t.uploaded, hipEventDisableTiming), "hipEventCreate(parameter table)");
    }
    return t;
}

void DeviceScene::TraceBatch(const float* const* d_offsets, float* const* d_rgba, int* const* d_ids, std::size_t frames,
                             std::size_t row_begin, std::size_t row_count, int variant, hipStream_t stream,
                             std::size_t row_interleave, int id_planes, bool rgba_frame_rows,
                             const std::size_t* row_begins, std::size_t plan_frames) const {
    if (id_planes >= 0 && (id_planes != IdPlanes(m_n) || variant != kTraceCull)) {
        throw std::runtime_error("TraceBatch: packed ids need the cull variant and " + std::to_string(IdPlanes(m_n)) +
                                 " bit planes for this scene");
    }
    if (m_width == 0) {
        throw std::runtime_error("TraceBatch: Prepare() has not been called");
    }
    if (!BandFits(row_begin, row_count, row_interleave, m_height)) {
        throw std::runtime_error("TraceBatch: row band outside the frame");
    }
    bool same_begin = true;  // render.hip LaunchCullFrames: per-frame first rows compute their tile info first
    for (std::size_t f = 0; row_begins != nullptr && f < frames; ++f) {
        if (!BandFits(row_begins[f], row_count, row_interleave, m_height)) {
            throw std::runtime_error("TraceBatch: per-frame bands must lie inside the frame");
        }
        same_begin = same_begin && row_begins[f] == row_begins[0];
    }
    if (row_begins != nullptr && (variant != kTraceCull || !CullBinningEnabled() || !CullBinnable(m_width, row_count))) {
        throw std::runtime_error("TraceBatch: per-frame bands need the binned cull variant");
    }
    if (frames > static_cast<std::size_t>(kMaxTableFrames)) {
        throw std::runtime_error("TraceBatch: at most " + std::to_string(kMaxTableFrames) + " frames per batch");
    }
    if (frames == 0 || row_count == 0) {
        return;
    }
    if (variant != kTraceCull || !CullBinningEnabled() || !CullBinnable(m_width, row_count)) {
        for (std::size_t f = 0; f < frames; ++f) {  // frame by frame, each with its own record setup
            m_prepare_pending = true;
            int* ids_f = d_ids != nullptr ? d_ids[f] : nullptr;
            Trace(d_offsets[f], d_rgba != nullptr ? d_rgba[f] : nullptr, row_begin, row_count, variant, stream, ids_f,
                  row_interleave, ids_f != nullptr ? id_planes : -1, rgba_frame_rows);
        }
        return;
    }
    if (row_begins == nullptr && OnSharedSetup(row_begin, row_count, row_interleave)) {
        TraceShared(d_offsets, d_rgba, d_ids, frames, stream, id_planes, rgba_frame_rows,
                    std::max(frames, plan_frames));
        return;
    }
    m_setup_stats.per_frame_frames += frames;
    LogSetupStats();
    OrderAfterPrevious(stream);
    EnsureEdgeSlots(frames, stream);
    EnsureCullWork(frames, row_count, stream);
    EnsureBlockExtents(stream);
    std::vector<CullBins> bins(frames);
    std::vector<CullFrame> cf(frames);
    const std::size_t floats = PaddedTriangleCount(m_n) * kEdgeFloatsPerTriangle;
    // The trace grid for the whole batch: its frames' parts together fill the chip sooner (a
    // 135-row band alone splits 5 ways; eight of them do not need to).
    const unsigned batch_descs = CullDescriptors(CullTiles(m_width, row_count), frames);
    const bool recompute = RecomputeRecords(frames);
    for (std::size_t f = 0; f < frames; ++f) {
        bins[f] = CullSlot(f, row_count, batch_descs);
        bins[f].recompute = recompute;
        cf[f].edges = m_edges + f * floats;
        cf[f].bins = &bins[f];
        cf[f].band = BandArgs{d_offsets[f], d_rgba != nullptr ? d_rgba[f] : nullptr, m_width, m_height,
                              row_begins != nullptr ? row_begins[f] : row_begin, row_count,
                              d_ids != nullptr ? d_ids[f] : nullptr, row_interleave, id_planes, rgba_frame_rows};
    }
    const StageEvents ev = BindStageEvents(
        !same_begin || !CullFusedInfo(row_begins != nullptr ? row_begins[0] : row_begin, row_count, m_height, row_interleave),
        true);
    ParamTable* table = frames > static_cast<std::size_t>(kMaxBatch) ? &AcquireTable(frames, stream) : nullptr;
    const CullTable ct{table != nullptr ? table->device : nullptr, table != nullptr ? table->host : nullptr,
                       table != nullptr ? table->frames : 0, table != nullptr ? table->host_device : nullptr,
                       table != nullptr ? table->uploaded : nullptr};
    const hipError_t launched = LaunchCullFrames(cf.data(), frames, m_n, m_vertices, m_shade, m_frame, m_background,
                                                 m_rank, stream, m_timing ? &ev : nullptr,
                                                 table != nullptr ? &ct : nullptr);
    if (launched != hipSuccess) {
        DropPlans(frames);
    }
    HipCheck(launched, "batched trace launch");
    if (table != nullptr) {
        table->pending = true;  // (LaunchCullFrames recorded `uploaded` after the upload)
    }
    RecordOrder(stream);
}

void DeviceScene::Trace(const float* d_offsets, float* d_rgba, std::size_t row_begin, std::size_t row_count,
                        int variant, hipStream_t stream, int* d_ids, std::size_t row_interleave, int id_planes,
                        bool rgba_frame_rows) const {
    if (id_planes >= 0 && (d_ids == nullptr || id_planes != IdPlanes(m_n) || variant != kTraceCull)) {
        throw std::runtime_error("Trace: packed ids need an id output, the cull variant and " +
                                 std::to_string(IdPlanes(m_n)) + " bit planes for this scene");
    }
    if (m_width == 0) {
        throw std::runtime_error("Trace: Prepare() has not been called");
    }
    if (!BandFits(row_begin, row_count, row_interleave, m_height)) {
        throw std::runtime_error("Trace: row band outside the frame");
    }
    const bool binned = variant == kTraceCull && row_count != 0 && CullBinningEnabled() && CullBinnable(m_width, row_count);
    if (binned && OnSharedSetup(row_begin, row_count, row_interleave)) {
        float* const rgba1[1] = {d_rgba};
        int* const ids1[1] = {d_ids};
        TraceShared(&d_offsets, rgba1, d_ids != nullptr ? ids1 : nullptr, 1, stream, id_planes, rgba_frame_rows, 1);
        return;
    }
    OrderAfterPrevious(stream);
    BandArgs band{d_offsets, d_rgba, m_width, m_height, row_begin, row_count, d_ids, row_interleave, id_planes,
                  rgba_frame_rows};
    CullBins bins{};
    const CullBins* use_bins = nullptr;
    if (binned) {
        ++m_setup_stats.per_frame_frames;
        LogSetupStats();
        EnsureCullWork(1, row_count, stream);
        EnsureBlockExtents(stream);
        bins = CullSlot(0, row_count);
        bins.recompute = RecomputeRecords(1);
        use_bins = &bins;
    }
    if (variant == kTraceBvh && m_bvh == nullptr && row_count != 0) {
        m_bvh = DeviceAlloc<unsigned char>(BvhBytes(m_n), "hipMalloc(bvh)");
    }
    // The full record pass for every path but the binned cull one, which computes its records in
    // its bin kernel (its "prepare" stage is the tile-info kernel).
    const bool prepare = use_bins == nullptr && m_prepare_pending && row_count != 0;
    const bool fused_info = use_bins != nullptr && CullFusedInfo(row_begin, row_count, m_height, row_interleave);
    const StageEvents ev = BindStageEvents(prepare || (use_bins != nullptr && row_count != 0 && !fused_info),
                                           use_bins != nullptr || (variant == kTraceBvh && m_n != 0));
    const hipError_t launched = LaunchTrace(m_edges, m_n, m_vertices, m_shade, m_frame, m_background, band, variant,
                                            use_bins, stream, m_timing ? &ev : nullptr, prepare ? m_rank : nullptr,
                                            m_bvh);
    if (launched != hipSuccess && use_bins != nullptr) {
        DropPlans(1);
    }
    HipCheck(launched, "trace kernel launch");
    if (prepare) {
        m_prepare_pending = false;
    }
    RecordOrder(stream);
}

// With stage timing on: events for one traced call (a batch counts as one call).
StageEvents DeviceScene::BindStageEvents(bool prep, bool staged) const {
    StageEvents ev{};
    if (!m_timing) {
        return ev;
    }
    if (prep) {
        ev.prep_begin = TimingEvent(m_prep_events, 2 * m_prep_timed);
        ev.prep_end = TimingEvent(m_prep_events, 2 * m_prep_timed + 1);
        ++m_prep_timed;
    }
    const std::size_t k = 4 * m_timed;
    ev.bin_begin = staged ? TimingEvent(m_events, k) : nullptr;
    ev.bin_end = staged ? TimingEvent(m_events, k + 1) : nullptr;
    ev.begin = TimingEvent(m_events, k + 2);
    ev.end = TimingEvent(m_events, k + 3);
    if (m_binned.size() <= m_timed) {
        m_binned.resize(m_timed + 1);
    }
    m_binned[m_timed] = staged;
    ++m_timed;
    return ev;
}

hipEvent_t DeviceScene::TimingEvent(std::vector<hipEvent_t>& pool, std::size_t i) const {
    while (pool.size() <= i) {
        hipEvent_t e = nullptr;
        HipCheck(hipEventCreate(&e), "hipEventCreate(stage timing)");
        pool.push_back(e);
    }
    return pool[i];
}

void DeviceScene::SetTiming(bool on) {
    m_timing = on;
}

namespace {
// SRT_TRACE_RECORDS: stored | recompute | auto (render.h RecordMode); -1 when unset. Read per launch
// (like SRT_CULL_BIN), so a process can compare the modes.
int RecordModeFromEnv() {
    const char* e = std::getenv("SRT_TRACE_RECORDS");
    if (e == nullptr || *e == '\0') {
        return -1;
    }
    const std::string v(e);
    if (v == "auto") {
        return static_cast<int>(kRecordsAuto);
    }
    if (v == "stored") {
        return static_cast<int>(kRecordsStored);
    }
    if (v == "recompute") {
        return static_cast<int>(kRecordsRecompute);
    }
    throw std::runtime_error("SRT_TRACE_RECORDS must be stored, recompute or auto, got '" + v + "'");
}

// SRT_TRACE_STREAM = 1 (default) | 0, read per call (like SRT_SETUP): whether the shared setup builds
// its record stream and the traces read it; 0 keeps the indexed path (records through the lists).
bool TraceStreamFromEnv() {
    const char* e = std::getenv("SRT_TRACE_STREAM");
    const std::string v = e == nullptr || *e == '\0' ? "1" : e;
    if (v != "1" && v != "0") {
        throw std::runtime_error("SRT_TRACE_STREAM must be 1 or 0, got '" + v + "'");
    }
    return v == "1";
}

// SRT_EMPTY_SWEEP = 1 (default) | 0, read per call (like SRT_TRACE_STREAM) and part of the setup's
// key: whether the shared setup's plan lists its statically empty descriptors last and the traces
// sweep them in groups (render.h CullSetup::sweep); 0 keeps one trace block per descriptor.
bool EmptySweepFromEnv() {
    const char* e = std::getenv("SRT_EMPTY_SWEEP");
    const std::string v = e == nullptr || *e == '\0' ? "1" : e;
    if (v != "1" && v != "0") {
        throw std::runtime_error("SRT_EMPTY_SWEEP must be 1 or 0, got '" + v + "'");
    }
    return v == "1";
}

// SRT_EMPTY_GROUP (measurements and tests), read per call: empty descriptors per sweep block instead
// of kDefaultEmptyGroup. A launch parameter, not part of what is built.
unsigned EmptyGroupFromEnv() {
    const char* e = std::getenv("SRT_EMPTY_GROUP");
    if (e == nullptr || *e == '\0') {
        return kDefaultEmptyGroup;
    }
    char* end = nullptr;
    const unsigned long long v = std::strtoull(e, &end, 10);
    if (end == e || *end != '\0' || *e == '-' || v == 0 || v > kMaxEmptyGroup) {
        throw std::runtime_error("SRT_EMPTY_GROUP must be 1 to " + std::to_string(kMaxEmptyGroup) + ", got '" +
                                 std::string(e) + "'");
    }
    return static_cast<unsigned>(v);
}

// SRT_EMPTY_FILL = sweep (default) | facts, read per call: who stores the misses of the statically
// empty tiles whose offsets are valid in the frame -- the trace's sweep blocks, or the frame's
// tile-facts launch (render.h CullSetup::facts_fill; measured slower on the headline, kept for
// measurements: profiles/facts_fill/README.md). A launch parameter, not part of what is built;
// without the sweep (SRT_EMPTY_SWEEP=0) one block per empty descriptor fills, whatever this says.
bool EmptyFillFromEnv() {
    const char* e = std::getenv("SRT_EMPTY_FILL");
    const std::string v = e == nullptr || *e == '\0' ? "sweep" : e;
    if (v != "facts" && v != "sweep") {
        throw std::runtime_error("SRT_EMPTY_FILL must be facts or sweep, got '" + v + "'");
    }
    return v == "facts";
}

// SRT_FACTS_KERNEL = auto (default) | lean | block, read per call: the facts kernel of a shared-setup
// launch (render.h CullSetup::lean_facts). auto: lean when some frames of the launch share an offsets
// buffer -- a sample pattern reused across frames stays in cache, where the lean kernel beside the
// other queue's trace is the faster one --, block when every frame brings its own (a single frame,
// rotating inputs: read from memory once, where the block kernel is). -1: auto.
int FactsKernelFromEnv() {
    const char* e = std::getenv("SRT_FACTS_KERNEL");
    const std::string v = e == nullptr || *e == '\0' ? "auto" : e;
    if (v != "auto" && v != "lean" && v != "block") {
        throw std::runtime_error("SRT_FACTS_KERNEL must be auto, lean or block, got '" + v + "'");
    }
    return v == "auto" ? -1 : v == "lean" ? 1 : 0;
}

// SRT_FACTS_PINS = 1 (default) | 0, read per call: whether a whole-frame trace on the shared setup
// reads the stored facts of its pinned offsets buffers (DeviceScene::PinOffsets); 0: it computes
// every frame's facts as if nothing were pinned -- the same frames, the A/B leg of a measurement.
// SRT_TRACE_POS = auto (default) | table, read per call: whether a shared launch whose frames are
// all pinned with an all-regular summary may run the trace kernel without the position table
// (renderer.h PinOffsets). table: always the general kernel -- the same frames, the A/B leg.
bool TracePosAutoFromEnv() {
    const char* e = std::getenv("SRT_TRACE_POS");
    const std::string v = e == nullptr || *e == '\0' ? "auto" : e;
    if (v != "auto" && v != "table") {
        throw std::runtime_error("SRT_TRACE_POS must be auto or table, got '" + v + "'");
    }
    return v == "auto";
}

bool FactsPinsFromEnv() {
    const char* e = std::getenv("SRT_FACTS_PINS");
    const std::string v = e == nullptr || *e == '\0' ? "1" : e;
    if (v != "1" && v != "0") {
        throw std::runtime_error("SRT_FACTS_PINS must be 1 or 0, got '" + v + "'");
    }
    return v == "1";
}

// SRT_TRACE_STREAM_CAP (tests only): the longest record stream, in records, instead of
// kStreamCapRecords -- forces the indexed fallback at small sizes, as SRT_CULL_BIN_CAP forces list overflow.
std::size_t StreamCapFromEnv() {
    const char* e = std::getenv("SRT_TRACE_STREAM_CAP");
    if (e == nullptr || *e == '\0') {
        return kStreamCapRecords;
    }
    char* end = nullptr;
    const unsigned long long v = std::strtoull(e, &end, 10);
    if (end == e || *end != '\0' || *e == '-' || v > kStreamCapRecords) {
        throw std::runtime_error("SRT_TRACE_STREAM_CAP must be a record count up to " +
                                 std::to_string(kStreamCapRecords) + ", got '" + std::string(e) + "'");
    }
    return static_cast<std::size_t>(v);
}
}  // namespace

void DeviceScene::SetRecordMode(int mode) {
    if (mode != kRecordsAuto && mode != kRecordsStored && mode != kRecordsRecompute) {
        throw std::runtime_error("SetRecordMode: unknown record mode " + std::to_string(mode));
    }
    m_records = mode;
}

// Whether a binned launch of `frames` frames has its trace recompute the records: the bin launch
// then writes 16 B per record instead of 64, which shortens it by a fifth, and the trace rebuilds each
// candidate's record (~5 % longer). It pays where the bin launch is on the critical path: a launch of one
// frame, or an engine with one frame queue (nothing overlaps its bin launches).
bool DeviceScene::RecomputeRecords(std::size_t frames) const {
    const int env = RecordModeFromEnv();
    const int mode = env >= 0 ? env : m_records;
    return mode == kRecordsRecompute || (mode == kRecordsAuto && frames == 1);
}

// SRT_SETUP = prepare (default) | frame, read per call (like SRT_TRACE_RECORDS): `prepare` runs the
// whole-frame binned traces on the shared setup; `frame` keeps the per-frame setup for every band.
// The shared setup serves the bands whose bin launch ignores the offsets already: whole frames with
// the tile info fused into it (CullFusedInfo).
bool DeviceScene::OnSharedSetup(std::size_t row_begin, std::size_t row_count, std::size_t row_interleave) const {
    const char* e = std::getenv("SRT_SETUP");
    const std::string v = e == nullptr || *e == '\0' ? "prepare" : e;
    if (v != "prepare" && v != "frame") {
        throw std::runtime_error("SRT_SETUP must be prepare or frame, got '" + v + "'");
    }
    return v == "prepare" && row_begin == 0 && row_count == m_height && row_interleave == 1 &&
           CullFusedInfo(row_begin, row_count, m_height, row_interleave);
}

// Env SRT_SETUP_LOG (read per call; unset, empty or "0": off): after every binned cull, query,
// G-buffer and resolve call one line on stderr with the scene's counters so far -- what tells a run on the shared setup from a silent
// per-frame one (tests/test_gpu_shared_setup.py; the C ABI has no entry for them).
void DeviceScene::LogSetupStats() const {
    const char* e = std::getenv("SRT_SETUP_LOG");
    if (e == nullptr || *e == '\0' || std::strcmp(e, "0") == 0) {
        return;
    }
    std::fprintf(stderr,
                 "srt setup: scene %p builds %llu shared_frames %llu per_frame_frames %llu stream_frames %llu "
                 "stream_records %llu empty_descs %llu sweep_blocks %llu facts_fill_frames %llu "
                 "lean_facts_frames %llu pinned_frames %llu facts_launches %llu regular_launches %llu\n",
                 static_cast<const void*>(this), m_setup_stats.builds, m_setup_stats.shared_frames,
                 m_setup_stats.per_frame_frames, m_setup_stats.stream_frames, m_setup_stats.stream_records,
                 m_setup_stats.empty_descs, m_setup_stats.sweep_blocks, m_setup_stats.facts_fill_frames,
                 m_setup_stats.lean_facts_frames, m_setup_stats.pinned_frames, m_setup_stats.facts_launches,
                 m_setup_stats.regular_launches);
    std::fflush(stderr);
}

void DeviceScene::TraceShared(const float* const* d_offsets, float* const* d_rgba, int* const* d_ids,
                              std::size_t frames, hipStream_t stream, int id_planes, bool rgba_frame_rows,
                              std::size_t plan_frames) const {
    // An explicit SRT_FACTS_KERNEL=lean|block asks for that facts kernel in the launch (the switch of
    // the facts kernels' own measurements and tests), so such a call computes its facts too.
    const int want = FactsKernelFromEnv();
    const bool use_pins = FactsPinsFromEnv() && want < 0 && !m_pins.empty();  // (junk is an error, pins or none)
    const bool pos_auto = TracePosAutoFromEnv();
    OrderAfterPrevious(stream);
    // The frame slots' own state (tile facts, split key slices, arrival counters) lives in the cull
    // work of the whole-frame shape; no edge slots: the records are the setup's.
    EnsureCullWork(frames, m_height, stream);
    const CullArena& a = m_arenas.at(m_arena);
    const std::size_t tiles = CullTiles(m_width, m_height);
    const unsigned descs = std::min(CullBinLayout(a.work, m_n, m_width, m_height).descs, CullDescriptors(tiles, plan_frames));
    CullSetup setup = EnsureSetup(descs, stream);
    // The launch's order: the frames that need their facts computed first, those whose offsets are
    // pinned after them, so the facts launch is the first `unpinned` frames of the grid (render.h
    // LaunchSharedCullFrames). A frame's parameters are self-contained: its place in the launch is
    // not part of its result. SRT_EMPTY_FILL=facts on the sweep: that facts launch stores pixels,
    // so it runs for every frame and no pin is used.
    std::vector<const void*> facts(frames, nullptr);
    std::vector<std::size_t> at(frames);  // launch position -> the caller's frame
    std::size_t unpinned = 0;
    if (use_pins && !(setup.sweep && setup.facts_fill)) {
        for (std::size_t f = 0; f < frames; ++f) {
            facts[f] = m_pins.Find(d_offsets[f]);
        }
    }
    for (std::size_t f = 0; f < frames; ++f) {
        if (facts[f] == nullptr) {
            at[unpinned++] = f;
        }
    }
    for (std::size_t f = 0, k = unpinned; f < frames; ++f) {
        if (facts[f] != nullptr) {
            at[k++] = f;
        }
    }
    std::vector<CullBins> bins(frames);
    std::vector<CullFrame> cf(frames);
    for (std::size_t k = 0; k < frames; ++k) {
        const std::size_t f = at[k];
        // (not CullSlot: the slot's count parity and its per-frame plan stay as the per-frame path left them)
        bins[k] = CullBinLayout(a.work + k * a.layout, m_n, m_width, m_height);
        bins[k].descs = descs;
        bins[k].order = m_order;
        bins[k].svertices = m_svertices;
        cf[k].edges = nullptr;
        cf[k].bins = &bins[k];
        cf[k].band = BandArgs{d_offsets[f], d_rgba != nullptr ? d_rgba[f] : nullptr, m_width, m_height, 0, m_height,
                              d_ids != nullptr ? d_ids[f] : nullptr, 1, id_planes, rgba_frame_rows};
        cf[k].facts = facts[f];
    }
    {
        bool reused = false;  // some frames of the facts launch read the same offsets buffer
        for (std::size_t k = 1; k < unpinned && !reused; ++k) {
            for (std::size_t g = 0; g < k && !reused; ++g) {
                reused = cf[k].band.offsets == cf[g].band.offsets;
            }
        }
        setup.lean_facts = want < 0 ? reused : want == 1;
    }
    // A regular launch: RGBA frames that all bring the stored facts of a pin whose summary is known
    // to be all regular and valid (a summary still unknown is not waited for: the general kernel
    // gives the same bits), on a plan none of whose sweep blocks can have a descriptor to trace.
    bool regular = pos_auto && unpinned == 0 && d_ids == nullptr && d_rgba != nullptr && setup.full_empty_descs == 0;
    for (std::size_t f = 0; f < frames && regular; ++f) {
        regular = PinSummary(d_offsets[f], false) == PinTable::kRegular;
    }
    setup.regular_trace = regular;
    // (the last trace's grid: sweep blocks per frame, 0 with the sweep off)
    m_setup_stats.sweep_blocks =
        setup.sweep ? SharedTraceBlocks(setup.descs, setup.list_descs, setup.empty_descs, setup.empty_group) - setup.list_descs
                    : 0;
    // (no facts launch: no bin events, and TakeTimes reports a bin stage of 0 for the call)
    const StageEvents ev = BindStageEvents(false, unpinned != 0);
    ParamTable* table = frames > static_cast<std::size_t>(kMaxBatch) ? &AcquireTable(frames, stream) : nullptr;
    const CullTable ct{table != nullptr ? table->device : nullptr, table != nullptr ? table->host : nullptr,
                       table != nullptr ? table->frames : 0, table != nullptr ? table->host_device : nullptr,
                       table != nullptr ? table->uploaded : nullptr};
    HipCheck(LaunchSharedCullFrames(cf.data(), frames, setup, m_n, m_vertices, m_shade, m_frame, m_background, stream,
                                    m_timing ? &ev : nullptr, table != nullptr ? &ct : nullptr),
             "shared-setup trace launch");
    if (table != nullptr) {
        table->pending = true;  // (LaunchSharedCullFrames recorded `uploaded` after the upload)
    }
    m_setup_stats.shared_frames += frames;
    m_setup_stats.stream_frames += setup.stream != nullptr ? frames : 0;
    m_setup_stats.facts_fill_frames += setup.sweep && setup.facts_fill ? frames : 0;
    m_setup_stats.lean_facts_frames += setup.lean_facts || (setup.sweep && setup.facts_fill) ? unpinned : 0;
    m_setup_stats.pinned_frames += frames - unpinned;
    m_setup_stats.facts_launches += unpinned != 0 ? 1 : 0;
    m_setup_stats.regular_launches += regular ? 1 : 0;
    LogSetupStats();
    RecordOrder(stream);
}

// Pinned offsets (renderer.h): the facts kernel once, for one frame, into the pin's own buffer.
void DeviceScene::PinOffsets(const float* d_offsets, hipStream_t stream) {
    if (d_offsets == nullptr) {
        throw std::runtime_error("PinOffsets: null offsets pointer");
    }
    if (m_width == 0) {
        throw std::runtime_error("PinOffsets: Prepare() has not been called");
    }
    if (!CullBinnable(m_width, m_height)) {
        throw std::runtime_error("PinOffsets: no tile facts for a frame of this size (its traces are not binned)");
    }
    // A launch of one frame brings its own buffer: the block kernel, unless the env names one.
    const int want = FactsKernelFromEnv();
    PinTable::Buffers buf = m_pins.FindBuffers(d_offsets);
    const bool fresh = buf.facts == nullptr;
    const std::size_t tiles = CullTiles(m_width, m_height);
    if (fresh) {
        if (m_pins.full()) {
            throw std::runtime_error("PinOffsets: at most " + std::to_string(PinTable::kMaxPins) +
                                     " pinned buffers per scene (unpin one first)");
        }
        buf = NewPinBuffers(tiles);
    } else {
        // A pin again rewrites the facts: their summary is unknown from here on, before the launch
        // is queued, and is read again only after the event recorded below -- a later record of the
        // same event, so that hipEventQuery speaks of the new facts alone.
        m_pins.MarkPending(d_offsets);
    }
    OrderAfterPrevious(stream);  // (a pin again: earlier traces read the buffer this launch rewrites)
    const BandArgs band{d_offsets, nullptr, m_width, m_height, 0, m_height};
    hipError_t launched = LaunchTileFacts(band, buf.facts, want == 1, stream);
    if (launched == hipSuccess) {
        void* d_word = nullptr;
        launched = hipHostGetDevicePointer(&d_word, buf.word, 0);
        if (launched == hipSuccess) {
            launched = LaunchFactsSummary(buf.facts, tiles, static_cast<unsigned*>(d_word), stream);
        }
        if (launched == hipSuccess) {
            launched = hipEventRecord(static_cast<hipEvent_t>(buf.event), stream);
        }
    }
    RecordOrder(stream);
    if (launched != hipSuccess) {
        // Facts that were not computed must not be read, nor a summary whose event was not recorded
        // (the event's earlier record would answer for it): the pin is gone (a fresh buffer was never
        // visible to any launch; a standing one may be read by queued traces: retired, released later).
        if (fresh) {
            (void)hipStreamSynchronize(stream);  // (what was queued may write the buffers)
            ReleasePinBuffers(buf);
        } else {
            m_pins.Remove(d_offsets);
        }
    } else if (fresh) {
        m_pins.Insert(d_offsets, buf);
    }
    HipCheck(launched, "pinned facts launch");
    ++m_setup_stats.facts_launches;
    LogSetupStats();
}

void DeviceScene::UnpinOffsets(const float* d_offsets) {
    m_pins.Remove(d_offsets);
    ReleaseRetiredPins();
}

std::size_t DeviceScene::pinned() const { return m_pins.size(); }

PinTable::Summary DeviceScene::PinSummary(const void* key, bool wait) const {
    const PinTable::Summary known = m_pins.summary(key);
    const PinTable::Buffers buf = m_pins.FindBuffers(key);
    if (known != PinTable::kUnknown || buf.event == nullptr || buf.word == nullptr) {
        return known;
    }
    // The event's newest record stands behind the summary launch of the facts now in the buffer
    // (PinOffsets): completed means the word is theirs.
    const hipEvent_t event = static_cast<hipEvent_t>(buf.event);
    if (wait) {
        HipCheck(hipEventSynchronize(event), "hipEventSynchronize(pin summary)");
    } else {
        const hipError_t q = hipEventQuery(event);
        if (q == hipErrorNotReady) {
            (void)hipGetLastError();  // (not an error: nothing of it is left for the next launch's check)
            return PinTable::kUnknown;
        }
        HipCheck(q, "hipEventQuery(pin summary)");
    }
    const unsigned word = *static_cast<const volatile unsigned*>(buf.word);
    const bool regular = (word & kFactsSummaryDone) != 0u && (word & kFactsSummaryRegular) != 0u;
    const PinTable::Summary s = regular ? PinTable::kRegular : PinTable::kOther;
    m_pins.SetSummary(key, m_pins.generation(key), s);
    return s;
}

void DeviceScene::ResolvePinSummaries() {
    for (const void* key : m_pins.Pending()) {
        PinSummary(key, true);
    }
}

// Calls on one scene form one chain (OrderAfterPrevious), so the newest order event stands for all
// of the scene's work so far.
void DeviceScene::WaitForPrevious() const {
    if (!m_used) {
        return;
    }
#if SRT_ORDER_EVENTS == 0
    HipCheck(hipEventRecord(m_order_events[0], m_last_stream), "hipEventRecord(scene order)");
    HipCheck(hipEventSynchronize(m_order_events[0]), "hipEventSynchronize(scene order)");
#else
    HipCheck(hipEventSynchronize(m_order_events[m_order_next]), "hipEventSynchronize(scene order)");
#endif
}

void DeviceScene::ReleaseRetiredPins() {
    if (m_pins.retired() == 0) {
        return;
    }
    WaitForPrevious();  // (throws: the buffers stay retired, and are freed with the scene at the latest)
    for (const PinTable::Buffers& b : m_pins.TakeRetired()) {
        ReleasePinBuffers(b);
    }
}

// A pin's buffers (pin_table.h Buffers): the facts, and a summary word and an event from the scene's
// free lists (renderer.h). The word is zero: nothing says "done" before the pin's own summary launch.
PinTable::Buffers DeviceScene::NewPinBuffers(std::size_t tiles) {
    if (m_free_pin_words.empty()) {
        // Page-locked and mapped: the summary kernel stores the word over the bus, the host reads it
        // once the pin's event has completed.
        void* chunk = nullptr;
        HipCheck(hipHostMalloc(&chunk, PinTable::kMaxPins * sizeof(unsigned), hipHostMallocMapped),
                 "hipHostMalloc(pin summary words)");
        m_pin_word_chunks.push_back(chunk);
        for (std::size_t i = 0; i < PinTable::kMaxPins; ++i) {
            m_free_pin_words.push_back(static_cast<unsigned*>(chunk) + i);
        }
    }
    if (m_free_pin_events.empty()) {
        hipEvent_t event = nullptr;
        HipCheck(hipEventCreateWithFlags(&event, hipEventDisableTiming), "hipEventCreate(pin summary)");
        m_free_pin_events.push_back(event);
    }
    PinTable::Buffers b;
    b.facts = DeviceAlloc<unsigned char>(tiles * 16, "hipMalloc(pinned facts)");  // (throws: the lists keep theirs)
    b.word = m_free_pin_words.back();
    m_free_pin_words.pop_back();
    b.event = m_free_pin_events.back();
    m_free_pin_events.pop_back();
    *static_cast<unsigned*>(b.word) = 0u;
    return b;
}

void DeviceScene::ReleasePinBuffers(const PinTable::Buffers& b) {
    (void)hipFree(b.facts);
    if (b.word != nullptr) {
        m_free_pin_words.push_back(b.word);
    }
    if (b.event != nullptr) {
        m_free_pin_events.push_back(b.event);
    }
}

// The shared setup of the prepared frame for a trace grid of `descs` descriptors: (re)allocated,
// keyed and (re)built on `stream` if need be (after OrderAfterPrevious(stream)), counted in
// SetupStats::builds. What TraceShared and Query have in common.
CullSetup DeviceScene::EnsureSetup(unsigned descs, hipStream_t stream) const {
    // Stored records unless the env asks for recomputed ones: the engine's one-queue hint
    // (SetRecordMode) shortened a bin launch that this path does not run.
    const bool recompute = RecordModeFromEnv() == static_cast<int>(kRecordsRecompute);
    const std::size_t bytes = CullSetupBytes(m_n, m_width, m_height, descs);
    if (bytes > m_setup_bytes) {
        // (earlier readers of the old copy ran before this stream's end: OrderAfterPrevious)
        HipCheck(hipStreamSynchronize(stream), "hipStreamSynchronize(cull setup)");
        (void)hipFree(m_setup);
        m_setup = nullptr;
        m_setup_bytes = 0;
        m_setup = DeviceAlloc<unsigned char>(bytes, "hipMalloc(cull setup)");
        m_setup_bytes = bytes;
        m_setup_pending = true;
    }
    CullSetup setup = CullSetupLayout(m_setup, m_n, m_width, m_height, descs, recompute);
    // The record stream is for stored records; its cap is part of the key (a test lowers it).
    const bool want_stream = TraceStreamFromEnv() && !recompute;
    setup.sweep = EmptySweepFromEnv();
    setup.empty_group = EmptyGroupFromEnv();
    setup.facts_fill = EmptyFillFromEnv();
    const SetupKey key{m_width,         m_height,    setup.capacity, setup.descs,
                       setup.min_chunk, setup.recompute, want_stream,    want_stream ? StreamCapFromEnv() : 0,
                       setup.sweep};
    const SetupKey& k = m_setup_key;
    if (m_setup_pending || key.width != k.width || key.height != k.height || key.capacity != k.capacity ||
        key.descs != k.descs || key.min_chunk != k.min_chunk || key.recompute != k.recompute ||
        key.stream != k.stream || key.stream_cap != k.stream_cap || key.sweep != k.sweep) {
        m_setup_pending = true;  // (a failed build leaves none)
        m_stream_on = false;
        m_stream_records = 0;
        HipCheck(LaunchCullSetup(setup, m_n, m_frame, m_width, m_height, m_order, m_svertices, stream),
                 "cull setup launch");
        // The stream's length and the plan's list and empty descriptor counts are known only from
        // the built plan: one host read per build (never per frame), with a stream or without.
        unsigned long long plan[3] = {0, 0, 0};
        HipCheck(LaunchStreamPlan(setup, stream), "record stream plan launch");
        HipCheck(hipMemcpyAsync(plan, setup.stream_count, sizeof(plan), hipMemcpyDeviceToHost, stream),
                 "hipMemcpyAsync(plan counts)");
        HipCheck(hipStreamSynchronize(stream), "hipStreamSynchronize(plan counts)");
        m_list_descs = static_cast<unsigned>(plan[1]);
        m_empty_descs = static_cast<unsigned>(plan[1] >> 32);
        m_full_empty_descs = static_cast<unsigned>(plan[2]);
        if (want_stream) {
            // Over the cap, this setup's frames keep the indexed path.
            const unsigned long long records = plan[0];
            if (records <= key.stream_cap) {
                const std::size_t need = std::max<std::size_t>(static_cast<std::size_t>(records), 2);
                if (need > m_stream_capacity) {
                    // (earlier readers of the old stream ran before this stream's end, as for m_setup)
                    (void)hipFree(m_stream);
                    m_stream = nullptr;
                    m_stream_capacity = 0;
                    m_stream = DeviceAlloc<unsigned char>(need * kCullRecordBytes, "hipMalloc(record stream)");
                    m_stream_capacity = need;
                }
                HipCheck(LaunchStreamPack(setup, m_stream, stream), "record stream pack launch");
                m_stream_on = true;
                m_stream_records = static_cast<std::size_t>(records);
            }
        }
        m_setup_key = key;
        m_setup_pending = false;
        ++m_setup_stats.builds;
        m_setup_stats.stream_records = m_stream_records;
        m_setup_stats.empty_descs = m_empty_descs;
    }
    setup.stream = m_stream_on ? m_stream : nullptr;
    setup.list_descs = m_list_descs;
    setup.empty_descs = m_empty_descs;
    setup.full_empty_descs = m_full_empty_descs;
    return setup;
}

// Point queries on the prepared frame (render.h LaunchQuery). The setup is built for the one-frame
// trace grid, so a one-frame whole-frame trace before or after shares the build. No usable setup
// (SRT_SETUP=frame, SRT_CULL_BIN=0, a shape that cannot be binned): every query streams.
void DeviceScene::Query(const float* d_positions, std::size_t count, int* d_ids, float* d_t, unsigned char* d_how,
                        hipStream_t stream) const {
    if (m_width == 0) {
        throw std::runtime_error("Query: Prepare() has not been called");
    }
    if (count == 0) {
        return;
    }
    OrderAfterPrevious(stream);
    CullSetup setup{};
    const bool shared = QuerySetup(setup, stream);
    const QueryArgs args{d_positions, count, d_ids, d_t, d_how};
    HipCheck(LaunchQuery(shared ? &setup : nullptr, m_n, m_frame, m_width, m_height, m_svertices, m_edges, args, stream),
             "query launch");
    RecordOrder(stream);
}

// Depth layers on the prepared frame (render.h LaunchLayers): Query keeping K hits. The setup is
// Query's, shared with it, Shadow and a one-frame whole-frame trace.
void DeviceScene::Layers(bool points, const float* d_where, std::size_t row_begin, std::size_t count,
                         std::size_t layers, int* d_ids, float* d_t, unsigned char* d_how, hipStream_t stream) const {
    if (m_width == 0) {
        throw std::runtime_error("Layers: Prepare() has not been called");
    }
    if (layers == 0 || layers > static_cast<std::size_t>(kMaxLayers)) {
        throw std::runtime_error("Layers: layers must be 1 to " + std::to_string(kMaxLayers) + ", got " +
                                 std::to_string(layers));
    }
    if (!points && (row_begin > m_height || count > m_height - row_begin)) {
        throw std::runtime_error("Layers: row band outside the frame");
    }
    if (count == 0) {
        return;
    }
    OrderAfterPrevious(stream);
    CullSetup setup{};
    const bool shared = QuerySetup(setup, stream);
    const LayersArgs args{points, d_where, points ? count : 0, points ? 0 : row_begin, points ? 0 : count, layers,
                          d_ids,  d_t,     d_how};
    HipCheck(LaunchLayers(shared ? &setup : nullptr, m_n, m_frame, m_width, m_height, m_svertices, m_edges, args, stream),
             "layers launch");
    RecordOrder(stream);
}

void DeviceScene::Composite(const float* d_offsets, const int* d_ids, std::size_t layers, const float* d_opacity,
                            std::size_t row_begin, std::size_t row_count, float* d_rgba, hipStream_t stream) const {
    if (m_width == 0) {
        throw std::runtime_error("Composite: Prepare() has not been called");
    }
    if (layers == 0 || layers > static_cast<std::size_t>(kMaxLayers)) {
        throw std::runtime_error("Composite: layers must be 1 to " + std::to_string(kMaxLayers) + ", got " +
                                 std::to_string(layers));
    }
    if (row_begin > m_height || row_count > m_height - row_begin) {
        throw std::runtime_error("Composite: row band outside the frame");
    }
    if (row_count == 0) {
        return;
    }
    OrderAfterPrevious(stream);
    const CompositeArgs args{d_offsets, d_ids, layers, d_opacity, m_width, m_height, row_begin, row_count, d_rgba};
    HipCheck(LaunchComposite(m_shade, m_n, m_frame, m_background, args, stream), "composite launch");
    LogSetupStats();  // (the counters as they stand: this call builds nothing)
    RecordOrder(stream);
}

bool DeviceScene::QuerySetup(CullSetup& setup, hipStream_t stream) const {
    const bool shared = QuerySetupUsable();
    if (shared) {
        // (a query reads no plan: a setup standing for another grid, a batch's, serves as it is)
        const bool standing = !m_setup_pending && m_setup_key.width == m_width && m_setup_key.height == m_height;
        setup = EnsureSetup(standing ? m_setup_key.descs : CullDescriptors(CullTiles(m_width, m_height), 1), stream);
        LogSetupStats();
    }
    return shared;
}

void DeviceScene::CheckLightScene(const DeviceScene& f, const DeviceScene& first, const LightWords& w) const {
    const auto who = [&w] { return std::string(w.who); };  // (built only to be thrown)
    if (f.m_width == 0) {
        throw std::runtime_error(who() + w.unprepared);
    }
    if (f.m_width != first.m_width || f.m_height != first.m_height) {
        throw std::runtime_error(who() + ": " + w.faces + " are prepared at different sizes");
    }
    if (f.m_device != m_device) {
        throw std::runtime_error(who() + ": the view scene lives on device " + std::to_string(m_device) + ", " + w.light +
                                 " on device " + std::to_string(f.m_device));
    }
    if (f.m_n != m_n) {
        throw std::runtime_error(who() + ": the view scene has " + std::to_string(m_n) + " triangles, " + w.its_scene + " " +
                                 std::to_string(f.m_n));
    }
}

ShadowLight DeviceScene::AsLightFrame(const DeviceScene& view, CullSetup& setup, hipStream_t stream) const {
    if (this != &view) {  // (the view scene orders itself)
        OrderAfterPrevious(stream);
    }
    const bool shared = QuerySetup(setup, stream);
    return ShadowLight{shared ? &setup : nullptr, m_frame, m_width, m_height, m_svertices, m_edges, m_rank};
}

// The shadow mask of a band of this scene's prepared frame under `light`'s prepared frame (render.h
// LaunchShadow). The launch reads both scenes' buffers, so it is ordered after the previous call
// of either and both record it. The light's vertices are a second copy of this scene's (the scenes
// are loaded separately).
void DeviceScene::Shadow(const DeviceScene& light, const float* d_offsets, const int* d_ids, std::size_t row_begin,
                         std::size_t row_count, float bias, unsigned char* d_mask, float* d_rgba, float dim,
                         hipStream_t stream) const {
    if (m_width == 0) {
        throw std::runtime_error("Shadow: Prepare() has not been called on the view scene");
    }
    CheckLightScene(light, light,
                    {"Shadow", ": Prepare() has not been called on the light scene", "", "the light scene", "the light scene"});
    if (!(bias >= 0.f) || !std::isfinite(bias)) {
        throw std::runtime_error("Shadow: bias must be finite and >= 0");
    }
    if (!std::isfinite(dim)) {
        throw std::runtime_error("Shadow: dim must be finite");
    }
    if (row_begin > m_height || row_count > m_height - row_begin) {
        throw std::runtime_error("Shadow: row band outside the frame");
    }
    if (row_count == 0) {
        return;
    }
    OrderAfterPrevious(stream);
    CullSetup setup{};
    const ShadowLight sl = light.AsLightFrame(*this, setup, stream);
    const ShadowArgs args{d_offsets, d_ids, m_width, m_height, row_begin, row_count, bias, d_mask, d_rgba, dim};
    HipCheck(LaunchShadow(m_vertices, m_shade, m_n, m_frame, m_background, sl, args, stream), "shadow launch");
    RecordOrder(stream);
    if (&light != this) {
        light.RecordOrder(stream);
    }
}

// Shadow under a point light's six face scenes (render.h LaunchOmniShadow): the launch reads this
// scene's buffers and all six faces', so it is ordered after the previous call of each and every
// one records it.
void DeviceScene::OmniShadow(const DeviceScene* const faces[6], const float* d_offsets, const int* d_ids,
                             std::size_t row_begin, std::size_t row_count, float bias, unsigned char* d_mask,
                             unsigned char* d_face, float* d_rgba, float dim, hipStream_t stream) const {
    if (m_width == 0) {
        throw std::runtime_error("Omni shadow: Prepare() has not been called on the view scene");
    }
    for (int k = 0; k < 6; ++k) {
        CheckLightScene(*faces[k], *faces[0],
                        {"Omni shadow", ": the light has not been prepared", "the light's faces", "the light", "the light's scene"});
    }
    if (!(bias >= 0.f) || !std::isfinite(bias)) {
        throw std::runtime_error("Omni shadow: bias must be finite and >= 0");
    }
    if (!std::isfinite(dim)) {
        throw std::runtime_error("Omni shadow: dim must be finite");
    }
    if (row_begin > m_height || row_count > m_height - row_begin) {
        throw std::runtime_error("Omni shadow: row band outside the frame");
    }
    if (row_count == 0) {
        return;
    }
    OrderAfterPrevious(stream);
    CullSetup setups[6] = {};
    ShadowLight lights[6];
    for (int k = 0; k < 6; ++k) {
        lights[k] = faces[k]->AsLightFrame(*this, setups[k], stream);
    }
    const ShadowArgs args{d_offsets, d_ids, m_width, m_height, row_begin, row_count, bias, d_mask, d_rgba, dim};
    HipCheck(LaunchOmniShadow(m_vertices, m_shade, m_n, m_frame, m_background, lights, args, d_face, stream),
             "omni shadow launch");
    RecordOrder(stream);
    for (int k = 0; k < 6; ++k) {
        faces[k]->RecordOrder(stream);
    }
}

bool DeviceScene::QuerySetupUsable() const {
    return OnSharedSetup(0, m_height, 1) && CullBinningEnabled() && CullBinnable(m_width, m_height);
}

// (no setup: the records are recomputed from the scene's vertices -- render.hip QueryRecords; EnsureSetup's rule else)
bool DeviceScene::QueryRecomputes() const {
    return !QuerySetupUsable() || RecordModeFromEnv() == static_cast<int>(kRecordsRecompute);
}

void DeviceScene::CheckLightCount(std::size_t count) {
    if (count > static_cast<std::size_t>(kLightingMaxLights)) {
        throw std::runtime_error("Lighting: at most " + std::to_string(kLightingMaxLights) + " lights per call, got " +
                                 std::to_string(count));
    }
}

void DeviceScene::CheckLights(const LightTerms* lights, std::size_t count, const float ambient[3]) {
    CheckLightCount(count);
    for (int k = 0; k < 3; ++k) {
        if (!std::isfinite(ambient[k])) {
            throw std::runtime_error("Lighting: ambient value " + std::to_string(k) + " is not finite");
        }
    }
    std::size_t frames = 0;
    for (std::size_t l = 0; l < count; ++l) {
        const LightTerms& in = lights[l];
        const std::string who = "Lighting: light " + std::to_string(l);
        frames += in.point ? 6 : 1;
        if (frames > static_cast<std::size_t>(kLightingMaxFrames)) {
            throw std::runtime_error(who + " brings the call to " + std::to_string(frames) + " light frames, at most " +
                                     std::to_string(kLightingMaxFrames) + " (1 per spot, 6 per point light)");
        }
        for (int k = 0; k < 3; ++k) {
            if (!std::isfinite(in.color[k])) {
                throw std::runtime_error(who + ": color value " + std::to_string(k) + " is not finite");
            }
        }
        if (!(in.falloff >= 0.f) || !std::isfinite(in.falloff)) {
            throw std::runtime_error(who + ": falloff must be finite and >= 0");
        }
        if (!(in.bias >= 0.f) || !std::isfinite(in.bias)) {
            throw std::runtime_error(who + ": bias must be finite and >= 0");
        }
    }
}

// Direct lighting (render.h LaunchLighting): the launch reads this scene's buffers and every light
// frame's, so it is ordered after the previous call of each and every one records it (a scene that
// appears twice is ordered and recorded twice: harmless). Every refusal comes before the first
// side effect: a refused call orders nothing, builds no setup and leaves every scene as it was.
void DeviceScene::Lighting(const Light* lights, std::size_t count, const float ambient[3], const float* d_offsets,
                           const int* d_ids, std::size_t row_begin, std::size_t row_count, float* d_rgba,
                           unsigned char* d_classes, hipStream_t stream) const {
    LightingWith(nullptr, lights, count, ambient, d_offsets, d_ids, row_begin, row_count, d_rgba, d_classes, stream);
}

void DeviceScene::LitSurface(const Light* lights, std::size_t count, const float ambient[3], const srt::LitSurface& surface,
                             const float* d_offsets, const int* d_ids, std::size_t row_begin, std::size_t row_count,
                             float* d_rgba, unsigned char* d_classes, hipStream_t stream) const {
    LightingWith(&surface, lights, count, ambient, d_offsets, d_ids, row_begin, row_count, d_rgba, d_classes, stream);
}

// What Lighting, LitSurface and LightHits check of their lights before anything is enqueued or built:
// CheckLights' rules, then every light frame against this scene and the one record source.
void DeviceScene::CheckLightFrames(const Light* lights, std::size_t count, const float ambient[3]) const {
    CheckLightCount(count);
    LightTerms terms[kLightingMaxLights];
    for (std::size_t l = 0; l < count; ++l) {
        terms[l] = LightTerms{lights[l].point, lights[l].color, lights[l].falloff, lights[l].bias};
    }
    CheckLights(terms, count, ambient);
    bool recompute = false;
    for (std::size_t l = 0; l < count; ++l) {
        const Light& in = lights[l];
        const std::string who = "Lighting: light " + std::to_string(l);
        for (std::size_t k = 0; k < (in.point ? 6u : 1u); ++k) {
            const DeviceScene& f = *in.scenes[k];
            CheckLightScene(f, *in.scenes[0],
                            {who.c_str(), " has not been prepared", "the faces", "the light", "the light's scene"});
            // One record source per launch (the kernel's template argument; LaunchOmniShadow's rule
            // for its six faces). A frame that cannot be binned has no shared cull setup and
            // recomputes its records; a frame with one reads stored records unless the env says otherwise.
            const bool rc = f.QueryRecomputes();
            if ((l != 0 || k != 0) && rc != recompute) {
                throw std::runtime_error(
                    who + ": its " + std::to_string(f.m_width) + " x " + std::to_string(f.m_height) + " frame reads " +
                    (rc ? "recomputed" : "stored") + " records, the light frames before it " +
                    (rc ? "stored" : "recomputed") +
                    " ones: a light frame too large for a shared cull setup (more than " + std::to_string(kMaxBinTiles) +
                    " tiles of 64 x 16 pixels, or more than " + std::to_string(kMaxBoundTiles) +
                    " tile columns plus tile rows) cannot share a call with a smaller one");
            }
            recompute = rc;
        }
    }
}

// The checked lights as a launch takes them: this scene and every light frame ordered after their
// previous calls on `stream`, every light frame's setup (re)built if it has one, launch(ll), and the
// call recorded on each.
template <class Launch>
void DeviceScene::WithLightFrames(const Light* lights, std::size_t count, hipStream_t stream, Launch&& launch) const {
    OrderAfterPrevious(stream);
    CullSetup setups[kLightingMaxFrames] = {};
    ShadowLight sl[kLightingMaxFrames];
    LightingLight ll[kLightingMaxLights];
    std::size_t frames = 0;
    for (std::size_t l = 0; l < count; ++l) {
        const Light& in = lights[l];
        ll[l] = LightingLight{sl + frames, in.point, {in.color[0], in.color[1], in.color[2]}, in.falloff, in.bias};
        for (std::size_t k = 0; k < (in.point ? 6u : 1u); ++k, ++frames) {
            sl[frames] = in.scenes[k]->AsLightFrame(*this, setups[frames], stream);
        }
    }
    launch(ll);
    RecordOrder(stream);
    for (std::size_t l = 0; l < count; ++l) {
        for (std::size_t k = 0; k < (lights[l].point ? 6u : 1u); ++k) {
            if (lights[l].scenes[k] != this) {
                lights[l].scenes[k]->RecordOrder(stream);
            }
        }
    }
}

void DeviceScene::LightingWith(const srt::LitSurface* surface, const Light* lights, std::size_t count,
                               const float ambient[3], const float* d_offsets, const int* d_ids, std::size_t row_begin,
                               std::size_t row_count, float* d_rgba, unsigned char* d_classes, hipStream_t stream) const {
    if (m_width == 0) {
        throw std::runtime_error("Lighting: Prepare() has not been called on the view scene");
    }
    CheckLightFrames(lights, count, ambient);
    if (row_begin > m_height || row_count > m_height - row_begin) {
        throw std::runtime_error("Lighting: row band outside the frame");
    }
    if (row_count == 0) {
        return;
    }
    const LightingArgs args{d_offsets, d_ids,  m_width,  m_height, row_begin, row_count, {ambient[0], ambient[1], ambient[2]},
                            d_rgba,    d_classes};
    WithLightFrames(lights, count, stream, [&](const LightingLight* ll) {
        if (surface != nullptr) {
            HipCheck(LaunchLitSurface(m_vertices, m_shade, m_n, m_frame, m_background, ll, count, args, *surface, stream),
                     "lit surface launch");
        } else {
            HipCheck(LaunchLighting(m_vertices, m_shade, m_n, m_frame, m_background, ll, count, args, stream),
                     "lighting launch");
        }
    });
}

// Lit ray hits (render.h LaunchLightHits): Lighting's checks, ordering and setups for elements that
// are (ray, id, t). This scene need not be prepared: the launch reads its shading table, its
// triangle count and its background only.
void DeviceScene::LightHits(const Light* lights, std::size_t count, const float ambient[3], const float* d_rays,
                            const int* d_ids, const float* d_t, std::size_t elements, const float* d_base,
                            const float weight[3], float* d_rgba, unsigned char* d_classes, hipStream_t stream) const {
    CheckLightFrames(lights, count, ambient);
    if (elements > 0x7FFFFFFFull) {
        throw std::runtime_error("Light hits: at most 2147483647 elements per call, got " + std::to_string(elements));
    }
    for (int k = 0; k < 3; ++k) {
        if (d_base != nullptr && !std::isfinite(weight[k])) {
            throw std::runtime_error("Light hits: weight value " + std::to_string(k) + " is not finite");
        }
    }
    if (elements == 0) {
        return;
    }
    LightHitsArgs args{d_rays, d_ids, d_t, elements, {ambient[0], ambient[1], ambient[2]}, d_base, {0.f, 0.f, 0.f}, d_rgba, d_classes};
    for (int k = 0; k < 3 && d_base != nullptr; ++k) {
        args.weight[k] = weight[k];
    }
    WithLightFrames(lights, count, stream, [&](const LightingLight* ll) {
        HipCheck(LaunchLightHits(m_shade, m_n, m_background, ll, count, args, stream), "light hits launch");
    });
}

// Sampled radiance (radiance.h LaunchRadiance): Visibility's frame checks, Lighting's light checks,
// then -- nothing enqueued or built before every check has passed -- the ordering and the light
// frames' setups of Lighting, the ray tree of Closest, and one launch.
void DeviceScene::Radiance(const Light* lights, std::size_t count, const float ambient[3], bool points,
                           const float* d_where, const int* d_ids, std::size_t row_begin, std::size_t elements,
                           const VisibilityGen& gen, bool modulate, const float* d_base, const float weight[3],
                           float* d_rgba, hipStream_t stream) const {
    if (m_width == 0) {
        throw std::runtime_error("Radiance: Prepare() has not been called");
    }
    CheckLightFrames(lights, count, ambient);
    if (!points && (row_begin > m_height || elements > m_height - row_begin)) {
        throw std::runtime_error("Radiance: row band outside the frame");
    }
    const VisibilityElements e = ElementsOf(points, d_where, d_ids, row_begin, elements, m_width, m_height);
    if (static_cast<unsigned long long>(e.width) * e.rows > 0x7FFFFFFFull) {
        throw std::runtime_error("Radiance: at most 2147483647 elements per call, got " +
                                 std::to_string(static_cast<unsigned long long>(e.width) * e.rows));
    }
    if (elements == 0) {
        return;
    }
    RadianceStore store{modulate, d_base, {0.f, 0.f, 0.f}, d_rgba};
    for (int k = 0; k < 3 && d_base != nullptr; ++k) {
        store.weight[k] = weight[k];
    }
    WithLightFrames(lights, count, stream, [&](const LightingLight* ll) {
        try {
            const RayTree* tree = EnsureRayTree(stream);
            HipCheck(LaunchRadiance(tree, m_vertices, m_shade, m_n, m_frame, m_background, ll, count, ambient, e, gen, store,
                                    stream),
                     "radiance launch");
        } catch (...) {
            RecordOrder(stream);
            throw;
        }
    });
    LogRayStats();
}

DeviceScene::StageTimes DeviceScene::TakeTimes() {
    auto elapsed = [](hipEvent_t a, hipEvent_t b) {
        HipCheck(hipEventSynchronize(b), "hipEventSynchronize(stage timing)");
        float ms = 0.f;
        HipCheck(hipEventElapsedTime(&ms, a, b), "hipEventElapsedTime(stage timing)");
        return static_cast<double>(ms);
    };
    StageTimes t;
    for (std::size_t i = 0; i < m_prep_timed; ++i) {
        t.prepare_ms += elapsed(m_prep_events[2 * i], m_prep_events[2 * i + 1]);
    }
    std::size_t binned = 0;
    for (std::size_t i = 0; i < m_timed; ++i) {
        if (m_binned[i]) {
            t.bin_ms += elapsed(m_events[4 * i], m_events[4 * i + 1]);
            ++binned;
        }
        t.kernel_ms += elapsed(m_events[4 * i + 2], m_events[4 * i + 3]);
    }
    t.launches = static_cast<unsigned>(m_timed);
    t.prepare_ms /= m_prep_timed != 0 ? static_cast<double>(m_prep_timed) : 1.0;
    t.bin_ms /= binned != 0 ? static_cast<double>(binned) : 1.0;
    t.kernel_ms /= m_timed != 0 ? static_cast<double>(m_timed) : 1.0;
    m_prep_timed = 0;
    m_timed = 0;
    return t;
}

struct Renderer::Slot {
    int device = 0;
    hipStream_t stream = nullptr;
    std::unique_ptr<DeviceScene> scene;
    std::size_t band = 0;  // band index (= slot index)
    std::size_t row_begin = 0;
    std::size_t row_count = 0;
    // Pipelined single-device render (Renderer::RenderPipelined): copy streams and per-chunk
    // events (H2D done, chunk traced); `traced[0]` also orders the device-copy gather.
    hipStream_t copy_in = nullptr;
    hipStream_t copy_out = nullptr;
    std::vector<hipEvent_t> in_done;
    std::vector<hipEvent_t> traced;
    hipEvent_t done = nullptr;  // band path: end of the frame's work on this device (polled, comm.h)
};

// The buffers of one frame size (Configure builds a new set before releasing the old one).
struct Renderer::Buffers {
    std::vector<int> devices;
    std::vector<float*> offsets;           // band rows x W x 2 per slot (one device: the frame)
    std::vector<std::uint16_t*> offsets16;  // FLOAT16 input: H2D staging
    std::vector<float*> rgba;              // band rows x W x 4 (direct mode, one device)
    std::vector<std::uint16_t*> rgba16;    // FLOAT16 output staging of rgba
    std::vector<int*> ids;                 // band rows x W hit ids (gather modes)
    int root = 0;
    float* full = nullptr;                 // root: the frame's offsets (shading), H x W x 2
    std::uint16_t* full16 = nullptr;
    int* gather = nullptr;                 // root: bands x band rows x W gathered ids
    float* frame = nullptr;                // root: H x W x 4 shaded frame
    std::uint16_t* frame16 = nullptr;
};

namespace {
// Row chunks of the pipelined single-device render: env SRT_E2E_CHUNKS (1 = no pipelining).
std::size_t E2eChunks() {
    const char* v = std::getenv("SRT_E2E_CHUNKS");
    const long c = v == nullptr || *v == '\0' ? 4 : std::strtol(v, nullptr, 10);
    return c < 1 ? 1 : (c > 16 ? 16 : static_cast<std::size_t>(c));
}

bool InterleavedFromEnv() {
    const char* v = std::getenv("SRT_BAND_ROWS");
    return v == nullptr || std::strcmp(v, "contiguous") != 0;
}

template <class T>
void FreeOn(int device, T*& p) noexcept {
    if (p != nullptr) {
        (void)hipSetDevice(device);
        (void)hipFree(p);
        p = nullptr;
    }
}
}  // namespace

Renderer::Renderer(const Scene& scene, std::vector<int> devices)
    : m_interleaved(InterleavedFromEnv()),
      m_variant(TraceVariantFromEnv()),
      m_in_half((scene.flags & kFlagInputFloat16) != 0u),
      m_out_half((scene.flags & kFlagOutputFloat16) != 0u) {
    for (std::size_t i = 0; i < devices.size(); ++i) {
        auto slot = std::make_unique<Slot>();
        slot->device = devices[i];
        slot->band = i;
        DeviceGuard guard(devices[i]);
        HipCheck(hipStreamCreateWithFlags(&slot->stream, hipStreamNonBlocking), "hipStreamCreate");
        m_slots.push_back(std::move(slot));
        m_slots.back()->scene = std::make_unique<DeviceScene>(scene, devices[i]);
    }
    m_gather_mode = m_slots.size() > 1 ? GatherModeFor(devices) : GatherMode::kDirect;
    if (m_slots.size() == 1) {  // SRT_GATHER=rccl on one device: the band path with a one-rank gather (tests)
        const char* v = std::getenv("SRT_GATHER");
        if (v != nullptr && std::strcmp(v, "rccl") == 0) {
            m_gather_mode = GatherMode::kRccl;
        }
    }
    // Gathered payload: packed ids (render.h PackedIds: 16 + k bits per pixel) with the cull variant
    // (env SRT_EXCHANGE_IDS=32: int32 ids), about half the bytes over xGMI.
    {
        const char* v = std::getenv("SRT_EXCHANGE_IDS");
        const bool force32 = v != nullptr && std::strcmp(v, "32") == 0;
        m_id_planes = m_variant == kTraceCull && !force32 ? IdPlanes(scene.triangle_count()) : -1;
    }
    if (m_gather_mode == GatherMode::kRccl) {
        try {
            m_comms = CommInitAll(devices);  // nonblocking communicators (comm.h)
        } catch (const std::exception& e) {
            throw std::runtime_error(std::string(e.what()) + " (a repeated device needs SRT_GATHER=copy or direct)");
        }
    }
}

Renderer::~Renderer() {
    if (!SyncAll()) {
        // Work that never finished still uses the device buffers (hipFree would wait for it): leak them.
        CommAbortAll(m_comms);
        for (auto& slot : m_slots) {
            (void)slot->scene.release();
        }
        (void)m_buf.release();
        return;
    }
    if (m_buf) {
        ReleaseBuffers(*m_buf);
    }
    CommDestroyAll(m_comms);
    for (auto& slot : m_slots) {
        (void)hipSetDevice(slot->device);
        slot->scene.reset();
        if (slot->done != nullptr) {
            (void)hipEventDestroy(slot->done);
        }
        for (hipEvent_t e : slot->in_done) {
            (void)hipEventDestroy(e);
        }
        for (hipEvent_t e : slot->traced) {
            (void)hipEventDestroy(e);
        }
        if (slot->copy_in != nullptr) {
            (void)hipStreamDestroy(slot->copy_in);
        }
        if (slot->copy_out != nullptr) {
            (void)hipStreamDestroy(slot->copy_out);
        }
        (void)hipStreamDestroy(slot->stream);
    }
}

std::size_t Renderer::BandIdBytes(std::size_t rows, std::size_t width) const {
    // int32 ids, or one packed band frame (a multiple of 256 B) -- in whole ints either way
    const std::size_t b = m_id_planes >= 0 ? PackedIdLayout(m_id_planes, rows, width).bytes : rows * width * sizeof(int);
    return (b + sizeof(int) - 1) / sizeof(int) * sizeof(int);
}

void Renderer::ReleaseBuffers(Buffers& b) noexcept {
    for (std::size_t i = 0; i < b.devices.size(); ++i) {
        FreeOn(b.devices[i], b.offsets[i]);
        FreeOn(b.devices[i], b.offsets16[i]);
        FreeOn(b.devices[i], b.rgba[i]);
        FreeOn(b.devices[i], b.rgba16[i]);
        FreeOn(b.devices[i], b.ids[i]);
    }
    FreeOn(b.root, b.full);
    FreeOn(b.root, b.full16);
    FreeOn(b.root, b.gather);
    FreeOn(b.root, b.frame);
    FreeOn(b.root, b.frame16);
}

void Renderer::Configure(std::size_t width, std::size_t height) {
    const std::size_t bands = m_slots.size();
    const bool multi = bands > 1;
    const bool gather = (multi || m_gather_mode == GatherMode::kRccl) && m_gather_mode != GatherMode::kDirect;
    const BandSplit split = BandSplit::Make(height, bands, m_interleaved);
    const std::size_t band_rows = split.BufferRows();
    // Allocate everything new before releasing the old buffers (strong guarantee).
    auto nb = std::make_unique<Buffers>();
    nb->offsets.assign(bands, nullptr);
    nb->offsets16.assign(bands, nullptr);
    nb->rgba.assign(bands, nullptr);
    nb->rgba16.assign(bands, nullptr);
    nb->ids.assign(bands, nullptr);
    nb->root = m_slots.front()->device;
    for (auto& sp : m_slots) {
        nb->devices.push_back(sp->device);
    }
    auto alloc = [](auto*& p, std::size_t count, const char* what) {
        void* q = nullptr;
        HipCheck(hipMalloc(&q, (count == 0 ? 1 : count) * sizeof(*p)), what);
        p = static_cast<std::remove_reference_t<decltype(p)>>(q);
    };
    try {
        for (std::size_t i = 0; i < bands; ++i) {
            DeviceGuard guard(m_slots[i]->device);
            alloc(nb->offsets[i], band_rows * width * 2, "hipMalloc(band offsets)");
            if (m_in_half) {
                alloc(nb->offsets16[i], band_rows * width * 2, "hipMalloc(band offsets f16)");
            }
            if (gather) {
                alloc(nb->ids[i], BandIdBytes(band_rows, width) / sizeof(int), "hipMalloc(band ids)");
            } else {
                alloc(nb->rgba[i], band_rows * width * 4, "hipMalloc(band framebuffer)");
                if (m_out_half) {
                    alloc(nb->rgba16[i], band_rows * width * 4, "hipMalloc(band framebuffer f16)");
                }
            }
        }
        if (gather) {
            DeviceGuard guard(nb->root);
            alloc(nb->full, height * width * 2, "hipMalloc(frame offsets)");
            if (m_in_half) {
                alloc(nb->full16, height * width * 2, "hipMalloc(frame offsets f16)");
            }
            alloc(nb->gather, bands * BandIdBytes(band_rows, width) / sizeof(int), "hipMalloc(gathered ids)");
            alloc(nb->frame, height * width * 4, "hipMalloc(frame)");
            if (m_out_half) {
                alloc(nb->frame16, height * width * 4, "hipMalloc(frame f16)");
            }
        }
    } catch (...) {
        ReleaseBuffers(*nb);
        throw;
    }
    if (m_buf) {
        if (!SyncAll()) {
            ReleaseBuffers(*nb);
            throw std::runtime_error("Configure: the devices did not finish earlier work");
        }
        ReleaseBuffers(*m_buf);
    }
    m_buf = std::move(nb);
    for (std::size_t i = 0; i < bands; ++i) {
        m_slots[i]->row_begin = split.RowBegin(i);
        m_slots[i]->row_count = split.RowCount(i);
    }
    m_band_rows = band_rows;
    m_width = width;
    m_height = height;
}

// On an exception mid-frame, copies already queued may still target the caller's host
// buffers: wait for every stream used (ignoring their errors) before the error propagates. Bounded
// (comm.h): false when a stream did not drain within the comm timeout.
bool Renderer::SyncAll() noexcept {
    const double t = CommTimeoutSeconds();
    bool ok = true;
    for (auto& sp : m_slots) {
        (void)hipSetDevice(sp->device);
        for (hipStream_t st : {sp->stream, sp->copy_in, sp->copy_out}) {
            if (st != nullptr && ok && !StreamDrain(st, t)) {
                ok = false;
            }
        }
    }
    return ok;
}

void Renderer::Render(const void* host_offsets, void* host_rgba) {
    if (!configured()) {
        throw std::runtime_error("Renderer used before Configure()");
    }
    int prev = -1;
    (void)hipGetDevice(&prev);
    try {
        if (m_slots.size() == 1 && m_gather_mode != GatherMode::kRccl && E2eChunks() > 1 &&
            m_height >= 2 * E2eChunks()) {
            RenderPipelined(host_offsets, host_rgba, E2eChunks());
        } else {
            RenderBands(host_offsets, host_rgba);
        }
    } catch (...) {
        // A failed gather may leave RCCL kernels waiting on peers: abort the communicators first
        // (their kernels exit, the streams drain); the model's later renders then fail loudly.
        if (!m_comms.empty()) {
            CommAbortAll(m_comms);
            m_comms_aborted = true;
        }
        (void)SyncAll();
        if (prev >= 0) {
            (void)hipSetDevice(prev);
        }
        throw;
    }
    if (prev >= 0) {
        (void)hipSetDevice(prev);
    }
}

// Copies band i's rows between a host frame (row_bytes per frame row) and a band-local device
// buffer: interleaved bands move one 16-row tile row per copy, contiguous bands one copy.
void Renderer::CopyBandRows(std::size_t i, const unsigned char* host, std::size_t row_bytes, unsigned char* dev,
                            hipMemcpyKind kind, bool to_host, hipStream_t stream) const {
    const Slot& s = *m_slots[i];
    const std::size_t interleave = m_interleaved && m_slots.size() > 1 ? m_slots.size() : 1;
    const std::size_t step = interleave > 1 ? static_cast<std::size_t>(kCullTileRows) : s.row_count;
    for (std::size_t l = 0; l < s.row_count; l += step) {
        const std::size_t n = std::min(step, s.row_count - l);
        const std::size_t fr = BandFrameRow(s.row_begin, interleave, l);
        unsigned char* h = const_cast<unsigned char*>(host) + fr * row_bytes;
        if (to_host) {
            HipCheck(hipMemcpyAsync(h, dev + l * row_bytes, n * row_bytes, kind, stream), "hipMemcpyAsync(band rows D2H)");
        } else {
            HipCheck(hipMemcpyAsync(dev + l * row_bytes, h, n * row_bytes, kind, stream), "hipMemcpyAsync(band rows H2D)");
        }
    }
}

// One band per device (module doc): band offsets in, hit ids traced, gathered to the first device,
// shaded there and copied out; "direct": every device shades its own rows and copies them out.
void Renderer::RenderBands(const void* host_offsets, void* host_rgba) {
    Buffers& b = *m_buf;
    const std::size_t w = m_width, h = m_height, P = m_slots.size();
    const std::size_t in_elem = m_in_half ? 2 : 4, out_elem = m_out_half ? 2 : 4;
    const auto* in_bytes = static_cast<const unsigned char*>(host_offsets);
    auto* out_bytes = static_cast<unsigned char*>(host_rgba);
    const std::size_t interleave = m_interleaved && P > 1 ? P : 1;
    const bool direct = (P == 1 && m_gather_mode != GatherMode::kRccl) || m_gather_mode == GatherMode::kDirect;
    if (m_comms_aborted) {
        throw std::runtime_error("RCCL communicators were aborted after an earlier failure; create the model again");
    }
    for (std::size_t i = 0; i < P; ++i) {
        Slot& s = *m_slots[i];
        DeviceGuard guard(s.device);
        if (s.row_count != 0) {
            auto* dst = m_in_half ? reinterpret_cast<unsigned char*>(b.offsets16[i])
                                  : reinterpret_cast<unsigned char*>(b.offsets[i]);
            CopyBandRows(i, in_bytes, w * 2 * in_elem, dst, hipMemcpyHostToDevice, false, s.stream);
            if (m_in_half) {
                HipCheck(LaunchHalfToFloat(b.offsets16[i], b.offsets[i], s.row_count * w * 2, s.stream),
                         "offsets f16 -> f32");
            }
        }
        s.scene->Prepare(w, h, s.stream);
        if (direct) {
            s.scene->Trace(b.offsets[i], b.rgba[i], s.row_begin, s.row_count, m_variant, s.stream, nullptr, interleave);
            auto* src = reinterpret_cast<unsigned char*>(b.rgba[i]);
            if (m_out_half) {
                HipCheck(LaunchFloatToHalf(b.rgba[i], b.rgba16[i], s.row_count * w * 4, s.stream),
                         "framebuffer f32 -> f16");
                src = reinterpret_cast<unsigned char*>(b.rgba16[i]);
            }
            CopyBandRows(i, out_bytes, w * 4 * out_elem, src, hipMemcpyDeviceToHost, true, s.stream);
        } else {
            s.scene->Trace(b.offsets[i], nullptr, s.row_begin, s.row_count, m_variant, s.stream, b.ids[i], interleave,
                           m_id_planes);
        }
    }
    if (!direct) {
        Slot& root = *m_slots.front();
        {
            DeviceGuard guard(root.device);  // the frame's offsets for shading
            void* dst = m_in_half ? static_cast<void*>(b.full16) : static_cast<void*>(b.full);
            HipCheck(hipMemcpyAsync(dst, in_bytes, h * w * 2 * in_elem, hipMemcpyHostToDevice, root.stream),
                     "hipMemcpyAsync(frame offsets H2D)");
            if (m_in_half) {
                HipCheck(LaunchHalfToFloat(b.full16, b.full, h * w * 2, root.stream), "offsets f16 -> f32");
            }
        }
        if (m_gather_mode == GatherMode::kRccl) {
            // Equal-size id bands (buffer rows each) gathered to the first device over xGMI, one
            // group; nonblocking communicators, so the gathers are on the streams once they settle.
            NcclCheck(ncclGroupStart(), "ncclGroupStart");
            ncclResult_t first = ncclSuccess;
            for (std::size_t i = 0; i < P; ++i) {
                Slot& s = *m_slots[i];
                const ncclResult_t r = ncclGather(b.ids[i], i == 0 ? b.gather : nullptr, BandIdBytes(m_band_rows, w), ncclUint8, 0,
                                                  static_cast<ncclComm_t>(m_comms[i]), s.stream);
                if (r != ncclSuccess && r != ncclInProgress && first == ncclSuccess) {
                    first = r;
                }
            }
            const ncclResult_t end = ncclGroupEnd();
            NcclCheck(first, "ncclGather");
            NcclCheck(end, "ncclGroupEnd (gather)", true);
            CommSettle(m_comms.data(), m_comms.size(), "gather enqueue");
        } else {
            // The same gather as device copies into the root's buffer (band i at i x buffer rows);
            // the root's stream then waits for every band's copy (an event per band).
            for (std::size_t i = 0; i < P; ++i) {
                Slot& s = *m_slots[i];
                DeviceGuard guard(s.device);
                HipCheck(hipMemcpyPeerAsync(reinterpret_cast<unsigned char*>(b.gather) + i * BandIdBytes(m_band_rows, w),
                                            root.device, b.ids[i], s.device, BandIdBytes(m_band_rows, w), s.stream),
                         "hipMemcpyPeerAsync(band gather)");
                if (i != 0) {
                    if (s.traced.empty()) {
                        hipEvent_t e = nullptr;
                        HipCheck(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate(band gather)");
                        s.traced.push_back(e);
                    }
                    HipCheck(hipEventRecord(s.traced[0], s.stream), "hipEventRecord(band gather)");
                    DeviceGuard root_guard(root.device);
                    HipCheck(hipStreamWaitEvent(root.stream, s.traced[0], 0), "hipStreamWaitEvent(band gather)");
                }
            }
        }
        DeviceGuard guard(root.device);
        root.scene->Shade(b.full, b.gather, b.frame, 0, h, root.stream, 1, m_band_rows, interleave > 1 ? P : 0, 0,
                          m_id_planes);
        const void* src = b.frame;
        if (m_out_half) {
            HipCheck(LaunchFloatToHalf(b.frame, b.frame16, h * w * 4, root.stream), "framebuffer f32 -> f16");
            src = b.frame16;
        }
        HipCheck(hipMemcpyAsync(out_bytes, src, h * w * 4 * out_elem, hipMemcpyDeviceToHost, root.stream),
                 "hipMemcpyAsync(frame D2H)");
    }
    // Every device's work done: polled with a deadline and the communicators' async errors (a
    // peer that stopped becomes an error here, not a hang).
    for (auto& sp : m_slots) {
        DeviceGuard guard(sp->device);
        if (sp->done == nullptr) {
            HipCheck(hipEventCreateWithFlags(&sp->done, hipEventDisableTiming), "hipEventCreate(done)");
        }
        HipCheck(hipEventRecord(sp->done, sp->stream), "hipEventRecord(done)");
    }
    for (auto& sp : m_slots) {
        DeviceGuard guard(sp->device);
        CommWaitEvent(sp->done, m_comms.data(), m_comms.size(), "render");
    }
}

// One device: the frame in row chunks, H2D of chunk c+1 and D2H of chunk c-1 overlapping the
// trace of chunk c (three streams, event-ordered). Every chunk is an ordinary band trace of
// the same prepared frame, so the image is bit-identical to the unchunked render.
void Renderer::RenderPipelined(const void* host_offsets, void* host_rgba, std::size_t chunks) {
    Slot& s = *m_slots.front();
    Buffers& b = *m_buf;
    DeviceGuard guard(s.device);
    const std::size_t w = m_width, h = m_height;
    const std::size_t in_elem = m_in_half ? 2 : 4, out_elem = m_out_half ? 2 : 4;
    const auto* in_bytes = static_cast<const unsigned char*>(host_offsets);
    auto* out_bytes = static_cast<unsigned char*>(host_rgba);
    if (s.copy_in == nullptr) {
        HipCheck(hipStreamCreateWithFlags(&s.copy_in, hipStreamNonBlocking), "hipStreamCreate(copy in)");
        HipCheck(hipStreamCreateWithFlags(&s.copy_out, hipStreamNonBlocking), "hipStreamCreate(copy out)");
    }
    while (s.in_done.size() < chunks) {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        HipCheck(hipEventCreateWithFlags(&e0, hipEventDisableTiming), "hipEventCreate(chunk)");
        HipCheck(hipEventCreateWithFlags(&e1, hipEventDisableTiming), "hipEventCreate(chunk)");
        s.in_done.push_back(e0);
        s.traced.push_back(e1);
    }
    float* offsets = b.offsets[0];
    float* rgba = b.rgba[0];
    const std::size_t rows = (h + chunks - 1) / chunks;
    s.scene->Prepare(w, h, s.stream);
    // Direct output (f32 output images; env SRT_E2E_DIRECT=0: off): the trace stores each chunk's
    // framebuffer rows straight into the page-locked host image through its device mapping -- the stores
    // cross PCIe from the CUs while the copy engine moves the next chunk's offsets in, instead of both
    // directions queuing on copy engines (pinned H2D + D2H at once measured 57 GB/s together, no faster
    // than one after the other). 1080p C3: 1.41 -> 0.89 ms per frame on a box whose copy path read
    // 1.41 (another box: 0.82 with copies); bit-identical (test_ml_pipelined_chunks_bitwise).
    float* direct = nullptr;
    {
        static const bool want = [] {
            const char* v = std::getenv("SRT_E2E_DIRECT");
            return v == nullptr || std::strcmp(v, "0") != 0;
        }();
        void* dp = nullptr;
        if (want && !m_out_half && hipHostGetDevicePointer(&dp, host_rgba, 0) == hipSuccess && dp != nullptr) {
            direct = static_cast<float*>(dp);
        }
        (void)hipGetLastError();  // (a pageable image: no mapping, the copy path)
    }
    for (std::size_t c = 0; c < chunks; ++c) {
        const std::size_t r0 = c * rows;
        if (r0 >= h) {
            break;
        }
        const std::size_t n = std::min(rows, h - r0);
        const std::size_t count = n * w * 2;
        void* dst = m_in_half ? static_cast<void*>(b.offsets16[0] + r0 * w * 2) : static_cast<void*>(offsets + r0 * w * 2);
        HipCheck(hipMemcpyAsync(dst, in_bytes + r0 * w * 2 * in_elem, count * in_elem, hipMemcpyHostToDevice, s.copy_in),
                 "hipMemcpyAsync(offsets chunk H2D)");
        HipCheck(hipEventRecord(s.in_done[c], s.copy_in), "hipEventRecord(chunk in)");
        HipCheck(hipStreamWaitEvent(s.stream, s.in_done[c], 0), "hipStreamWaitEvent(chunk in)");
        if (m_in_half) {
            HipCheck(LaunchHalfToFloat(b.offsets16[0] + r0 * w * 2, offsets + r0 * w * 2, count, s.stream),
                     "offsets f16 -> f32");
        }
        if (direct != nullptr) {
            s.scene->Trace(offsets + r0 * w * 2, direct + r0 * w * 4, r0, n, m_variant, s.stream);
            continue;
        }
        s.scene->Trace(offsets + r0 * w * 2, rgba + r0 * w * 4, r0, n, m_variant, s.stream);
        if (m_out_half) {
            HipCheck(LaunchFloatToHalf(rgba + r0 * w * 4, b.rgba16[0] + r0 * w * 4, n * w * 4, s.stream),
                     "framebuffer f32 -> f16");
        }
        HipCheck(hipEventRecord(s.traced[c], s.stream), "hipEventRecord(chunk traced)");
        HipCheck(hipStreamWaitEvent(s.copy_out, s.traced[c], 0), "hipStreamWaitEvent(chunk traced)");
        const void* src = m_out_half ? static_cast<const void*>(b.rgba16[0] + r0 * w * 4)
                                     : static_cast<const void*>(rgba + r0 * w * 4);
        HipCheck(hipMemcpyAsync(out_bytes + r0 * w * 4 * out_elem, src, n * w * 4 * out_elem, hipMemcpyDeviceToHost,
                                s.copy_out),
                 "hipMemcpyAsync(frame chunk D2H)");
    }
    HipCheck(hipStreamSynchronize(s.copy_out), "render (copy out)");
    HipCheck(hipStreamSynchronize(s.stream), "render");
}

}  // namespace srt
