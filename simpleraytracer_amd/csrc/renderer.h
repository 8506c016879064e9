// Device side of an ml_model: per-GPU scene copies, row-band split, RCCL gather.
//
// Replaces the reference's compute layer (tensorflow::Session):
// mlInfer -> Model::Infer -> Renderer::Render = H2D sample offsets per band -> prepare + trace
// kernels per GPU -> ncclGather of the bands to the first GPU -> D2H into the output Image.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "pin_table.h"
#include "scene.h"

namespace srt {

struct CullBins;     // render.h
struct CullSetup;    // render.h
struct ShadowLight;  // render.h
struct StageEvents;  // render.h
struct OrderScratch;  // render.h
struct SurfaceArgs;   // render.h
struct LitSurface;    // render.h
struct RayTree;       // rays.h
struct VisibilityGen;  // visibility.h

// Throws std::runtime_error("HIP error: <what>: <reason>") on failure.
void HipCheck(hipError_t err, const char* what);

// Restores the caller's current HIP device on scope exit (the C ABI must not leak a
// hipSetDevice into the host application).
class DeviceGuard {
public:
    explicit DeviceGuard(int device) {
        if (hipGetDevice(&m_prev) != hipSuccess) {
            m_prev = -1;
        }
        HipCheck(hipSetDevice(device), "hipSetDevice");
    }
    ~DeviceGuard() {
        if (m_prev >= 0) {
            (void)hipSetDevice(m_prev);
        }
    }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;

private:
    int m_prev = -1;
};

// GPU list from env ML_VISIBLE_DEVICES ("0,1,2"; unset = device 0; "cpu" or empty selects the CPU
// backend instead, cpu_render.h, and is never passed here). Validated against hipGetDeviceCount;
// throws when no HIP device is present.
std::vector<int> VisibleDevices();

// One device's resident copy of a scene plus its edge-record buffer.
class DeviceScene {
public:
    DeviceScene(const Scene& scene, int device);
    ~DeviceScene();
    DeviceScene(const DeviceScene&) = delete;
    DeviceScene& operator=(const DeviceScene&) = delete;

    int device() const { return m_device; }
    std::uint64_t triangles() const { return m_n; }
    const Camera& camera() const { return m_camera; }
    const float* background() const { return m_background; }

    // Edge setup for a W x H frame. The records are computed by the next Trace, on its stream
    // (fused into its first kernel); they stay valid until the next Prepare.
    void Prepare(std::size_t width, std::size_t height, hipStream_t stream);
    // Trace rows [row_begin, row_begin + row_count) of the prepared frame into RGBA, or (d_ids
    // non-null, d_rgba ignored) into hit ids for deferred shading.
    // row_interleave > 1: the band deals the frame's tile rows round-robin (render.h BandArgs).
    // id_planes >= 0: d_ids receives packed ids with that many bit planes (render.h PackedIds; the
    // cull variant; IdPlanes(triangles) must equal it).
    void Trace(const float* d_offsets, float* d_rgba, std::size_t row_begin, std::size_t row_count, int variant,
               hipStream_t stream, int* d_ids = nullptr, std::size_t row_interleave = 1, int id_planes = -1,
               bool rgba_frame_rows = false) const;
    // Deferred shading of rows [row_begin, row_begin + row_count) of the prepared frame from hit
    // ids (as Trace writes them) and sample offsets: the RGBA the fused trace would store.
    // frames > 1: a batch of that many frames of this camera, ids band-major as a gather of
    // band_rows-row bands leaves them (render.h LaunchShade), rgba [frames][row_count][width].
    // interleaved > 0: the gathered bands are that many interleaved bands. offsets_stride: floats
    // between consecutive frames' offsets (0: the batch shares d_offsets).
    void Shade(const float* d_offsets, const int* d_ids, float* d_rgba, std::size_t row_begin, std::size_t row_count,
               hipStream_t stream, std::size_t frames = 1, std::size_t band_rows = 0,
               std::size_t interleaved = 0, std::size_t offsets_stride = 0, int id_planes = -1,
               long skip_band = -1,  // skip_band: rows of that band are left as they are
               std::size_t own_bands = 0,  // and of bands [0, own_bands) (render.h LaunchShade)
               std::size_t first_rows = 0) const;  // contiguous: band 0's rows (BandSplit::first_rows)
    // `frames` (<= render.h kMaxTableFrames) frames of the prepared camera, rows [row_begin,
    // row_begin + row_count) each: frame f's offsets d_offsets[f], its RGBA d_rgba[f] or (d_ids
    // non-null) its hit ids d_ids[f]. Each frame gets the whole per-frame pipeline (record setup,
    // bins, work list, trace), as `frames` Prepare + Trace calls would; the cull variant runs all
    // frames in one launch per stage (render.h LaunchCullFrames; more than kMaxBatch frames read
    // their parameters from a device table uploaded once per call), the others frame by frame.
    // Whole frames of the binned cull variant run on the shared setup instead (below; env SRT_SETUP):
    // the record setup, bins and work plan once per prepared frame, tile facts + trace per frame.
    void TraceBatch(const float* const* d_offsets, float* const* d_rgba, int* const* d_ids, std::size_t frames,
                    std::size_t row_begin, std::size_t row_count, int variant, hipStream_t stream,
                    std::size_t row_interleave = 1, int id_planes = -1, bool rgba_frame_rows = false,
                    const std::size_t* row_begins = nullptr, std::size_t plan_frames = 0) const;
    // (A frame f with d_ids non-null but d_ids[f] null and d_rgba[f] non-null is traced to RGBA;
    // rgba_frame_rows: RGBA outputs are whole frames, band rows stored at their frame rows;
    // row_begins: frame f's band starts at row_begins[f] instead -- one row count and pattern, so one
    // band shape, for every frame; cull variant, bands short of the whole frame.
    // plan_frames > frames: on the shared setup the trace grid is the one of a plan_frames-frame
    // call, so the chunks of a longer frame set -- RenderSamples' -- share one setup build.)

    // Pinned offsets (include/srt_pins.h rtnPinOffsetsAsync). The tile facts of a whole-frame offsets
    // buffer -- per tile its first offset and whether its offsets are all equal, usable and in range
    // -- are a function of the buffer's contents and of W x H alone, and a caller that keeps a sample
    // pattern for many frames says so here: PinOffsets computes them once, on `stream`, with the
    // facts kernel of the traces themselves (render.h LaunchTileFacts; the same bits) into a buffer
    // the scene owns, keyed by the pointer. TraceShared then gives a frame with that pointer the
    // stored facts, and a launch whose frames are all pinned runs no facts launch. The scene cannot
    // see a buffer change: while pinned, the caller does not write it, and unpins it before freeing
    // it; pinning it again recomputes the facts (new contents). At most PinTable::kMaxPins, one more
    // is an error. A call on the scene for the ordering rule; needs a prepared scene. Prepare at the
    // same size, SetCamera and SetVertices keep the pins; Prepare at another size drops them all.
    // Bands, SRT_SETUP=frame, the other variants, SRT_EMPTY_FILL=facts and an explicit
    // SRT_FACTS_KERNEL=lean|block (which asks for that facts kernel in the launch) compute their own
    // facts whatever is pinned; env SRT_FACTS_PINS=0 (read per call; default 1) makes every trace do so.
    // A pin also learns its summary: whether every tile of the buffer is regular, usable and in range
    // (render.h LaunchFactsSummary, queued behind the facts launch; PinOffsets stays asynchronous).
    // It is unknown until that work has completed -- a trace finds out with hipEventQuery, without
    // waiting --, and a pin again makes it unknown before the new facts launch is queued. A launch
    // whose frames are all pinned with a known all-regular summary runs the trace kernel without the
    // position table (a regular launch: render.h CullSetup::regular_trace; counted in
    // SetupStats::regular_launches); any other launch runs the general kernel: the same bits. Env
    // SRT_TRACE_POS = auto (default) | table, read per call: table never takes the regular form.
    void PinOffsets(const float* d_offsets, hipStream_t stream);
    // Waits for the summaries of the standing pins that are still unknown (a caller outside its timed
    // region, such as FrameEngine::SetInputs: the launches that follow then find them known).
    void ResolvePinSummaries();
    // Forgets the pin of d_offsets (not pinned: nothing). Waits for the scene's previous work, which
    // may read the facts, before it frees them.
    void UnpinOffsets(const float* d_offsets);
    std::size_t pinned() const;

    // Point queries: the closest hit at `count` image positions (fx, fy) of the prepared frame
    // (d_positions: count x 2) into d_ids (-1 = miss), d_t (+inf = miss) and, non-null, d_how
    // (render.h QueryArgs), answered from the shared setup's lists (built here if the prepared
    // frame has none yet, for the one-frame trace grid).
    void Query(const float* d_positions, std::size_t count, int* d_ids, float* d_t, unsigned char* d_how,
               hipStream_t stream) const;

    // Depth layers (render.h LaunchLayers): the `layers` (1 .. kMaxLayers) nearest hits, front to
    // back, at `count` image positions (points: d_where = count x 2 positions, row_begin unused) or
    // at the pixels of the band rows [row_begin, row_begin + count) (d_where = the band's sample
    // offsets, band-local as Shade's) into d_ids (layers x elements, layer-major), d_t (the same
    // shape, may be null) and d_how (elements, may be null). The shared setup is Query's.
    void Layers(bool points, const float* d_where, std::size_t row_begin, std::size_t count, std::size_t layers,
                int* d_ids, float* d_t, unsigned char* d_how, hipStream_t stream) const;
    // Composite (render.h LaunchComposite): the band rows [row_begin, row_begin + row_count) from
    // `layers` id planes (d_ids: layers x row_count x width) under the opacity table d_opacity (one
    // float per triangle) into d_rgba. Reads the shading table only: no cull setup is built or read.
    void Composite(const float* d_offsets, const int* d_ids, std::size_t layers, const float* d_opacity,
                   std::size_t row_begin, std::size_t row_count, float* d_rgba, hipStream_t stream) const;

    // Spot-light shadow mask (render.h LaunchShadow) of the band rows [row_begin, row_begin +
    // row_count) of this scene's prepared frame, the light being `light`'s prepared frame: d_offsets
    // and d_ids band-local as Shade's, d_mask row_count x width class bytes, d_rgba (may be null)
    // the shaded pixels dimmed by class. Both scenes are prepared, on one device, with the same
    // number of triangles. Builds the light's shared setup if its prepared frame has none yet, as
    // Query does; both scenes' calls are ordered against this one (OrderAfterPrevious / RecordOrder).
    void Shadow(const DeviceScene& light, const float* d_offsets, const int* d_ids, std::size_t row_begin,
                std::size_t row_count, float bias, unsigned char* d_mask, float* d_rgba, float dim,
                hipStream_t stream) const;

    // Omni-light shadow mask (render.h LaunchOmniShadow): Shadow under a point light given as its six
    // cube-face scenes (omni_math.h), all prepared at one size, on this scene's device, with this
    // scene's number of triangles. d_face (may be null): the selected face per pixel. Builds every
    // face's shared setup that its prepared frame lacks; one launch; this scene's and the six faces'
    // calls are ordered against this one.
    void OmniShadow(const DeviceScene* const faces[6], const float* d_offsets, const int* d_ids, std::size_t row_begin,
                    std::size_t row_count, float bias, unsigned char* d_mask, unsigned char* d_face, float* d_rgba,
                    float dim, hipStream_t stream) const;

    // Direct lighting (render.h LaunchLighting) of the band rows [row_begin, row_begin + row_count) of
    // this scene's prepared frame under `count` (0 .. kLightingMaxLights) lights, each one prepared
    // scene (spot) or six cube-face scenes (point), at most kLightingMaxFrames scenes in all, on this
    // scene's device, with this scene's number of triangles; a scene may appear more than once.
    // d_rgba row_count x width x 4; d_classes (may be null) count x row_count x width class bytes.
    // Builds every light frame's shared setup that its prepared frame lacks; one launch; this
    // scene's and every light scene's calls are ordered against this one. Every rule about the
    // lights is checked here, before anything is enqueued or built, and the message names the light
    // and the field; CheckLights is that part for a caller without device scenes (the host call):
    // the count, the ambient colour, the frame total and every light's colour, falloff and bias.
    struct LightTerms {
        bool point;
        const float* color;
        float falloff, bias;
    };
    static void CheckLights(const LightTerms* lights, std::size_t count, const float ambient[3]);
    static void CheckLightCount(std::size_t count);  // (before a caller reads `count` structs)
    struct Light {
        const DeviceScene* const* scenes;  // 1 (spot) or 6 (point)
        bool point;
        float color[3];
        float falloff, bias;
    };
    void Lighting(const Light* lights, std::size_t count, const float ambient[3], const float* d_offsets,
                  const int* d_ids, std::size_t row_begin, std::size_t row_count, float* d_rgba,
                  unsigned char* d_classes, hipStream_t stream) const;
    // Lit surfaces (render.h LaunchLitSurface): Lighting with the pixel's normal and albedo from the
    // caller's device tables in `surface` and, if it holds one, a material. Every rule of Lighting
    // applies; the caller has checked the surface and the material (render.h LitSurface).
    void LitSurface(const Light* lights, std::size_t count, const float ambient[3], const srt::LitSurface& surface,
                    const float* d_offsets, const int* d_ids, std::size_t row_begin, std::size_t row_count,
                    float* d_rgba, unsigned char* d_classes, hipStream_t stream) const;
    // Lit ray hits (render.h LaunchLightHits): Lighting for `elements` (at most 2^31 - 1) hits given
    // as (ray, id, t) -- d_rays elements x 8, d_ids and d_t elements each -- into d_rgba (elements x
    // 4) and d_classes (may be null; count x elements). d_base (may be null: store; may be d_rgba)
    // with weight[3] (finite; read with a base only): the element is added onto it. This scene need
    // not be prepared; every rule of Lighting about the lights applies, in Lighting's words.
    void LightHits(const Light* lights, std::size_t count, const float ambient[3], const float* d_rays, const int* d_ids,
                   const float* d_t, std::size_t elements, const float* d_base, const float weight[3], float* d_rgba,
                   unsigned char* d_classes, hipStream_t stream) const;
    // Sampled radiance (radiance.h LaunchRadiance): per element of the prepared frame -- Visibility's
    // elements -- the generator's rays walked to their closest hits, the hits shaded as LightHits shades
    // them and averaged in ascending sample order, one launch. gen.kind: hemisphere or mirror.
    // modulate: times the albedo of the element's own triangle. d_base (may be null: store; may be
    // d_rgba) with weight[3] (finite; read with a base only). The ray tree as Closest's; every rule of
    // Lighting about the lights applies, in Lighting's words.
    void Radiance(const Light* lights, std::size_t count, const float ambient[3], bool points, const float* d_where,
                  const int* d_ids, std::size_t row_begin, std::size_t elements, const VisibilityGen& gen, bool modulate,
                  const float* d_base, const float weight[3], float* d_rgba, hipStream_t stream) const;

    // G-buffer: the surface attributes (render.h GBufferArgs: depth, bary, normal, albedo; a null
    // plane is not written) of hit ids on the prepared frame. points: `count` positions d_where
    // (count x 2) with d_ids (count), row_begin unused. Else the band rows [row_begin, row_begin +
    // count) of the frame, d_where its sample offsets and d_ids its ids, band-local as Shade's.
    // Reads the scene's vertices and shading table only: no cull setup is built or read.
    void GBuffer(bool points, const float* d_where, const int* d_ids, std::size_t row_begin, std::size_t count,
                 float* d_depth, float* d_bary, float* d_normal, float* d_albedo, hipStream_t stream) const;

    // Vertex attributes (render.h SurfaceArgs / InterpolateArgs) of hit ids on the prepared frame:
    // elements as GBuffer's (points, d_where, d_ids, row_begin, count). Surface: the planes of
    // `planes` asked for (its element fields are ignored) from the caller's device tables in it.
    // Interpolate: one corner table (n x 3 x channels) into d_out (elements x channels). The scene
    // keeps no table. Both read the scene's vertices and shading table only: no cull setup is built
    // or read (neither calls EnsureSetup).
    void Surface(bool points, const float* d_where, const int* d_ids, std::size_t row_begin, std::size_t count,
                 const SurfaceArgs& planes, hipStream_t stream) const;
    void Interpolate(bool points, const float* d_where, const int* d_ids, std::size_t row_begin, std::size_t count,
                     const float* d_table, std::size_t channels, float* d_out, hipStream_t stream) const;

    // Multi-sample frames (render.h LaunchResolve). Resolve: the band rows [row_begin, row_begin +
    // row_count) of the prepared frame from `samples` (1 .. kMaxSamples) planes of sample offsets
    // and hit ids -- host arrays of device pointers, band-local as Shade's -- into d_rgba: the mean
    // of the shaded samples, alpha = the share that hit. Reads the shading table only: no cull
    // setup is built or read. RenderSamples: the whole frame -- the id planes traced into the
    // caller's d_ids through TraceBatch in chunks of at most kMaxBatch (one setup build for all of
    // them on the shared setup), then resolved.
    void Resolve(const float* const* d_offsets, const int* const* d_ids, std::size_t samples, std::size_t row_begin,
                 std::size_t row_count, float* d_rgba, hipStream_t stream) const;
    void RenderSamples(const float* const* d_offsets, int* const* d_ids, std::size_t samples, float* d_rgba,
                       int variant, hipStream_t stream) const;

    // Motion (include/srt_motion.h): the scene takes another camera, or other vertices (d_vertices:
    // device, triangles x 9, copied on `stream`), in place. Afterwards it is the scene a fresh
    // construction over the new pose would be, for every call above, bit for bit; a prepared scene
    // stays prepared at its W x H. reorder: the spatial order is rebuilt under the new pose on
    // `stream` (keys, radix sort, gather; the sort scratch is allocated by the first such update);
    // else it stands -- a camera change then enqueues nothing, a vertex change the normals and the
    // gather. A call on the scene for the ordering rule; no allocation besides that scratch, no
    // host synchronisation.
    void SetCamera(const Camera& camera, bool reorder, hipStream_t stream);
    void SetVertices(const float* d_vertices, bool reorder, hipStream_t stream);

    // Ray queries (include/srt_rays.h; rays.h): the closest hit (d_ids, d_t and, non-null, d_bary:
    // count x 2) or the occlusion byte (d_out) of `count` caller-supplied rays (d_rays: count x 8
    // floats, 16-byte aligned), answered from the scene's world-space tree -- or, env SRT_RAYS=brute
    // (read per call), by brute force over the vertices, which needs no tree. The tree depends on
    // the vertices only: no Prepare is needed, a camera move leaves it alone, SetVertices marks it
    // stale. It is built by the first call that needs it (or BuildRays), on that call's stream, and
    // rebuilt in the same buffers by the first call after SetVertices: allocation at the first
    // build only, no host synchronisation. Calls on the scene for the ordering rule.
    void BuildRays(hipStream_t stream) const;
    void Closest(const float* d_rays, std::size_t count, int* d_ids, float* d_t, float* d_bary,
                 hipStream_t stream) const;
    void Occluded(const float* d_rays, std::size_t count, unsigned char* d_out, hipStream_t stream) const;
    // Builds of the tree so far and the builds that allocated (0 or 1). Env SRT_SETUP_LOG=1 prints
    // them to stderr after every ray call ("srt rays: ...").
    struct RayStats {
        unsigned long long builds = 0;
        unsigned long long allocations = 0;
    };
    RayStats ray_stats() const { return m_ray_stats; }

    // Sampled visibility (include/srt_visibility.h; visibility.h): the generator's S rays from the
    // surface point of every element of the prepared frame -- elements as GBuffer's (points,
    // d_where, d_ids, row_begin, count) -- traced through the ray queries' tree in the same launch
    // and counted (Visibility: d_visible, d_fraction, a null plane is not written), or exported
    // sample-major (VisibilityRays: d_rays, S x elements x 8 floats). Visibility builds or rebuilds
    // the tree as Closest does (EnsureRayTree; env SRT_RAYS=brute); VisibilityRays reads the vertices
    // only. The caller has checked the generator. Calls on the scene for the ordering rule.
    void Visibility(bool points, const float* d_where, const int* d_ids, std::size_t row_begin, std::size_t count,
                    const VisibilityGen& gen, unsigned char* d_visible, float* d_fraction, hipStream_t stream) const;
    void VisibilityRays(bool points, const float* d_where, const int* d_ids, std::size_t row_begin, std::size_t count,
                        const VisibilityGen& gen, float* d_rays, hipStream_t stream) const;

    std::size_t width() const { return m_width; }
    // The spatial order (device, triangles entries) and the time its build took at load (ms).
    const unsigned* order() const { return m_order; }
    double build_ms() const { return m_build_ms; }
    std::size_t height() const { return m_height; }

    // Stage timing: while on, Prepare and Trace bind HIP events to their kernels' dispatch
    // packets (render.h StageEvents). TakeTimes waits for them and returns the mean durations
    // (ms) of the calls timed since the previous TakeTimes, then forgets them.
    struct StageTimes {
        unsigned launches = 0;     // timed Trace calls
        double prepare_ms = 0.0;   // PrepareKernel (mean over timed Prepare calls)
        double bin_ms = 0.0;       // bin stage (cull: BinTriangles start .. WorkOrder end; on the shared setup
                                   // the per-frame tile-facts launch, the one-off build uncounted, and a launch
                                   // of pinned frames, which has none, not counted as a stage); 0 otherwise
        double kernel_ms = 0.0;    // the trace kernel alone
    };
    void SetTiming(bool on);
    StageTimes TakeTimes();
    // Records of the binned traces (render.h RecordMode; the env SRT_TRACE_RECORDS overrides it):
    // the frame engine sets kRecordsRecompute when it keeps one frame queue per device.
    void SetRecordMode(int mode);
    // Which setup the binned cull traces ran on (env SRT_SETUP, read per call): builds of the shared
    // setup, frames traced on it, frames traced with a per-frame setup (the bin launch of
    // bands, per-frame row_begins and SRT_SETUP=frame). The other variants and the unbinned cull
    // trace count in none of them. Env SRT_SETUP_LOG=1 prints them to stderr after every such call.
    struct SetupStats {
        unsigned long long builds = 0;
        unsigned long long shared_frames = 0;
        unsigned long long per_frame_frames = 0;
        // Of shared_frames, those whose trace read the setup's record stream (env SRT_TRACE_STREAM,
        // read per call; default 1), and the records of the stream now standing (0: none).
        unsigned long long stream_frames = 0;
        unsigned long long stream_records = 0;
        unsigned long long empty_descs = 0;   // statically empty descriptors of the standing setup's plan
        unsigned long long sweep_blocks = 0;  // sweep blocks per frame of the last shared trace (0: sweep off)
        // Of shared_frames, those whose tile-facts launch was asked to fill the statically empty
        // tiles (env SRT_EMPTY_FILL=facts, with the sweep on; the default is sweep: 0).
        unsigned long long facts_fill_frames = 0;
        // Of shared_frames, those whose facts launch was the lean kernel (env SRT_FACTS_KERNEL; auto:
        // launches in which frames share an offsets buffer).
        unsigned long long lean_facts_frames = 0;
        // Of shared_frames, those whose trace read the stored facts of a pinned offsets buffer, and
        // the facts launches issued: one per shared launch with an unpinned frame, one per PinOffsets.
        unsigned long long pinned_frames = 0;
        unsigned long long facts_launches = 0;
        // Shared launches that ran the regular trace kernel (every frame pinned, all-regular summary).
        unsigned long long regular_launches = 0;
    };
    SetupStats setup_stats() const { return m_setup_stats; }

private:
    int m_device;
    std::uint64_t m_n;
    Camera m_camera;
    float m_background[3];
    float* m_vertices = nullptr;
    float* m_shade = nullptr;  // shading table: 8 floats per triangle (LaunchShadeTable)
    mutable float* m_edges = nullptr;        // kEdgeFloatsPerTriangle per padded record, per frame slot
    mutable std::size_t m_edge_slots = 1;    // frame slots of m_edges (TraceBatch grows it; slot 0 = Trace's)
    // Sort scratch of the reordering updates (render.h OrderScratch): sizes depend on the triangle
    // count only; allocated by the first such update, freed with the scene.
    OrderScratch* m_scratch = nullptr;
    // The world-space tree of the ray queries (rays.h): null until the first build; stale after
    // SetVertices until the next ray call rebuilds it in place.
    mutable RayTree* m_rays = nullptr;
    mutable bool m_rays_stale = true;
    mutable RayStats m_ray_stats{};
    const RayTree* EnsureRayTree(hipStream_t stream) const;  // (re)built on `stream` if need be; null: brute force
    void LogRayStats() const;
    // The one place that knows what a pose (camera, vertices) shapes: every cache below that is a
    // function of it is dropped or marked for its lazy rebuild (renderer.cpp).
    void PoseChanged(bool vertices);
    unsigned* m_order = nullptr;  // record ids in spatial order (BuildSpatialOrder), for the cull bins
    unsigned* m_rank = nullptr;   // its inverse: record id -> position
    float* m_svertices = nullptr; // vertices in spatial order (svertices[i] = vertices[order[i]])
    double m_build_ms = 0.0;      // spatial order build (BuildSpatialOrder) at load
    // Per 256-position block of the spatial order: the y extent of its records' screen boxes under the
    // prepared frame (render.h LaunchBlockExtents), the band record pass's skip hint; computed on the
    // first binned trace after a Prepare (m_ext_pending). Env SRT_BLOCK_SKIP=0: never (no skip).
    mutable float2* m_block_ext = nullptr;
    mutable bool m_ext_pending = true;
    void EnsureBlockExtents(hipStream_t stream) const;
    // The shared cull setup of the prepared frame (render.h CullSetup): records, bins and work plan
    // of a whole-frame binned trace, which depend on the scene, the camera and W x H only. Its own
    // buffers (edge slot 0 belongs to the record passes of the other variants). Built on the stream
    // of the first such trace after a Prepare that changed the frame (m_setup_pending), and again
    // whenever what shapes it changed (m_setup_key); calls on one scene are stream-ordered
    // (OrderAfterPrevious), so later traces on any stream see it complete.
    struct SetupKey {
        std::size_t width = 0, height = 0;
        unsigned capacity = 0, descs = 0, min_chunk = 0;
        bool recompute = false;
        bool stream = false;         // the record stream was asked for (SRT_TRACE_STREAM, stored records)
        std::size_t stream_cap = 0;  // ... up to this many records (a longer one: the indexed path)
        bool sweep = false;          // the plan is in the empty sweep's order (SRT_EMPTY_SWEEP)
    };
    mutable unsigned char* m_setup = nullptr;
    mutable std::size_t m_setup_bytes = 0;
    // The setup's record stream (render.h): sized from the built plan, so an allocation of its own;
    // m_stream_on: the standing setup has one (m_stream_records records of it are in use).
    mutable unsigned char* m_stream = nullptr;
    mutable std::size_t m_stream_capacity = 0;  // records allocated
    mutable std::size_t m_stream_records = 0;
    mutable bool m_stream_on = false;
    mutable unsigned m_list_descs = 0, m_empty_descs = 0;  // the standing setup's plan (render.h CullSetup)
    mutable unsigned m_full_empty_descs = 0;                // (its stream_count[2]: bars regular launches)
    mutable bool m_setup_pending = true;
    mutable SetupKey m_setup_key{};
    mutable SetupStats m_setup_stats{};
    void LogSetupStats() const;
    // Pinned offsets: pointer -> facts buffer (CullTiles(W, H) x 16 B each, hipMalloc'ed here). A
    // removed pin's buffer is freed by ReleaseRetiredPins, after the scene's previous work. With each
    // facts buffer go the pin's summary word (page-locked, mapped) and the event recorded behind the
    // launch that writes it. mutable: a trace (const) records a summary it finds completed.
    mutable PinTable m_pins;
    // The words and events are recycled: page-locked memory is allocated a chunk of kMaxPins words at
    // a time (hipHostMalloc and hipHostFree per pin doubled SetInputs' time), an event is created
    // when none is free; both go back to the free lists when a pin's buffers are released and are
    // destroyed with the scene.
    std::vector<void*> m_pin_word_chunks;
    std::vector<void*> m_free_pin_words;
    std::vector<void*> m_free_pin_events;
    PinTable::Buffers NewPinBuffers(std::size_t tiles);      // throws; nothing is left allocated then
    void ReleasePinBuffers(const PinTable::Buffers& b);      // after the work that uses them
    // The summary of `key`'s pin: known, or read now if its event has completed (wait: after waiting
    // for it); kUnknown otherwise, and for a key that is not pinned.
    PinTable::Summary PinSummary(const void* key, bool wait) const;
    void WaitForPrevious() const;  // the host waits for the scene's last call
    void ReleaseRetiredPins();
    // Whether a binned cull trace of this band runs on the shared setup (env SRT_SETUP).
    bool OnSharedSetup(std::size_t row_begin, std::size_t row_count, std::size_t row_interleave) const;
    // Whole frames on the shared setup: the setup (re)built if need be, then tile facts + trace.
    // plan_frames: the call whose trace grid is used (TraceBatch; at least `frames`).
    void TraceShared(const float* const* d_offsets, float* const* d_rgba, int* const* d_ids, std::size_t frames,
                     hipStream_t stream, int id_planes, bool rgba_frame_rows, std::size_t plan_frames) const;
    // The setup for a trace grid of `descs` descriptors, (re)built on `stream` if need be.
    CullSetup EnsureSetup(unsigned descs, hipStream_t stream) const;
    // The setup a point query of the prepared frame reads (Query, Shadow), (re)built on `stream` if
    // need be; false: no usable setup (SRT_SETUP=frame, SRT_CULL_BIN=0, a shape that cannot be binned).
    bool QuerySetup(CullSetup& setup, hipStream_t stream) const;
    // Whether QuerySetup would give a setup, and whether a launch on it (or without one) recomputes
    // its records: known without building anything.
    bool QuerySetupUsable() const;
    bool QueryRecomputes() const;
    // A light frame's scene `f` against this view scene (Shadow, OmniShadow, Lighting): prepared, at
    // its light's size (`first`: the light's first frame), on this device, of as many triangles --
    // else thrown in the family's own words.
    struct LightWords {
        const char* who;         // "Shadow", "Omni shadow", "Lighting: light 3"
        const char* unprepared;  // who + this
        const char* faces;       // "the light's faces" or "the faces": prepared at different sizes
        const char* light;       // "the light scene" or "the light": what lives on another device
        const char* its_scene;   // "the light scene" or "the light's scene": whose triangles are counted
    };
    void CheckLightScene(const DeviceScene& f, const DeviceScene& first, const LightWords& w) const;
    // What Lighting, LitSurface and LightHits share: the lights checked before any side effect, and
    // the launch between the ordering, the light frames' setups and the recording (renderer.cpp).
    void CheckLightFrames(const Light* lights, std::size_t count, const float ambient[3]) const;
    template <class Launch>
    void WithLightFrames(const Light* lights, std::size_t count, hipStream_t stream, Launch&& launch) const;
    // Lighting (surface == nullptr) and LitSurface: the same checks, ordering and setups, one launch.
    void LightingWith(const srt::LitSurface* surface, const Light* lights, std::size_t count, const float ambient[3],
                      const float* d_offsets, const int* d_ids, std::size_t row_begin, std::size_t row_count,
                      float* d_rgba, unsigned char* d_classes, hipStream_t stream) const;
    // This scene as a light frame of `view`'s launch on `stream`: ordered after its previous call,
    // its query setup (re)built into `setup` if it has one.
    ShadowLight AsLightFrame(const DeviceScene& view, CullSetup& setup, hipStream_t stream) const;
    Frame m_frame{};
    std::size_t m_width = 0;
    std::size_t m_height = 0;
    // Cull variant work buffers (render.h CullBins: tile info, bin lists, split-tile keys), grown on
    // demand by Trace; disabled by env SRT_CULL_BIN=0 (every tile then streams every record). One
    // arena per band shape in use (a band-sharing engine traces two or three shapes per batch on one
    // scene; one arena re-carved per call cost a counter fill and a new work plan every call), at most
    // kCullArenas, the least recently used re-carved for a new shape.
    // Per frame slot: frames binned in it (their parity picks the count buffer) and the trace grid
    // its work plan was built for (0: none; render.h CullBins::plan).
    struct CullSlotState {
        unsigned uses = 0;
        unsigned plan_descs = 0;
    };
    struct CullArena {
        unsigned char* work = nullptr;
        std::size_t bytes = 0;       // allocated
        std::uint64_t shape = 0;     // (width << 32) | rows of its carve-up (0: none)
        std::size_t layout = 0;      // bytes per slot (they change with the split width too)
        std::size_t zeroed = 0;      // frame slots of the carve-up whose counters are zero-filled
        std::uint64_t used = 0;      // last use (m_cull_clock)
        std::vector<CullSlotState> state;
    };
    static constexpr std::size_t kCullArenas = 4;
    mutable std::vector<CullArena> m_arenas;
    mutable std::size_t m_arena = 0;         // the arena of the current call
    mutable std::uint64_t m_cull_clock = 0;
    mutable unsigned m_cull_gen = 0;         // frames binned (render.h CullBins::gen)
    // The cull work of frame slots [0, slots) for a row_count-row band (grown, zeroed on first use
    // of a slot with this carve-up), and slot `slot`'s carve-up with a fresh frame number for a trace
    // grid of at most `descs` descriptors; it (re)builds the slot's work plan when the slot has none
    // for that grid.
    void EnsureCullWork(std::size_t slots, std::size_t row_count, hipStream_t stream) const;
    CullBins CullSlot(std::size_t slot, std::size_t row_count, unsigned descs = ~0u) const;
    void DropPlans(std::size_t slots) const;  // slots [0, slots) of every arena rebuild their plans
    void EnsureEdgeSlots(std::size_t slots, hipStream_t stream) const;
    // BVH variant: node boxes + depth bounds (render.h BvhLayout), allocated by the first bvh Trace.
    mutable unsigned char* m_bvh = nullptr;
    // Parameter tables of TraceBatch calls of more than kMaxBatch frames (render.h CullTable): a
    // ring of device tables with page-locked host staging; a staging buffer is rewritten only after
    // its previous upload has executed (its event), the device copy is protected by stream order.
    struct ParamTable {
        void* device = nullptr;
        void* host = nullptr;
        void* host_device = nullptr;  // `host` mapped into the device's address space (render.h CullTable)
        hipEvent_t uploaded = nullptr;
        std::size_t frames = 0;
        bool pending = false;
    };
    static constexpr std::size_t kParamTables = 4;
    mutable ParamTable m_tables[kParamTables];
    mutable std::size_t m_table_next = 0;
    ParamTable& AcquireTable(std::size_t frames, hipStream_t stream) const;  // after OrderAfterPrevious(stream)
    // Stage-timing events, reused: per timed Prepare (begin, end), per timed Trace (bin begin,
    // bin end, begin, end); the first m_prep_timed / m_timed entries hold pending launches.
    hipEvent_t TimingEvent(std::vector<hipEvent_t>& pool, std::size_t i) const;
    StageEvents BindStageEvents(bool prep, bool staged) const;
    bool m_timing = false;
    int m_records = 0;  // render.h RecordMode (kRecordsAuto)
    bool RecomputeRecords(std::size_t frames) const;
    // Calls on one scene are stream-ordered: the per-frame edge records and the cull work buffer
    // are shared state, so a call on another stream than the previous one first waits for it.
    void OrderAfterPrevious(hipStream_t stream) const;
    void RecordOrder(hipStream_t stream) const;
    mutable hipStream_t m_last_stream = nullptr;
    mutable bool m_used = false;
#ifndef SRT_ORDER_EVENTS
#define SRT_ORDER_EVENTS 4
#endif
    static constexpr std::size_t kOrderEvents = SRT_ORDER_EVENTS > 0 ? SRT_ORDER_EVENTS : 1;
    mutable hipEvent_t m_order_events[kOrderEvents] = {};
    mutable std::size_t m_order_next = 0;
    mutable std::vector<hipEvent_t> m_prep_events;
    mutable std::vector<hipEvent_t> m_events;
    mutable std::vector<bool> m_binned;
    mutable std::size_t m_prep_timed = 0;
    mutable bool m_prepare_pending = false;  // the full record pass has not run for the prepared frame
    mutable std::size_t m_timed = 0;
};

// Trace kernel variant from env SRT_TRACE_VARIANT ("lds" | "scalar" | "cull", default cull).
int TraceVariantFromEnv();

// How Renderer assembles a multi-device frame (env SRT_GATHER): "rccl" = the devices' hit-id bands
// gathered to the first device with ncclGather, which shades the frame and copies it out
// (default for distinct devices; on ONE device it selects a one-rank gather through the same band
// path, which puts the RCCL calls, their waits and the abort on a one-GPU box); "copy" = the same gather by device-to-device copies (default
// when a device repeats: RCCL needs distinct devices); "direct" = every device traces and shades
// its own band and copies its rows straight into the host image (no gather).
enum class GatherMode { kRccl, kCopy, kDirect };

// The device side of an ml_model (mlInfer). One device: the frame in row chunks, copies in and out
// overlapping the traces. Several (ML_VISIBLE_DEVICES): the frame's 16-row tile rows dealt
// round-robin to the devices (env SRT_BAND_ROWS=contiguous: one block each), every device traces
// its band into hit ids (4 B per pixel), the bands are gathered to the first device, which shades
// the whole frame from them (bit-identical to the fused trace) and copies it out. All launches
// from the calling thread; the RCCL gathers of all devices in one group.
class Renderer {
public:
    Renderer(const Scene& scene, std::vector<int> devices);
    ~Renderer();
    Renderer(const Renderer&) = delete;
    Renderer& operator=(const Renderer&) = delete;

    // (Re)allocate band buffers for a W x H frame. Strong guarantee: on failure the previous
    // configuration is kept.
    void Configure(std::size_t width, std::size_t height);
    bool configured() const { return m_width != 0; }

    // Render one frame: host offsets (H x W x 2) -> host RGBA (H x W x 4). Synchronous.
    // Element types from the scene's flags (kFlagInputFloat16 / kFlagOutputFloat16): float,
    // or IEEE binary16 bit patterns, converted on the device (the copies then move half the bytes).
    void Render(const void* host_offsets, void* host_rgba);
    bool input_half() const { return m_in_half; }
    bool output_half() const { return m_out_half; }

    std::size_t bands() const { return m_slots.size(); }
    GatherMode gather_mode() const { return m_gather_mode; }

private:
    struct Slot;
    struct Buffers;
    void ReleaseBuffers(Buffers& b) noexcept;
    void RenderPipelined(const void* host_offsets, void* host_rgba, std::size_t chunks);
    void RenderBands(const void* host_offsets, void* host_rgba);
    bool SyncAll() noexcept;  // bounded drain of every stream; false when one did not drain
    std::size_t BandIdBytes(std::size_t rows, std::size_t width) const;  // one band's id payload
    // Host-to-device copy of rows [0, rows) of band `i` (band-local order) from a host frame.
    void CopyBandRows(std::size_t i, const unsigned char* host, std::size_t row_bytes, unsigned char* dst,
                      hipMemcpyKind kind, bool to_host, hipStream_t stream) const;

    std::vector<std::unique_ptr<Slot>> m_slots;
    std::vector<void*> m_comms;  // ncclComm_t per slot when gathering with RCCL (nonblocking, comm.h)
    bool m_comms_aborted = false;  // a failed gather aborted them: later renders fail
    int m_id_planes = -1;          // gathered ids: packed with this many bit planes (render.h PackedIds), -1 int32
    GatherMode m_gather_mode = GatherMode::kDirect;
    bool m_interleaved = true;
    std::size_t m_band_rows = 0;  // rows of every band buffer
    int m_variant = 0;
    std::size_t m_width = 0;
    std::size_t m_height = 0;
    std::unique_ptr<Buffers> m_buf;
    bool m_in_half = false;
    bool m_out_half = false;
};

}  // namespace srt
