// Host-side interface of the HIP render kernels (render.hip).
//
// Pipeline for one frame (or one row band of it), all on one HIP stream:
//   1. prepare: triangle list + frame -> per-triangle edge-function records (48 B each)
//   2. trace:   per pixel: primary ray from the sample offsets -> brute-force closest hit
//               over every triangle (LDS-tiled) -> shade -> RGBA float4 store
// The canonical arithmetic both kernels implement is specified in DESIGN.md "Canonical math"
// and restated independently by oracle/srt_oracle.c.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "scene.h"

namespace srt {

// Triangles per edge tile. The edge buffer is padded with disabled (all-NaN) records to a
// multiple of kPadTriangles (the largest cull step: 256 threads x 16 records) so no trace
// loop has a tail; the per-ray variants stop after the last tile holding a real record.
constexpr int kTileTriangles = 256;
constexpr int kPadTriangles = 4096;
// Floats per position of the scene's spatial-order record inputs (DeviceScene svertices): the 9
// vertex coordinates, the record id's bits, two zero words -- 48 B, three 16-B loads.
constexpr int kSpatialStride = 12;

// Edge records, tile-planar: tile t (256 records, 10 KiB) = four planes, each indexed by the
// record's position j in the tile, so a lane-per-record load is one coalesced 16-B or 4-B
// access per plane and an LDS copy of the tile is a straight 10 KiB memcpy.
//   plane 0: float4[256] (c0A, cxA, cyA, c0B)
//   plane 1: float4[256] (cxB, cyB, c0C, cxC)
//   plane 2: float [256] cyC
//   plane 3: float [256] vol
// E_k(fx, fy) = fma(fy, cy_k, fma(fx, cx_k, c0_k)) for the three edges k = A, B, C.
constexpr int kTileFloat4 = kTileTriangles * 5 / 2;  // 640 float4 = 10 KiB per tile

// Screen boxes (render.hip ScreenBox): one float4 (xlo, xhi, ylo, yhi) per record, in record
// order, right after the tiles. They bound only rays with |fx|, |fy| <= kScreenBoxRange.
constexpr float kScreenBoxRange = 4.0f;

// Quantized screen boxes (the cull kernel's streamed copy): one uint2 per record, in record
// order, after the float boxes: x = hi | (-lo) << 16, y likewise, as int16 fixed point
// q = v * kQuantScale, lo rounded down and hi up, clamped to [-32767, 32767].
constexpr float kQuantScale = 4096.0f;

// Cull records (trace_device.h CullRecord): 64 B per record, at the record's rank in the scene's
// spatial order, after the quantized boxes.
// Floats per record in the edge allocation: 10 (tiles) + 4 (screen box) + 2 (quantized box)
// + 16 (cull record). (Shading computes a hit triangle's normal from its vertices: no per-frame
// normal buffer -- round 2 scattered one, 16 B by triangle id, in every band's record pass.)
constexpr int kEdgeFloatsPerTriangle = 32;

inline std::uint64_t PaddedTriangleCount(std::uint64_t n) {
    const std::uint64_t p = (n + kPadTriangles - 1) / kPadTriangles * kPadTriangles;
    return p == 0 ? kPadTriangles : p;
}

// Trace kernel variants (DESIGN.md "Kernels"); selectable for A/B measurement.
enum TraceVariant : int {
    kTraceLds = 0,     // LDS-tiled triangle stream, every ray tests every record
    kTraceScalar = 1,  // wave-uniform scalar-cache triangle stream, no LDS, 1 wave per block
    kTraceCull = 2,    // hierarchical: block-box cull of every record, compacted survivors in LDS
    kTraceBvh = 3,     // screen-space 8-wide BVH over the records in spatial order, wave-packet traversal
};

struct BandArgs {
    const float* offsets;  // device, row_count x width x 2 (band-local rows)
    float* rgba;           // device, row_count x width x 4
    std::size_t width;
    std::size_t height;     // full frame height (fy denominator)
    std::size_t row_begin;  // first frame row of the band
    std::size_t row_count;
    int* ids = nullptr;     // device, row_count x width: non-null = store hit ids (-1 miss), not RGBA
    // The band's row pattern. 1: frame rows [row_begin, row_begin + row_count). P > 1: the band deals
    // the frame's tile rows (kCullTileRows each) round-robin over P bands: frame tile rows
    // row_begin / kCullTileRows + k P, k = 0, 1, ..., concatenated (row_begin a multiple of
    // kCullTileRows; only the band's last tile row may be partial, and then it is the frame's last).
    // RowPattern(P, g): g consecutive tile rows out of every P (the compositor's share, engine.h).
    std::size_t row_interleave = 1;
    // ids holds packed hit ids (PackedIds) with this many bit planes above the 16-bit low plane;
    // -1: int32 ids (-1 = miss). The multi-GPU exchange payload (cull variant).
    int id_planes = -1;
    // RGBA output only: rgba is the whole frame (height x width x 4) and band row y is stored at its
    // frame row (BandFrameRow) -- the compositor's own band traced straight into its frame.
    bool rgba_frame_rows = false;
};

// Packed hit ids (the multi-GPU exchange payload; cull variant): a pixel's code -- its triangle id, or
// all ones for a miss -- in 16 + k bits, k = the bits the triangle count needs beyond 16 (C3's 100 000
// triangles: 1, 2.125 B per pixel against int32's 4; under 65 535 triangles: 0; C5's 1M: 4). Row-major
// rows, each: the row's u16 low 16 bits (padded to 8 B), then per plane j one 64-bit word per 64
// columns (bit x % 64 of word x / 64 is bit 16 + j of pixel x's code). Rows come in tile rows of
// kCullTileRows, each followed by its tiles' sample offset: one float2 per 64-column tile, the
// offset every ray of the tile has (the tile is "regular"), or NaNs (0.4 % more bytes at 1080p), so
// the shading of a regular tile reads no per-pixel offsets. A band frame is its tile rows (padded to
// 256 B), so a band's actual rows and its buffer's rows index it alike. Written by the trace (one
// ballot per plane and row segment; the tile's offset by its first block), read by the deferred
// shading: no decode work.
constexpr int kMaxIdPlanes = 8;
int IdPlanes(std::uint64_t triangles);  // k; -1 when the ids need more than 16 + kMaxIdPlanes bits
struct PackedIds {
    int planes = 0;
    std::size_t rows = 0, width = 0;
    std::size_t words = 0;          // 64-bit words per row and plane
    std::size_t low_row_bytes = 0;  // a row's u16 values, padded to 8 B
    std::size_t row_bytes = 0;      // a row
    std::size_t tile_row_bytes = 0; // kCullTileRows rows, then words float2 tile offsets
    std::size_t bytes = 0;          // one band frame
};
PackedIds PackedIdLayout(int planes, std::size_t rows, std::size_t width);

// A band row pattern (BandArgs::row_interleave) taking `group` consecutive tile rows out of every
// `interleave`, group a power of two (the kernels split a band's tile row index with a shift and a
// mask, no division): interleave in the low 16 bits, log2(group) above (group 1: the plain interleave).
constexpr std::size_t RowPattern(std::size_t interleave, std::size_t group) {
    std::size_t log2 = 0;
    while ((std::size_t{2} << log2) <= group) {
        ++log2;
    }
    return interleave | log2 << 16;
}
// Frame row of band-local row `local` (BandArgs::row_interleave: an interleave or a RowPattern).
inline std::size_t BandFrameRow(std::size_t row_begin, std::size_t pattern, std::size_t local);
// Rows of the band of pattern `pattern` starting at frame row `row_begin` of a `height`-row frame.
std::size_t PatternBandRows(std::size_t height, std::size_t row_begin, std::size_t pattern);
// Whether a binned cull frame computes its tile info inside the bin launch (one launch fewer, the
// tile info and the bins concurrent): full frames (the band is the whole frame), unless env
// SRT_FUSED_INFO=0. Its bins then use the analytic tile bounds (valid for offsets in [0, 1]) and
// write every cull record; a frame with an offset outside [0, 1] streams every record in every
// tile (the work order sees the range tag), which is exact.
bool CullFusedInfo(std::size_t row_begin, std::size_t row_count, std::size_t height, std::size_t interleave);
// Whether a band fits a frame of `height` rows (row_count may be 0).
bool BandFits(std::size_t row_begin, std::size_t row_count, std::size_t interleave, std::size_t height);
// Rows of band `band` of `bands` interleaved bands of a `height`-row frame.
std::size_t InterleavedBandRows(std::size_t height, std::size_t bands, std::size_t band);

// Launch the prepare kernel: writes PaddedTriangleCount(n) / kTileTriangles tiles into `edges`,
// then the screen boxes, quantized boxes and cull records (d_rank: id -> spatial-order rank).
hipError_t LaunchPrepare(const float* d_vertices, const unsigned* d_rank, std::uint64_t n, const Frame& frame,
                         float* d_edges, hipStream_t stream, hipEvent_t ev_begin = nullptr,
                         hipEvent_t ev_end = nullptr);

// Cull tiles: 64 columns x 16 rows of rays, one trace block each (render.hip "Cull bins"; 32-row
// tiles of two 16-row trace blocks measured 3 % slower at C3: each block filtered the candidates of
// both halves).
constexpr int kCullTileCols = 64;
#ifndef SRT_TILE_ROWS
#define SRT_TILE_ROWS 16
#endif
constexpr int kCullTileRows = SRT_TILE_ROWS;

inline std::size_t BandFrameRow(std::size_t row_begin, std::size_t pattern, std::size_t local) {
    const std::size_t interleave = pattern & 0xFFFFu, log2 = pattern >> 16;
    const std::size_t lt = local / kCullTileRows;
    return row_begin + ((lt >> log2) * interleave + (lt & ((std::size_t{1} << log2) - 1))) * kCullTileRows +
           local % kCullTileRows;
}
constexpr int kMaxBatch = 8;          // frames of a batched cull launch with its parameters as kernel arguments
constexpr int kMaxBoundTiles = 2048;  // binning needs tiles_x + tiles_y <= this
constexpr int kMaxBinTiles = 8192;    // and tiles_x * tiles_y <= this (bin kernel LDS histogram)

// Work buffers of the cull variant's bins for one band shape (one allocation, carved by
// CullBinLayout; its first CullBinCounterBytes -- the counters, which reset themselves -- must be
// zero-filled when it is carved up for a shape; every other byte is written before it is read).
struct CullBins {
    const unsigned* order; // the scene's record ids in spatial order (DeviceScene; not in the buffer)
    const float* svertices;  // the scene's vertices in that order (DeviceScene; not in the buffer)
    // Per 256-position block of the spatial order: (lowest ylo, highest yhi) of its records' screen
    // boxes under the prepared frame (LaunchBlockExtents; DeviceScene). A band's record pass skips a
    // block whose extent meets none of its rows (a skip hint, exact: render.hip BandMayReach); null: none.
    const float2* block_ext = nullptr;
    void* tile_info;       // tiles x 32 B: ray box, uniform offset (TileInfoKernel)
    unsigned* counts;      // tiles + 1: list lengths, then the large-list length (this frame's buffer)
    unsigned* counts_next; // the slot's other count buffer (its next frame's): zeroed by this frame's trace
    unsigned* lists;       // tiles x capacity candidate ids (BinTrianglesKernel)
    unsigned* large_list;  // PaddedTriangleCount(n) ids binned to every tile
    void* work;            // trace work plan (WorkOrderKernel): descs descriptors, 32 B each
    unsigned* work_count;  // its length
    unsigned* arrive;      // per split slot: split chunks finished (self-resetting counters)
    void* split_keys;      // key slices of split parts: one per split slot (<= descs), 8 KiB each
    unsigned descs;        // trace grid = work descriptors per frame (<= CullDescriptors(tiles, 1))
    unsigned* range_tag;   // = gen when some sample offset of the frame lies outside [0, 1] (tile blocks)
    unsigned gen;          // the scene's frame number (never 0): tags are compared with it, not reset
    unsigned capacity;
    std::size_t tiles;
    bool plan = true;      // (re)build the slot's work plan with this frame (else the trace uses the last one)
    // Records recomputed by the trace (trace_device.h TraceRecords<true>): the bin launch writes a 16-B
    // screen box per position instead of the 64-B cull record, the trace rebuilds the record from the
    // scene's 48-B spatial inputs. Same frame bit for bit; trades bin-launch bytes for trace VALU, so
    // it pays where the bin launch is on the critical path (one frame queue, one-frame launches).
    // One value for every frame of a launch.
    bool recompute = false;
};
// Which records a DeviceScene's binned traces read (DeviceScene::SetRecordMode; env SRT_TRACE_RECORDS
// = stored | recompute | auto overrides): auto = recomputed for one-frame launches, stored otherwise.
enum RecordMode : int { kRecordsAuto = 0, kRecordsStored = 1, kRecordsRecompute = 2 };

// Tiles (64 x 32 rays) of a width x row_count band.
std::size_t CullTiles(std::size_t width, std::size_t row_count);

// Whether a band shape can be binned (its tile grid fits the bin kernel's LDS).
bool CullBinnable(std::size_t width, std::size_t row_count);

// Per-tile list capacity for n triangles (a list that overflows makes its tile stream every
// record; results are unaffected). Env SRT_CULL_BIN_CAP overrides it (tests).
unsigned CullBinCapacity(std::uint64_t n, std::size_t tiles);

// Trace grid of a band shape in a launch of `frames` frames: work descriptors per frame. A tile
// part's candidates may be cut into up to kMaxChunks chunks (blocks); WorkOrderKernel picks the
// chunk size so that a frame's descriptors fit. Room = max(parts x M, parts + E / frames): M =
// ceil(resident trace blocks / the launch's parts) (small bands: > 1), E = env SRT_CULL_SPLIT
// (default: the resident trace blocks) for cutting the heavy parts. Env SRT_CULL_CHUNKS = m
// forces parts x m (tests, measurement).
constexpr int kMaxChunks = 16;
unsigned CullDescriptors(std::size_t tiles, std::size_t frames);

// Bytes of the bin work buffer for n triangles and a band shape, and its carve-up.
std::size_t CullBinBytes(std::uint64_t n, std::size_t width, std::size_t row_count);
std::size_t CullBinCounterBytes(std::uint64_t n, std::size_t width, std::size_t row_count);  // the leading counters
// parity: which of the slot's two count buffers this frame bins into (alternate per frame of a slot).
CullBins CullBinLayout(void* base, std::uint64_t n, std::size_t width, std::size_t row_count, unsigned parity = 0);

// Optional stage timing events (null = not recorded). They are bound to the kernels' own
// dispatch packets (hipExtLaunchKernelGGL start / stop events), so timing adds no marker
// packets to the stream: `prep_*` = the prepare kernel (fused with the tile-info blocks in
// the binned cull variant: PrepareInfoKernel; TileInfoKernel alone when no prepare is
// pending), `bin_*` = BinTrianglesKernel (its last block also orders the tiles),
// `begin` / `end` = the trace kernel.
struct StageEvents {
    hipEvent_t prep_begin = nullptr;
    hipEvent_t prep_end = nullptr;
    hipEvent_t bin_begin = nullptr;
    hipEvent_t bin_end = nullptr;
    hipEvent_t begin = nullptr;
    hipEvent_t end = nullptr;
};

// Launch the trace kernel over one band (cull variant: bin + trace; bins == nullptr streams
// every record for every tile). prepare_rank != null: first (re)compute the edge records for
// `frame` (LaunchPrepare's work; fused with the tile-info blocks when binning).
hipError_t LaunchTrace(const float* d_edges, std::uint64_t n, const float* d_vertices, const float* d_shade,
                       const Frame& frame, const float background[3], const BandArgs& band, int variant,
                       const CullBins* bins, hipStream_t stream, const StageEvents* events = nullptr,
                       const unsigned* prepare_rank = nullptr, void* bvh = nullptr);

// Screen-space BVH (render.hip "BVH variant"): an implicit 8-wide tree over the cull records
// in spatial order. Level 0 node i = records [8i, 8i+8); level L node i = level L-1 nodes
// [8i, 8i+8); the top level has one node. Per node: screen box (float4) + depth lower bound.
constexpr int kBvhWidth = 8;
constexpr int kBvhMaxLevels = 16;
struct BvhLayout {
    unsigned levels = 0;                  // levels (the last one holds the root)
    unsigned count[kBvhMaxLevels] = {};   // nodes per level
    unsigned offset[kBvhMaxLevels] = {};  // first node of each level in the node arrays
    unsigned nodes = 0;                   // total
};
BvhLayout MakeBvhLayout(std::uint64_t n);
std::size_t BvhBytes(std::uint64_t n);  // node boxes (16 B) + depth bounds (4 B), 256-B aligned

// One frame of a batched cull launch: its edge-record slot, its bins (one band shape for the
// whole batch) and its band buffers.
struct CullFrame {
    const float* edges;
    const CullBins* bins;
    BandArgs band;
    // LaunchSharedCullFrames only: the frame's tile facts stand here already (tiles x 16 B, written by
    // LaunchTileFacts for this offsets buffer and W x H: a pinned buffer, DeviceScene::PinOffsets), so
    // the facts launch leaves the frame out and its trace reads these. Read-only: any number of
    // launches may read one such buffer at once. Null: the launch computes the frame's facts.
    const void* facts = nullptr;
};
// Frames of one launch whose parameters travel in a device table instead of the kernel
// arguments (count > kMaxBatch): `device` and `host` (page-locked) of CullTableBytes(frames) bytes
// each, caller-owned. LaunchCullFrames fills `host` and uploads it to `device` on the stream; the
// caller must not rewrite `host` before that upload has executed (`uploaded`), and the stream order
// keeps the device copy alive for the launches that read it.
constexpr int kMaxTableFrames = 256;
struct CullTable {
    void* device;
    void* host;
    std::size_t frames;  // capacity
    // `host` as the device sees it (page-locked, mapped): the upload is then a small kernel reading it
    // over the bus instead of hipMemcpyAsync, which on ROCm 7.2 blocked the calling thread for 7 ms
    // at the first upload from some staging buffers (measured: tools/first_run_probe.py). Null: copy.
    const void* host_device = nullptr;
    // Recorded on the stream once the upload has read `host` (null: not recorded): the caller may
    // rewrite `host` after it, while the frames' launches still run.
    hipEvent_t uploaded = nullptr;
};
std::size_t CullTableBytes(std::size_t frames);

// The cull pipeline for `count` frames of one camera in four launches (tile info; record setup +
// bins; work lists; trace), block z of each working on frame z: the same per-frame work as
// `count` single-frame calls, with four launches per call. Up to kMaxBatch frames carry their
// parameters as kernel arguments; up to kMaxTableFrames through `table` (required then). The
// records are computed in the bin launch every call (bins->order: position -> id; d_rank unused).
// Events (optional): prep = tile info, bin = record setup + bins + work list, trace.
hipError_t LaunchCullFrames(const CullFrame* frames, std::size_t count, std::uint64_t n, const float* d_vertices,
                            const float* d_shade, const Frame& frame, const float background[3], const unsigned* d_rank,
                            hipStream_t stream, const StageEvents* events, const CullTable* table = nullptr);

// The shared cull setup of a prepared frame (DeviceScene: one copy, built once per Prepare). For a
// whole-frame binned trace (CullFusedInfo) the record pass, the bins and the work plan are a function
// of the scene, the camera and W x H only: the bin kernel tests every record against the analytic
// tile boxes, which do not depend on the sample offsets. So they are built once (LaunchCullSetup:
// the per-frame path's own PrepareBinKernel and WorkOrderKernel, run on this copy) and every later
// frame runs two launches (LaunchSharedCullFrames): the tile facts of its offsets, and the trace,
// which reads the setup and never writes it. One allocation of CullSetupBytes, carved by
// CullSetupLayout; a build zero-fills its first zero_bytes itself.
struct CullSetup {
    void* screen_boxes;    // per position: screen box (read by traces that recompute their records)
    void* qboxes;          // per position: quantized screen box (the FULL stream)
    void* cull;            // per position: 64-B cull record
    void* tile_info;       // tiles x 32 B: the analytic tile boxes (the work order's input)
    unsigned* counts;      // tiles + 1: list lengths, then the large-list length
    unsigned* range_tag;   // stays zero (no frame of the build is tagged)
    unsigned* lists;       // tiles x capacity candidate positions
    unsigned* large_list;  // positions binned to every tile
    void* work;            // the plan: descs descriptors, heaviest first, facts baked in
    void* work_tmp;        // descs descriptors of scratch (LaunchStreamPlan's partition)
    unsigned* work_count;
    // [0]: records of the record stream (LaunchStreamPlan), pad records included; [1]: the plan's
    // descriptors that are not statically empty (low word) and those that are (high word); [2]:
    // non-zero when some descriptor is statically empty and FULL at once (full_empty_descs below)
    unsigned long long* stream_count;
    // The record stream (below): an allocation of its own, sized from stream_count after the plan;
    // null: the traces read the records through the lists (the indexed path).
    const void* stream;
    std::size_t zero_bytes;
    std::size_t tiles;
    unsigned capacity;
    unsigned descs;        // the trace grid the plan was made for
    unsigned min_chunk;    // smallest candidate chunk of a split part (env SRT_CULL_CHUNK at the carve-up)
    bool recompute;        // CullBins::recompute of the traces it serves
    // The empty sweep (below). sweep: LaunchStreamPlan lists the statically empty descriptors last and
    // the traces sweep them in groups; list_descs, empty_descs: the built plan's counts (the caller
    // reads stream_count[1] once per build); empty_group: descriptors per sweep block, 1 to
    // kMaxEmptyGroup (read per launch: not part of what is built).
    bool sweep;
    unsigned list_descs, empty_descs, empty_group;
    // Per tile, non-zero exactly when the plan's descriptors of the tile are statically empty
    // (kItemEmpty without kItemFull: what a sweep block fills by). Written by LaunchStreamPlan with
    // every build of the plan. facts_fill (read per launch, like empty_group; ignored without sweep):
    // the tile-facts launch of a frame stores the misses of the tiles that are empty by this map and
    // valid in the frame, and the sweep blocks store none: they only trace the invalid ones.
    unsigned* empty_map;
    bool facts_fill;
    // Which of the two facts kernels a launch runs (read per launch; render.hip LaunchSharedStages):
    // the lean one-wave-per-tile kernel, or the block kernel. facts_fill implies the lean one.
    bool lean_facts;
    // A regular launch (read per launch; render.hip TraceCullKernel<RegularFrames<..>, ..>): the trace runs the kernel
    // without the per-pixel position table, at seven blocks per CU. The caller vouches that every
    // tile of every frame is regular, usable and in range -- every frame brings its facts
    // (CullFrame::facts) and their summary says so (LaunchFactsSummary) --, for a tile that is not
    // would be traced wrongly; a launch with a facts stage is refused. full_empty_descs (the built
    // plan's, stream_count[2]): non-zero when a sweep block could have a descriptor to trace whatever
    // the facts say, which that kernel does not do: such a setup's regular launch is refused too.
    bool regular_trace = false;
    unsigned full_empty_descs = 0;
};
// The empty sweep: with setup.sweep the trace grid is the list descriptors, one block each, and one
// sweep block per empty_group statically empty descriptors (render.hip TraceCullKernel), instead of
// one block per descriptor of the plan's room.
constexpr unsigned kDefaultEmptyGroup = 16;
constexpr unsigned kMaxEmptyGroup = 64;  // one lane of a wave per descriptor of the group
unsigned SharedTraceBlocks(unsigned descs, unsigned list_descs, unsigned empty_descs, unsigned group);
// The record stream of a built setup: the 64-B cull records of every (tile, chunk) of the plan, in
// the order its trace blocks walk them (chunk [begin, end) of the tile's bin list, then the large
// list), each range starting at a multiple of 128 B (an even record index). The parts of a tile walk
// the same lists, so they share the tile's ranges. A statically FULL or empty descriptor has no
// range. LaunchStreamPlan (after LaunchCullSetup, same stream; run for every build, stream or not)
// first puts the plan into the empty sweep's order (setup.sweep) and counts its list and empty
// descriptors into setup.stream_count[1]; then it writes every descriptor's first record
// index and record count into its w1.x and w1.y -- unused on the shared path otherwise --, zeroes
// the second half of the end marks, and writes the stream's length into setup.stream_count; the
// caller reads that once, allocates, and LaunchStreamPack fills `stream`.
// A trace launched with setup.stream != null reads its candidates from there (stored records only).
constexpr std::size_t kCullRecordBytes = 64;
constexpr std::size_t kStreamCapRecords = std::size_t{1} << 22;  // 256 MiB (the sizes measured)
hipError_t LaunchStreamPlan(const CullSetup& setup, hipStream_t stream);
hipError_t LaunchStreamPack(const CullSetup& setup, void* records, hipStream_t stream);
std::size_t CullSetupBytes(std::uint64_t n, std::size_t width, std::size_t height, unsigned descs);
CullSetup CullSetupLayout(void* base, std::uint64_t n, std::size_t width, std::size_t height, unsigned descs,
                          bool recompute);
// Builds the setup on `stream`: zero fill, analytic tile info, records + bins, work plan.
hipError_t LaunchCullSetup(const CullSetup& setup, std::uint64_t n, const Frame& frame, std::size_t width,
                           std::size_t height, const unsigned* d_order, const float* d_svertices, hipStream_t stream);
// `count` whole frames on the setup. frames[f].bins: the frame slot's own state -- tile_info (the
// frame's 16-B tile facts are written there), arrive, split_keys, and descs == setup.descs; edges
// unused. Events: bin = the tile-facts launch, begin / end = the trace.
// Frames with CullFrame::facts set come last in `frames`: the facts launch runs over the frames in
// front of them only (the kernels take a frame's parameters by blockIdx.z: a smaller grid z), and
// not at all when every frame has its facts. Such frames are refused with setup.facts_fill on the
// sweep, whose facts launch stores pixels of every frame.
hipError_t LaunchSharedCullFrames(const CullFrame* frames, std::size_t count, const CullSetup& setup, std::uint64_t n,
                                  const float* d_vertices, const float* d_shade, const Frame& frame,
                                  const float background[3], hipStream_t stream, const StageEvents* events,
                                  const CullTable* table = nullptr);
// The facts launch of LaunchSharedCullFrames alone, for one whole frame (band: offsets, width,
// height = row_count; the outputs unused) into d_facts (CullTiles(width, height) x 16 B): the same
// kernels on the same parameters, so the same bits. lean: which of the two (CullSetup::lean_facts).
// A function of the offsets' contents and W x H only: no scene, camera or setup is read.
hipError_t LaunchTileFacts(const BandArgs& band, void* d_facts, bool lean, hipStream_t stream);
// The summary of such a facts buffer, after its facts launch on the same stream: one small block ANDs
// regular, usable and in-range over the `tiles` tiles and stores one word, kFactsSummaryDone with
// kFactsSummaryRegular when every tile has all three. d_word: the device's address of a word the
// host can read (page-locked, mapped), valid once the work queued behind this launch has completed.
constexpr unsigned kFactsSummaryDone = 0x80000000u;
constexpr unsigned kFactsSummaryRegular = 1u;
hipError_t LaunchFactsSummary(const void* d_facts, std::size_t tiles, unsigned* d_word, hipStream_t stream);

// Point queries (query.hip QueryKernel): the closest hit at `count` arbitrary image positions
// (fx, fy) of the frame -- the quantity ray generation produces, nothing about pixels: ids[i] = the
// hit record's id or -1, t[i] = its t = vol / det or +inf, the lexicographic (t, id) minimum, bit
// for bit what the traces compute for a ray at that position. how[i] (null: not stored): 0 = answered
// from the list of the tile whose analytic box contains the position plus the large list, 1 = every
// record streamed (position outside [0, 1]^2 or NaN, overflowed list, unusable tile box, no setup).
struct QueryArgs {
    const float* positions;  // device, count x 2
    std::size_t count;
    int* ids;                // device, count
    float* t;                // device, count
    unsigned char* how;      // device, count, or null
};
// `setup`: the built shared setup of the width x height frame (read-only here), or null: none, every
// query streams the records recomputed from d_svertices. d_edges: the scene's edge allocation
// (kEdgeFloatsPerTriangle per padded record; not written). One launch; count == 0: none.
hipError_t LaunchQuery(const CullSetup* setup, std::uint64_t n, const Frame& frame, std::size_t width,
                       std::size_t height, const float* d_svertices, const float* d_edges, const QueryArgs& args,
                       hipStream_t stream);

// Depth layers (query.hip LayersKernel; DESIGN.md section 2 "Layers"): at every position the
// `layers` (1 .. kMaxLayers) lexicographically smallest (t, id) keys among the records passing the
// exact test, front to back: ids[k * E + i] = layer k's id at element i of E, or -1, t[...] = its t
// or +inf (t null: not stored). Layer 0 is LaunchQuery's answer. how[i] as QueryArgs::how.
constexpr int kMaxLayers = 8;
struct LayersArgs {
    // points: `where` = count x 2 positions, E = count (row_begin, row_count unused). Else `where` =
    // the band's sample offsets, row_count x width x 2, element (x, y) is pixel (x, row_begin + y) of
    // the frame at ray generation's position, E = row_count x width (band-local, as LaunchShade's).
    bool points;
    const float* where;  // device
    std::size_t count;
    std::size_t row_begin;
    std::size_t row_count;
    std::size_t layers;
    int* ids;            // device, layers x E
    float* t;            // device, layers x E, or null
    unsigned char* how;  // device, E, or null
};
// `setup`, d_svertices, d_edges: as LaunchQuery's. One launch; no elements: none.
hipError_t LaunchLayers(const CullSetup* setup, std::uint64_t n, const Frame& frame, std::size_t width,
                        std::size_t height, const float* d_svertices, const float* d_edges, const LayersArgs& args,
                        hipStream_t stream);

// Composite (query.hip CompositeKernel; layers_math.h; DESIGN.md section 2 "Composite"): one RGBA
// pixel from `layers` id planes of a band -- each layer shaded as LaunchShade shades it and
// composited front to back under the per-triangle opacity table; alpha = 1 - the transmittance
// left. Reads the shading table and the opacity table only. The composite of a pixel stops at its
// first id outside [0, n); nothing is read through such an id.
struct CompositeArgs {
    // Band-local, as LaunchShade's: pixel (x, row_begin + y) of the width x height frame.
    const float* offsets;  // device, row_count x width x 2
    const int* ids;        // device, layers x row_count x width, layer-major (LaunchLayers' ids)
    std::size_t layers;
    const float* opacity;  // device, n
    std::size_t width;
    std::size_t height;
    std::size_t row_begin;
    std::size_t row_count;
    float* rgba;  // device, row_count x width x 4
};
// One launch; no rows: none.
hipError_t LaunchComposite(const float* d_shade, std::uint64_t n, const Frame& frame, const float background[3],
                           const CompositeArgs& args, hipStream_t stream);

// Spot-light shadow mask (render.hip ShadowKernel; shadow_math.h; DESIGN.md section 2 "Shadow"): the
// class of every pixel of a band of the view frame -- 0 shadowed, 1 lit, 2 outside the light's
// frustum, 3 no surface -- from its hit id, the light being a second prepared frame of a scene with
// the same triangles: the canonical closest hit of the light frame at the position the pixel's
// surface point projects to, compared with the pixel's own triangle and depth. Exact: bit for bit
// the composition of the G-buffer's depth, shadow_math.h's projection and a point query.
struct ShadowLight {
    const CullSetup* setup;  // the light frame's built shared setup (read-only here), or null: pixels stream
    Frame frame;             // the light's prepared frame, width x height
    std::size_t width;
    std::size_t height;
    const float* svertices;  // the light scene's, as LaunchQuery's
    const float* edges;
    const unsigned* rank;    // the light scene's record id -> spatial-order position
};
struct ShadowArgs {
    // Band-local, as LaunchShade's: pixel (x, row_begin + y) of the width x height view frame.
    const float* offsets;  // device, row_count x width x 2
    const int* ids;        // device, row_count x width
    std::size_t width;
    std::size_t height;
    std::size_t row_begin;
    std::size_t row_count;
    float bias;            // relative depth bias, finite, >= 0
    unsigned char* mask;   // device, row_count x width classes
    float* rgba;           // device, row_count x width x 4, or null: the shaded pixel, rgb times
    float dim;             //   1 (class 1) or dim (classes 0, 2); class 3: the background pixel
};
// d_vertices, d_shade, n, frame, background: the view scene's (n: of both scenes). One launch; no
// rows: none.
hipError_t LaunchShadow(const float* d_vertices, const float* d_shade, std::uint64_t n, const Frame& frame,
                        const float background[3], const ShadowLight& light, const ShadowArgs& args,
                        hipStream_t stream);

// Omni-light shadow mask (render.hip OmniShadowKernel; omni_math.h; DESIGN.md section 2 "Omni
// shadow"): LaunchShadow's class byte under a point light given as six cube-face frames of one
// size, each a ShadowLight. Every pixel selects its face from q = surface point - light (OmniFace)
// and runs LaunchShadow's test in that face's frame only: bit for bit LaunchShadow's class for the
// selected face. args: LaunchShadow's; d_face (device, row_count x width bytes, or null): the
// selected face, kOmniNoFace for a class-3 pixel. The six faces share one origin, one frame size and
// one record source (all with a setup of the same kind, or all without). One launch; no rows: none.
hipError_t LaunchOmniShadow(const float* d_vertices, const float* d_shade, std::uint64_t n, const Frame& frame,
                            const float background[3], const ShadowLight faces[6], const ShadowArgs& args,
                            unsigned char* d_face, hipStream_t stream);

// Direct lighting (render.hip LightingKernel; lighting_math.h; DESIGN.md section 2 "Lighting"): the
// lit RGBA of every pixel of a band of the view frame from its hit id under `count` (0 to
// kLightingMaxLights) lights -- albedo . (ambient + the sum over the lights that reach the pixel from
// the eye's side of its triangle of color . cosine . falloff / distance^2), alpha = float(id); an id
// outside [0, n): the background, alpha -1. A spot light is one ShadowLight frame, a point light six
// (LaunchOmniShadow's faces); at most kLightingMaxFrames in a call, all of one record source. The
// class a light gives a pixel is LaunchShadow's / LaunchOmniShadow's byte at that light's bias.
struct LightingLight {
    const ShadowLight* frames;  // 1 (spot) or 6 (point: one origin, one size)
    bool point;
    float color[3];
    float falloff;  // finite, >= 0; 0: no distance term
    float bias;     // finite, >= 0
};
struct LightingArgs {
    // Band-local, as LaunchShade's: pixel (x, row_begin + y) of the width x height view frame.
    const float* offsets;  // device, row_count x width x 2
    const int* ids;        // device, row_count x width
    std::size_t width;
    std::size_t height;
    std::size_t row_begin;
    std::size_t row_count;
    float ambient[3];
    float* rgba;             // device, row_count x width x 4
    unsigned char* classes;  // device, count x row_count x width (light-major), or null
};
// d_vertices, d_shade, n, frame, background: the view scene's (n: of every scene). One launch
// whatever `count`; no rows: none. Without class planes a light on the far side of a pixel's
// triangle is not scanned for it (it adds nothing): the RGBA is the same either way.
hipError_t LaunchLighting(const float* d_vertices, const float* d_shade, std::uint64_t n, const Frame& frame,
                          const float background[3], const LightingLight* lights, std::size_t count,
                          const LightingArgs& args, hipStream_t stream);

// Lit ray hits (render.hip LightHitsKernel; hits_math.h; DESIGN.md section 2 "Hits"): LaunchLighting
// for elements given as (ray, id, t) -- the surface point is o + t d of the element's own ray, no
// view frame is read -- with an optional blend onto a base picture. An element whose direction is
// zero is absent ((0, 0, 0, -1), or the base element unchanged); one whose id lies outside [0, n) or
// whose t, o or d is not finite is a miss (the background, alpha -1) and reads nothing through its
// id. For the eye rays of a frame with the G-buffer's depth the answer is LaunchLighting's, bit for
// bit.
struct LightHitsArgs {
    const float* rays;  // device, elements x 8 (ray_math.h Ray), 16-byte aligned; the range is not read
    const int* ids;     // device, elements
    const float* t;     // device, elements
    std::size_t elements;  // at most 2^31 - 1
    float ambient[3];
    const float* base;  // device, elements x 4, 16-byte aligned, or null: the element is stored; may be rgba
    float weight[3];    // finite (read with a base only): base.rgb + weight . rgb, base's alpha
    float* rgba;        // device, elements x 4, 16-byte aligned
    unsigned char* classes;  // device, count x elements (light-major), or null
};
// d_shade, n, background: the shaded scene's (n: of every scene). One launch whatever `count`; no
// elements: none. With class planes a light that is not facing is still scanned, as LaunchLighting's.
hipError_t LaunchLightHits(const float* d_shade, std::uint64_t n, const float background[3], const LightingLight* lights,
                           std::size_t count, const LightHitsArgs& args, hipStream_t stream);

// Lit surfaces (render.hip LitSurfaceKernel; material_math.h; DESIGN.md section 2 "Lit surfaces"):
// LaunchLighting with the pixel's normal and albedo taken from LaunchSurface's tables instead of the
// shading table, and with a material a Blinn-Phong term: the textured, smooth-shaded, shadowed frame
// in one launch. Classes, and which lights contribute, are LaunchLighting's; with no table and no
// material so is the pixel, bit for bit.
struct LitSurface {
    // The surface as SurfaceArgs' (device; null: none).
    const float* normals;
    const float* uvs;
    const float* texture;
    std::size_t tex_width;
    std::size_t tex_height;
    unsigned flags;
    bool material;  // specular, shininess_log2 hold one
    float specular[3];
    int shininess_log2;  // 0 .. kMaterialMaxShininessLog2: the exponent is 2^shininess_log2
};
hipError_t LaunchLitSurface(const float* d_vertices, const float* d_shade, std::uint64_t n, const Frame& frame,
                            const float background[3], const LightingLight* lights, std::size_t count,
                            const LightingArgs& args, const LitSurface& surface, hipStream_t stream);

// G-buffer (outputs.hip GBufferKernel): the surface attributes of (image position, triangle id)
// pairs of the frame -- depth, barycentrics, normal + shading cosine, albedo + id (gbuffer_math.h;
// DESIGN.md section 2 "Surface attributes") -- from hit ids, a deferred pass like LaunchShade with
// more outputs. The record of an id is recomputed from the scene's vertices (ComputeEdges under
// `frame`, the traces' bits): no edge buffer, no cull setup is read. An id outside [0, n) gives the
// miss values and reads nothing through it.
struct GBufferArgs {
    // points: `where` = count x 2 positions (fx, fy), ids = count ids (count = width; height,
    // row_begin unused, row_count 1). Else `where` = the band's sample offsets, row_count x width x 2,
    // ids = row_count x width (band-local, as LaunchShade's): pixel (x, row_begin + y) of the
    // width x height frame, its position ray generation's expression.
    bool points;
    const float* where;  // device
    const int* ids;      // device
    std::size_t width;
    std::size_t height;
    std::size_t row_begin;
    std::size_t row_count;
    // The planes (device; null: not written), each row_count x width elements, count-major.
    float* depth;   // [1]
    float* bary;    // [2]: (w1, w2)
    float* normal;  // [4]: (unit normal towards the eye, cos)
    float* albedo;  // [4]: (r, g, b, float(id))
};
// One launch; no elements or no plane: none.
hipError_t LaunchGBuffer(const float* d_vertices, const float* d_shade, std::uint64_t n, const Frame& frame,
                         const float background[3], const GBufferArgs& args, hipStream_t stream);

// Vertex attributes (outputs.hip SurfaceKernel / InterpolateKernel): what the surface looks like at
// (image position, triangle id) pairs -- a smooth normal, a UV, a textured albedo and the shaded
// pixel (surface_math.h; DESIGN.md section 2 "Vertex attributes") -- from hit ids and the caller's
// per-triangle corner tables, a deferred pass like LaunchGBuffer. The weights come from the record
// recomputed from the scene's vertices: no edge buffer, no cull setup is read. An id outside
// [0, n) gives the miss values and reads nothing through it.
struct SurfaceArgs {
    // Elements as GBufferArgs'.
    bool points;
    const float* where;  // device
    const int* ids;      // device
    std::size_t width;
    std::size_t height;
    std::size_t row_begin;
    std::size_t row_count;
    // The surface (device; null: none): corner normals n x 9, corner uvs n x 6, texture th x tw x 4.
    const float* normals;
    const float* uvs;
    const float* texture;
    std::size_t tex_width;
    std::size_t tex_height;
    unsigned flags;  // surface_math.h kSurface*
    // The planes (device; null: not written), each row_count x width elements.
    float* normal;  // [4]: (unit normal towards the eye, cos)
    float* albedo;  // [4]: (r, g, b, float(id))
    float* rgba;    // [4]: (albedo.rgb * cos, float(id))
    float* uv;      // [2]
};
// One launch; no elements or no plane: none.
hipError_t LaunchSurface(const float* d_vertices, const float* d_shade, std::uint64_t n, const Frame& frame,
                         const float background[3], const SurfaceArgs& args, hipStream_t stream);

// The interpolation of one corner table (device, n x 3 x channels, 1 <= channels <= 4) at the
// elements (as SurfaceArgs'): out = row_count x width x channels floats.
struct InterpolateArgs {
    bool points;
    const float* where;
    const int* ids;
    std::size_t width;
    std::size_t height;
    std::size_t row_begin;
    std::size_t row_count;
    const float* table;
    std::size_t channels;
    float* out;
};
hipError_t LaunchInterpolate(const float* d_vertices, std::uint64_t n, const Frame& frame, const InterpolateArgs& args,
                             hipStream_t stream);

// Resolve (outputs.hip ResolveKernel): one RGBA pixel from `samples` (sample offset, hit id) planes
// of a band -- every sample shaded as LaunchShade shades it, summed in ascending order and divided
// by the count; alpha = the share of samples that hit (samples_math.h; DESIGN.md section 2
// "Resolve"). Reads the shading table only. An id outside [0, n) is a miss and reads nothing
// through it.
constexpr int kMaxSamples = 16;
struct ResolveArgs {
    // Host arrays of `samples` (1 .. kMaxSamples) device pointers, band-local as LaunchShade's:
    // offsets[s] = row_count x width x 2, ids[s] = row_count x width.
    const float* const* offsets;
    const int* const* ids;
    std::size_t samples;
    std::size_t width;
    std::size_t height;
    std::size_t row_begin;
    std::size_t row_count;
    float* rgba;  // device, row_count x width x 4
};
// One launch (the plane pointers travel in the kernel's arguments); no rows: none.
hipError_t LaunchResolve(const float* d_shade, std::uint64_t n, const Frame& frame, const float background[3],
                         const ResolveArgs& args, hipStream_t stream);

// Deferred shading of a band from hit ids (band.ids) and sample offsets into band.rgba (normals
// from the vertices, d_edges unused): bit-identical to the fused trace.
// frames > 1 shades a batch whose ids are band-major, ids[band][frame][band_rows][width] (a
// gather of `frames` frames of band_rows-row bands; band_rows 0 = one band of row_count rows),
// into band.rgba[frame][row_count][width].
// interleaved > 0: the ids' bands are that many interleaved bands (BandArgs::row_interleave).
// offsets_stride: floats between consecutive frames' sample offsets (0: every frame of the batch
// shares band.offsets; a multiple of 2).
// The scene's shading table (once, at load): per triangle two float4, (the shading normal
// cross(v1 - v0, v2 - v0), its length) and (albedo, 0); d_table holds 8 floats per triangle. The
// d_shade arguments of the launches below take it.
// Screen-box y extent of every 256-position block of the spatial order under `frame` (records computed
// as the bin kernel computes them; n_pad / 256 float2 into d_ext): the band record pass's skip hint,
// keyed to (scene, camera, W x H) like the spatial order itself.
// Block extents LaunchBlockExtents writes for n triangles (one per bin block of the record pass:
// render.hip kBinThreads records each): the size of its d_ext.
std::size_t BlockExtentCount(std::uint64_t n);
hipError_t LaunchBlockExtents(const float* d_svertices, std::uint64_t n, const Frame& frame, float2* d_ext,
                              hipStream_t stream);
hipError_t LaunchShadeTable(const float* d_vertices, const float* d_albedo, std::uint64_t n, float* d_table,
                            hipStream_t stream);

hipError_t LaunchShade(const float* d_vertices, const float* d_shade, const float* d_edges, std::uint64_t n,
                       const Frame& frame, const float background[3], const BandArgs& band, hipStream_t stream,
                       std::size_t frames = 1, std::size_t band_rows = 0, std::size_t interleaved = 0,
                       std::size_t offsets_stride = 0, long skip_band = -1, std::size_t own_bands = 0,
                       std::size_t first_rows = 0);
// (skip_band >= 0: the rows of that band are left as they are; own_bands > 0: so are the rows of
// bands [0, own_bands), and the ids start at band own_bands -- the compositor's share, engine.h.
// first_rows > 0, contiguous bands only: band 0 has first_rows rows, the later ones band_rows each --
// BandSplit::first_rows.)

// Spatial order of the records (spatial.hip): ids sorted by the Morton code of their centroid's
// image-plane position under the scene camera, on the device (keys + rocPRIM radix sort), and
// its inverse; synchronous on `stream`. Optional events bracket the build (timing).
void BuildSpatialOrder(const float* d_vertices, std::uint64_t n, const Camera& camera, unsigned* d_order,
                       unsigned* d_rank, float* d_svertices, hipStream_t stream, hipEvent_t ev_begin = nullptr,
                       hipEvent_t ev_end = nullptr);

// Motion (spatial.hip; include/srt_motion.h): the same order rebuilt in place after the camera or
// the vertices moved, enqueued on `stream` only -- no allocation, no host synchronisation. The sort
// scratch (keys, sorted keys, ids and the rocPRIM temporary: 3 x 4 n bytes + temp_bytes, a function
// of n alone) belongs to the scene: allocated by its first reordering update, freed with it.
struct OrderScratch {
    unsigned* keys = nullptr;
    unsigned* keys_sorted = nullptr;
    unsigned* ids = nullptr;
    void* temp = nullptr;
    std::size_t temp_bytes = 0;
};
void AllocOrderScratch(OrderScratch& scratch, std::uint64_t n, hipStream_t stream);  // throws; leaves none on failure
void FreeOrderScratch(OrderScratch& scratch) noexcept;
// One pass over the n triangles (MotionKeysKernel): d_shade non-null, row 0 of its shading table
// (ShadingNormal; row 1, the albedo, is not touched); scratch non-null, the Morton keys under
// `camera` and the ids, then the stable radix sort into d_order. Then the gather (RankKernel) of
// d_vertices through d_order into d_rank and d_svertices -- through the standing d_order when
// scratch is null. Throws std::runtime_error on a failed enqueue.
void EnqueueMotion(const float* d_vertices, std::uint64_t n, const Camera& camera, float* d_shade,
                   const OrderScratch* scratch, unsigned* d_order, unsigned* d_rank, float* d_svertices,
                   hipStream_t stream);
// The host twin (rtmOrderHost): MortonKey and ShadingNormal themselves over host vertices, a stable
// sort by key; order (n) and normals (n x 4) may each be null.
void OrderHost(const float* vertices, std::uint64_t n, const Camera& camera, unsigned* order, float* normals);

// Element-wise IEEE binary16 <-> binary32 conversion on the device (ML_FLOAT16 images):
// float -> half rounds to nearest even (overflow -> inf, NaN stays NaN); half -> float is exact.
// `half` buffers are uint16 bit patterns on the host side.
hipError_t LaunchFloatToHalf(const float* src, std::uint16_t* dst, std::size_t count, hipStream_t stream);
hipError_t LaunchHalfToFloat(const std::uint16_t* src, float* dst, std::size_t count, hipStream_t stream);

#ifdef SRT_DIAG
// Diagnostic build only: copy the cull kernel's per-block phase counters to host memory.
hipError_t DiagRead(void* host, std::size_t bytes);
#endif

}  // namespace srt
