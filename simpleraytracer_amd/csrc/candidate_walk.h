#pragma once

#include <hip/hip_runtime.h>

#include "tile_lookup.h"
#include "trace_device.h"

namespace srt {

// ---------------------------------------------------------------------------------------
// The candidate walk (DESIGN.md section 5 "Point queries"): every record that can pass the exact
// test at one position of a prepared frame, visited by the LANES lanes that share the position.
// The query, layers, shadow, omni-shadow and lighting kernels all answer "what does this position
// see" with it, so their exactness rests on this one argument.
// The setup's lists were binned against the analytic tile boxes, and that binning is about boxes,
// not pixel grids: BoxMayHit bounds the edge functions at every (fx, fy) of the box, and a record's
// screen box contains every position with |fx|, |fy| <= kScreenBoxRange at which its float test can
// pass. So a position inside a usable tile box passes the exact test of no record outside that
// tile's list and the large list (listed: entries [0, cnt) of the tile's list, then the large
// list's). A position outside [0, 1]^2 (NaN included), a tile whose list overflowed or whose box is
// not ScreenBoxUsable, and a frame without a setup (tile_info null) stream every record instead:
// positions [0, stream_end), pad records included (disabled: they pass nowhere).
// FindCandidates serves TraceParams and LightFrame through their common field names and copies each
// field it uses into a local once: a frame selected per lane is read with vector loads from the
// argument segment, a uniform one with scalar loads.
// WalkCandidates: the lanes stride the candidates (a coalesced 4-B entry load, then each lane
// gathers its record), AHEAD candidates per lane and round, so a round has that many dependent
// load pairs in flight: AHEAD entries, AHEAD record loads, AHEAD tests. A lane past the end repeats
// the last candidate (no divergent tail), so `test` must be idempotent: a (t, id) minimum and
// KeyList::Insert are. stop() is evaluated once per round, by every lane of the group alike;
// returns whether it ended the walk.
// ---------------------------------------------------------------------------------------
struct Candidates {
    const unsigned* list;        // the tile's list
    const unsigned* large_list;
    unsigned cnt;                // entries of the tile's list
    unsigned total;              // candidates: cnt + the large list's entries, or stream_end
    bool listed;                 // from the lists; else streamed
    __device__ __forceinline__ unsigned Entry(unsigned k) const {
        if (!listed) {
            return k;
        }
        const unsigned* at = k < cnt ? list + k : large_list + (k - cnt);
        return *at;
    }
};

template <class F>
__device__ __forceinline__ Candidates FindCandidates(const F& f, int tiles_y, unsigned stream_end, float fx, float fy) {
    Candidates c{nullptr, nullptr, 0u, stream_end, false};
    int col = 0, row = 0;
    const TileInfo* tile_info = f.tile_info;
    const int tiles_x = f.tiles_x;
    if (tile_info != nullptr && TileOfPosition(fx, fy, f.wf, f.hf, kCullTileCols, kTileRows, tiles_x, tiles_y, col, row)) {
        const unsigned tile = static_cast<unsigned>(row) * static_cast<unsigned>(tiles_x) + static_cast<unsigned>(col);
        const unsigned* counts = f.bin_counts;
        const unsigned capacity = f.bin_capacity;
        c.cnt = counts[tile];
        const unsigned large = counts[f.tiles];
        c.list = f.bin_lists + static_cast<size_t>(tile) * capacity;
        c.large_list = f.large_list;
        c.listed = c.cnt <= capacity && tile_info[tile].usable != 0u;
        c.total = c.listed ? c.cnt + large : stream_end;
    }
    return c;
}

template <int LANES, int AHEAD, class Raw, class Load, class Test, class Stop>
__device__ __forceinline__ bool WalkCandidates(const Candidates& c, unsigned lane, Load load, Test test, Stop stop) {
    for (unsigned base = 0u; base < c.total; base += AHEAD * LANES) {
        unsigned pos[AHEAD];
        Raw raw[AHEAD];
#pragma unroll
        for (int a = 0; a < AHEAD; ++a) {
            pos[a] = c.Entry(min(base + a * LANES + lane, c.total - 1u));
        }
#pragma unroll
        for (int a = 0; a < AHEAD; ++a) {
            raw[a] = load(pos[a]);
        }
#pragma unroll
        for (int a = 0; a < AHEAD; ++a) {
            test(raw[a]);
        }
        if (stop()) {
            return true;
        }
    }
    return false;
}

// One record source per launch: the kernel's template argument.
template <class P>
inline hipError_t LaunchBySource(bool recompute, void (*recomputed)(P), void (*stored)(P), dim3 grid, int threads,
                                 hipStream_t stream, const P& q) {
    hipLaunchKernelGGL(recompute ? recomputed : stored, grid, dim3(threads), 0, stream, q);
    return hipGetLastError();
}

// The records a point query (or a shadow test) reads, as TraceParams: the setup's, or -- setup ==
// null -- the scene's spatial inputs for TraceRecords<true>. Returns whether the records are
// recomputed (the kernel's RC).
inline bool QueryRecords(TraceParams& p, int& tiles_y, const CullSetup* setup, std::uint64_t n, const Frame& frame,
                         std::size_t width, std::size_t height, const float* d_svertices, const float* d_edges) {
    // Without a setup the records are recomputed from the scene's spatial inputs; TraceRecords<true>
    // also loads the position's screen box, which the exact test does not use: the scene's edge
    // allocation has room for one per padded record, so the address is valid whatever it holds.
    const EdgeLayout e = setup != nullptr ? SetupRecords(*setup) : EdgeBuffers(d_edges, n);
    p.screen_boxes = e.screen_boxes;
    p.cull = e.cull;
    p.svertices = d_svertices;
    p.n = static_cast<unsigned>(n);
    p.n_pad = static_cast<unsigned>(PaddedTriangleCount(n));
    for (int k = 0; k < 3; ++k) {
        p.base[k] = frame.base[k];
        p.du[k] = frame.du[k];
        p.dv[k] = frame.dv[k];
        p.eye[k] = frame.origin[k];
    }
    bool recompute = true;
    tiles_y = 0;
    if (setup != nullptr) {
        recompute = setup->recompute;
        p.tile_info = static_cast<const TileInfo*>(setup->tile_info);
        p.bin_lists = setup->lists;
        p.bin_counts = setup->counts;
        p.large_list = setup->large_list;
        p.bin_capacity = setup->capacity;
        p.tiles_x = static_cast<int>((width + kWave - 1) / kWave);
        tiles_y = static_cast<int>((height + kTileRows - 1) / kTileRows);
        p.tiles = static_cast<unsigned>(setup->tiles);
        p.wf = static_cast<float>(width);
        p.hf = static_cast<float>(height);
    }
    return recompute;
}

}  // namespace srt
