/*
 * srt_query.h -- point queries of libModelRunner.so: the closest hit at arbitrary image
 * positions of a prepared frame (picking, probes, sparse re-sampling, spot checks).
 *
 * A family of its own (prefix rtq, its own export macro) beside the reference's 14 ml* entry
 * points (model_runner.h) and the 38 srt* ones (srt_render.h): those two sets are a fixed ABI,
 * and this header adds to neither. Conventions as in srt_render.h: plain pointers and sizes,
 * `stream` is a hipStream_t passed as void*, 0 on success and -1 on failure, the failure text from
 * srtGetLastError() (thread-local).
 *
 * A query is an image position (fx, fy), float32, in the prepared W x H frame -- the quantity ray
 * generation produces for a pixel: fx = (float(x) + sx) / float(W), fy = (float(y) + sy) / float(H).
 * Its answer is canonical, bit for bit: the hit triangle's id (-1: miss) and
 * t = vol / det of the winner (+inf: miss), the lexicographic minimum of (t, id) over every
 * triangle passing the exact test -- at a pixel's own position, what srtTraceIdsAsync stores for
 * that pixel. Any float pair is a legal query; positions outside [0, 1]^2, NaN and infinities get
 * the brute-force answer (a NaN position misses).
 */
#ifndef SRT_QUERY_H
#define SRT_QUERY_H

#include <stddef.h>

#include "srt_render.h" /* srt_device_scene, srtGetLastError */

#if defined(__GNUC__) && defined(RADEONPROML_BUILD)
#define RTQ_API __attribute__((visibility("default")))
#else
#define RTQ_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* count positions (count x 2 float, device) of the prepared frame -> d_ids (count int32), d_t (count float);
 * d_how (count bytes, may be NULL): 0 = answered from the tile's list, 1 = streamed every record.
 * Enqueued on `stream`; the first query (or whole-frame trace) after srtPrepareAsync builds the
 * frame's shared cull setup on it. count == 0: nothing is enqueued. */
RTQ_API int rtqQueryAsync(srt_device_scene scene, const float* d_positions, size_t count,
                          int* d_ids, float* d_t, unsigned char* d_how, void* stream);

/* The same answer on the host, no device: brute force with the library's own canonical math. */
RTQ_API int rtqQueryHost(const char* scene_path, size_t width, size_t height, const float* positions,
                         size_t count, int* ids, float* t);

/* Host self-test of the kernel's tile lookup: 0 and the tile, or -1 when the position is not in [0,1]^2. */
RTQ_API int rtqTileHost(size_t width, size_t height, float fx, float fy, int* tile_col, int* tile_row);

#ifdef __cplusplus
}
#endif

#endif /* SRT_QUERY_H */
