/*
 * srt_layers.h -- depth layers of libModelRunner.so: the K nearest hits at image positions of a
 * prepared frame, front to back, and an over-composite of them (transparent surfaces, layered
 * depth images, thickness and "pick the thing behind the thing", entry/exit pairs).
 *
 * A family of its own (prefix rtk, its own export macro) beside the reference's 14 ml* entry
 * points (model_runner.h), the 38 srt* ones (srt_render.h) and the rtq / rtg / rts / rtl families:
 * those sets are fixed, and this header adds to none of them. Conventions as in srt_render.h: plain
 * pointers and sizes, `stream` is a hipStream_t passed as void*, 0 on success and -1 on failure, the
 * failure text from srtGetLastError() (thread-local).
 *
 * Layers. At an image position (fx, fy) of the prepared W x H frame -- a
 * query of srt_query.h -- let P be the triangles that pass the exact test there, each with the key
 * (t, id), t = vol / det. Layer k, 0 <= k < K, is the k-th smallest key of P in lexicographic
 * order; a position with no more than k passing triangles has layer k = (-1, +inf). So layer 0 is
 * rtqQueryAsync's answer (at a pixel's own position srtTraceIdsAsync's id, bit for bit), the layers
 * of a call with K are the first K of a call with K + 1, triangles with equal t appear in ascending
 * id order, and a NaN position has no layers. K is 1 .. RTK_MAX_LAYERS.
 *
 * Outputs are layer-major: d_ids is K planes of E int32, plane k holding layer k of every element,
 * so each plane feeds rtgFrameAsync, rtgPointsAsync or srtShadeAsync as it is; d_t likewise.
 *
 * Composite. A pixel's K layer ids, a per-triangle opacity table (n floats, the caller's: not
 * range-checked, NaN propagates) and the scene's background, float32 with separate multiply and
 * add in the order written: T = 1, acc = 0; for k = 0 .. K-1, stopping at the first id outside
 * [0, n): a = opacity[id_k], w = T a, acc = acc + w c_k (c_k: srtShadeAsync's rgb of the pixel for
 * id_k), T = T - w; then rgb = acc + T background, alpha = 1 - T. Every opacity 1 gives
 * srtShadeAsync's rgb bit for bit and alpha 1 (hit) or 0 (miss); every opacity 0 the background.
 */
#ifndef SRT_LAYERS_H
#define SRT_LAYERS_H

#include <stddef.h>

#include "srt_render.h" /* srt_device_scene, srtGetLastError */

#if defined(__GNUC__) && defined(RADEONPROML_BUILD)
#define RTK_API __attribute__((visibility("default")))
#else
#define RTK_API
#endif

#define RTK_MAX_LAYERS 8

#ifdef __cplusplus
extern "C" {
#endif

/* count positions (count x 2 float, device) of the prepared frame -> d_ids (layers x count int32),
 * d_t (layers x count float, may be NULL), d_how (count bytes, may be NULL: 0 = answered from the
 * tile's list, 1 = streamed every record). Enqueued on `stream`; the first call (or query, or
 * whole-frame trace) after srtPrepareAsync builds the frame's shared cull setup on it.
 * count == 0: nothing is enqueued. */
RTK_API int rtkLayersAsync(srt_device_scene scene, const float* d_positions, size_t count, size_t layers,
                           int* d_ids, float* d_t, unsigned char* d_how, void* stream);

/* The same at the pixels of the band rows [row_begin, row_begin + row_count) of the prepared frame:
 * d_offsets (row_count x W x 2 float) are the sample offsets, band-local as srtShadeAsync's; d_ids
 * layers x row_count x W, d_t the same shape or NULL, d_how row_count x W or NULL.
 * row_count == 0: nothing is enqueued. */
RTK_API int rtkFrameAsync(srt_device_scene scene, const float* d_offsets, size_t row_begin, size_t row_count,
                          size_t layers, int* d_ids, float* d_t, unsigned char* d_how, void* stream);

/* The over-composite of the band's layers: d_offsets and d_ids as rtkFrameAsync's, d_opacity one
 * float per triangle of the scene -> d_rgba (row_count x W x 4 float). Reads no cull setup.
 * row_count == 0: nothing is enqueued. */
RTK_API int rtkCompositeAsync(srt_device_scene scene, const float* d_offsets, const int* d_ids, size_t layers,
                              const float* d_opacity, size_t row_begin, size_t row_count, float* d_rgba,
                              void* stream);

/* The same answers on the host, no device: brute force with the library's own canonical math.
 * ids, t: layers x count (t may be NULL). */
RTK_API int rtkLayersHost(const char* scene_path, size_t width, size_t height, const float* positions,
                          size_t count, size_t layers, int* ids, float* t);

/* offsets row_count x width x 2, ids layers x row_count x width, opacity one float per triangle ->
 * rgba row_count x width x 4. */
RTK_API int rtkCompositeHost(const char* scene_path, size_t width, size_t height, const float* offsets,
                             const int* ids, size_t layers, const float* opacity, size_t row_begin,
                             size_t row_count, float* rgba);

#ifdef __cplusplus
}
#endif

#endif /* SRT_LAYERS_H */
