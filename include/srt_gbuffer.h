/*
 * srt_gbuffer.h -- G-buffer outputs of libModelRunner.so: the surface under a hit -- depth,
 * barycentrics, normal and albedo -- from hit ids (denoisers, compositing, edge-aware filters,
 * texture lookup, depth tests against other content, debugging views).
 *
 * A family of its own (prefix rtg, its own export macro) beside the reference's 14 ml* entry
 * points (model_runner.h), the 38 srt* ones (srt_render.h) and the rtq* point queries
 * (srt_query.h): those sets are a fixed ABI, and this header adds to none of them. Conventions as
 * in srt_render.h: plain pointers and sizes, `stream` is a hipStream_t passed as void*, 0 on
 * success and -1 on failure, the failure text from srtGetLastError() (thread-local).
 *
 * An element is an image position (fx, fy) of the prepared W x H frame and a triangle id -- what
 * srtTraceIdsAsync stores for a pixel, or rtqQueryAsync for a position. Its attributes are
 * canonical (DESIGN.md section 2 "Surface attributes"), with E_k, det and vol the trace's own
 * values for that triangle at that position:
 *   depth   t = vol / det: bit for bit rtqQueryAsync's t. The planar (view-axis) depth in world
 *           units, not a distance along a normalised ray.
 *   bary    (w1, w2) = (E_B / det, E_C / det): the weights of v1 and v2 (the Moller-Trumbore
 *           (u, v)); w0 = E_A / det is not stored.
 *   normal  the unit geometric normal turned towards the eye, and in .w the shading cosine.
 *   albedo  the triangle's unshaded (r, g, b), and in .a float(id).
 * albedo.rgb * normal.w and albedo.a are the RGBA pixel srtTraceAsync stores, bit for bit. An id
 * outside the scene (-1, the miss; any sentinel) gives depth +inf, bary (0, 0), normal
 * (0, 0, 0, 1), albedo (background, -1), and no memory is read through it. The hit test is not
 * run again: for an id that does not hit at its position the values are simply the formulas'.
 */
#ifndef SRT_GBUFFER_H
#define SRT_GBUFFER_H

#include <stddef.h>

#include "srt_render.h" /* srt_device_scene, srtGetLastError */

#if defined(__GNUC__) && defined(RADEONPROML_BUILD)
#define RTG_API __attribute__((visibility("default")))
#else
#define RTG_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

/* The output planes, float32, element-major: depth[count], bary[count][2], normal[count][4],
 * albedo[count][4]. A NULL plane is not written. struct_size = sizeof(rtg_outputs). */
typedef struct rtg_outputs {
    size_t struct_size;
    float* depth;
    float* bary;
    float* normal;
    float* albedo;
} rtg_outputs;

/* The band rows [row_begin, row_begin + row_count) of the prepared frame: element (x, y) is pixel
 * (x, row_begin + y) at its sample offset. d_offsets (row_count x W x 2), d_ids (row_count x W) and
 * the planes (row_count x W elements) are band-local device buffers, as srtShadeAsync's. Enqueued on
 * `stream`; row_count == 0 or no plane: nothing is enqueued. Builds and reads no cull setup. */
RTG_API int rtgFrameAsync(srt_device_scene scene, const float* d_offsets, const int* d_ids, size_t row_begin,
                          size_t row_count, const rtg_outputs* outputs, void* stream);

/* count elements: positions d_positions (count x 2) with ids d_ids (count), device buffers -- the
 * inputs and outputs of rtqQueryAsync. count == 0 or no plane: nothing is enqueued. */
RTG_API int rtgPointsAsync(srt_device_scene scene, const float* d_positions, const int* d_ids, size_t count,
                           const rtg_outputs* outputs, void* stream);

/* The same answer on the host, no device, with the library's own canonical math. */
RTG_API int rtgPointsHost(const char* scene_path, size_t width, size_t height, const float* positions,
                          const int* ids, size_t count, const rtg_outputs* outputs);

#ifdef __cplusplus
}
#endif

#endif /* SRT_GBUFFER_H */
