/*
 * srt_rays.h -- ray queries of libModelRunner.so: the closest hit and the occlusion of
 * caller-supplied rays, each with an origin, a direction and a range of its own (mirror bounces,
 * ambient occlusion, area-light shadows, visibility between two points, picking and physics probes
 * that do not look through the camera).
 *
 * A family of its own (prefix rtr, its own export macro) beside the reference's 14 ml* entry
 * points (model_runner.h) and the 38 srt* ones (srt_render.h): those two sets are a fixed ABI,
 * and this header adds to neither. Conventions as in srt_render.h: plain pointers and sizes,
 * `stream` is a hipStream_t passed as void*, 0 on success and -1 on failure, the failure text from
 * srtGetLastError() (thread-local).
 *
 * A ray is 8 float32 values, (ox, oy, oz, tmin, dx, dy, dz, tmax): the direction is not normalised
 * and t is in units of d. Its answer is canonical, bit for bit (DESIGN.md section 2 "Rays"): a
 * triangle counts iff its own padded box passes the box clause, the edge test passes and
 * tmin <= t <= tmax. Closest hit: the lexicographic minimum of (t, id) over the triangles that
 * count -- id, t and the barycentrics (w1, w2) of v1 and v2; a miss is (-1, +inf, (0, 0)).
 * Occlusion: one byte, 1 iff any triangle counts. A ray with a non-finite origin or direction
 * component, d = 0, a NaN range or tmin > tmax misses; a triangle with a non-finite vertex is
 * never hit. Origins far outside the scene (100 times its extent) lose the triangle to
 * cancellation in the edge test: the answer is still canonical, but not a useful one.
 *
 * The device calls answer from a world-space tree of the scene's triangles, which depends on the
 * vertices only: no srtPrepareAsync is needed and a moved camera leaves it alone. It is built on
 * the stream of the first rtr call (or by rtrBuildAsync); rtmSetVerticesAsync marks it stale and
 * the next rtr call rebuilds it, on its own stream, in the same buffers. Only the first build
 * allocates; nothing here waits for the device. Env SRT_RAYS=brute (read per call) answers by
 * brute force over the vertices instead, with no structure: the same bytes. Every call is a call
 * on the scene for srt_render.h's ordering rule.
 */
#ifndef SRT_RAYS_H
#define SRT_RAYS_H

#include <stddef.h>

#include "srt_render.h" /* srt_device_scene, srtGetLastError */

#if defined(__GNUC__) && defined(RADEONPROML_BUILD)
#define RTR_API __attribute__((visibility("default")))
#else
#define RTR_API
#endif

#define RTR_RAY_FLOATS 8
#define RTR_BOX_CLAUSE 0    /* the definition (default) */
#define RTR_NO_BOX_CLAUSE 1 /* host only: the edge test and the range alone, for measuring what the clause costs */

#ifdef __cplusplus
extern "C" {
#endif

/* (Re)builds the scene's tree on `stream` if it is missing or stale; else nothing is enqueued. */
RTR_API int rtrBuildAsync(srt_device_scene scene, void* stream);

/* count rays (count x 8 float, device, 16-byte aligned) -> d_ids (count int32), d_t (count float) and
 * d_bary (count x 2 float, may be NULL). count == 0: nothing is enqueued. A scene without triangles
 * stores misses. */
RTR_API int rtrClosestAsync(srt_device_scene scene, const float* d_rays, size_t count, int* d_ids, float* d_t,
                            float* d_bary, void* stream);

/* count rays -> d_out (count bytes): 1 iff any triangle counts. A ray stops at its first counted hit. */
RTR_API int rtrOccludedAsync(srt_device_scene scene, const float* d_rays, size_t count, unsigned char* d_out,
                             void* stream);

/* The same answers on the host, no device: brute force over every triangle in ascending id with the
 * library's own canonical math, no tree. bary may be NULL. The *Flags forms take RTR_BOX_CLAUSE or
 * RTR_NO_BOX_CLAUSE; the plain forms are the definition. */
RTR_API int rtrClosestHost(const char* scene_path, const float* rays, size_t count, int* ids, float* t, float* bary);
RTR_API int rtrOccludedHost(const char* scene_path, const float* rays, size_t count, unsigned char* out);
RTR_API int rtrClosestHostFlags(const char* scene_path, const float* rays, size_t count, int* ids, float* t,
                                float* bary, int flags);
RTR_API int rtrOccludedHostFlags(const char* scene_path, const float* rays, size_t count, unsigned char* out,
                                 int flags);

#ifdef __cplusplus
}
#endif

#endif /* SRT_RAYS_H */
