/*
 * srt_motion.h -- dynamic scenes of libModelRunner.so: move a device scene's camera, an omni
 * light's origin or the triangles themselves in place, instead of creating the scene again.
 *
 * A family of its own (prefix rtm, its own export macro) beside the reference's 14 ml* entry
 * points (model_runner.h) and the 38 srt* ones (srt_render.h): those two sets are a fixed ABI,
 * and this header adds to neither. Conventions as in srt_render.h: plain pointers and sizes,
 * `stream` is a hipStream_t passed as void*, 0 on success and -1 on failure, the failure text
 * from srtGetLastError() (thread-local).
 *
 * Equivalence (DESIGN.md section 5 "Motion"): after an update the scene is, for every call of
 * every family, the scene rtlSceneCreate would give on a file holding the new vertices, the old
 * albedo and background, under the new camera -- the same answers on every bit. A prepared scene
 * stays prepared at its W x H (no srtPrepareAsync is needed after a move, and one is harmless), an
 * unprepared one stays unprepared, an omni light keeps its face size. The triangle count and the
 * albedo never change.
 *
 * Every update is a call on the scene for srt_render.h's ordering rule: enqueued on `stream`, it
 * runs after the scene's earlier calls on any stream, and later calls on any stream run after it.
 * Apart from the scene's sort scratch, allocated by its first reordering update, an update
 * allocates and frees nothing and never waits for the device.
 *
 * Arguments are checked in the order flags, camera / origin, handle, device buffer; a refused call
 * changes nothing.
 */
#ifndef SRT_MOTION_H
#define SRT_MOTION_H

#include <stddef.h>

#include "srt_omni.h" /* rto_light; srt_render.h: srt_device_scene, srtGetLastError */

#if defined(__GNUC__) && defined(RADEONPROML_BUILD)
#define RTM_API __attribute__((visibility("default")))
#else
#define RTM_API
#endif

#define RTM_REORDER 0    /* rebuild the spatial order under the new pose (default) */
#define RTM_KEEP_ORDER 1 /* keep the standing order: same frames bit for bit, only speed differs */

#ifdef __cplusplus
extern "C" {
#endif

/* The scene's camera becomes camera10 = eye, lookat, up, vfov_deg (rtlSceneCreate's rules: finite
 * values, vfov in (0, 180), eye != lookat, up not parallel to the view). RTM_REORDER: Morton keys,
 * a device radix sort and the gather of the vertices into the new order, on `stream`.
 * RTM_KEEP_ORDER: no kernel at all. Any other flag bit is refused. */
RTM_API int rtmSetCameraAsync(srt_device_scene scene, const float camera10[10], int flags, void* stream);

/* The scene's triangles become d_vertices (device, triangles x 9 floats: v0.xyz v1.xyz v2.xyz per
 * triangle, read on `stream` during the call's enqueued work; the caller may reuse the buffer
 * once the stream has passed the call). Not range-checked: non-finite vertices give what the
 * formulas give. One pass rewrites the shading normals (and, RTM_REORDER, the keys), then the
 * sort and the gather; RTM_KEEP_ORDER: the normals and the gather through the standing order. */
RTM_API int rtmSetVerticesAsync(srt_device_scene scene, const float* d_vertices, int flags, void* stream);

/* The camera last set (or the creation's): host state, no device work. */
RTM_API int rtmGetCamera(srt_device_scene scene, float camera10[10]);

/* The six per-face updates of a light on one stream: the faces' cameras become those
 * rtoFaceCameraHost reports for origin3 (rtoLightCreate's rule: finite, |o_k| <= 2^16), or all six
 * faces take the new triangles. One call on all six faces for the ordering rule. (A face borrowed
 * through rtoLightFace may also be updated on its own with the scene calls above.) */
RTM_API int rtmLightSetOriginAsync(rto_light light, const float origin3[3], int flags, void* stream);
RTM_API int rtmLightSetVerticesAsync(rto_light light, const float* d_vertices, int flags, void* stream);

/* The host twin, no device: the spatial order of n host triangles (n x 9 floats) under camera10
 * -- the library's own Morton key, then a stable sort by (key, id) -- into order (n entries, may
 * be NULL) and each triangle's shading-table row 0, (cross(v1 - v0, v2 - v0), its length), into
 * normals (n x 4 floats, may be NULL). */
RTM_API int rtmOrderHost(const float* vertices, unsigned long long n, const float camera10[10], unsigned* order,
                         float* normals);

#ifdef __cplusplus
}
#endif

#endif /* SRT_MOTION_H */
