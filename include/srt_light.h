/*
 * srt_light.h -- spot-light shadow masks of libModelRunner.so: which pixels of a prepared frame a
 * spot light reaches, the light given as a second prepared frame of the same triangles.
 *
 * A family of its own (prefix rtl, its own export macro) beside the reference's 14 ml* entry
 * points (model_runner.h) and the 38 srt* ones (srt_render.h): those two sets are a fixed ABI,
 * and this header adds to neither. Conventions as in srt_render.h: plain pointers and sizes,
 * `stream` is a hipStream_t passed as void*, 0 on success and -1 on failure (rtlSceneCreate: NULL),
 * the failure text from srtGetLastError() (thread-local).
 *
 * Shadow rays from a spot light share an origin, the light, as primary rays share the eye: so the
 * light is a device scene of the same triangles under the light's camera (rtlSceneCreate), prepared
 * at a resolution WL x HL of its own (srtPrepareAsync), and a pixel's shadow test is the canonical
 * closest hit of that frame at the position where the pixel's surface point projects. The answer is
 * one class byte per pixel, canonical bit for bit (DESIGN.md section 2 "Shadow"):
 *   0  shadowed    the light frame's closest hit there is another triangle, nearer than the point
 *   1  lit         it is the pixel's own triangle, or nothing nearer than thr = z - bias z
 *   2  outside     the surface point is not in the light's frustum
 *   3  no surface  the pixel's hit id is no triangle of the scene (a miss)
 * The id test makes the mask free of self-shadowing without a bias; `bias` (relative, >= 0) only
 * rescues pixels whose light ray lands on a coplanar neighbour of their own triangle.
 */
#ifndef SRT_LIGHT_H
#define SRT_LIGHT_H

#include <stddef.h>

#include "srt_render.h" /* srt_device_scene, srtGetLastError */

#if defined(__GNUC__) && defined(RADEONPROML_BUILD)
#define RTL_API __attribute__((visibility("default")))
#else
#define RTL_API
#endif

#define RTL_SHADOWED 0
#define RTL_LIT 1
#define RTL_OUTSIDE 2
#define RTL_NO_SURFACE 3

#ifdef __cplusplus
extern "C" {
#endif

/* srtDeviceSceneCreate with the file's camera replaced by camera10 = eye[3], lookat[3], up[3],
 * vfov_deg (NULL: the file's camera): the same spatial order built under that camera, released by
 * srtDeviceSceneRelease, usable with every srt / rtq / rtg / rts call. The ten values are finite, vfov
 * in (0, 180) degrees, eye != lookat, up not parallel to the view direction. NULL on failure. */
RTL_API srt_device_scene rtlSceneCreate(const char* path, int device, const float camera10[10]);

/* The shadow mask of rows [row_begin, row_begin + row_count) of `view`'s prepared frame under
 * `light`'s prepared frame. d_offsets (row_count x W x 2 float) and d_ids (row_count x W int32, as
 * srtTraceIdsAsync stores them) are band-local like srtShadeAsync's; d_mask receives row_count x W
 * class bytes; d_rgba (row_count x W x 4 float, may be NULL) the pixel srtShadeAsync stores with rgb
 * multiplied by 1 (class 1) or `dim` (classes 0 and 2), a class-3 pixel the background unmultiplied.
 * Both scenes are prepared, live on one device and hold the same number of triangles; bias is
 * finite and >= 0, dim finite. Enqueued on `stream`; the first use after the light's
 * srtPrepareAsync builds the light's shared cull setup on it. row_count == 0: nothing is enqueued.
 * The call counts as a call on both scenes for srt_render.h's ordering rule. */
RTL_API int rtlShadowAsync(srt_device_scene view, srt_device_scene light, const float* d_offsets, const int* d_ids,
                           size_t row_begin, size_t row_count, float bias, unsigned char* d_mask, float* d_rgba,
                           float dim, void* stream);

/* The same answer on the host, no device: brute force with the library's own canonical math. The
 * view is scene_path's camera at width x height, the light light_camera10 at light_width x light_height. */
RTL_API int rtlShadowHost(const char* scene_path, size_t width, size_t height, const float light_camera10[10],
                          size_t light_width, size_t light_height, const float* offsets, const int* ids,
                          size_t row_begin, size_t row_count, float bias, unsigned char* mask, float* rgba, float dim);

/* The three projection rows (px, py, pz) the library uses for a light camera at its resolution. */
RTL_API int rtlProjectionHost(const float camera10[10], size_t light_width, size_t light_height, float rows9[9]);

#ifdef __cplusplus
}
#endif

#endif /* SRT_LIGHT_H */
