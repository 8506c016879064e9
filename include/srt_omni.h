/*
 * srt_omni.h -- omni-light shadow masks of libModelRunner.so: which pixels of a prepared frame a
 * point light reaches, the light given as six cube-face frames of the same triangles.
 *
 * A family of its own (prefix rto, its own export macro) beside the reference's 14 ml* entry
 * points (model_runner.h) and the 38 srt* ones (srt_render.h): those two sets are a fixed ABI,
 * and this header adds to neither. Conventions as in srt_render.h: plain pointers and sizes,
 * `stream` is a hipStream_t passed as void*, 0 on success and -1 on failure (rtoLightCreate,
 * rtoLightFace: NULL), the failure text from srtGetLastError() (thread-local).
 *
 * Shadow rays of a point light share an origin, as a spot light's do (srt_light.h), so the light is
 * six device scenes of the same triangles: face k is the camera (eye = origin, lookat = origin +
 * axis_k, up_k, vfov 92 degrees) at face_size x face_size,
 *   k  axis         up                k  axis         up
 *   0  (+1, 0, 0)   (0, 1, 0)         3  (0, -1, 0)   (0, 0, +1)
 *   1  (-1, 0, 0)   (0, 1, 0)         4  (0, 0, +1)   (0, 1, 0)
 *   2  (0, +1, 0)   (0, 0, -1)        5  (0, 0, -1)   (0, 1, 0)
 * built by the path rtlSceneCreate takes. A pixel's surface point P selects one face from q = P -
 * origin (the largest |q_k|, ties to the lower axis; the sign of that component) and srt_light.h's
 * exact shadow test runs in that face's prepared frame only: one launch per band, the class byte
 * srt_light.h's (RTL_SHADOWED 0, RTL_LIT 1, RTL_OUTSIDE 2, RTL_NO_SURFACE 3), canonical bit for bit
 * (DESIGN.md section 2 "Omni shadow"). The 92 degree faces overlap by 1.7 % of the frame on every
 * side, so the selected face always contains the point: class 2 is left to a surface point at the
 * light or one that is not finite.
 */
#ifndef SRT_OMNI_H
#define SRT_OMNI_H

#include <stddef.h>

#include "srt_light.h" /* the class bytes; srt_render.h: srt_device_scene, srtGetLastError */

#if defined(__GNUC__) && defined(RADEONPROML_BUILD)
#define RTO_API __attribute__((visibility("default")))
#else
#define RTO_API
#endif

#define RTO_FACES 6
#define RTO_NO_FACE 255

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rto_light_t* rto_light;

/* The six device scenes of the light at origin (3 finite floats, each |o_k| <= 2^16) over the
 * triangles of the scene file. NULL on failure. */
RTO_API rto_light rtoLightCreate(const char* path, int device, const float origin[3]);
RTO_API void rtoLightRelease(rto_light light);

/* srtPrepareAsync of the six faces at face_size x face_size (> 0). A second call with another size
 * re-prepares them. */
RTO_API int rtoLightPrepareAsync(rto_light light, size_t face_size, void* stream);

/* Face `face` (0 .. 5) as a device scene: borrowed, NOT to be released by the caller, valid until
 * rtoLightRelease; usable with every srt / rtq / rtg / rtk call (a cube map of the scene from the
 * light is six ordinary traces). NULL on failure. */
RTO_API srt_device_scene rtoLightFace(rto_light light, int face);

/* The shadow mask of rows [row_begin, row_begin + row_count) of `view`'s prepared frame under the
 * light. d_offsets, d_ids, d_mask, d_rgba, bias, dim: rtlShadowAsync's. d_face (row_count x W bytes,
 * may be NULL) receives the selected face, RTO_NO_FACE for a class-3 pixel. View and light are
 * prepared, live on one device and hold the same number of triangles. One kernel launch on `stream`;
 * the first use after rtoLightPrepareAsync builds the faces' shared cull setups on it.
 * row_count == 0: nothing is enqueued. The call counts as a call on the view scene and on all six
 * face scenes for srt_render.h's ordering rule. */
RTO_API int rtoShadowAsync(srt_device_scene view, rto_light light, const float* d_offsets, const int* d_ids,
                           size_t row_begin, size_t row_count, float bias, unsigned char* d_mask,
                           unsigned char* d_face, float* d_rgba, float dim, void* stream);

/* The same answer on the host, no device: brute force with the library's own canonical math. The
 * view is scene_path's camera at width x height; face and rgba may be NULL. */
RTO_API int rtoShadowHost(const char* scene_path, size_t width, size_t height, const float origin[3], size_t face_size,
                          const float* offsets, const int* ids, size_t row_begin, size_t row_count, float bias,
                          unsigned char* mask, unsigned char* face, float* rgba, float dim);

/* camera10 = eye, lookat, up, vfov_deg of face `face` of the light at origin. */
RTO_API int rtoFaceCameraHost(const float origin[3], int face, float camera10[10]);

/* The face the kernel selects for q = surface point - origin (0 .. 5); -1 for a NULL q. */
RTO_API int rtoFaceOfHost(const float q[3]);

#ifdef __cplusplus
}
#endif

#endif /* SRT_OMNI_H */
