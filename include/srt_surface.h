/*
 * srt_surface.h -- vertex attributes of libModelRunner.so: what the surface under a hit looks like
 * -- per-corner data interpolated with perspective-correct weights, a smooth normal, a UV and a
 * texture lookup -- from hit ids, in one launch (smooth or textured pictures, texture-space
 * lookups, any per-vertex quantity carried to the pixels).
 *
 * A family of its own (prefix rtv, its own export macro) beside the reference's 14 ml* entry
 * points (model_runner.h), the 38 srt* ones (srt_render.h) and the later families: those sets are
 * a fixed ABI, and this header adds to none of them. Conventions as in srt_render.h: plain
 * pointers and sizes, `stream` is a hipStream_t passed as void*, 0 on success and -1 on failure,
 * the failure text from srtGetLastError() (thread-local). For the stream-ordering rule every
 * *Async call here is a call on the scene.
 *
 * An element is an image position (fx, fy) of the prepared W x H frame and a triangle id, as in
 * srt_gbuffer.h. Every per-triangle table is the caller's buffer, passed per call and indexed by
 * the id the traces report (the triangle's index in the scene file): the scene keeps none of them,
 * so no update of the scene (srt_motion.h) can invalidate one. The math is canonical (DESIGN.md
 * section 2 "Vertex attributes"): float32, separate multiply and add, in the order written, so a
 * numpy float32 restatement reproduces the bits.
 *
 *   weights  w0 = E_A / det, w1 = E_B / det, w2 = E_C / det with the trace's own E_k and det for
 *            that triangle at that position: (w1, w2) are rtgFrameAsync's bary, bit for bit. They
 *            are object-space barycentrics of the hit point, so perspective-correct.
 *   table    a corner table holds n x 3 x C floats, 1 <= C <= 4: row id = corner 0's C values,
 *            then corner 1's, then corner 2's. out_c = (w0 a[id][0][c] + w1 a[id][1][c]) + w2 a[id][2][c].
 *   normal   Ns = the interpolation of `normals` (n x 3 x 3, any length); the plane holds the unit
 *            normal Ns / |Ns| turned towards the eye and in .w the shading cosine, rtg's format.
 *            Without `normals`: rtg's normal plane (the geometric normal), bit for bit.
 *   uv       the interpolation of `uvs` (n x 3 x 2); without `uvs`: (0, 0).
 *   albedo   (texel.rgb, float(id)), the texel of `texture` (tex_height x tex_width x 4 float32,
 *            16-byte aligned, .a ignored, row j covers v in [j / TH, (j + 1) / TH): no flip) at
 *            (u, v): repeat or clamp wrap, bilinear or nearest filter. With RTV_MODULATE the texel
 *            times the scene's albedo of the triangle (OBJ's Kd * map_Kd). Without `texture`: rtg's
 *            albedo plane, bit for bit.
 *   rgba     (albedo.rgb * normal.w, float(id)): the shaded pixel. Without `normals` and `texture`
 *            it is srtShadeAsync's pixel, bit for bit.
 * An id outside the scene (-1, the miss; any sentinel) gives 0 in every channel of an interpolation,
 * normal (0, 0, 0, 1), uv (0, 0), albedo (background, -1), rgba (background, -1), and no memory is
 * read through it. The hit test is not run again: for an id that does not hit at its position the
 * values are simply the formulas'.
 */
#ifndef SRT_SURFACE_H
#define SRT_SURFACE_H

#include <stddef.h>

#include "srt_render.h" /* srt_device_scene, srtGetLastError */

#if defined(__GNUC__) && defined(RADEONPROML_BUILD)
#define RTV_API __attribute__((visibility("default")))
#else
#define RTV_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define RTV_MAX_CHANNELS 4    /* floats per corner of a table */
#define RTV_MAX_TEXTURE 16384 /* texels per side of a texture */

#define RTV_WRAP_CLAMP 1     /* clamp (u, v) to [0, 1]; default: repeat */
#define RTV_FILTER_NEAREST 2 /* the texel (u, v) falls in; default: bilinear */
#define RTV_MODULATE 4       /* albedo = texel * the scene's albedo of the triangle */

/* What the surface is made of. Every pointer may be NULL: no such input. `texture` needs `uvs`.
 * struct_size = sizeof(rtv_surface); any flag bit other than the three above is refused. Device
 * buffers for the *Async calls, host arrays for rtvSurfaceHost. */
typedef struct rtv_surface {
    size_t struct_size;
    const float* normals; /* n x 3 x 3 */
    const float* uvs;     /* n x 3 x 2 */
    const float* texture; /* tex_height x tex_width x 4 */
    size_t tex_width;
    size_t tex_height;
    unsigned flags;
} rtv_surface;

/* The output planes, float32, element-major: normal[count][4], albedo[count][4], rgba[count][4],
 * uv[count][2]. A NULL plane is not written. struct_size = sizeof(rtv_outputs). */
typedef struct rtv_outputs {
    size_t struct_size;
    float* normal;
    float* albedo;
    float* rgba;
    float* uv;
} rtv_outputs;

/* The band rows [row_begin, row_begin + row_count) of the prepared frame: element (x, y) is pixel
 * (x, row_begin + y) at its sample offset. d_offsets (row_count x W x 2), d_ids (row_count x W)
 * and the planes (row_count x W elements) are band-local device buffers, as rtgFrameAsync's.
 * Enqueued on `stream`; row_count == 0 or no plane: nothing is enqueued. Builds and reads no cull
 * setup. */
RTV_API int rtvSurfaceFrameAsync(srt_device_scene scene, const float* d_offsets, const int* d_ids, size_t row_begin,
                                 size_t row_count, const rtv_surface* surface, const rtv_outputs* outputs,
                                 void* stream);

/* count elements: positions d_positions (count x 2) with ids d_ids (count), device buffers -- the
 * inputs and outputs of rtqQueryAsync. count == 0 or no plane: nothing is enqueued. */
RTV_API int rtvSurfacePointsAsync(srt_device_scene scene, const float* d_positions, const int* d_ids, size_t count,
                                  const rtv_surface* surface, const rtv_outputs* outputs, void* stream);

/* The interpolation of one corner table d_table (n x 3 x channels) alone: d_out holds
 * row_count x W x channels (frame) or count x channels (points) floats. */
RTV_API int rtvInterpolateFrameAsync(srt_device_scene scene, const float* d_offsets, const int* d_ids,
                                     size_t row_begin, size_t row_count, const float* d_table, size_t channels,
                                     float* d_out, void* stream);
RTV_API int rtvInterpolatePointsAsync(srt_device_scene scene, const float* d_positions, const int* d_ids, size_t count,
                                      const float* d_table, size_t channels, float* d_out, void* stream);

/* The same answers on the host, no device, with the library's own canonical math: host arrays. */
RTV_API int rtvSurfaceHost(const char* scene_path, size_t width, size_t height, const float* positions, const int* ids,
                           size_t count, const rtv_surface* surface, const rtv_outputs* outputs);
RTV_API int rtvInterpolateHost(const char* scene_path, size_t width, size_t height, const float* positions,
                               const int* ids, size_t count, const float* table, size_t channels, float* out);

/* The corner normals (`vn`) and texture coordinates (`vt`) of a Wavefront OBJ file, one row per
 * triangle of the scene srtReadScene loads from it (the same fan triangulation, the same order):
 * normals n x 3 x 3, uvs n x 3 x 2, n = srtSceneTriangles(path); either may be NULL. A corner
 * without `vn` takes its triangle's shading normal cross(v1 - v0, v2 - v0), one without `vt`
 * (0, 0). have[0] / have[1]: whether any corner carried a `vn` / a `vt` (have may be NULL). */
RTV_API int rtvObjAttributesHost(const char* path, float* normals, float* uvs, int have[2]);

#ifdef __cplusplus
}
#endif

#endif /* SRT_SURFACE_H */
