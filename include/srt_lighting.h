/*
 * srt_lighting.h -- direct lighting of libModelRunner.so: the lit picture of a prepared frame under
 * several spot and point lights, one kernel launch per band.
 *
 * A family of its own (prefix rtd, its own export macro) beside the reference's 14 ml* entry
 * points (model_runner.h) and the 38 srt* ones (srt_render.h): those two sets are a fixed ABI,
 * and this header adds to neither. Conventions as in srt_render.h: plain pointers and sizes,
 * `stream` is a hipStream_t passed as void*, 0 on success and -1 on failure, the failure text from
 * srtGetLastError() (thread-local).
 *
 * A spot light is a prepared light scene as rtlShadowAsync takes it (srt_light.h), a point light a
 * prepared rto_light (srt_omni.h); each carries a colour, a falloff and its shadow bias. Per pixel
 * with hit id `id` (DESIGN.md section 2 "Lighting"; float32, no fma, in this order):
 *   d = (base + fx du) + fy dv, P = eye + t d          t: the depth of the hit, as the shadow calls'
 *   N, albedo: the triangle's shading-table row; nn = N.N, nd = N.d
 *   E = ambient; for every light in the order given:
 *     q = P - origin; cls = the class byte rtlShadowAsync / rtoShadowAsync give the pixel at `bias`
 *     nl = N.q; the light contributes iff cls == RTL_LIT and nl, nd are both < 0 or both > 0 (the
 *     light and the eye on one side of the triangle); then
 *       cosl = min(|nl| / (sqrt(nn) sqrt(q.q)), 1); w = falloff > 0 ? cosl (falloff / q.q) : cosl
 *       E += color w
 *   rgba = (albedo E, float(id)), not clamped; an id outside the scene: (background, -1), class 3.
 * Canonical bit for bit: the device call, the host call and a numpy float32 restatement agree.
 */
#ifndef SRT_LIGHTING_H
#define SRT_LIGHTING_H

#include <stddef.h>

#include "srt_omni.h" /* rto_light; srt_light.h: the class bytes; srt_render.h: srt_device_scene */

#if defined(__GNUC__) && defined(RADEONPROML_BUILD)
#define RTD_API __attribute__((visibility("default")))
#else
#define RTD_API
#endif

#define RTD_MAX_LIGHTS 8
#define RTD_MAX_FRAMES 16 /* light frames per call: 1 per spot light, 6 per point light */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rtd_light { /* device call */
    size_t struct_size;    /* sizeof(rtd_light): checked */
    srt_device_scene spot; /* exactly one of spot / point is non-NULL */
    rto_light point;
    float color[3]; /* finite */
    float falloff;  /* finite, >= 0; 0: no distance term */
    float bias;     /* finite, >= 0: the relative depth bias of the shadow test */
} rtd_light;

typedef struct rtd_light_host { /* host call */
    size_t struct_size;
    int kind;             /* 0 spot, 1 point */
    float camera10[10];   /* spot: eye, lookat, up, vfov */
    size_t width, height; /* spot: the light frame */
    float origin[3];      /* point */
    size_t face_size;     /* point */
    float color[3], falloff, bias;
} rtd_light_host;

/* The lit RGBA of rows [row_begin, row_begin + row_count) of `view`'s prepared frame under `count`
 * (0 .. RTD_MAX_LIGHTS; 0 with lights == NULL is valid) lights and the ambient colour (3 finite
 * floats). d_offsets (row_count x W x 2) and d_ids (row_count x W): rtlShadowAsync's. d_rgba:
 * row_count x W x 4. d_classes (count x row_count x W bytes, light-major, may be NULL): plane l is
 * the mask of the single-light shadow call of light l at its bias. The `lights` array is read during
 * the call. Every light is prepared, lives on the view's device and holds the view's number of
 * triangles; a light may appear more than once; at most RTD_MAX_FRAMES light frames in all, all
 * reading their records from one source. One kernel launch on `stream` whatever `count`; the first
 * use of a light frame after its prepare builds its shared cull setup on it. row_count == 0: nothing
 * is enqueued. The call counts as a call on the view scene and on every light frame for
 * srt_render.h's ordering rule. A refused argument names the light and the field; a refused call
 * enqueues and builds nothing.
 * "One source": a light frame normally reads the stored records of its shared cull setup. A frame
 * too large for one -- more than 8192 cull tiles of 64 x 16 pixels (3072 x 3072, 4096 x 4096), or
 * more than 2048 tile columns plus tile rows -- recomputes its records instead, and so cannot share
 * a call with a smaller light frame: such a light works alone (and in rtlShadowAsync), beside other
 * frames of that kind, or beside any frame when every setup recomputes (env
 * SRT_TRACE_RECORDS=recompute); otherwise the call is refused and the message names the light. */
RTD_API int rtdLightAsync(srt_device_scene view, const rtd_light* lights, size_t count, const float ambient[3],
                          const float* d_offsets, const int* d_ids, size_t row_begin, size_t row_count,
                          float* d_rgba, unsigned char* d_classes, void* stream);

/* The same answer on the host, no device: brute force with the library's own canonical math. The
 * view is scene_path's camera at width x height; every light holds scene_path's triangles; classes
 * may be NULL. */
RTD_API int rtdLightHost(const char* scene_path, size_t width, size_t height, const rtd_light_host* lights, size_t count,
                         const float ambient[3], const float* offsets, const int* ids, size_t row_begin, size_t row_count,
                         float* rgba, unsigned char* classes);

#ifdef __cplusplus
}
#endif

#endif /* SRT_LIGHTING_H */
