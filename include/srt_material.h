/*
 * srt_material.h -- lit surfaces of libModelRunner.so: the textured, smooth-shaded, shadowed picture
 * of a prepared frame -- the lights and shadows of srt_lighting.h on the surface of srt_surface.h,
 * with an optional Blinn-Phong highlight -- in one kernel launch per band.
 *
 * A family of its own (prefix rtp, its own export macro) beside the reference's 14 ml* entry
 * points (model_runner.h), the 38 srt* ones (srt_render.h) and the later families: those sets are
 * a fixed ABI, and this header adds to none of them. Conventions as in srt_render.h: plain pointers
 * and sizes, `stream` is a hipStream_t passed as void*, 0 on success and -1 on failure, the failure
 * text from srtGetLastError() (thread-local).
 *
 * Per pixel with hit id `id` (DESIGN.md section 2 "Lit surfaces"; float32, no fma, in this order):
 *   d, P, the geometric N, nn, nd and for every light q = P - origin, its class byte cls, nl = N.q
 *   and `facing` are rtdLightAsync's: shadows and the set of contributing lights depend on geometry
 *   alone, and the class planes are rtdLightAsync's bit for bit whatever the surface.
 *   (u, cosv) = the normal plane and A = the albedo plane rtvSurfaceFrameAsync gives the pixel for
 *   the same rtv_surface (a NULL surface: one with every pointer NULL).
 *   E = ambient, S = 0; for every light in order with cls == RTL_LIT and facing:
 *     qq = q.q
 *     without surface->normals: w = rtdLightAsync's weight (the geometric normal's cosine)
 *     with them: c = (0 - u.q) / sqrt(qq); cosl = c > 0 ? (c < 1 ? c : 1) : 0
 *                w = falloff > 0 ? cosl (falloff / qq) : cosl
 *     E += color w
 *     with a material, where w > 0:
 *       g = q / sqrt(qq) + d / sqrt(d.d); s = (0 - u.g) / sqrt(g.g) clamped as cosl;
 *       shininess_log2 times s = s s;  ws = falloff > 0 ? s (falloff / qq) : s;  S += color ws
 *   rgba = (A E [+ specular S], float(id)), not clamped; an id outside the scene: (background, -1)
 *   and class 3 in every plane, nothing read through it.
 * With no normals, no texture and no material the pixel is rtdLightAsync's, bit for bit. Canonical
 * bit for bit: the device call, the host call and a numpy float32 restatement agree (where the
 * normal comes from a normals table; the fallback normal is rtg's fma arithmetic).
 */
#ifndef SRT_MATERIAL_H
#define SRT_MATERIAL_H

#include <stddef.h>

#include "srt_lighting.h" /* rtd_light, rtd_light_host */
#include "srt_surface.h"  /* rtv_surface */

#if defined(__GNUC__) && defined(RADEONPROML_BUILD)
#define RTP_API __attribute__((visibility("default")))
#else
#define RTP_API
#endif

#define RTP_MAX_SHININESS_LOG2 12 /* the Blinn-Phong exponent is 2^shininess_log2: 1 .. 4096 */

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rtp_material {
    size_t struct_size;  /* sizeof(rtp_material): checked */
    float specular[3];   /* finite */
    int shininess_log2;  /* 0 .. RTP_MAX_SHININESS_LOG2 */
} rtp_material;

/* rtdLightAsync (every rule about the lights, their frames, the one record source, the ordering and
 * the refusals unchanged) on the surface `surface` describes (may be NULL: none; every rule of
 * rtvSurfaceFrameAsync about it unchanged: device tables, texture needs uvs, the texture size limits,
 * unknown flag bits refused, struct_size checked) with `material` (may be NULL: no specular term).
 * One kernel launch on `stream` whatever `count`. A refusal enqueues and builds nothing and names
 * the argument and the field. */
RTP_API int rtpLightSurfaceAsync(srt_device_scene view, const rtd_light* lights, size_t count, const float ambient[3],
                                 const rtv_surface* surface, const rtp_material* material, const float* d_offsets,
                                 const int* d_ids, size_t row_begin, size_t row_count, float* d_rgba,
                                 unsigned char* d_classes, void* stream);

/* The same answer on the host, no device: rtdLightHost's arguments with the surface's host arrays. */
RTP_API int rtpLightSurfaceHost(const char* scene_path, size_t width, size_t height, const rtd_light_host* lights,
                                size_t count, const float ambient[3], const rtv_surface* surface,
                                const rtp_material* material, const float* offsets, const int* ids, size_t row_begin,
                                size_t row_count, float* rgba, unsigned char* classes);

#ifdef __cplusplus
}
#endif

#endif /* SRT_MATERIAL_H */
