/*
 * srt_hits.h -- lit ray hits of libModelRunner.so: what the hit of a caller's ray looks like under
 * the scene's lights, one kernel launch whatever the number of lights.
 *
 * A family of its own (prefix rth, its own export macro) beside the reference's 14 ml* entry
 * points (model_runner.h) and the 38 srt* ones (srt_render.h): those two sets are a fixed ABI,
 * and this header adds to neither. Conventions as in srt_lighting.h: plain pointers and sizes,
 * `stream` is a hipStream_t passed as void*, 0 on success and -1 on failure, the failure text from
 * srtGetLastError() (thread-local).
 *
 * rtdLightAsync (srt_lighting.h) lights the pixels of a prepared frame; these calls light the hits
 * of rays -- a mirror bounce, a probe ray, a ray from another vantage point -- given as
 * (ray, id, t): the ray in srt_rays.h's format, the id and the t as rtrClosestAsync returns them.
 * The lights are rtdLightAsync's. Per element (DESIGN.md section 2 "Hits"; float32, no fma, in this
 * order):
 *   absent  iff dx == 0 and dy == 0 and dz == 0 (the zero ray rtaRays* stores for "no ray here")
 *   surface iff not absent, 0 <= id < n, t finite and o, d finite; else nothing is read through id
 *   absent: c = (0, 0, 0), a = -1; no surface: c = the background, a = -1; class bytes 3
 *   surface: P = o + t d; N, albedo: the triangle's shading-table row; nn = N.N, nd = N.d
 *     E = ambient; for every light in the order given, srt_lighting.h's rule with this P, N, nd, id:
 *       q = P - origin; cls = the light's class of P (its frame's closest hit at q's projection
 *       against id and the bias' threshold); nl = N.q; the light contributes iff cls == RTL_LIT and
 *       nl, nd are both < 0 or both > 0 (the light and the ray's origin on one side of the triangle)
 *       E += color w, w as srt_lighting.h's
 *     c = albedo E (not clamped), a = float(id)
 *   stored: (c, a); with a blend an absent element stores the base element's four floats
 *   unchanged, any other (base.rgb + weight c, base.a), multiply then add.
 * The range (tmin, tmax) of a ray is not read. For o = the eye, d = (base + fx du) + fy dv, t the
 * G-buffer depth and id the traced id the answer is rtdLightAsync's bit for bit.
 * Canonical bit for bit: the device call, the host call and a numpy float32 restatement agree.
 */
#ifndef SRT_HITS_H
#define SRT_HITS_H

#include <stddef.h>

#include "srt_lighting.h" /* rtd_light, rtd_light_host; srt_render.h: srt_device_scene */

#if defined(__GNUC__) && defined(RADEONPROML_BUILD)
#define RTH_API __attribute__((visibility("default")))
#else
#define RTH_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rth_blend {
    size_t struct_size;  /* sizeof(rth_blend): checked */
    const float* d_base; /* elements x 4 floats, 16-byte aligned (the host call: a host array); non-NULL */
    float weight[3];     /* finite */
} rth_blend;

/* The lit RGBA of `elements` (at most 2^31 - 1) ray hits of `scene` under `count` lights and the
 * ambient colour. d_rays: elements x 8 floats (ox, oy, oz, tmin, dx, dy, dz, tmax), 16-byte aligned;
 * d_ids, d_t: elements each; d_rgba: elements x 4, 16-byte aligned; d_classes (count x elements
 * bytes, light-major, may be NULL): plane l is light l's class of every element. blend NULL: the
 * element is stored; else it is added onto blend->d_base as above. d_rgba == blend->d_base (the same
 * pointer) is allowed, any other overlap of the buffers is not.
 * `scene` needs no srtPrepareAsync: only its triangle count, its shading table and its background
 * are read. The lights obey every rule of rtdLightAsync (prepared, on the scene's device, of the
 * scene's triangle count, at most RTD_MAX_LIGHTS lights and RTD_MAX_FRAMES frames of one record
 * source, finite colour, falloff >= 0, bias >= 0) and are refused in its words. One kernel launch
 * on `stream` whatever `count`; the first use of a light frame after its prepare builds its shared
 * cull setup on it; no allocation after that, no host synchronisation. elements == 0: nothing is
 * enqueued. The call counts as a call on `scene` and on every light frame for srt_render.h's
 * ordering rule. A refused call enqueues and builds nothing. */
RTH_API int rthLightHitsAsync(srt_device_scene scene, const rtd_light* lights, size_t count, const float ambient[3],
                              const float* d_rays, const int* d_ids, const float* d_t, size_t elements,
                              const rth_blend* blend /* NULL: store */, float* d_rgba,
                              unsigned char* d_classes /* may be NULL */, void* stream);

/* The same answer on the host, no device: brute force with the library's own canonical math. Every
 * light holds scene_path's triangles; classes may be NULL; blend->d_base is a host array, and
 * rgba == blend->d_base is allowed. */
RTH_API int rthLightHitsHost(const char* scene_path, const rtd_light_host* lights, size_t count, const float ambient[3],
                             const float* rays, const int* ids, const float* t, size_t elements,
                             const rth_blend* blend, float* rgba, unsigned char* classes);

#ifdef __cplusplus
}
#endif

#endif /* SRT_HITS_H */
