/*
 * srt_radiance.h -- sampled radiance of libModelRunner.so: one bounce of indirect light. For each
 * element -- an image position of the prepared frame and a triangle id, srt_visibility.h's
 * definition -- a generator's S rays leave the surface point, each is walked to its closest hit, the
 * hit is shaded under the lights, and the S colours are averaged: colour bleeding, sky light that
 * carries the background's colour, a mirror bounce that ends in a colour. One kernel launch; a ray
 * lives in registers and LDS from its generation to the resolved element.
 *
 * A family of its own (prefix rti, its own export macro) beside the reference's 14 ml* entry points
 * (model_runner.h), the 38 srt* ones (srt_render.h) and the other families: this header adds to no
 * other header's ABI. Conventions as in srt_visibility.h and srt_hits.h: plain pointers and sizes,
 * `stream` is a hipStream_t passed as void*, 0 on success and -1 on failure, the failure text from
 * srtGetLastError() (thread-local).
 *
 * The answer is the composition's, bit for bit (DESIGN.md section 2 "Radiance"): float32, separate
 * multiply and add, the order written, IEEE divide. Per element:
 *   1. r_0 ... r_(S-1) are the rays rtaRays* exports for the element and the generator, zero rays
 *      included. RTA_HEMISPHERE with S = 1 ... 64 and RTA_MIRROR with S = 1 are taken; RTA_AREA is
 *      refused (its rays aim at a light, not at surfaces).
 *   2. (id_s, t_s) = rtrClosestAsync's answer for r_s on the same scene.
 *   3. (c_s, a_s) = rthLightHitsAsync's unblended answer for (r_s, id_s, t_s) on the same scene under
 *      the call's lights and ambient colour: a miss gives the background, a zero ray c = 0.
 *   4. sum = (+0, +0, +0); for s = 0 ... S - 1 ascending: sum_k = sum_k + c_s,k. hits = the number of
 *      samples with a_s >= 0. The order is part of the answer.
 *   5. m_k = sum_k / float(S); with modulate m_k = albedo_k m_k, albedo the shading-table row of the
 *      element's own id.
 *   6. Stored: an element on a surface (srt_visibility.h steps 1 to 3) (m, float(hits) / float(S));
 *      any other (0, 0, 0, 0), nothing read through its id. With a blend an element not on a surface
 *      stores the base element's four floats unchanged, any other (base.rgb + weight m, base.a),
 *      multiply then add.
 * Canonical bit for bit: the device calls, the host call and the composition of the three families'
 * calls with a float32 sum in ascending s agree, with the tree or with SRT_RAYS=brute.
 */
#ifndef SRT_RADIANCE_H
#define SRT_RADIANCE_H

#include <stddef.h>

#include "srt_hits.h"       /* rth_blend; srt_lighting.h: rtd_light, rtd_light_host */
#include "srt_visibility.h" /* rta_generator */

#if defined(__GNUC__) && defined(RADEONPROML_BUILD)
#define RTI_API __attribute__((visibility("default")))
#else
#define RTI_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rti_options {
    size_t struct_size;     /* sizeof(rti_options): checked */
    int modulate;           /* non-zero: the mean is multiplied by the element's own albedo */
    const rth_blend* blend; /* NULL: store; else add onto blend->d_base (elements x 4, 16-byte aligned) */
} rti_options;

/* Frame call: the band rows [row_begin, row_begin + row_count) of the prepared frame, d_offsets
 * (row_count x W x 2) its sample offsets and d_ids (row_count x W) its ids, band-local. Points call:
 * `elements` positions (elements x 2) with their ids. At most 2^31 - 1 elements per call. d_rgba:
 * elements x 4 floats, 16-byte aligned. options NULL: no modulate, no blend. d_rgba == blend->d_base
 * (the same pointer) is allowed, any other overlap of the buffers is not.
 * `scene` needs srtPrepareAsync, as the rta calls do. The lights obey every rule of rtdLightAsync and
 * are refused in its words. The ray tree is built or rebuilt on `stream` exactly as the rtr and rta
 * calls do it; SRT_RAYS=brute is honoured. After the first build and the first use of each light frame:
 * one kernel launch per call whatever `count` and S, no allocation, no host synchronisation, no device
 * scratch. Zero elements or rows enqueue nothing. A refused call enqueues and builds nothing. The call
 * counts as a call on `scene` and on every light frame for srt_render.h's ordering rule. */
RTI_API int rtiRadianceFrameAsync(srt_device_scene scene, const rtd_light* lights, size_t count, const float ambient[3],
                                  const float* d_offsets, const int* d_ids, size_t row_begin, size_t row_count,
                                  const rta_generator* gen, const rti_options* options, float* d_rgba, void* stream);
RTI_API int rtiRadiancePointsAsync(srt_device_scene scene, const rtd_light* lights, size_t count, const float ambient[3],
                                   const float* d_positions, const int* d_ids, size_t elements,
                                   const rta_generator* gen, const rti_options* options, float* d_rgba, void* stream);

/* The same answer on the host, no device: the composition of rtaRaysHost, rtrClosestHost and
 * rthLightHitsHost and the sum of step 4. Points elements on the scene file's width x height frame;
 * every light holds scene_path's triangles; gen's and the blend's pointers are host arrays, and
 * rgba == blend->d_base is allowed. */
RTI_API int rtiRadianceHost(const char* scene_path, size_t width, size_t height, const rtd_light_host* lights,
                            size_t count, const float ambient[3], const float* positions, const int* ids,
                            size_t elements, const rta_generator* gen, const rti_options* options, float* rgba);

#ifdef __cplusplus
}
#endif

#endif /* SRT_RADIANCE_H */
