/*
 * srt_visibility.h -- sampled visibility of libModelRunner.so: ambient occlusion and area-light
 * soft shadows, and the rays behind them. For each element -- an image position (fx, fy) of the
 * prepared frame and a triangle id, srt_gbuffer.h's definition -- a generator produces S rays that
 * start at the surface point. The rays are either exported in srt_rays.h's 8-float format, or traced
 * through the scene's world-space tree in the same launch, which returns how many are unoccluded.
 *
 * A family of its own (prefix rta, its own export macro) beside the reference's 14 ml* entry points
 * (model_runner.h), the 38 srt* ones (srt_render.h) and the other families: this header adds to no
 * other header's ABI. Conventions as in srt_render.h: plain pointers and sizes, `stream` is a
 * hipStream_t passed as void*, 0 on success and -1 on failure, the failure text from
 * srtGetLastError() (thread-local).
 *
 * The answer is canonical, bit for bit (DESIGN.md section 2 "Visibility"), in Shadow's convention:
 * float32, separate multiply and add, the order written, IEEE divide and square root.
 *   1. id outside [0, n): no surface. Every ray is eight zeros (d = 0 misses), visible = S; nothing
 *      is read through the id.
 *   2. t = the depth of (fx, fy, id) (the G-buffer's), d and P = eye + t d the position's direction
 *      and surface point, N the triangle's shading normal, nn = dotp(N, N), nd = dotp(N, d).
 *   3. Unless t and nn are finite and nn > 0 the rays are zero rays as in 1.
 *   4. n = N / sqrt(nn), negated if nd > 0: the unit normal towards the eye.
 *   5. The rays (P, tmin, dir, tmax), by kind:
 *      RTA_HEMISPHERE  sample (lx, ly, lz) around n in the branch-free orthonormal basis
 *                      sg = n.z < 0 ? -1 : 1, a = -1 / (sg + n.z), b = (n.x n.y) a,
 *                      T = (1 + ((sg n.x) n.x) a, sg b, (-sg) n.x), B = (b, sg + (n.y n.y) a, -n.y);
 *                      with a rotation (c, s): lx' = lx c - ly s, ly' = lx s + ly c;
 *                      dir = (lx' T + ly' B) + lz n.
 *      RTA_AREA        sample (a, b) on the parallelogram: L = (corner + a eu) + b ev, dir = L - P, so
 *                      t is in units of dir and the range is typically [2^-10, 1 - 2^-10]. No facing
 *                      rule: pure geometric visibility; the caller's clamped cosine removes
 *                      back-facing light.
 *      RTA_MIRROR      S = 1, export only: dn = dotp(d, n), dir = d - (2 dn) n.
 *   6. visible = the number of the S rays whose srt_rays.h occlusion byte is 0 (uint8);
 *      fraction = float(visible) / float(S).
 * Every counted ray is srt_rays.h's canonical answer, so the fused result does not depend on the tree.
 *
 * The range alone keeps a ray off its own surface. Measured on the Cornell box at 48 x 32 with a
 * hemisphere of S = 8 and tmax = 0.5: with tmin = 0, 408 of the 1 024 surface pixels come out fully
 * occluded; with tmin = 2^-10, none do.
 *
 * Exported rays are sample-major: the ray of sample s for element e sits at (s count + e) 8 floats
 * (count = the elements of the call: row_count x W for a frame call), the plane layout of
 * multi-sample offsets. Neighbouring rays of a follow-on rtrOccludedAsync then share one sample
 * direction.
 *
 * The device calls need srtPrepareAsync (the elements live on the prepared frame) and are calls on
 * the scene for srt_render.h's ordering rule. The visibility calls build or rebuild the ray tree on
 * their own stream exactly as the rtr calls do; after the first build nothing is allocated and
 * nothing waits for the device. Env SRT_RAYS=brute is honoured as by rtr. A zero count or row_count,
 * or a call with no output plane, enqueues nothing.
 */
#ifndef SRT_VISIBILITY_H
#define SRT_VISIBILITY_H

#include <stddef.h>

#include "srt_render.h" /* srt_device_scene, srtGetLastError */

#if defined(__GNUC__) && defined(RADEONPROML_BUILD)
#define RTA_API __attribute__((visibility("default")))
#else
#define RTA_API
#endif

#define RTA_HEMISPHERE 0
#define RTA_AREA 1
#define RTA_MIRROR 2
#define RTA_MAX_SAMPLES 64
#define RTA_ROTATIONS 16 /* entries of d_rotations */

#ifdef __cplusplus
extern "C" {
#endif

/* The generator. struct_size = sizeof(rta_generator). d_samples: samples x 3 floats (lx, ly, lz) for
 * RTA_HEMISPHERE, samples x 2 floats (a, b) for RTA_AREA, unused (may be NULL) for RTA_MIRROR.
 * d_rotations: RTA_HEMISPHERE only, NULL or 16 x 2 floats (c, s); a frame call indexes it by
 * ((y & 3) << 2) | (x & 3) with y the absolute frame row, a points call by i & 15. corner, eu, ev:
 * RTA_AREA's parallelogram. Device pointers for the device calls, host pointers for the Host forms. */
typedef struct rta_generator {
    size_t struct_size;
    int kind;
    unsigned samples; /* S, 1 .. RTA_MAX_SAMPLES */
    const float* d_samples;
    const float* d_rotations;
    float corner[3], eu[3], ev[3];
    float tmin, tmax;
} rta_generator;

/* The planes of a visibility call, one value per element; a NULL plane is not written. */
typedef struct rta_outputs {
    size_t struct_size;
    unsigned char* visible; /* 0 .. S */
    float* fraction;        /* float(visible) / float(S) */
} rta_outputs;

/* Frame calls: the band rows [row_begin, row_begin + row_count) of the prepared frame, d_offsets
 * (row_count x W x 2) its sample offsets and d_ids (row_count x W) its ids, band-local. Points
 * calls: count positions (count x 2) with their ids. d_rays: samples x elements x 8 floats, 16-byte
 * aligned. RTA_MIRROR is refused by the visibility calls. */
RTA_API int rtaVisibilityFrameAsync(srt_device_scene scene, const float* d_offsets, const int* d_ids, size_t row_begin,
                                    size_t row_count, const rta_generator* gen, const rta_outputs* outputs,
                                    void* stream);
RTA_API int rtaVisibilityPointsAsync(srt_device_scene scene, const float* d_positions, const int* d_ids, size_t count,
                                     const rta_generator* gen, const rta_outputs* outputs, void* stream);
RTA_API int rtaRaysFrameAsync(srt_device_scene scene, const float* d_offsets, const int* d_ids, size_t row_begin,
                              size_t row_count, const rta_generator* gen, float* d_rays, void* stream);
RTA_API int rtaRaysPointsAsync(srt_device_scene scene, const float* d_positions, const int* d_ids, size_t count,
                               const rta_generator* gen, float* d_rays, void* stream);

/* The same answers on the host, no device: the library's own canonical math and rtrOccludedHost's
 * brute force. Points elements on the scene file's width x height frame. */
RTA_API int rtaVisibilityHost(const char* scene_path, size_t width, size_t height, const float* positions,
                              const int* ids, size_t count, const rta_generator* gen, const rta_outputs* outputs);
RTA_API int rtaRaysHost(const char* scene_path, size_t width, size_t height, const float* positions, const int* ids,
                        size_t count, const rta_generator* gen, float* rays);

#ifdef __cplusplus
}
#endif

#endif /* SRT_VISIBILITY_H */
