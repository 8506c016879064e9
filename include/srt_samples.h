/*
 * srt_samples.h -- multi-sample frames of libModelRunner.so: S samples per pixel, shaded and
 * resolved to one RGBA pixel on the device (anti-aliased edges, sub-pixel coverage).
 *
 * A family of its own (prefix rts, its own export macro) beside the reference's 14 ml* entry
 * points (model_runner.h), the 38 srt* ones (srt_render.h), the rtq* point queries (srt_query.h)
 * and the rtg* G-buffer outputs (srt_gbuffer.h): those sets are a fixed ABI, and this header adds
 * to none of them. Conventions as in srt_render.h: plain pointers and sizes, `stream` is a
 * hipStream_t passed as void*, 0 on success and -1 on failure, the failure text from
 * srtGetLastError() (thread-local).
 *
 * A sample plane is what a frame's input already is: a sample offset per pixel, and with it the
 * hit id srtTraceIdsAsync stores for the pixel under that offset. The resolve of a pixel with
 * samples s = 0 .. S-1 is canonical (DESIGN.md section 2 "Resolve"):
 *   c_s    the rgb srtShadeAsync stores for (offset_s, id_s); an id outside the scene (-1, the
 *          miss; any sentinel) is a miss -- the background -- and no memory is read through it
 *   rgb    ((c_0 + c_1) + ... + c_{S-1}) / float(S): float32, ascending s, one rounding per add,
 *          one correctly rounded division
 *   alpha  float(hits) / float(S), hits = the samples that hit: the pixel's coverage, not an id
 * For S = 1, and for the same plane passed S times with S = 2 or 4, rgb is bit for bit
 * srtShadeAsync's.
 */
#ifndef SRT_SAMPLES_H
#define SRT_SAMPLES_H

#include <stddef.h>

#include "srt_render.h" /* srt_device_scene, srtGetLastError, SRT_MAX_BATCH */

#if defined(__GNUC__) && defined(RADEONPROML_BUILD)
#define RTS_API __attribute__((visibility("default")))
#else
#define RTS_API
#endif

#define RTS_MAX_SAMPLES 16 /* sample planes per call */

#ifdef __cplusplus
extern "C" {
#endif

/* The band rows [row_begin, row_begin + row_count) of the prepared frame from `samples`
 * (1 .. RTS_MAX_SAMPLES) sample planes. d_offsets and d_ids are host arrays of `samples` device
 * pointers, read during the call; d_offsets[s] (row_count x W x 2 float32), d_ids[s] (row_count x W
 * int32, as srtTraceIdsAsync stores them) and d_rgba (row_count x W x 4 float32) are band-local
 * device buffers, as srtShadeAsync's. Enqueued on `stream`; row_count == 0: nothing is enqueued.
 * Reads the scene's shading table only: builds and reads no cull setup. */
RTS_API int rtsResolveAsync(srt_device_scene scene, const float* const* d_offsets, const int* const* d_ids,
                            size_t samples, size_t row_begin, size_t row_count, float* d_rgba, void* stream);

/* The whole prepared frame: traces the `samples` id planes into the caller's d_ids[s] (H x W int32
 * each; they stay available, for rtgFrameAsync for instance), in batches of at most SRT_MAX_BATCH
 * frames, then resolves them into d_rgba (H x W x 4) -- the bits of the separate calls. variant:
 * SRT_TRACE_*; with SRT_TRACE_CULL and the default environment one build of the shared cull setup
 * serves all the planes. */
RTS_API int rtsRenderAsync(srt_device_scene scene, const float* const* d_offsets, int* const* d_ids, size_t samples,
                           float* d_rgba, int variant, void* stream);

/* rtsResolveAsync's answer on the host, from host arrays, no device, with the library's own
 * canonical math: the band rows [row_begin, row_begin + row_count) of the width x height frame of
 * the scene file. */
RTS_API int rtsResolveHost(const char* scene_path, size_t width, size_t height, const float* const* offsets,
                           const int* const* ids, size_t samples, size_t row_begin, size_t row_count, float* rgba);

#ifdef __cplusplus
}
#endif

#endif /* SRT_SAMPLES_H */
