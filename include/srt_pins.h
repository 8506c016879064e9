/*
 * srt_pins.h -- pinned sample-offset buffers of libModelRunner.so: an application that keeps a
 * sample pattern for many frames says so, and the whole-frame traces stop classifying it per frame.
 *
 * A family of its own (prefix rtn, its own export macro) beside the reference's 14 ml* entry
 * points (model_runner.h) and the 38 srt* ones (srt_render.h): those two sets are a fixed ABI,
 * and this header adds to neither. Conventions as in srt_render.h: plain pointers and sizes,
 * `stream` is a hipStream_t passed as void*, 0 on success and -1 on failure, the failure text
 * from srtGetLastError() (thread-local).
 *
 * What is pinned. A whole-frame cull trace (srtTraceAsync, srtTraceIdsAsync, srtTraceBatchAsync
 * over rows [0, height)) first classifies its sample offsets per 64 x 16 tile -- the tile's first
 * offset; whether its offsets are all equal, usable, all in [0, 1] -- in a launch of its own in
 * front of the trace: a pass over the whole buffer whose result depends on the buffer's contents
 * and on the prepared W x H only, not on the scene, the camera or the frame. rtnPinOffsetsAsync
 * computes that classification once and the scene keeps it, keyed by the pointer. Every later
 * whole-frame trace frame given that pointer reads the stored classification; a call whose frames
 * are all pinned runs one launch instead of two, a mixed call classifies its unpinned frames only.
 * The frames are the same on every bit: the stored classification is the per-frame launch's own.
 *
 * The contract. The library cannot see a buffer change. While a buffer is pinned the caller does
 * not write it and does not free it; rtnUnpinOffsets comes first. Pinning a pinned pointer again
 * recomputes its classification: the way to announce new contents (written before the call in
 * stream order). srtPrepareAsync at the same size and the rtm* moves keep every pin;
 * srtPrepareAsync at another size drops them all -- later traces classify per frame again, and the
 * caller pins again if it wants.
 *
 * What ignores pins, and stays correct: bands short of the frame, the lds / scalar / bvh variants,
 * SRT_SETUP=frame, SRT_EMPTY_FILL=facts (whose classification launch also stores pixels), and an
 * explicit SRT_FACTS_KERNEL=lean|block (which asks for that classification kernel in the launch). Env
 * SRT_FACTS_PINS=0 (read per call; default 1; anything else is an error) makes every trace ignore
 * them: the same frames, for measurements.
 *
 * A pin also learns, behind the same launch and still without blocking, whether every tile of the
 * buffer has one offset, usable and in [0, 1] -- a pixel-centre or per-tile sample pattern. A call
 * whose RGBA frames are all pinned so, and whose pins' summaries have arrived (the work queued by
 * rtnPinOffsetsAsync has completed), traces with a kernel that keeps no per-pixel position table and
 * fits one more block per compute unit; any other call traces as before. The same bits either way.
 * Env SRT_TRACE_POS=table (read per call; default auto; anything else is an error) never does so.
 */
#ifndef SRT_PINS_H
#define SRT_PINS_H

#include <stddef.h>

#include "srt_render.h" /* srt_device_scene, srtGetLastError */

#if defined(__GNUC__) && defined(RADEONPROML_BUILD)
#define RTN_API __attribute__((visibility("default")))
#else
#define RTN_API
#endif

/* Pinned buffers per device scene. One more is an error: nothing is evicted. */
#define RTN_MAX_PINS 64

#ifdef __cplusplus
extern "C" {
#endif

/* Pins d_offsets (device, height x width x 2 floats at the prepared size): its classification is
 * computed on `stream` into a buffer the scene owns (16 B per tile). A call on the scene for
 * srt_render.h's ordering rule. Errors: a NULL handle or pointer, a scene that is not prepared, a
 * frame size whose traces are not binned, RTN_MAX_PINS pins standing already. */
RTN_API int rtnPinOffsetsAsync(srt_device_scene scene, const float* d_offsets, void* stream);

/* Forgets the pin of d_offsets; a pointer that is not pinned: nothing happens, 0. Queued traces may
 * still read the pin, so the call waits on the host for the scene's work enqueued so far and then
 * frees the pin's buffer. */
RTN_API int rtnUnpinOffsets(srt_device_scene scene, const float* d_offsets);

#ifdef __cplusplus
}
#endif

#endif /* SRT_PINS_H */
