"""ctypes binding of libModelRunner.so (include/model_runner.h + include/srt_render.h + include/srt_query.h +
include/srt_gbuffer.h + include/srt_samples.h and the later families' headers, include/srt_rays.h the last).

The shared library is built in-tree by ``make`` (or ``__graft_entry__.build()``) into
``simpleraytracer_amd/lib/libModelRunner.so``. There is no fallback: importing the renderer
without the library raises immediately.
"""
from __future__ import annotations

import ctypes
import os
from pathlib import Path

PACKAGE_DIR = Path(__file__).resolve().parent
LIB_PATH = PACKAGE_DIR / "lib" / "libModelRunner.so"
# Diagnostic runs only (tools/diag_cull.py): SRT_LIB points at the `make diag` build.
if os.environ.get("SRT_LIB"):
    LIB_PATH = Path(os.environ["SRT_LIB"])

ML_OK = 0
ML_FAIL = 1
ML_FLOAT32 = 0
ML_FLOAT16 = 1

SRT_SCENE_TRIANGLE = 0
SRT_SCENE_CORNELL = 1
SRT_SCENE_SOUP = 2
SRT_TRACE_LDS = 0
SRT_TRACE_SCALAR = 1
SRT_TRACE_CULL = 2
SRT_TRACE_BVH = 3
SRT_MAX_BATCH = 8  # include/srt_render.h: frames per srtTraceBatchAsync call
SRT_ROWS_INTERLEAVED = 0
SRT_ROWS_CONTIGUOUS = 1
SRT_ROWS_ROTATED = 2  # contiguous bands rotated per compositor (all-to-all)
SRT_EXCHANGE_ALLTOALL = 0
SRT_EXCHANGE_ROTATING = 1
SRT_EXCHANGE_ROOT = 2
SRT_EXCHANGE_SHARE = 3
SRT_SPLIT_BANDS = 0
SRT_SPLIT_FRAMES = 1
SRT_ENGINE_RCCL_SELF = 1  # srt_engine_options.flags
SRT_TILE_ROWS = 16  # include/srt_render.h: rows per tile row (interleaved bands deal these)
RTS_MAX_SAMPLES = 16  # include/srt_samples.h: sample planes per rtsResolveAsync / rtsRenderAsync call
RTK_MAX_LAYERS = 8  # include/srt_layers.h: layers per rtkLayersAsync / rtkFrameAsync / rtkCompositeAsync call
RTM_REORDER = 0     # include/srt_motion.h: rebuild the spatial order under the new pose
RTM_KEEP_ORDER = 1  # keep the standing order
RTR_RAY_FLOATS = 8     # include/srt_rays.h: (ox, oy, oz, tmin, dx, dy, dz, tmax)
RTR_BOX_CLAUSE = 0     # the definition
RTR_NO_BOX_CLAUSE = 1  # host only: the edge test and the range alone


class ImageInfo(ctypes.Structure):
    """``ml_image_info`` (model_runner.h:100-106): 32 bytes, dtype at 0, width at 8."""

    _fields_ = [
        ("dtype", ctypes.c_int),
        ("width", ctypes.c_size_t),
        ("height", ctypes.c_size_t),
        ("channels", ctypes.c_size_t),
    ]

    def as_tuple(self):
        return (self.dtype, self.width, self.height, self.channels)


class ModelParams(ctypes.Structure):
    """``ml_model_params`` (model_runner.h:53-60): 24 bytes."""

    _fields_ = [
        ("model_path", ctypes.c_char_p),
        ("input_node", ctypes.c_char_p),
        ("output_node", ctypes.c_char_p),
    ]


class EngineOptions(ctypes.Structure):
    """``srt_engine_options`` (include/srt_render.h)."""

    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("variant", ctypes.c_int),
        ("queues", ctypes.c_size_t),
        ("batch", ctypes.c_size_t),
        ("rows", ctypes.c_int),
        ("exchange", ctypes.c_int),
        ("split", ctypes.c_int),
        ("simulate", ctypes.c_int),
        ("launch", ctypes.c_size_t),
        ("flags", ctypes.c_int),
        ("share", ctypes.c_size_t),
        ("own_rows", ctypes.c_size_t),
    ]


class RtgOutputs(ctypes.Structure):
    """``rtg_outputs`` (include/srt_gbuffer.h): the planes as raw addresses, 0 = not written."""

    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("depth", ctypes.c_void_p),
        ("bary", ctypes.c_void_p),
        ("normal", ctypes.c_void_p),
        ("albedo", ctypes.c_void_p),
    ]


RTA_HEMISPHERE = 0    # include/srt_visibility.h: rta_generator.kind
RTA_AREA = 1
RTA_MIRROR = 2
RTA_MAX_SAMPLES = 64
RTA_ROTATIONS = 16


class RtaGenerator(ctypes.Structure):
    """``rta_generator`` (include/srt_visibility.h): the tables as raw addresses, 0 = none."""

    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("kind", ctypes.c_int),
        ("samples", ctypes.c_uint),
        ("d_samples", ctypes.c_void_p),
        ("d_rotations", ctypes.c_void_p),
        ("corner", ctypes.c_float * 3),
        ("eu", ctypes.c_float * 3),
        ("ev", ctypes.c_float * 3),
        ("tmin", ctypes.c_float),
        ("tmax", ctypes.c_float),
    ]


class RtaOutputs(ctypes.Structure):
    """``rta_outputs`` (include/srt_visibility.h): the planes as raw addresses, 0 = not written."""

    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("visible", ctypes.c_void_p),
        ("fraction", ctypes.c_void_p),
    ]


RTV_MAX_CHANNELS = 4     # include/srt_surface.h: floats per corner of a table
RTV_MAX_TEXTURE = 16384  # texels per side of a texture
RTV_WRAP_CLAMP = 1       # rtv_surface.flags
RTV_FILTER_NEAREST = 2
RTV_MODULATE = 4


class RtvSurface(ctypes.Structure):
    """``rtv_surface`` (include/srt_surface.h): the tables as raw addresses, 0 = none."""

    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("normals", ctypes.c_void_p),
        ("uvs", ctypes.c_void_p),
        ("texture", ctypes.c_void_p),
        ("tex_width", ctypes.c_size_t),
        ("tex_height", ctypes.c_size_t),
        ("flags", ctypes.c_uint),
    ]


class RtvOutputs(ctypes.Structure):
    """``rtv_outputs`` (include/srt_surface.h): the planes as raw addresses, 0 = not written."""

    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("normal", ctypes.c_void_p),
        ("albedo", ctypes.c_void_p),
        ("rgba", ctypes.c_void_p),
        ("uv", ctypes.c_void_p),
    ]


RTD_MAX_LIGHTS = 8   # include/srt_lighting.h: lights per rtdLightAsync / rtdLightHost call
RTD_MAX_FRAMES = 16  # light frames per call: 1 per spot light, 6 per point light


class RtdLight(ctypes.Structure):
    """``rtd_light`` (include/srt_lighting.h): exactly one of spot / point is non-NULL."""

    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("spot", ctypes.c_void_p),
        ("point", ctypes.c_void_p),
        ("color", ctypes.c_float * 3),
        ("falloff", ctypes.c_float),
        ("bias", ctypes.c_float),
    ]


class RtdLightHost(ctypes.Structure):
    """``rtd_light_host`` (include/srt_lighting.h): kind 0 spot (camera10, width, height), 1 point
    (origin, face_size)."""

    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("kind", ctypes.c_int),
        ("camera10", ctypes.c_float * 10),
        ("width", ctypes.c_size_t),
        ("height", ctypes.c_size_t),
        ("origin", ctypes.c_float * 3),
        ("face_size", ctypes.c_size_t),
        ("color", ctypes.c_float * 3),
        ("falloff", ctypes.c_float),
        ("bias", ctypes.c_float),
    ]


class RthBlend(ctypes.Structure):
    """``rth_blend`` (include/srt_hits.h): the base picture as a raw address and the weight."""

    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("d_base", ctypes.c_void_p),
        ("weight", ctypes.c_float * 3),
    ]


class RtiOptions(ctypes.Structure):
    """``rti_options`` (include/srt_radiance.h): modulate and the blend (an RthBlend's address, or None)."""

    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("modulate", ctypes.c_int),
        ("blend", ctypes.POINTER(RthBlend)),
    ]


RTP_MAX_SHININESS_LOG2 = 12  # include/srt_material.h: the Blinn-Phong exponent is 2^shininess_log2


class RtpMaterial(ctypes.Structure):
    """``rtp_material`` (include/srt_material.h)."""

    _fields_ = [
        ("struct_size", ctypes.c_size_t),
        ("specular", ctypes.c_float * 3),
        ("shininess_log2", ctypes.c_int),
    ]


_SZ = ctypes.c_size_t
_PSZ = ctypes.POINTER(ctypes.c_size_t)
_PD = ctypes.POINTER(ctypes.c_double)
_PVP = ctypes.POINTER(ctypes.c_void_p)

# name -> (restype, argtypes)
_SIGNATURES = {
    "mlCreateContext": (ctypes.c_void_p, []),
    "mlGetContextError": (ctypes.c_char_p, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]),
    "mlReleaseContext": (None, [ctypes.c_void_p]),
    "mlCreateImage": (ctypes.c_void_p, [ctypes.c_void_p, ctypes.POINTER(ImageInfo)]),
    "mlGetImageInfo": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ImageInfo)]),
    "mlMapImage": (ctypes.c_void_p, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]),
    "mlUnmapImage": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "mlReleaseImage": (None, [ctypes.c_void_p]),
    "mlCreateModel": (ctypes.c_void_p, [ctypes.c_void_p, ctypes.POINTER(ModelParams)]),
    "mlGetModelError": (ctypes.c_char_p, [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_size_t]),
    "mlGetModelInfo": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ImageInfo), ctypes.POINTER(ImageInfo)]),
    "mlSetModelInputInfo": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ImageInfo)]),
    "mlInfer": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "mlReleaseModel": (None, [ctypes.c_void_p]),
    "srtGetLastError": (ctypes.c_char_p, []),
    "srtWriteScene": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int, ctypes.c_ulonglong, ctypes.c_ulonglong,
                                     ctypes.c_float]),
    "srtSceneTriangles": (ctypes.c_int, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_ulonglong)]),
    "srtReadScene": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_ulonglong, ctypes.POINTER(ctypes.c_ulonglong),
                                    ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                    ctypes.POINTER(ctypes.c_uint)]),
    "srtConvertScene": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_int]),
    "srtSceneFrame": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_size_t,
                                     ctypes.POINTER(ctypes.c_float)]),
    "srtDeviceSceneCreate": (ctypes.c_void_p, [ctypes.c_char_p, ctypes.c_int]),
    "srtDeviceSceneRelease": (None, [ctypes.c_void_p]),
    "srtDeviceSceneTriangles": (ctypes.c_ulonglong, [ctypes.c_void_p]),
    "srtDeviceSceneOrder": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_ulonglong,
                                           ctypes.POINTER(ctypes.c_double)]),
    "srtPrepareAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]),
    "srtTraceAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                     ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]),
    "srtTraceIdsAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t,
                                        ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]),
    "srtTraceBatchAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p),
                                          ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_size_t,
                                          ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]),
    "rtnPinOffsetsAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rtnUnpinOffsets": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "srtShadeAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]),
    "srtShadeBandsAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                          ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]),
    "srtSetStageTiming": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int]),
    "srtTakeStageTimes": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint), ctypes.POINTER(ctypes.c_double),
                                         ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]),
    "srtEngineUniqueId": (ctypes.c_int, [ctypes.c_void_p]),
    "srtEngineCreate": (ctypes.c_void_p, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_int), _SZ, _SZ, _SZ,
                                          ctypes.POINTER(EngineOptions)]),
    "srtEngineCreateRank": (ctypes.c_void_p, [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                              _SZ, _SZ, ctypes.POINTER(EngineOptions)]),
    "srtEngineRelease": (None, [ctypes.c_void_p]),
    "srtEngineSetInputs": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, _SZ]),
    "srtEngineRun": (ctypes.c_int, [ctypes.c_void_p, _SZ]),
    "srtEngineVerify": (ctypes.c_int, [ctypes.c_void_p, _PSZ, _PSZ]),
    "srtEngineReadFrame": (ctypes.c_int, [ctypes.c_void_p, _SZ, ctypes.c_void_p]),
    "srtEngineStageTimes": (ctypes.c_int, [ctypes.c_void_p, _SZ, _SZ, ctypes.POINTER(ctypes.c_uint), _PD, _PD, _PD]),
    "srtEngineStageTimesBatch": (ctypes.c_int, [ctypes.c_void_p, _SZ, _SZ, _SZ, ctypes.POINTER(ctypes.c_uint), _PD, _PD,
                                                _PD]),
    "srtEnginePoolSelfTest": (ctypes.c_int, [_SZ, _SZ, ctypes.c_int, ctypes.c_double, _PD, ctypes.POINTER(ctypes.c_int),
                                             ctypes.c_char_p, _SZ]),
    "srtShareAuto": (_SZ, [_SZ, _SZ]),
    "srtRotateOwnRows": (_SZ, [_SZ]),
    "srtRotateSplitForLink": (_SZ, [_SZ, _SZ, ctypes.c_double, ctypes.c_double, ctypes.c_double]),
    "srtEngineSplit": (ctypes.c_int, [ctypes.c_void_p, _PSZ, _PSZ, _PD, _PD, ctypes.POINTER(ctypes.c_int)]),
    "srtEngineInfo": (ctypes.c_int, [ctypes.c_void_p, _PSZ, _PSZ, _PSZ, _PSZ, ctypes.POINTER(ctypes.c_int), _PD]),
    "srtExchangeHost": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), _SZ, _SZ, _SZ, ctypes.c_int, ctypes.c_int, _SZ,
                                       _SZ, ctypes.POINTER(ctypes.c_void_p), _PSZ, _PSZ]),
    "srtEngineExchangeStats": (ctypes.c_int, [ctypes.c_void_p, _SZ, _PSZ, _PD, _PD]),
    "srtExchangeHostShare": (ctypes.c_int, [ctypes.POINTER(ctypes.c_void_p), _SZ, _SZ, _SZ, _SZ, _SZ, _SZ,
                                            ctypes.POINTER(ctypes.c_void_p), _PSZ, _PSZ]),
    "srtScreenBoxHost": (ctypes.c_int, [ctypes.POINTER(ctypes.c_float), ctypes.c_int, ctypes.POINTER(ctypes.c_float)]),
    # include/srt_query.h: point queries
    "rtqQueryAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, _SZ, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_void_p]),
    "rtqQueryHost": (ctypes.c_int, [ctypes.c_char_p, _SZ, _SZ, ctypes.c_void_p, _SZ, ctypes.c_void_p, ctypes.c_void_p]),
    "rtqTileHost": (ctypes.c_int, [_SZ, _SZ, ctypes.c_float, ctypes.c_float, ctypes.POINTER(ctypes.c_int),
                                   ctypes.POINTER(ctypes.c_int)]),
    # include/srt_gbuffer.h: G-buffer outputs
    "rtgFrameAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _SZ, _SZ,
                                     ctypes.POINTER(RtgOutputs), ctypes.c_void_p]),
    "rtgPointsAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _SZ,
                                      ctypes.POINTER(RtgOutputs), ctypes.c_void_p]),
    "rtgPointsHost": (ctypes.c_int, [ctypes.c_char_p, _SZ, _SZ, ctypes.c_void_p, ctypes.c_void_p, _SZ,
                                     ctypes.POINTER(RtgOutputs)]),
    # include/srt_samples.h: multi-sample frames (the plane arrays: ctypes.c_void_p arrays, or None)
    "rtsResolveAsync": (ctypes.c_int, [ctypes.c_void_p, _PVP, _PVP, _SZ, _SZ, _SZ, ctypes.c_void_p, ctypes.c_void_p]),
    "rtsRenderAsync": (ctypes.c_int, [ctypes.c_void_p, _PVP, _PVP, _SZ, ctypes.c_void_p, ctypes.c_int,
                                      ctypes.c_void_p]),
    "rtsResolveHost": (ctypes.c_int, [ctypes.c_char_p, _SZ, _SZ, _PVP, _PVP, _SZ, _SZ, _SZ, ctypes.c_void_p]),
    # include/srt_light.h: spot-light shadow masks (camera10: a ctypes float array, or None)
    "rtlSceneCreate": (ctypes.c_void_p, [ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]),
    "rtlShadowAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _SZ, _SZ,
                                      ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, ctypes.c_void_p]),
    "rtlShadowHost": (ctypes.c_int, [ctypes.c_char_p, _SZ, _SZ, ctypes.POINTER(ctypes.c_float), _SZ, _SZ,
                                     ctypes.c_void_p, ctypes.c_void_p, _SZ, _SZ, ctypes.c_float, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_float]),
    "rtlProjectionHost": (ctypes.c_int, [ctypes.POINTER(ctypes.c_float), _SZ, _SZ, ctypes.POINTER(ctypes.c_float)]),
    # include/srt_omni.h: omni-light shadow masks (origin, camera10, q: ctypes float arrays)
    "rtoLightCreate": (ctypes.c_void_p, [ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_float)]),
    "rtoLightRelease": (None, [ctypes.c_void_p]),
    "rtoLightPrepareAsync": (ctypes.c_int, [ctypes.c_void_p, _SZ, ctypes.c_void_p]),
    "rtoLightFace": (ctypes.c_void_p, [ctypes.c_void_p, ctypes.c_int]),
    "rtoShadowAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _SZ, _SZ,
                                      ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float,
                                      ctypes.c_void_p]),
    "rtoShadowHost": (ctypes.c_int, [ctypes.c_char_p, _SZ, _SZ, ctypes.POINTER(ctypes.c_float), _SZ, ctypes.c_void_p,
                                     ctypes.c_void_p, _SZ, _SZ, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_float]),
    "rtoFaceCameraHost": (ctypes.c_int, [ctypes.POINTER(ctypes.c_float), ctypes.c_int, ctypes.POINTER(ctypes.c_float)]),
    "rtoFaceOfHost": (ctypes.c_int, [ctypes.POINTER(ctypes.c_float)]),
    # include/srt_lighting.h: direct lighting (lights: an array of RtdLight / RtdLightHost, or None; ambient: 3 floats)
    "rtdLightAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, _SZ, ctypes.POINTER(ctypes.c_float),
                                     ctypes.c_void_p, ctypes.c_void_p, _SZ, _SZ, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_void_p]),
    "rtdLightHost": (ctypes.c_int, [ctypes.c_char_p, _SZ, _SZ, ctypes.c_void_p, _SZ, ctypes.POINTER(ctypes.c_float),
                                    ctypes.c_void_p, ctypes.c_void_p, _SZ, _SZ, ctypes.c_void_p, ctypes.c_void_p]),
    # include/srt_layers.h: depth layers and their over-composite
    "rtkLayersAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, _SZ, _SZ, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_void_p, ctypes.c_void_p]),
    "rtkFrameAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, _SZ, _SZ, _SZ, ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.c_void_p, ctypes.c_void_p]),
    "rtkCompositeAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _SZ, ctypes.c_void_p, _SZ, _SZ,
                                         ctypes.c_void_p, ctypes.c_void_p]),
    "rtkLayersHost": (ctypes.c_int, [ctypes.c_char_p, _SZ, _SZ, ctypes.c_void_p, _SZ, _SZ, ctypes.c_void_p,
                                     ctypes.c_void_p]),
    "rtkCompositeHost": (ctypes.c_int, [ctypes.c_char_p, _SZ, _SZ, ctypes.c_void_p, ctypes.c_void_p, _SZ, ctypes.c_void_p,
                                        _SZ, _SZ, ctypes.c_void_p]),
    # include/srt_motion.h: dynamic scenes (camera10, origin3: ctypes float arrays; d_vertices: a device address)
    "rtmSetCameraAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.c_int, ctypes.c_void_p]),
    "rtmSetVerticesAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "rtmGetCamera": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float)]),
    "rtmLightSetOriginAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.POINTER(ctypes.c_float), ctypes.c_int,
                                              ctypes.c_void_p]),
    "rtmLightSetVerticesAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]),
    "rtmOrderHost": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_ulonglong, ctypes.POINTER(ctypes.c_float), ctypes.c_void_p,
                                    ctypes.c_void_p]),
    # include/srt_surface.h: vertex attributes (tables and planes: device or host addresses)
    "rtvSurfaceFrameAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _SZ, _SZ,
                                            ctypes.POINTER(RtvSurface), ctypes.POINTER(RtvOutputs), ctypes.c_void_p]),
    "rtvSurfacePointsAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _SZ,
                                             ctypes.POINTER(RtvSurface), ctypes.POINTER(RtvOutputs), ctypes.c_void_p]),
    "rtvInterpolateFrameAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _SZ, _SZ,
                                                ctypes.c_void_p, _SZ, ctypes.c_void_p, ctypes.c_void_p]),
    "rtvInterpolatePointsAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _SZ, ctypes.c_void_p,
                                                 _SZ, ctypes.c_void_p, ctypes.c_void_p]),
    "rtvSurfaceHost": (ctypes.c_int, [ctypes.c_char_p, _SZ, _SZ, ctypes.c_void_p, ctypes.c_void_p, _SZ,
                                      ctypes.POINTER(RtvSurface), ctypes.POINTER(RtvOutputs)]),
    "rtvInterpolateHost": (ctypes.c_int, [ctypes.c_char_p, _SZ, _SZ, ctypes.c_void_p, ctypes.c_void_p, _SZ,
                                          ctypes.c_void_p, _SZ, ctypes.c_void_p]),
    "rtvObjAttributesHost": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_void_p, ctypes.c_void_p,
                                            ctypes.POINTER(ctypes.c_int)]),
    # include/srt_material.h: lit surfaces (rtdLight*'s arguments with a surface and a material, each or None)
    "rtpLightSurfaceAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, _SZ, ctypes.POINTER(ctypes.c_float),
                                            ctypes.POINTER(RtvSurface), ctypes.POINTER(RtpMaterial), ctypes.c_void_p,
                                            ctypes.c_void_p, _SZ, _SZ, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rtpLightSurfaceHost": (ctypes.c_int, [ctypes.c_char_p, _SZ, _SZ, ctypes.c_void_p, _SZ,
                                           ctypes.POINTER(ctypes.c_float), ctypes.POINTER(RtvSurface),
                                           ctypes.POINTER(RtpMaterial), ctypes.c_void_p, ctypes.c_void_p, _SZ, _SZ,
                                           ctypes.c_void_p, ctypes.c_void_p]),
    # include/srt_rays.h: ray queries (rays: count x 8 floats; device addresses for *Async, host ones for *Host)
    "rtrBuildAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p]),
    "rtrClosestAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, _SZ, ctypes.c_void_p, ctypes.c_void_p,
                                       ctypes.c_void_p, ctypes.c_void_p]),
    "rtrOccludedAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, _SZ, ctypes.c_void_p, ctypes.c_void_p]),
    "rtrClosestHost": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_void_p, _SZ, ctypes.c_void_p, ctypes.c_void_p,
                                      ctypes.c_void_p]),
    "rtrOccludedHost": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_void_p, _SZ, ctypes.c_void_p]),
    "rtrClosestHostFlags": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_void_p, _SZ, ctypes.c_void_p, ctypes.c_void_p,
                                           ctypes.c_void_p, ctypes.c_int]),
    "rtrOccludedHostFlags": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_void_p, _SZ, ctypes.c_void_p, ctypes.c_int]),
    # include/srt_visibility.h: sampled visibility (generator tables: device addresses for *Async, host ones for *Host)
    "rtaVisibilityFrameAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _SZ, _SZ,
                                               ctypes.POINTER(RtaGenerator), ctypes.POINTER(RtaOutputs),
                                               ctypes.c_void_p]),
    "rtaVisibilityPointsAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _SZ,
                                                ctypes.POINTER(RtaGenerator), ctypes.POINTER(RtaOutputs),
                                                ctypes.c_void_p]),
    "rtaRaysFrameAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _SZ, _SZ,
                                         ctypes.POINTER(RtaGenerator), ctypes.c_void_p, ctypes.c_void_p]),
    "rtaRaysPointsAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _SZ,
                                          ctypes.POINTER(RtaGenerator), ctypes.c_void_p, ctypes.c_void_p]),
    "rtaVisibilityHost": (ctypes.c_int, [ctypes.c_char_p, _SZ, _SZ, ctypes.c_void_p, ctypes.c_void_p, _SZ,
                                         ctypes.POINTER(RtaGenerator), ctypes.POINTER(RtaOutputs)]),
    "rtaRaysHost": (ctypes.c_int, [ctypes.c_char_p, _SZ, _SZ, ctypes.c_void_p, ctypes.c_void_p, _SZ,
                                   ctypes.POINTER(RtaGenerator), ctypes.c_void_p]),
    # include/srt_hits.h: lit ray hits (lights, ambient: rtdLight*'s; blend: an RthBlend or None)
    "rthLightHitsAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, _SZ, ctypes.POINTER(ctypes.c_float),
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _SZ, ctypes.POINTER(RthBlend),
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]),
    "rthLightHitsHost": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_void_p, _SZ, ctypes.POINTER(ctypes.c_float),
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, _SZ, ctypes.POINTER(RthBlend),
                                        ctypes.c_void_p, ctypes.c_void_p]),
    # include/srt_radiance.h: sampled radiance (lights, ambient: rtdLight*'s; gen: rta's; options: an RtiOptions or None)
    "rtiRadianceFrameAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, _SZ, ctypes.POINTER(ctypes.c_float),
                                             ctypes.c_void_p, ctypes.c_void_p, _SZ, _SZ, ctypes.POINTER(RtaGenerator),
                                             ctypes.POINTER(RtiOptions), ctypes.c_void_p, ctypes.c_void_p]),
    "rtiRadiancePointsAsync": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_void_p, _SZ, ctypes.POINTER(ctypes.c_float),
                                              ctypes.c_void_p, ctypes.c_void_p, _SZ, ctypes.POINTER(RtaGenerator),
                                              ctypes.POINTER(RtiOptions), ctypes.c_void_p, ctypes.c_void_p]),
    "rtiRadianceHost": (ctypes.c_int, [ctypes.c_char_p, _SZ, _SZ, ctypes.c_void_p, _SZ, ctypes.POINTER(ctypes.c_float),
                                       ctypes.c_void_p, ctypes.c_void_p, _SZ, ctypes.POINTER(RtaGenerator),
                                       ctypes.POINTER(RtiOptions), ctypes.c_void_p]),
}

_lib = None


def _share_torch_hip_runtime():
    """Load torch's HIP runtime first when torch is installed.

    torch ships its own libamdhip64.so / libhsa-runtime64.so / librccl.so with the same
    SONAMEs (libamdhip64.so.7, ...) as /opt/rocm. If torch is imported first, the dynamic
    loader satisfies this library's NEEDED entries with torch's copies, so the process has ONE
    HIP runtime and torch streams/pointers passed to srt* calls belong to it. Loading this
    library first would pull /opt/rocm's copies, and torch would then load a second runtime.
    """
    try:
        import torch  # noqa: F401
    except ImportError:
        pass


def lib() -> ctypes.CDLL:
    """Load libModelRunner.so once; raise loudly if it has not been built."""
    global _lib
    if _lib is None:
        _share_torch_hip_runtime()
        if not LIB_PATH.exists():
            raise RuntimeError(
                f"{LIB_PATH} is missing: build the HIP library first (`make` at the repo root or "
                "`python -c 'import __graft_entry__ as g; g.build()'`); there is no CPU fallback")
        handle = ctypes.CDLL(os.fspath(LIB_PATH))
        for name, (restype, argtypes) in _SIGNATURES.items():
            if os.environ.get("SRT_LIB") and not hasattr(handle, name):
                continue  # an older build under measurement (A/B): bind what it has
            fn = getattr(handle, name)
            fn.restype = restype
            fn.argtypes = argtypes
        _lib = handle
    return _lib


def exported_names():
    return list(_SIGNATURES)


def last_error() -> str:
    msg = lib().srtGetLastError()
    return msg.decode() if msg else ""
