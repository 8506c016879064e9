"""Scene files, the device-level render stages (include/srt_render.h), point queries
(include/srt_query.h), G-buffer outputs (include/srt_gbuffer.h), multi-sample frames
(include/srt_samples.h), spot-light shadow masks (include/srt_light.h), omni-light shadow masks
(include/srt_omni.h), direct lighting (include/srt_lighting.h; the lights: lighting.py), dynamic
scenes (include/srt_motion.h), vertex attributes (include/srt_surface.h), ray queries
(include/srt_rays.h), sampled visibility (include/srt_visibility.h) and lit ray hits
(include/srt_hits.h).

``DeviceScene`` keeps a scene resident on one GPU and launches the two stages on a caller's
HIP stream with caller-owned device buffers (torch tensors or raw pointers):

    scene = DeviceScene(path, device=0)
    scene.prepare(W, H, stream)                                  # edge records
    scene.trace(offsets, rgba, row_begin, row_count, stream=s)   # closest hit + shade
    scene.query(positions, ids, t, stream=s)                     # closest hit at arbitrary image positions
    scene.gbuffer(offsets, ids, depth=d, normal=n, albedo=a)     # the surface under the hits (also attributes())
    scene.render_samples(offsets_s, ids_s, rgba, stream=s)       # S samples per pixel, resolved (also resolve())
    scene.shadow(light, offsets, ids, mask, rgba, stream=s)      # which pixels a spot light (a second scene) reaches
    scene.layer_frame(offsets, ids_k, t_k, stream=s)             # the K nearest hits per pixel (also layers(), composite())
    scene.omni_shadow(omni, offsets, ids, mask, face, stream=s)  # which pixels a point light (an OmniLight) reaches
    scene.light(lights, offsets, ids, rgba, ambient, stream=s)   # the lit picture under several lights (also render_lit())
    scene.set_camera(camera, stream=s)                           # move the camera in place (also set_vertices(), OmniLight.set_origin())
    scene.surface_frame(offsets, ids, Surface(normals, uvs, texture), rgba=out)  # smooth, textured (also surface(), interpolate())
    scene.closest(rays, ids, t, bary, stream=s)                  # caller-supplied rays, no prepare() needed (also occluded())
    scene.visibility_frame(offsets, ids, Hemisphere(samples, tmin, tmax), fraction=ao)  # ambient occlusion, soft shadows (also visibility(), generate_rays())
    scene.light_hits(lights, rays, ids, t, rgba, ambient, stream=s)  # what closest()'s hits look like under the lights (also render_reflection())

This is the path bench.py times (inputs resident in HBM) and the one-process-per-GPU
band renderer uses; ``runner.render`` is the host-image ml* path.
"""
from __future__ import annotations

import ctypes
import os

from . import _native
from ._native import (RTK_MAX_LAYERS, RTM_KEEP_ORDER, RTM_REORDER, RTS_MAX_SAMPLES, RTV_MAX_CHANNELS, SRT_MAX_BATCH, SRT_SCENE_CORNELL, SRT_SCENE_SOUP, SRT_SCENE_TRIANGLE, SRT_TRACE_BVH,
                      SRT_TRACE_CULL, SRT_TRACE_LDS, SRT_TRACE_SCALAR)

SCENE_KINDS = {"triangle": SRT_SCENE_TRIANGLE, "cornell": SRT_SCENE_CORNELL, "soup": SRT_SCENE_SOUP}
TRACE_VARIANTS = {"lds": SRT_TRACE_LDS, "scalar": SRT_TRACE_SCALAR, "cull": SRT_TRACE_CULL, "bvh": SRT_TRACE_BVH}
MAX_BATCH = SRT_MAX_BATCH
MAX_PINS = 64  # include/srt_pins.h RTN_MAX_PINS: pinned offsets buffers per device scene
SOUP_SEED = 0x5EED  # 100k soup seed; the 1M soup uses SOUP_SEED + 1


class SrtError(RuntimeError):
    pass


def _check(rc: int):
    if rc != 0:
        raise SrtError(_native.last_error())


def write_scene(path: str, kind: str = "soup", triangles: int = 100_000, seed: int | None = None,
                size: float = 0.0) -> str:
    """Write a generated scene file; returns ``path``."""
    if seed is None:
        seed = SOUP_SEED + (1 if triangles >= 1_000_000 else 0)
    _check(_native.lib().srtWriteScene(os.fsencode(path), SCENE_KINDS[kind], triangles, seed, size))
    return path


def scene_triangles(path: str) -> int:
    n = ctypes.c_ulonglong()
    _check(_native.lib().srtSceneTriangles(os.fsencode(path), ctypes.byref(n)))
    return n.value


def read_scene(path: str):
    """Load a scene file (binary or .obj) through the library: dict of numpy arrays."""
    import numpy as np

    n = ctypes.c_ulonglong()
    _check(_native.lib().srtReadScene(os.fsencode(path), 0, ctypes.byref(n), None, None, None, None, None))
    v = np.empty((n.value, 9), np.float32)
    a = np.empty((n.value, 3), np.float32)
    cam = np.empty(10, np.float32)
    bg = np.empty(3, np.float32)
    flags = ctypes.c_uint()
    _check(_native.lib().srtReadScene(os.fsencode(path), n.value, ctypes.byref(n), v.ctypes.data, a.ctypes.data,
                                      cam.ctypes.data, bg.ctypes.data, ctypes.byref(flags)))
    return {"vertices": v, "albedo": a, "camera": cam, "background": bg, "flags": flags.value}


def convert_scene(src: str, dst: str, input_dtype: int = -1, output_dtype: int = -1) -> str:
    """Write src (binary or .obj) as a binary scene file with the given image data types."""
    _check(_native.lib().srtConvertScene(os.fsencode(src), os.fsencode(dst), input_dtype, output_dtype))
    return dst


def scene_frame(path: str, width: int, height: int):
    """(origin, base, du, dv) float32 triples of the affine primary-ray frame."""
    out = (ctypes.c_float * 12)()
    _check(_native.lib().srtSceneFrame(os.fsencode(path), width, height, out))
    vals = list(out)
    return tuple(tuple(vals[3 * k:3 * k + 3]) for k in range(4))


def pixel_positions(width: int, height: int, offsets):
    """The image positions ray generation produces for a frame's pixels: offsets (H, W, 2) (or a
    scalar / anything broadcastable to it) -> (H * W, 2) float32, row-major, by the canonical
    float32 expression fx = (float(x) + sx) / float(W), fy = (float(y) + sy) / float(H)."""
    import numpy as np

    off = np.broadcast_to(np.asarray(offsets, np.float32), (height, width, 2))
    x = np.arange(width, dtype=np.float32)[None, :]
    y = np.arange(height, dtype=np.float32)[:, None]
    out = np.empty((height, width, 2), np.float32)
    out[..., 0] = (x + off[..., 0]) / np.float32(width)
    out[..., 1] = (y + off[..., 1]) / np.float32(height)
    return out.reshape(height * width, 2)


def query_host(path: str, width: int, height: int, positions):
    """Point queries on the host (rtqQueryHost: brute force, the library's canonical math, no
    device): positions (count, 2) float32 -> (ids int32, t float32), a miss as (-1, +inf)."""
    import numpy as np

    pos = np.ascontiguousarray(positions, np.float32)
    if pos.ndim != 2 or pos.shape[1] != 2:
        raise ValueError(f"positions must be (count, 2), got {pos.shape}")
    ids = np.empty(pos.shape[0], np.int32)
    t = np.empty(pos.shape[0], np.float32)
    _check(_native.lib().rtqQueryHost(os.fsencode(path), width, height, pos.ctypes.data, pos.shape[0],
                                      ids.ctypes.data, t.ctypes.data))
    return ids, t


def attributes_host(path: str, width: int, height: int, positions, ids):
    """The G-buffer on the host (rtgPointsHost: the library's canonical math, no device):
    positions (count, 2) float32 and ids (count,) int32 -> (depth (count,), bary (count, 2),
    normal (count, 4), albedo (count, 4)), float32 numpy arrays."""
    import numpy as np

    pos = np.ascontiguousarray(positions, np.float32)
    idv = np.ascontiguousarray(ids, np.int32)
    if pos.ndim != 2 or pos.shape[1] != 2:
        raise ValueError(f"positions must be (count, 2), got {pos.shape}")
    if idv.shape != (pos.shape[0],):
        raise ValueError(f"ids must be {(pos.shape[0],)}, got {idv.shape}")
    count = pos.shape[0]
    depth = np.empty(count, np.float32)
    bary = np.empty((count, 2), np.float32)
    normal = np.empty((count, 4), np.float32)
    albedo = np.empty((count, 4), np.float32)
    out = _native.RtgOutputs(ctypes.sizeof(_native.RtgOutputs), depth.ctypes.data, bary.ctypes.data,
                             normal.ctypes.data, albedo.ctypes.data)
    _check(_native.lib().rtgPointsHost(os.fsencode(path), width, height, pos.ctypes.data, idv.ctypes.data, count,
                                       ctypes.byref(out)))
    return depth, bary, normal, albedo


def resolve_host(path: str, width: int, height: int, offsets, ids, row_begin: int = 0, row_count: int | None = None):
    """The resolve of S sample planes on the host (rtsResolveHost: the library's canonical math, no
    device): offsets, S arrays (rows, W, 2) float32, and ids, S arrays (rows, W) int32, of the band
    rows [row_begin, row_begin + row_count) -> rgba (rows, W, 4) float32: the mean of the shaded
    samples, alpha = the share that hit."""
    import numpy as np

    if row_count is None:
        row_count = height - row_begin
    if len(offsets) != len(ids):
        raise ValueError(f"one ids plane per offsets plane, got {len(offsets)} and {len(ids)}")
    samples = len(ids)
    if not 1 <= samples <= RTS_MAX_SAMPLES:
        raise ValueError(f"1 to {RTS_MAX_SAMPLES} sample planes, got {samples}")
    off = [np.ascontiguousarray(o, np.float32) for o in offsets]
    idv = [np.ascontiguousarray(i, np.int32) for i in ids]
    for s in range(samples):
        if off[s].shape != (row_count, width, 2):
            raise ValueError(f"offsets[{s}] must be {(row_count, width, 2)}, got {off[s].shape}")
        if idv[s].shape != (row_count, width):
            raise ValueError(f"ids[{s}] must be {(row_count, width)}, got {idv[s].shape}")
    rgba = np.empty((row_count, width, 4), np.float32)
    arr = ctypes.c_void_p * samples
    _check(_native.lib().rtsResolveHost(os.fsencode(path), width, height, arr(*[o.ctypes.data for o in off]),
                                        arr(*[i.ctypes.data for i in idv]), samples, row_begin, row_count,
                                        rgba.ctypes.data))
    return rgba


def layers_host(path: str, width: int, height: int, positions, layers: int):
    """Depth layers on the host (rtkLayersHost: brute force, the library's canonical math, no
    device): positions (count, 2) float32 -> (ids (layers, count) int32, t (layers, count) float32),
    front to back, a missing layer as (-1, +inf)."""
    import numpy as np

    pos = np.ascontiguousarray(positions, np.float32)
    if pos.ndim != 2 or pos.shape[1] != 2:
        raise ValueError(f"positions must be (count, 2), got {pos.shape}")
    if not 1 <= layers <= RTK_MAX_LAYERS:
        raise ValueError(f"1 to {RTK_MAX_LAYERS} layers, got {layers}")
    ids = np.empty((layers, pos.shape[0]), np.int32)
    t = np.empty((layers, pos.shape[0]), np.float32)
    _check(_native.lib().rtkLayersHost(os.fsencode(path), width, height, pos.ctypes.data, pos.shape[0], layers,
                                       ids.ctypes.data, t.ctypes.data))
    return ids, t


def composite_host(path: str, width: int, height: int, offsets, ids, opacity, row_begin: int = 0,
                   row_count: int | None = None):
    """The over-composite of depth layers on the host (rtkCompositeHost: the library's canonical
    math, no device): offsets (rows, W, 2) float32, ids (K, rows, W) int32 and opacity
    (triangles,) float32 of the band rows [row_begin, row_begin + row_count) -> rgba (rows, W, 4)."""
    import numpy as np

    if row_count is None:
        row_count = height - row_begin
    off = np.ascontiguousarray(offsets, np.float32)
    idv = np.ascontiguousarray(ids, np.int32)
    opa = np.ascontiguousarray(opacity, np.float32)
    if off.shape != (row_count, width, 2):
        raise ValueError(f"offsets must be {(row_count, width, 2)}, got {off.shape}")
    if idv.ndim != 3 or idv.shape[1:] != (row_count, width) or not 1 <= idv.shape[0] <= RTK_MAX_LAYERS:
        raise ValueError(f"ids must be (1..{RTK_MAX_LAYERS} layers, {row_count}, {width}), got {idv.shape}")
    n = scene_triangles(path)
    if opa.shape != (n,):
        raise ValueError(f"opacity must be {(n,)}, got {opa.shape}")
    rgba = np.empty((row_count, width, 4), np.float32)
    _check(_native.lib().rtkCompositeHost(os.fsencode(path), width, height, off.ctypes.data, idv.ctypes.data,
                                          idv.shape[0], opa.ctypes.data, row_begin, row_count, rgba.ctypes.data))
    return rgba


def _camera10(camera):
    """camera (10 floats: eye, lookat, up, vfov_deg) as the C array the rtl calls take."""
    vals = [float(v) for v in camera]
    if len(vals) != 10:
        raise ValueError(f"camera must be 10 floats (eye, lookat, up, vfov_deg), got {len(vals)}")
    return (ctypes.c_float * 10)(*vals)


def light_projection(camera, light_width: int, light_height: int):
    """The projection rows (px, py, pz) of a light camera at its resolution (rtlProjectionHost):
    (3, 3) float32. A world point X lies at light-frame position (px.q / pz.q, py.q / pz.q),
    q = X - eye, at planar depth pz.q."""
    import numpy as np

    rows = (ctypes.c_float * 9)()
    _check(_native.lib().rtlProjectionHost(_camera10(camera), light_width, light_height, rows))
    return np.array(list(rows), np.float32).reshape(3, 3)


def shadow_host(path: str, width: int, height: int, light_camera, light_width: int, light_height: int, offsets, ids,
                bias: float = 0.0, dim: float = 0.0, row_begin: int = 0, row_count: int | None = None):
    """The shadow mask on the host (rtlShadowHost: brute force, the library's canonical math, no
    device): the band rows of path's width x height frame under the light camera's light_width x
    light_height frame, offsets (rows, W, 2) float32 and ids (rows, W) int32 -> (mask (rows, W)
    uint8 of classes 0 shadowed / 1 lit / 2 outside the light's frustum / 3 no surface, rgba
    (rows, W, 4) float32: the shaded pixel, rgb times 1 (class 1) or dim (classes 0 and 2))."""
    import numpy as np

    if row_count is None:
        row_count = height - row_begin
    off = np.ascontiguousarray(offsets, np.float32)
    idv = np.ascontiguousarray(ids, np.int32)
    if off.shape != (row_count, width, 2):
        raise ValueError(f"offsets must be {(row_count, width, 2)}, got {off.shape}")
    if idv.shape != (row_count, width):
        raise ValueError(f"ids must be {(row_count, width)}, got {idv.shape}")
    mask = np.empty((row_count, width), np.uint8)
    rgba = np.empty((row_count, width, 4), np.float32)
    _check(_native.lib().rtlShadowHost(os.fsencode(path), width, height, _camera10(light_camera), light_width,
                                       light_height, off.ctypes.data, idv.ctypes.data, row_begin, row_count, bias,
                                       mask.ctypes.data, rgba.ctypes.data, dim))
    return mask, rgba


def _float3(name: str, values):
    vals = [float(v) for v in values]
    if len(vals) != 3:
        raise ValueError(f"{name} must be 3 floats, got {len(vals)}")
    return (ctypes.c_float * 3)(*vals)


def omni_face_camera(origin, face: int):
    """The camera (eye, lookat, up, vfov_deg: 10 floats) of cube face `face` (0 .. 5) of the point
    light at `origin` (rtoFaceCameraHost; include/srt_omni.h has the table)."""
    cam = (ctypes.c_float * 10)()
    _check(_native.lib().rtoFaceCameraHost(_float3("origin", origin), face, cam))
    return tuple(cam)


def omni_face_of(q) -> int:
    """The cube face (0 .. 5) the omni shadow kernel selects for q = surface point - light origin
    (rtoFaceOfHost): the largest |q_k|, ties to the lower axis, 2 k + (q_k < 0)."""
    return _native.lib().rtoFaceOfHost(_float3("q", q))


def omni_shadow_host(path: str, width: int, height: int, origin, face_size: int, offsets, ids, bias: float = 0.0,
                     dim: float = 0.0, row_begin: int = 0, row_count: int | None = None):
    """The omni-light shadow mask on the host (rtoShadowHost: brute force, the library's canonical
    math, no device): the band rows of path's width x height frame under the point light at
    `origin` with face_size x face_size cube faces, offsets (rows, W, 2) float32 and ids (rows, W)
    int32 -> (mask (rows, W) uint8 of shadow_host()'s classes, face (rows, W) uint8: the selected
    face, 255 for a class-3 pixel, rgba (rows, W, 4) float32 as shadow_host()'s)."""
    import numpy as np

    if row_count is None:
        row_count = height - row_begin
    off = np.ascontiguousarray(offsets, np.float32)
    idv = np.ascontiguousarray(ids, np.int32)
    if off.shape != (row_count, width, 2):
        raise ValueError(f"offsets must be {(row_count, width, 2)}, got {off.shape}")
    if idv.shape != (row_count, width):
        raise ValueError(f"ids must be {(row_count, width)}, got {idv.shape}")
    mask = np.empty((row_count, width), np.uint8)
    face = np.empty((row_count, width), np.uint8)
    rgba = np.empty((row_count, width, 4), np.float32)
    _check(_native.lib().rtoShadowHost(os.fsencode(path), width, height, _float3("origin", origin), face_size,
                                       off.ctypes.data, idv.ctypes.data, row_begin, row_count, bias, mask.ctypes.data,
                                       face.ctypes.data, rgba.ctypes.data, dim))
    return mask, face, rgba


def lighting_host(path: str, width: int, height: int, lights, ambient, offsets, ids, row_begin: int = 0,
                  row_count: int | None = None):
    """Direct lighting on the host (rtdLightHost: brute force, the library's canonical math, no
    device): the band rows of path's width x height frame under `lights`, a sequence of 0 to 8
    lighting.SpotLightHost / lighting.PointLightHost of path's triangles, and the ambient colour;
    offsets (rows, W, 2) float32 and ids (rows, W) int32 -> (rgba (rows, W, 4) float32, classes
    (len(lights), rows, W) uint8 of shadow_host()'s classes, light-major)."""
    import numpy as np

    from . import lighting

    if row_count is None:
        row_count = height - row_begin
    off = np.ascontiguousarray(offsets, np.float32)
    idv = np.ascontiguousarray(ids, np.int32)
    if off.shape != (row_count, width, 2):
        raise ValueError(f"offsets must be {(row_count, width, 2)}, got {off.shape}")
    if idv.shape != (row_count, width):
        raise ValueError(f"ids must be {(row_count, width)}, got {idv.shape}")
    arr, count = lighting.pack_host(lights)
    rgba = np.empty((row_count, width, 4), np.float32)
    classes = np.empty((count, row_count, width), np.uint8)
    _check(_native.lib().rtdLightHost(os.fsencode(path), width, height, ctypes.addressof(arr) if arr is not None else None,
                                      count, lighting.ambient3(ambient), off.ctypes.data, idv.ctypes.data, row_begin,
                                      row_count, rgba.ctypes.data, classes.ctypes.data))
    return rgba, classes


def _blend(base_address: int, weight):
    """The rth_blend of a base picture's address and a weight of 3 floats."""
    w = tuple(float(v) for v in weight)
    if len(w) != 3:
        raise ValueError(f"weight must be 3 floats, got {len(w)}")
    return _native.RthBlend(ctypes.sizeof(_native.RthBlend), base_address, w)


def light_hits_host(path: str, lights, ambient, rays, ids, t, base=None, weight=(1.0, 1.0, 1.0), classes: bool = False):
    """Lit ray hits on the host (rthLightHitsHost: brute force, the library's canonical math, no
    device): what the hits of `rays` (count, 8) float32 -- closest_host()'s ids (count,) int32 and t
    (count,) float32 -- look like under `lights`, a sequence of 0 to 8 lighting.SpotLightHost /
    lighting.PointLightHost of path's triangles, and the ambient colour -> rgba (count, 4) float32:
    albedo . (ambient + the lights that reach the hit from the ray's side of its triangle), alpha =
    the id; the background and -1 for a miss; zeros and -1 for a zero ray (no ray here). base
    (count, 4) float32 with weight (3 floats): rgba = (base.rgb + weight . rgb, base's alpha), a
    zero ray keeping base's element. classes=True: -> (rgba, classes (len(lights), count) uint8 of
    shadow_host()'s classes, light-major)."""
    import numpy as np

    from . import lighting

    r = _host_rays(rays)
    count = r.shape[0]
    idv = np.ascontiguousarray(ids, np.int32)
    tv = np.ascontiguousarray(t, np.float32)
    if idv.shape != (count,):
        raise ValueError(f"ids must be {(count,)}, got {idv.shape}")
    if tv.shape != (count,):
        raise ValueError(f"t must be {(count,)}, got {tv.shape}")
    blend = None
    if base is not None:
        b = np.ascontiguousarray(base, np.float32)
        if b.shape != (count, 4):
            raise ValueError(f"base must be {(count, 4)}, got {b.shape}")
        blend = ctypes.byref(_blend(b.ctypes.data, weight))
    arr, n_lights = lighting.pack_host(lights)
    rgba = np.empty((count, 4), np.float32)
    planes = np.empty((n_lights, count), np.uint8) if classes else None
    _check(_native.lib().rthLightHitsHost(os.fsencode(path), ctypes.addressof(arr) if arr is not None else None, n_lights,
                                          lighting.ambient3(ambient), r.ctypes.data, idv.ctypes.data, tv.ctypes.data,
                                          count, blend, rgba.ctypes.data, planes.ctypes.data if classes else None))
    return (rgba, planes) if classes else rgba


def tile_of(width: int, height: int, fx: float, fy: float):
    """The cull tile (col, row) the query kernel looks a position up in (rtqTileHost), or None
    when the position is not in [0, 1]^2."""
    c, r = ctypes.c_int(), ctypes.c_int()
    if _native.lib().rtqTileHost(width, height, fx, fy, ctypes.byref(c), ctypes.byref(r)) != 0:
        if _native.last_error().startswith("Position outside"):
            return None
        raise SrtError(_native.last_error())
    return c.value, r.value


def order_host(vertices, camera):
    """The spatial order and the shading normals on the host (rtmOrderHost: the library's own Morton
    key and a stable sort, no device): vertices (n, 9) or (n, 3, 3) float32 and camera (10 floats)
    -> (order (n,) uint32: what spatial_order() reports for these triangles under this camera,
    normals (n, 4) float32: (cross(v1 - v0, v2 - v0), its length), row 0 of the shading table)."""
    import numpy as np

    v = np.ascontiguousarray(vertices, np.float32)
    if v.ndim == 3 and v.shape[1:] == (3, 3):
        v = v.reshape(-1, 9)
    if v.ndim != 2 or v.shape[1] != 9:
        raise ValueError(f"vertices must be (n, 9) or (n, 3, 3), got {v.shape}")
    n = v.shape[0]
    order = np.empty(n, np.uint32)
    normals = np.empty((n, 4), np.float32)
    _check(_native.lib().rtmOrderHost(v.ctypes.data, n, _camera10(camera), order.ctypes.data, normals.ctypes.data))
    return order, normals


def _host_rays(rays):
    import numpy as np

    r = np.ascontiguousarray(rays, np.float32)
    if r.ndim != 2 or r.shape[1] != 8:
        raise ValueError(f"rays must be (count, 8), got {r.shape}")
    return r


def closest_host(path: str, rays, box_clause: bool = True):
    """Ray queries on the host (rtrClosestHost: brute force in ascending id, the library's canonical
    math, no tree, no device): rays (count, 8) float32 = (ox, oy, oz, tmin, dx, dy, dz, tmax) ->
    (ids int32, t float32, bary (count, 2) float32), a miss as (-1, +inf, (0, 0)).
    box_clause=False leaves the box clause out of the definition (to measure what it costs)."""
    import numpy as np

    r = _host_rays(rays)
    ids = np.empty(r.shape[0], np.int32)
    t = np.empty(r.shape[0], np.float32)
    bary = np.empty((r.shape[0], 2), np.float32)
    _check(_native.lib().rtrClosestHostFlags(os.fsencode(path), r.ctypes.data, r.shape[0], ids.ctypes.data,
                                             t.ctypes.data, bary.ctypes.data,
                                             _native.RTR_BOX_CLAUSE if box_clause else _native.RTR_NO_BOX_CLAUSE))
    return ids, t, bary


def occluded_host(path: str, rays, box_clause: bool = True):
    """Occlusion on the host (rtrOccludedHost): rays (count, 8) float32 -> (count,) uint8, 1 iff any
    triangle counts for the ray."""
    import numpy as np

    r = _host_rays(rays)
    out = np.empty(r.shape[0], np.uint8)
    _check(_native.lib().rtrOccludedHostFlags(os.fsencode(path), r.ctypes.data, r.shape[0], out.ctypes.data,
                                              _native.RTR_BOX_CLAUSE if box_clause else _native.RTR_NO_BOX_CLAUSE))
    return out


def camera_rays(camera, width: int, height: int, offsets):
    """The rays of a frame's pixels as ray queries: (H * W, 8) float32, row-major, o = eye,
    d = (base + fx du) + fy dv at pixel_positions(width, height, offsets), tmin = 0, tmax = +inf.
    camera: a scene file's path (its own camera, through srtSceneFrame) or 10 floats (eye, lookat,
    up, vfov_deg: DeviceScene.camera). NOT bit-equal to the trace: near a triangle's edges the ray
    test's arithmetic differs from the frame's edge records, so a pixel there may answer
    differently, and t is the trace's only up to rounding."""
    import numpy as np

    if isinstance(camera, (str, bytes, os.PathLike)):
        origin, base, du, dv = (np.array(v, np.float32) for v in scene_frame(os.fspath(camera), width, height))
    else:
        origin, base, du, dv = _frame_of_camera(camera, width, height)
    pos = pixel_positions(width, height, offsets)
    rays = np.empty((pos.shape[0], 8), np.float32)
    rays[:, 0:3] = origin
    rays[:, 3] = 0.0
    rays[:, 4:7] = (base[None, :] + pos[:, 0:1] * du[None, :]) + pos[:, 1:2] * dv[None, :]
    rays[:, 7] = np.inf
    return rays


def _frame_of_camera(camera, width: int, height: int):
    """(origin, base, du, dv) of 10 camera floats: the frame's definition in
    double, each component rounded once to float32."""
    import numpy as np

    c = np.array([float(v) for v in camera], np.float64)
    if c.shape != (10,):
        raise ValueError(f"camera must be 10 floats (eye, lookat, up, vfov_deg), got {c.shape}")
    eye, lookat, up, vfov = c[0:3], c[3:6], c[6:9], c[9]
    f = lookat - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, up)
    r /= np.linalg.norm(r)
    u = np.cross(r, f)
    half_h = np.tan(np.radians(vfov) / 2.0)
    half_w = half_h * width / height
    du = 2.0 * half_w * r
    dv = -2.0 * half_h * u
    base = f - half_w * r + half_h * u
    return tuple(np.asarray(v, np.float32) for v in (eye, base, du, dv))


def bounce_rays(rays, t, normal, tmin: float = 2.0 ** -10, tmax: float = float("inf")):
    """Mirror rays from G-buffer planes: rays (count, 8) float32 that found hits at depth t
    (count,) -- closest()'s or gbuffer()'s depth -- on surfaces with unit normals `normal`
    (count, 3) or (count, 4) (gbuffer()'s plane) -> (count, 8) float32: o' = o + t d,
    d' = d - 2 (d . n) n, range [tmin, tmax] (tmin > 0 keeps a bounce off its own surface). A ray
    that missed (t not finite) becomes a ray with d' = 0, which misses."""
    import numpy as np

    r = _host_rays(rays)
    tt = np.asarray(t, np.float32).reshape(-1)
    n = np.asarray(normal, np.float32).reshape(r.shape[0], -1)[:, :3]
    if tt.shape != (r.shape[0],):
        raise ValueError(f"t must be {(r.shape[0],)}, got {tt.shape}")
    hit = np.isfinite(tt)
    ts = np.where(hit, tt, np.float32(0))[:, None]
    d = r[:, 4:7]
    out = np.zeros_like(r)
    out[:, 0:3] = r[:, 0:3] + ts * d
    dn = np.sum(d * n, axis=1, dtype=np.float32)[:, None]
    out[:, 4:7] = np.where(hit[:, None], d - np.float32(2) * dn * n, np.float32(0))
    out[:, 3] = tmin
    out[:, 7] = tmax
    return out


class _Generator:
    """A ray generator of the sampled-visibility calls (``rta_generator``, include/srt_visibility.h).
    Device tensors for the DeviceScene calls, numpy arrays for visibility_host() / rays_host(); the
    holder keeps them alive and copies nothing."""

    kind = -1
    per_sample = 0  # floats per row of `samples`

    def __init__(self, samples, tmin, tmax, rotations=None, corner=(0.0, 0.0, 0.0), eu=(0.0, 0.0, 0.0),
                 ev=(0.0, 0.0, 0.0)):
        if samples is not None:
            shape = tuple(samples.shape)
            if len(shape) != 2 or shape[1] != self.per_sample:
                raise ValueError(f"samples must be (S, {self.per_sample}), got {shape}")
        if rotations is not None and tuple(rotations.shape) != (_native.RTA_ROTATIONS, 2):
            raise ValueError(f"rotations must be {(_native.RTA_ROTATIONS, 2)}, got {tuple(rotations.shape)}")
        self.samples, self.rotations = samples, rotations
        self.corner, self.eu, self.ev = _float3("corner", corner), _float3("eu", eu), _float3("ev", ev)
        self.tmin, self.tmax = float(tmin), float(tmax)

    @property
    def count(self) -> int:
        """S, the rays per element."""
        return 1 if self.samples is None else int(self.samples.shape[0])

    def _tables(self):
        return (("samples", self.samples), ("rotations", self.rotations))

    def _struct(self, address):
        return _native.RtaGenerator(ctypes.sizeof(_native.RtaGenerator), self.kind, self.count, address(self.samples),
                                    address(self.rotations), self.corner, self.eu, self.ev, self.tmin, self.tmax)


class Hemisphere(_Generator):
    """Ambient occlusion: samples (S, 3) float32 local directions (lx, ly, lz) around the normal
    (samples.cosine_hemisphere), each ray's range [tmin, tmax] in units of the direction; rotations:
    None or (16, 2) float32 (cos, sin) pairs (samples.rotations), one per pixel of a 4 x 4 block."""

    kind = _native.RTA_HEMISPHERE
    per_sample = 3

    def __init__(self, samples, tmin, tmax, rotations=None):
        super().__init__(samples, tmin, tmax, rotations)


class AreaLight(_Generator):
    """A parallelogram light corner + a eu + b ev: samples (S, 2) float32 (a, b) (samples.area_samples).
    A ray runs from the surface point to the light's point, t in units of that segment."""

    kind = _native.RTA_AREA
    per_sample = 2

    def __init__(self, corner, eu, ev, samples, tmin: float = 2.0 ** -10, tmax: float = 1.0 - 2.0 ** -10):
        super().__init__(samples, tmin, tmax, None, corner, eu, ev)


class Mirror(_Generator):
    """The mirror bounce of the primary ray, one ray per element; generate_rays() and radiance() only."""

    kind = _native.RTA_MIRROR

    def __init__(self, tmin: float = 2.0 ** -10, tmax: float = float("inf")):
        super().__init__(None, tmin, tmax)


def _host_generator(generator):
    """The generator's struct over contiguous float32 numpy copies of its tables (kept alive by the
    returned tuple)."""
    import numpy as np

    keep = {id(t): np.ascontiguousarray(t, np.float32) for _, t in generator._tables() if t is not None}
    return generator._struct(lambda a: 0 if a is None else keep[id(a)].ctypes.data), keep


def rays_host(path: str, width: int, height: int, positions, ids, generator):
    """The rays of a generator on the host (rtaRaysHost: the library's canonical math, no device):
    positions (count, 2) float32 and ids (count,) int32 on the file's width x height frame ->
    (S, count, 8) float32 rays, sample-major. An element off a surface gives zero rays."""
    import numpy as np

    pos, idv = _host_elements(positions, ids)
    g, keep = _host_generator(generator)
    rays = np.empty((generator.count, pos.shape[0], 8), np.float32)
    _check(_native.lib().rtaRaysHost(os.fsencode(path), width, height, pos.ctypes.data, idv.ctypes.data, pos.shape[0],
                                     ctypes.byref(g), rays.ctypes.data))
    del keep
    return rays


def visibility_host(path: str, width: int, height: int, positions, ids, generator):
    """Sampled visibility on the host (rtaVisibilityHost): positions (count, 2) float32 and ids
    (count,) int32 -> (visible (count,) uint8, fraction (count,) float32): how many of the
    generator's S rays are unoccluded, and that over S."""
    import numpy as np

    pos, idv = _host_elements(positions, ids)
    g, keep = _host_generator(generator)
    visible = np.empty(pos.shape[0], np.uint8)
    fraction = np.empty(pos.shape[0], np.float32)
    out = _native.RtaOutputs(ctypes.sizeof(_native.RtaOutputs), visible.ctypes.data, fraction.ctypes.data)
    _check(_native.lib().rtaVisibilityHost(os.fsencode(path), width, height, pos.ctypes.data, idv.ctypes.data,
                                           pos.shape[0], ctypes.byref(g), ctypes.byref(out)))
    del keep
    return visible, fraction


def _radiance_options(modulate: bool, base_address, weight):
    """The rti_options of a call and what keeps its blend alive."""
    blend = _blend(base_address, weight) if base_address is not None else None
    options = _native.RtiOptions(ctypes.sizeof(_native.RtiOptions), 1 if modulate else 0,
                                 ctypes.pointer(blend) if blend is not None else None)
    return options, blend


def radiance_host(path: str, width: int, height: int, lights, ambient, positions, ids, generator, modulate: bool = False,
                  base=None, weight=(1.0, 1.0, 1.0)):
    """Sampled radiance on the host (rtiRadianceHost: the composition rays_host() -> closest_host()
    -> light_hits_host() and the sum in ascending sample order, no device): positions (count, 2)
    float32 and ids (count,) int32 on the file's width x height frame, a Hemisphere or a Mirror of
    numpy tables, `lights` as lighting_host()'s -> rgba (count, 4) float32: the mean colour of what
    the generator's S rays hit (the background for a miss), times the element's own albedo with
    modulate, alpha = the share of rays that hit a surface; zeros off a surface. base (count, 4)
    float32 with weight (3 floats): rgba = (base.rgb + weight . mean, base's alpha), an element off a
    surface keeping base's."""
    import numpy as np

    from . import lighting

    pos, idv = _host_elements(positions, ids)
    count = pos.shape[0]
    g, keep = _host_generator(generator)
    b = None
    if base is not None:
        b = np.ascontiguousarray(base, np.float32)
        if b.shape != (count, 4):
            raise ValueError(f"base must be {(count, 4)}, got {b.shape}")
    options, blend = _radiance_options(modulate, b.ctypes.data if b is not None else None, weight)
    arr, n_lights = lighting.pack_host(lights)
    rgba = np.empty((count, 4), np.float32)
    _check(_native.lib().rtiRadianceHost(os.fsencode(path), width, height,
                                         ctypes.addressof(arr) if arr is not None else None, n_lights,
                                         lighting.ambient3(ambient), pos.ctypes.data, idv.ctypes.data, count,
                                         ctypes.byref(g), ctypes.byref(options), rgba.ctypes.data))
    del keep, blend
    return rgba


class Surface:
    """What a surface is made of (``rtv_surface``, include/srt_surface.h): per-triangle corner
    normals (triangles, 3, 3), corner uvs (triangles, 3, 2) and a texture (TH, TW, 4), float32, each
    optional (a texture needs uvs), indexed by the triangle's index in the scene file. wrap
    "repeat" | "clamp", filter "bilinear" | "nearest"; modulate: the texel times the scene's albedo
    of the triangle. Device tensors for DeviceScene.surface_frame() / surface(), numpy arrays for
    surface_host(); the holder keeps them alive and copies nothing."""

    WRAPS = {"repeat": 0, "clamp": _native.RTV_WRAP_CLAMP}
    FILTERS = {"bilinear": 0, "nearest": _native.RTV_FILTER_NEAREST}

    def __init__(self, normals=None, uvs=None, texture=None, wrap: str = "repeat", filter: str = "bilinear",
                 modulate: bool = False):
        if wrap not in self.WRAPS:
            raise ValueError(f"wrap must be one of {sorted(self.WRAPS)}, got {wrap!r}")
        if filter not in self.FILTERS:
            raise ValueError(f"filter must be one of {sorted(self.FILTERS)}, got {filter!r}")
        if texture is not None and uvs is None:
            raise ValueError("a texture needs uvs")
        self.normals, self.uvs, self.texture = normals, uvs, texture
        self.wrap, self.filter, self.modulate = wrap, filter, bool(modulate)

    @property
    def flags(self) -> int:
        return self.WRAPS[self.wrap] | self.FILTERS[self.filter] | (_native.RTV_MODULATE if self.modulate else 0)

    def _struct(self, address):
        th, tw = (int(self.texture.shape[0]), int(self.texture.shape[1])) if self.texture is not None else (0, 0)
        return _native.RtvSurface(ctypes.sizeof(_native.RtvSurface), address(self.normals), address(self.uvs),
                                  address(self.texture), tw, th, self.flags)


def _host_elements(positions, ids):
    import numpy as np

    pos = np.ascontiguousarray(positions, np.float32)
    idv = np.ascontiguousarray(ids, np.int32)
    if pos.ndim != 2 or pos.shape[1] != 2:
        raise ValueError(f"positions must be (count, 2), got {pos.shape}")
    if idv.shape != (pos.shape[0],):
        raise ValueError(f"ids must be {(pos.shape[0],)}, got {idv.shape}")
    return pos, idv


def surface_host(path: str, width: int, height: int, positions, ids, surface: Surface):
    """Vertex attributes on the host (rtvSurfaceHost: the library's canonical math, no device):
    positions (count, 2) float32, ids (count,) int32 and a Surface of numpy arrays -> (normal
    (count, 4), albedo (count, 4), rgba (count, 4), uv (count, 2)), float32 numpy arrays."""
    import numpy as np

    pos, idv = _host_elements(positions, ids)
    count = pos.shape[0]
    host = _host_surface(path, surface)
    normal = np.empty((count, 4), np.float32)
    albedo = np.empty((count, 4), np.float32)
    rgba = np.empty((count, 4), np.float32)
    uv = np.empty((count, 2), np.float32)
    s = host._struct(lambda a: 0 if a is None else a.ctypes.data)
    out = _native.RtvOutputs(ctypes.sizeof(_native.RtvOutputs), normal.ctypes.data, albedo.ctypes.data,
                             rgba.ctypes.data, uv.ctypes.data)
    _check(_native.lib().rtvSurfaceHost(os.fsencode(path), width, height, pos.ctypes.data, idv.ctypes.data, count,
                                        ctypes.byref(s), ctypes.byref(out)))
    return normal, albedo, rgba, uv


def _host_surface(path: str, surface: Surface) -> Surface:
    """`surface` with its tables as contiguous float32 numpy arrays, checked against path's triangles."""
    import numpy as np

    n = scene_triangles(path)
    held = {}
    for name, tail in (("normals", (3, 3)), ("uvs", (3, 2))):
        buf = getattr(surface, name)
        if buf is not None:
            a = np.ascontiguousarray(buf, np.float32)
            if a.shape not in ((n,) + tail, (n, tail[0] * tail[1])):
                raise ValueError(f"{name} must be {(n,) + tail}, got {a.shape}")
            held[name] = a
    if surface.texture is not None:
        a = np.ascontiguousarray(surface.texture, np.float32)
        if a.ndim != 3 or a.shape[2] != 4:
            raise ValueError(f"texture must be (TH, TW, 4), got {a.shape}")
        held["texture"] = a
    return Surface(held.get("normals"), held.get("uvs"), held.get("texture"), surface.wrap, surface.filter,
                   surface.modulate)


def lit_surface_host(path: str, width: int, height: int, lights, ambient, offsets, ids, surface, material=None,
                     row_begin: int = 0, row_count: int | None = None):
    """Lit surfaces on the host (rtpLightSurfaceHost: the library's canonical math, no device):
    lighting_host() on the surface a Surface of numpy arrays describes (None: none) with a
    lighting.Material (None: no highlight) -> (rgba (rows, W, 4) float32, classes (len(lights),
    rows, W) uint8). Without both it is lighting_host(), bit for bit."""
    import numpy as np

    from . import lighting

    if row_count is None:
        row_count = height - row_begin
    off = np.ascontiguousarray(offsets, np.float32)
    idv = np.ascontiguousarray(ids, np.int32)
    if off.shape != (row_count, width, 2):
        raise ValueError(f"offsets must be {(row_count, width, 2)}, got {off.shape}")
    if idv.shape != (row_count, width):
        raise ValueError(f"ids must be {(row_count, width)}, got {idv.shape}")
    if surface is not None and not isinstance(surface, Surface):
        raise ValueError(f"surface must be a Surface or None, got {type(surface).__name__}")
    host = _host_surface(path, surface) if surface is not None else None
    s = ctypes.byref(host._struct(lambda a: 0 if a is None else a.ctypes.data)) if host is not None else None
    arr, count = lighting.pack_host(lights)
    rgba = np.empty((row_count, width, 4), np.float32)
    classes = np.empty((count, row_count, width), np.uint8)
    _check(_native.lib().rtpLightSurfaceHost(os.fsencode(path), width, height,
                                             ctypes.addressof(arr) if arr is not None else None, count,
                                             lighting.ambient3(ambient), s, lighting.material_ref(material),
                                             off.ctypes.data, idv.ctypes.data, row_begin, row_count, rgba.ctypes.data,
                                             classes.ctypes.data))
    return rgba, classes


def interpolate_host(path: str, width: int, height: int, positions, ids, table):
    """One corner table interpolated on the host (rtvInterpolateHost): table (triangles, 3, C)
    float32, 1 <= C <= 4 -> out (count, C) float32."""
    import numpy as np

    pos, idv = _host_elements(positions, ids)
    tab = np.ascontiguousarray(table, np.float32)
    n = scene_triangles(path)
    if tab.ndim != 3 or tab.shape[:2] != (n, 3) or not 1 <= tab.shape[2] <= RTV_MAX_CHANNELS:
        raise ValueError(f"table must be ({n}, 3, C) with 1 <= C <= {RTV_MAX_CHANNELS}, got {tab.shape}")
    out = np.empty((pos.shape[0], tab.shape[2]), np.float32)
    _check(_native.lib().rtvInterpolateHost(os.fsencode(path), width, height, pos.ctypes.data, idv.ctypes.data,
                                            pos.shape[0], tab.ctypes.data, tab.shape[2], out.ctypes.data))
    return out


def obj_attributes(path: str):
    """The corner normals and texture coordinates of a Wavefront OBJ file (rtvObjAttributesHost), row
    i for triangle i of read_scene(path): (normals (n, 3, 3), uvs (n, 3, 2), have_normals,
    have_uvs). A corner without `vn` takes its triangle's shading normal, one without `vt` (0, 0)."""
    import numpy as np

    n = scene_triangles(path)
    normals = np.empty((n, 3, 3), np.float32)
    uvs = np.empty((n, 3, 2), np.float32)
    have = (ctypes.c_int * 2)()
    _check(_native.lib().rtvObjAttributesHost(os.fsencode(path), normals.ctypes.data, uvs.ctypes.data, have))
    return normals, uvs, bool(have[0]), bool(have[1])


def _ptr(x) -> int:
    if x is None:
        return 0
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    return int(x)


def _stream(s) -> int:
    if s is None:
        return 0
    if hasattr(s, "cuda_stream"):
        return s.cuda_stream
    return int(s)


class ReflectionScratch:
    """What DeviceScene.render_reflection() keeps of the bounce between its steps, for a width x
    height frame on cuda:device: rays (1, H, W, 8) float32, ids (H * W,) int32 and t (H * W,)
    float32 -- the bounce's hits, there to be read after the call."""

    def __init__(self, width: int, height: int, device: int = 0):
        import torch

        dev = torch.device("cuda", device)
        self.width, self.height = width, height
        self.rays = torch.empty((1, height, width, 8), dtype=torch.float32, device=dev)
        self.ids = torch.empty((height * width,), dtype=torch.int32, device=dev)
        self.t = torch.empty((height * width,), dtype=torch.float32, device=dev)


class DeviceScene:
    """A scene resident on one HIP device."""

    def __init__(self, path: str, device: int = 0, camera=None):
        """camera: 10 floats (eye, lookat, up, vfov_deg) replacing the file's camera (rtlSceneCreate),
        a spot light's for instance; None keeps the file's."""
        self._lib = _native.lib()
        self.handle = None
        self._owned = True
        if camera is None:
            self.handle = self._lib.srtDeviceSceneCreate(os.fsencode(path), device)
        else:
            self.handle = self._lib.rtlSceneCreate(os.fsencode(path), device, _camera10(camera))
        if not self.handle:
            raise SrtError(_native.last_error())
        self.device = device
        self.path = path
        self.triangles = self._lib.srtDeviceSceneTriangles(self.handle)
        self.width = 0
        self.height = 0

    @classmethod
    def _borrowed(cls, handle, device: int, path: str, size: int):
        """A view of a device scene another object owns (OmniLight.face): close() releases nothing."""
        self = cls.__new__(cls)
        self._lib = _native.lib()
        self.handle = handle
        self._owned = False
        self.device = device
        self.path = path
        self.triangles = self._lib.srtDeviceSceneTriangles(handle)
        self.width = self.height = size
        return self

    def prepare(self, width: int, height: int, stream=None):
        _check(self._lib.srtPrepareAsync(self.handle, width, height, _stream(stream)))
        self.width, self.height = width, height

    def _check_buffer(self, name, buf, rows, channels, dtype):
        """Shape / contiguity, and for torch tensors dtype and device: the kernels read and write
        raw pointers on self.device with these element types."""
        want = (rows, self.width) + ((channels,) if channels else ())
        if hasattr(buf, "shape") and tuple(buf.shape) != want:
            raise ValueError(f"{name} must be {want}, got {tuple(buf.shape)}")
        self._check_tensor(name, buf, dtype)

    def _check_tensor(self, name, buf, dtype):
        if hasattr(buf, "is_contiguous") and not buf.is_contiguous():
            raise ValueError(f"{name} must be contiguous")
        if hasattr(buf, "is_cuda"):
            import torch

            want_dtype = {"f32": torch.float32, "i32": torch.int32, "u8": torch.uint8}[dtype]
            if buf.dtype != want_dtype:
                raise ValueError(f"{name} must be {want_dtype}, got {buf.dtype}")
            if not buf.is_cuda or buf.device.index != self.device:
                raise ValueError(f"{name} must live on cuda:{self.device}, got {buf.device}")

    def trace(self, offsets, rgba, row_begin: int = 0, row_count: int | None = None, variant: str = "cull",
              stream=None):
        """offsets: (rows, W, 2) float32 device buffer; rgba: (rows, W, 4) float32 device buffer."""
        if row_count is None:
            row_count = self.height - row_begin
        self._check_buffer("offsets", offsets, row_count, 2, "f32")
        self._check_buffer("rgba", rgba, row_count, 4, "f32")
        _check(self._lib.srtTraceAsync(self.handle, _ptr(offsets), _ptr(rgba), row_begin, row_count,
                                       TRACE_VARIANTS[variant], _stream(stream)))

    def trace_ids(self, offsets, ids, row_begin: int = 0, row_count: int | None = None, variant: str = "cull",
                  stream=None):
        """Hit ids only (deferred shading): offsets (rows, W, 2) float32, ids (rows, W) int32."""
        if row_count is None:
            row_count = self.height - row_begin
        self._check_buffer("offsets", offsets, row_count, 2, "f32")
        self._check_buffer("ids", ids, row_count, 0, "i32")
        _check(self._lib.srtTraceIdsAsync(self.handle, _ptr(offsets), _ptr(ids), row_begin, row_count,
                                          TRACE_VARIANTS[variant], _stream(stream)))

    def bind_trace_ids(self, offsets, ids, row_begin: int = 0, row_count: int | None = None, variant: str = "cull",
                       stream=None):
        """prepare + trace_ids of this band as a zero-argument callable: the buffers are checked
        once here, each call is then just the two C-ABI calls (a frame loop's host cost is the
        HIP launches, not Python checks). The buffers must stay alive while it is used."""
        if row_count is None:
            row_count = self.height - row_begin
        self._check_buffer("offsets", offsets, row_count, 2, "f32")
        self._check_buffer("ids", ids, row_count, 0, "i32")
        lib, h, w, hh = self._lib, self.handle, self.width, self.height
        op, ip, s, v = _ptr(offsets), _ptr(ids), _stream(stream), TRACE_VARIANTS[variant]

        def run():
            _check(lib.srtPrepareAsync(h, w, hh, s))
            _check(lib.srtTraceIdsAsync(h, op, ip, row_begin, row_count, v, s))

        return run

    def bind_trace_batch(self, offsets, outs, row_begin: int = 0, row_count: int | None = None, variant: str = "cull",
                         stream=None, ids: bool = False, row_interleave: int = 1):
        """prepare + trace of len(outs) (<= MAX_BATCH) frames of this band as a zero-argument
        callable (srtTraceBatchAsync): frame f's sample offsets offsets[f] ((rows, W, 2) float32)
        and its output outs[f] ((rows, W) int32 hit ids with ids=True, else (rows, W, 4) float32
        RGBA). Every frame gets the whole per-frame work; the cull variant launches each stage
        once for the batch. row_interleave P > 1: the band is tile rows row_begin / 16 + k P of
        the frame (bands.interleaved_range). Checked once here; the buffers must stay alive
        while it is used."""
        if row_count is None:
            row_count = self.height - row_begin
        frames = len(outs)
        if frames > MAX_BATCH or len(offsets) != frames:
            raise ValueError(f"1 to {MAX_BATCH} frames, one offsets buffer per output")
        for f in range(frames):
            self._check_buffer(f"offsets[{f}]", offsets[f], row_count, 2, "f32")
            self._check_buffer(f"outs[{f}]", outs[f], row_count, 0 if ids else 4, "i32" if ids else "f32")
        arr = ctypes.c_void_p * max(1, frames)
        offs = arr(*[_ptr(o) for o in offsets])
        out = arr(*[_ptr(o) for o in outs])
        rgba, idp = (None, out) if ids else (out, None)
        lib, h, w, hh = self._lib, self.handle, self.width, self.height
        s, v = _stream(stream), TRACE_VARIANTS[variant]

        def run():
            _check(lib.srtPrepareAsync(h, w, hh, s))
            _check(lib.srtTraceBatchAsync(h, offs, rgba, idp, frames, row_begin, row_count, row_interleave, v, s))

        run.keep = (offsets, outs, offs, out)  # the pointer arrays live as long as the callable
        return run

    def trace_batch(self, offsets, outs, row_begin: int = 0, row_count: int | None = None, variant: str = "cull",
                    stream=None, ids: bool = False, row_interleave: int = 1):
        """One batched call (bind_trace_batch) run once."""
        self.bind_trace_batch(offsets, outs, row_begin, row_count, variant, stream, ids, row_interleave)()

    def pin_offsets(self, offsets, stream=None):
        """Pins a whole-frame offsets buffer ((H, W, 2) float32 on this device; rtnPinOffsetsAsync):
        its tile classification is computed once and every later whole-frame cull trace given this
        buffer skips that pass. While pinned the buffer is neither written nor freed; pinning it
        again announces new contents. At most MAX_PINS per scene; preparing at another size drops
        every pin."""
        if self.width:  # (an unprepared scene has no frame shape to check against: the library refuses it)
            self._check_buffer("offsets", offsets, self.height, 2, "f32")
        _check(self._lib.rtnPinOffsetsAsync(self.handle, _ptr(offsets), _stream(stream)))

    def unpin_offsets(self, offsets):
        """Forgets the pin of `offsets` (rtnUnpinOffsets; not pinned: nothing). Waits for the scene's
        enqueued work first."""
        _check(self._lib.rtnUnpinOffsets(self.handle, _ptr(offsets)))

    def shade(self, offsets, ids, rgba, row_begin: int = 0, row_count: int | None = None, stream=None):
        """Deferred shading of the prepared frame's rows from hit ids: the RGBA trace() stores."""
        if row_count is None:
            row_count = self.height - row_begin
        self._check_buffer("offsets", offsets, row_count, 2, "f32")
        self._check_buffer("ids", ids, row_count, 0, "i32")
        self._check_buffer("rgba", rgba, row_count, 4, "f32")
        _check(self._lib.srtShadeAsync(self.handle, _ptr(offsets), _ptr(ids), _ptr(rgba), row_begin, row_count,
                                       _stream(stream)))

    def shade_bands(self, offsets, ids, rgba, band_rows: int, stream=None, interleaved: int = 0):
        """Deferred shading of a batch of frames whose ids were gathered band-major:
        ids (bands, frames, band_rows, W) int32 (bands = ceil(H / band_rows) contiguous bands, or
        `interleaved` bands dealt the frame's tile rows round-robin), offsets (H, W, 2),
        rgba (frames, H, W, 4); one launch (srtShadeBandsAsync)."""
        if band_rows <= 0:
            raise ValueError("band_rows must be positive")
        bands = interleaved if interleaved else (self.height + band_rows - 1) // band_rows
        frames = ids.shape[1] if hasattr(ids, "shape") and len(ids.shape) == 4 else 0
        self._check_buffer("offsets", offsets, self.height, 2, "f32")
        # contiguous bands: a gather over P ranks may carry more (empty, trailing) bands than the
        # ceil(H / band_rows) that hold rows; the kernel never reads them
        if hasattr(ids, "shape") and (len(ids.shape) != 4 or tuple(ids.shape[2:]) != (band_rows, self.width) or
                                      (ids.shape[0] != bands if interleaved else ids.shape[0] < bands)):
            raise ValueError(f"ids must be {(bands, 'frames', band_rows, self.width)}, got {tuple(ids.shape)}")
        if hasattr(rgba, "shape") and tuple(rgba.shape) != (frames, self.height, self.width, 4):
            raise ValueError(f"rgba must be {(frames, self.height, self.width, 4)}, got {tuple(rgba.shape)}")
        for name, buf, dtype in (("ids", ids, "i32"), ("rgba", rgba, "f32")):
            self._check_tensor(name, buf, dtype)
        _check(self._lib.srtShadeBandsAsync(self.handle, _ptr(offsets), _ptr(ids), _ptr(rgba), frames, band_rows,
                                            interleaved, _stream(stream)))

    def query(self, positions, ids, t, how=None, stream=None):
        """Point queries (include/srt_query.h): the closest hit at arbitrary image positions of the
        prepared frame. positions (count, 2) float32 -> ids (count,) int32 (-1 = miss), t (count,)
        float32 (+inf = miss) and, optionally, how (count,) uint8: 0 = answered from the tile's
        list, 1 = every record streamed. Device buffers, checked like trace()'s."""
        count = None
        for name, buf, tail, dtype in (("positions", positions, (2,), "f32"), ("ids", ids, (), "i32"),
                                       ("t", t, (), "f32"), ("how", how, (), "u8")):
            if buf is None and name == "how":
                continue
            if hasattr(buf, "shape"):
                shape = tuple(buf.shape)
                if len(shape) != 1 + len(tail) or shape[1:] != tail or (count is not None and shape[0] != count):
                    want = ("count" if count is None else count,) + tail
                    raise ValueError(f"{name} must be {want}, got {shape}")
                count = shape[0]
            self._check_tensor(name, buf, dtype)
        if count is None:
            raise ValueError("positions must have a shape (count, 2): raw pointers carry no count")
        _check(self._lib.rtqQueryAsync(self.handle, _ptr(positions), count, _ptr(ids), _ptr(t), _ptr(how),
                                       _stream(stream)))

    def _layer_planes(self, ids, t, lead):
        """The layer count K of ids (K,) + lead int32, with t (the same shape, float32) checked
        against it."""
        if not hasattr(ids, "shape"):
            raise ValueError(f"ids must have a shape {('layers',) + lead}: raw pointers carry no layer count")
        shape = tuple(ids.shape)
        if len(shape) != 1 + len(lead) or shape[1:] != lead or not 1 <= shape[0] <= RTK_MAX_LAYERS:
            raise ValueError(f"ids must be {(f'1..{RTK_MAX_LAYERS} layers',) + lead}, got {shape}")
        self._check_tensor("ids", ids, "i32")
        if t is not None:
            if hasattr(t, "shape") and tuple(t.shape) != shape:
                raise ValueError(f"t must be {shape}, got {tuple(t.shape)}")
            self._check_tensor("t", t, "f32")
        return shape[0]

    def layers(self, positions, ids, t=None, how=None, stream=None):
        """Depth layers (include/srt_layers.h): the K nearest hits, front to back, at arbitrary
        image positions of the prepared frame. positions (count, 2) float32 -> ids (K, count) int32
        (-1 = no such layer) and, optionally, t (K, count) float32 (+inf) and how (count,) uint8 as
        query()'s; K = ids.shape[0], 1 to 8. Layer 0 is query()'s answer."""
        if not hasattr(positions, "shape") or len(positions.shape) != 2 or positions.shape[1] != 2:
            raise ValueError("positions must have a shape (count, 2): raw pointers carry no count")
        count = positions.shape[0]
        self._check_tensor("positions", positions, "f32")
        layers = self._layer_planes(ids, t, (count,))
        if how is not None:
            if hasattr(how, "shape") and tuple(how.shape) != (count,):
                raise ValueError(f"how must be {(count,)}, got {tuple(how.shape)}")
            self._check_tensor("how", how, "u8")
        _check(self._lib.rtkLayersAsync(self.handle, _ptr(positions), count, layers, _ptr(ids), _ptr(t), _ptr(how),
                                        _stream(stream)))

    def layer_frame(self, offsets, ids, t=None, how=None, row_begin: int = 0, row_count: int | None = None,
                    stream=None):
        """Depth layers at the pixels of the prepared frame's rows (rtkFrameAsync): offsets (rows, W,
        2) float32 -> ids (K, rows, W) int32, t (K, rows, W) float32 and how (rows, W) uint8, the
        last two optional. Plane ids[k] is what trace_ids() would store if the k nearer surfaces
        were not there: it feeds shade(), gbuffer() and composite()."""
        if row_count is None:
            row_count = self.height - row_begin
        self._check_buffer("offsets", offsets, row_count, 2, "f32")
        layers = self._layer_planes(ids, t, (row_count, self.width))
        if how is not None:
            self._check_buffer("how", how, row_count, 0, "u8")
        _check(self._lib.rtkFrameAsync(self.handle, _ptr(offsets), row_begin, row_count, layers, _ptr(ids), _ptr(t),
                                       _ptr(how), _stream(stream)))

    def composite(self, offsets, ids, opacity, rgba, row_begin: int = 0, row_count: int | None = None, stream=None):
        """Over-composite of the rows' depth layers (rtkCompositeAsync): offsets (rows, W, 2) float32,
        ids (K, rows, W) int32 as layer_frame() stores them and opacity (triangles,) float32, one
        value per triangle -> rgba (rows, W, 4) float32: the layers' shades composited front to back
        over the background, alpha = 1 - the transmittance left."""
        if row_count is None:
            row_count = self.height - row_begin
        self._check_buffer("offsets", offsets, row_count, 2, "f32")
        layers = self._layer_planes(ids, None, (row_count, self.width))
        if hasattr(opacity, "shape") and tuple(opacity.shape) != (self.triangles,):
            raise ValueError(f"opacity must be {(self.triangles,)}, got {tuple(opacity.shape)}")
        self._check_tensor("opacity", opacity, "f32")
        self._check_buffer("rgba", rgba, row_count, 4, "f32")
        _check(self._lib.rtkCompositeAsync(self.handle, _ptr(offsets), _ptr(ids), layers, _ptr(opacity), row_begin,
                                           row_count, _ptr(rgba), _stream(stream)))

    def _outputs(self, planes, lead):
        """rtg_outputs of the planes depth / bary / normal / albedo (None: not written), each
        checked to be `lead` + its channel tail."""
        out = _native.RtgOutputs(ctypes.sizeof(_native.RtgOutputs), 0, 0, 0, 0)
        for name, buf, tail in planes:
            if buf is None:
                continue
            if hasattr(buf, "shape") and tuple(buf.shape) != lead + tail:
                raise ValueError(f"{name} must be {lead + tail}, got {tuple(buf.shape)}")
            self._check_tensor(name, buf, "f32")
            setattr(out, name, _ptr(buf))
        return out

    def gbuffer(self, offsets, ids, depth=None, bary=None, normal=None, albedo=None, row_begin: int = 0,
                row_count: int | None = None, stream=None):
        """G-buffer of the prepared frame's rows from hit ids (include/srt_gbuffer.h): offsets
        (rows, W, 2) float32 and ids (rows, W) int32 -> any of depth (rows, W), bary (rows, W, 2),
        normal (rows, W, 4) = (unit normal towards the eye, shading cosine), albedo (rows, W, 4) =
        (r, g, b, float(id)), float32 device buffers; a plane left None is not written."""
        if row_count is None:
            row_count = self.height - row_begin
        self._check_buffer("offsets", offsets, row_count, 2, "f32")
        self._check_buffer("ids", ids, row_count, 0, "i32")
        out = self._outputs((("depth", depth, ()), ("bary", bary, (2,)), ("normal", normal, (4,)),
                             ("albedo", albedo, (4,))), (row_count, self.width))
        _check(self._lib.rtgFrameAsync(self.handle, _ptr(offsets), _ptr(ids), row_begin, row_count, ctypes.byref(out),
                                       _stream(stream)))

    def attributes(self, positions, ids, depth=None, bary=None, normal=None, albedo=None, stream=None):
        """G-buffer at arbitrary image positions: positions (count, 2) float32 and ids (count,)
        int32 -- query()'s input and output -- -> any of depth (count,), bary (count, 2), normal
        (count, 4), albedo (count, 4), as gbuffer()'s."""
        count = self._elements(positions, ids)
        out = self._outputs((("depth", depth, ()), ("bary", bary, (2,)), ("normal", normal, (4,)),
                             ("albedo", albedo, (4,))), (count,))
        _check(self._lib.rtgPointsAsync(self.handle, _ptr(positions), _ptr(ids), count, ctypes.byref(out),
                                        _stream(stream)))

    def _elements(self, positions, ids):
        """count of a (positions (count, 2) float32, ids (count,) int32) pair, checked as attributes() does."""
        count = None
        for name, buf, tail, dtype in (("positions", positions, (2,), "f32"), ("ids", ids, (), "i32")):
            if hasattr(buf, "shape"):
                shape = tuple(buf.shape)
                if len(shape) != 1 + len(tail) or shape[1:] != tail or (count is not None and shape[0] != count):
                    want = ("count" if count is None else count,) + tail
                    raise ValueError(f"{name} must be {want}, got {shape}")
                count = shape[0]
            self._check_tensor(name, buf, dtype)
        if count is None:
            raise ValueError("positions must have a shape (count, 2): raw pointers carry no count")
        return count

    def _surface(self, surface, planes, lead):
        """(rtv_surface, rtv_outputs) of a Surface and the planes normal / albedo / rgba / uv (None:
        not written), the tables checked against this scene and each plane to be `lead` + its tail."""
        if not isinstance(surface, Surface):
            raise ValueError(f"surface must be a Surface, got {type(surface).__name__}")
        n = self.triangles
        for name, buf, tail in (("normals", surface.normals, (3, 3)), ("uvs", surface.uvs, (3, 2))):
            if buf is None:
                continue
            flat = (n, tail[0] * tail[1])
            if hasattr(buf, "shape") and tuple(buf.shape) not in ((n,) + tail, flat):
                raise ValueError(f"{name} must be {(n,) + tail} or {flat}, got {tuple(buf.shape)}")
            self._check_tensor(name, buf, "f32")
        if surface.texture is not None:
            shape = tuple(surface.texture.shape) if hasattr(surface.texture, "shape") else None
            if shape is None or len(shape) != 3 or shape[2] != 4:
                raise ValueError(f"texture must be (TH, TW, 4), got {shape}")
            self._check_tensor("texture", surface.texture, "f32")
        out = _native.RtvOutputs(ctypes.sizeof(_native.RtvOutputs), 0, 0, 0, 0)
        for name, buf, tail in planes:
            if buf is None:
                continue
            if hasattr(buf, "shape") and tuple(buf.shape) != lead + tail:
                raise ValueError(f"{name} must be {lead + tail}, got {tuple(buf.shape)}")
            self._check_tensor(name, buf, "f32")
            setattr(out, name, _ptr(buf))
        return surface._struct(_ptr), out

    def _table(self, table, out, lead):
        """channels of a corner table (triangles, 3, C) or (triangles, 3 C) with out `lead` + (C,)."""
        if not hasattr(out, "shape") or len(out.shape) != len(lead) + 1 or tuple(out.shape[:-1]) != lead:
            raise ValueError(f"out must be {lead + ('C',)}, got {tuple(getattr(out, 'shape', ()))}")
        channels = int(out.shape[-1])
        if not 1 <= channels <= RTV_MAX_CHANNELS:
            raise ValueError(f"out must have 1 to {RTV_MAX_CHANNELS} channels, got {channels}")
        want = ((self.triangles, 3, channels), (self.triangles, 3 * channels))
        if hasattr(table, "shape") and tuple(table.shape) not in want:
            raise ValueError(f"table must be {want[0]} or {want[1]}, got {tuple(table.shape)}")
        self._check_tensor("table", table, "f32")
        self._check_tensor("out", out, "f32")
        return channels

    def surface_frame(self, offsets, ids, surface, normal=None, albedo=None, rgba=None, uv=None, row_begin: int = 0,
                      row_count: int | None = None, stream=None):
        """What the surface looks like at the prepared frame's rows, from hit ids (include/srt_surface.h):
        offsets (rows, W, 2) float32, ids (rows, W) int32 and a Surface of device tables -> any of
        normal (rows, W, 4) = (smooth unit normal towards the eye, shading cosine), albedo (rows, W,
        4) = (textured r, g, b, float(id)), rgba (rows, W, 4) = (albedo.rgb * cosine, float(id)), uv
        (rows, W, 2), float32 device buffers; a plane left None is not written."""
        if row_count is None:
            row_count = self.height - row_begin
        self._check_buffer("offsets", offsets, row_count, 2, "f32")
        self._check_buffer("ids", ids, row_count, 0, "i32")
        s, out = self._surface(surface, (("normal", normal, (4,)), ("albedo", albedo, (4,)), ("rgba", rgba, (4,)),
                                         ("uv", uv, (2,))), (row_count, self.width))
        _check(self._lib.rtvSurfaceFrameAsync(self.handle, _ptr(offsets), _ptr(ids), row_begin, row_count,
                                              ctypes.byref(s), ctypes.byref(out), _stream(stream)))

    def surface(self, positions, ids, surface, normal=None, albedo=None, rgba=None, uv=None, stream=None):
        """surface_frame() at arbitrary image positions: positions (count, 2) float32 and ids (count,)
        int32 -- query()'s input and output -- -> any of normal, albedo, rgba (count, 4), uv (count, 2)."""
        count = self._elements(positions, ids)
        s, out = self._surface(surface, (("normal", normal, (4,)), ("albedo", albedo, (4,)), ("rgba", rgba, (4,)),
                                         ("uv", uv, (2,))), (count,))
        _check(self._lib.rtvSurfacePointsAsync(self.handle, _ptr(positions), _ptr(ids), count, ctypes.byref(s),
                                               ctypes.byref(out), _stream(stream)))

    def interpolate_frame(self, offsets, ids, table, out, row_begin: int = 0, row_count: int | None = None,
                          stream=None):
        """One per-corner table carried to the prepared frame's rows (rtvInterpolateFrameAsync): table
        (triangles, 3, C) float32, 1 <= C <= 4, -> out (rows, W, C) float32, the three corner values
        of each pixel's triangle under its perspective-correct weights; 0 where the id is no triangle."""
        if row_count is None:
            row_count = self.height - row_begin
        self._check_buffer("offsets", offsets, row_count, 2, "f32")
        self._check_buffer("ids", ids, row_count, 0, "i32")
        channels = self._table(table, out, (row_count, self.width))
        _check(self._lib.rtvInterpolateFrameAsync(self.handle, _ptr(offsets), _ptr(ids), row_begin, row_count,
                                                  _ptr(table), channels, _ptr(out), _stream(stream)))

    def interpolate(self, positions, ids, table, out, stream=None):
        """interpolate_frame() at arbitrary image positions: positions (count, 2), ids (count,) -> out (count, C)."""
        count = self._elements(positions, ids)
        channels = self._table(table, out, (count,))
        _check(self._lib.rtvInterpolatePointsAsync(self.handle, _ptr(positions), _ptr(ids), count, _ptr(table),
                                                   channels, _ptr(out), _stream(stream)))

    def shadow(self, light, offsets, ids, mask, rgba=None, bias: float = 0.0, dim: float = 0.0, row_begin: int = 0,
               row_count: int | None = None, stream=None):
        """Spot-light shadow mask of the prepared frame's rows (include/srt_light.h): `light` is a
        prepared DeviceScene of the same triangles under the light's camera (DeviceScene(path,
        device, camera=...)). offsets (rows, W, 2) float32 and ids (rows, W) int32 as trace_ids()
        stores them -> mask (rows, W) uint8: 0 shadowed, 1 lit, 2 outside the light's frustum, 3 no
        surface; rgba (rows, W, 4) float32, optional: shade()'s pixel, rgb times 1 (class 1) or dim
        (classes 0 and 2). bias: relative depth bias >= 0. Device buffers, checked like trace()'s."""
        if row_count is None:
            row_count = self.height - row_begin
        self._check_buffer("offsets", offsets, row_count, 2, "f32")
        self._check_buffer("ids", ids, row_count, 0, "i32")
        self._check_buffer("mask", mask, row_count, 0, "u8")
        if rgba is not None:
            self._check_buffer("rgba", rgba, row_count, 4, "f32")
        _check(self._lib.rtlShadowAsync(self.handle, light.handle, _ptr(offsets), _ptr(ids), row_begin, row_count, bias,
                                        _ptr(mask), _ptr(rgba), dim, _stream(stream)))

    def _sample_planes(self, offsets, ids, rows):
        """The pointer arrays of S sample planes: offsets[s] (rows, W, 2) float32 and ids[s]
        (rows, W) int32, checked like trace_ids()'s."""
        if len(offsets) != len(ids):
            raise ValueError(f"one ids plane per offsets plane, got {len(offsets)} and {len(ids)}")
        samples = len(ids)
        if not 1 <= samples <= RTS_MAX_SAMPLES:
            raise ValueError(f"1 to {RTS_MAX_SAMPLES} sample planes, got {samples}")
        for s in range(samples):
            self._check_buffer(f"offsets[{s}]", offsets[s], rows, 2, "f32")
            self._check_buffer(f"ids[{s}]", ids[s], rows, 0, "i32")
        arr = ctypes.c_void_p * samples
        return arr(*[_ptr(o) for o in offsets]), arr(*[_ptr(i) for i in ids]), samples

    def resolve(self, offsets, ids, rgba, row_begin: int = 0, row_count: int | None = None, stream=None):
        """Resolve of the prepared frame's rows from S sample planes (include/srt_samples.h):
        offsets, a sequence of S (rows, W, 2) float32 buffers, and ids, S (rows, W) int32 buffers
        as trace_ids() stores them -> rgba (rows, W, 4) float32: the mean of the S shaded samples
        (summed in order), alpha = the share of the samples that hit. Device buffers: tensors or
        raw pointers."""
        if row_count is None:
            row_count = self.height - row_begin
        offs, idp, samples = self._sample_planes(offsets, ids, row_count)
        self._check_buffer("rgba", rgba, row_count, 4, "f32")
        _check(self._lib.rtsResolveAsync(self.handle, offs, idp, samples, row_begin, row_count, _ptr(rgba),
                                         _stream(stream)))

    def render_samples(self, offsets, ids, rgba, variant: str = "cull", stream=None):
        """S samples per pixel of the whole prepared frame (rtsRenderAsync): traces the S id planes
        into ids[s] ((H, W) int32; they stay available) for offsets[s] ((H, W, 2) float32), then
        resolves them into rgba (H, W, 4) as resolve() does."""
        offs, idp, samples = self._sample_planes(offsets, ids, self.height)
        self._check_buffer("rgba", rgba, self.height, 4, "f32")
        _check(self._lib.rtsRenderAsync(self.handle, offs, idp, samples, _ptr(rgba), TRACE_VARIANTS[variant],
                                        _stream(stream)))

    @property
    def camera(self):
        """The scene's camera (eye, lookat, up, vfov_deg: 10 floats): the file's, the constructor's
        or the last one set (rtmGetCamera; host state, no device work)."""
        cam = (ctypes.c_float * 10)()
        _check(self._lib.rtmGetCamera(self.handle, cam))
        return tuple(cam)

    def set_camera(self, camera, reorder: bool = True, stream=None):
        """Move the camera in place (include/srt_motion.h): afterwards every call answers as a fresh
        DeviceScene(path, device, camera=camera) would, bit for bit; a prepared scene stays prepared.
        reorder=True rebuilds the spatial order under the new camera on `stream`; False keeps the
        standing order (no kernel at all: the same answers, only speed differs)."""
        _check(self._lib.rtmSetCameraAsync(self.handle, _camera10(camera), RTM_REORDER if reorder else RTM_KEEP_ORDER,
                                           _stream(stream)))

    def _check_vertices(self, vertices):
        if hasattr(vertices, "shape") and tuple(vertices.shape) not in ((self.triangles, 9), (self.triangles, 3, 3)):
            raise ValueError(f"vertices must be {(self.triangles, 9)} or {(self.triangles, 3, 3)}, "
                             f"got {tuple(vertices.shape)}")
        self._check_tensor("vertices", vertices, "f32")

    def set_vertices(self, vertices, reorder: bool = True, stream=None):
        """Move the triangles in place (rtmSetVerticesAsync): vertices (n, 9) or (n, 3, 3) float32, a
        contiguous device buffer read on `stream` (reusable once the stream has passed the call). The
        triangle count and the albedo stay. Afterwards every call answers as a fresh scene over a
        file of these vertices would. reorder as set_camera()'s; with False the shading normals and
        the vertices' spatial copy are still rewritten."""
        self._check_vertices(vertices)
        _check(self._lib.rtmSetVerticesAsync(self.handle, _ptr(vertices), RTM_REORDER if reorder else RTM_KEEP_ORDER,
                                             _stream(stream)))

    def _ray_count(self, buffers):
        """count of a ray call's buffers, (name, buffer, tail, dtype) with the rays first: shapes
        (count,) + tail, checked like query()'s."""
        count = None
        for name, buf, tail, dtype in buffers:
            if buf is None:
                continue
            if hasattr(buf, "shape"):
                shape = tuple(buf.shape)
                if len(shape) != 1 + len(tail) or shape[1:] != tail or (count is not None and shape[0] != count):
                    want = ("count" if count is None else count,) + tail
                    raise ValueError(f"{name} must be {want}, got {shape}")
                count = shape[0]
            self._check_tensor(name, buf, dtype)
        if count is None:
            raise ValueError("rays must have a shape (count, 8): raw pointers carry no count")
        return count

    def build_rays(self, stream=None):
        """Build the world-space tree of the ray queries now (rtrBuildAsync), on `stream`, if it is
        missing or stale; closest() and occluded() do so themselves otherwise."""
        _check(self._lib.rtrBuildAsync(self.handle, _stream(stream)))

    def closest(self, rays, ids, t, bary=None, stream=None):
        """Ray queries (include/srt_rays.h): the closest hit of caller-supplied rays. rays (count, 8)
        float32 = (ox, oy, oz, tmin, dx, dy, dz, tmax), d not normalised, t in units of d -> ids
        (count,) int32 (-1 = miss), t (count,) float32 (+inf = miss) and, optionally, bary (count, 2)
        float32: the weights of v1 and v2. No prepare() is needed: the answer does not depend on the
        camera. Device buffers, checked like query()'s."""
        count = self._ray_count((("rays", rays, (8,), "f32"), ("ids", ids, (), "i32"), ("t", t, (), "f32"),
                                 ("bary", bary, (2,), "f32")))
        _check(self._lib.rtrClosestAsync(self.handle, _ptr(rays), count, _ptr(ids), _ptr(t), _ptr(bary),
                                         _stream(stream)))

    def occluded(self, rays, out, stream=None):
        """Occlusion of caller-supplied rays (rtrOccludedAsync): rays (count, 8) float32 as
        closest()'s -> out (count,) uint8: 1 iff any triangle counts for the ray within its range."""
        count = self._ray_count((("rays", rays, (8,), "f32"), ("out", out, (), "u8")))
        _check(self._lib.rtrOccludedAsync(self.handle, _ptr(rays), count, _ptr(out), _stream(stream)))

    def _generator(self, generator):
        """rta_generator of a holder of device tables, each checked to be float32 on this device."""
        for name, table in generator._tables():
            if table is not None:
                self._check_tensor(name, table, "f32")
        return generator._struct(_ptr)

    def _visibility_outputs(self, visible, fraction, lead):
        out = _native.RtaOutputs(ctypes.sizeof(_native.RtaOutputs), 0, 0)
        for name, buf, dtype in (("visible", visible, "u8"), ("fraction", fraction, "f32")):
            if buf is None:
                continue
            if hasattr(buf, "shape") and tuple(buf.shape) != lead:
                raise ValueError(f"{name} must be {lead}, got {tuple(buf.shape)}")
            self._check_tensor(name, buf, dtype)
            setattr(out, name, _ptr(buf))
        return out

    def _check_rays_out(self, rays, lead):
        if hasattr(rays, "shape") and tuple(rays.shape) != lead + (8,):
            raise ValueError(f"rays must be {lead + (8,)}, got {tuple(rays.shape)}")
        self._check_tensor("rays", rays, "f32")

    def visibility(self, positions, ids, generator, visible=None, fraction=None, stream=None):
        """Sampled visibility (include/srt_visibility.h) at arbitrary image positions of the prepared
        frame: positions (count, 2) float32 and ids (count,) int32 -- query()'s input and output --
        and a Hemisphere or an AreaLight of device tables -> visible (count,) uint8, how many of the
        generator's S rays from the surface point are unoccluded, and fraction (count,) float32 =
        visible / S; a plane left None is not written. One launch: the rays are generated and walked
        through the ray queries' tree in the kernel."""
        count = self._elements(positions, ids)
        g = self._generator(generator)
        out = self._visibility_outputs(visible, fraction, (count,))
        _check(self._lib.rtaVisibilityPointsAsync(self.handle, _ptr(positions), _ptr(ids), count, ctypes.byref(g),
                                                  ctypes.byref(out), _stream(stream)))

    def visibility_frame(self, offsets, ids, generator, visible=None, fraction=None, row_begin: int = 0,
                         row_count: int | None = None, stream=None):
        """Sampled visibility of the prepared frame's rows from hit ids: offsets (rows, W, 2) float32
        and ids (rows, W) int32, band-local -> visible (rows, W) uint8 and fraction (rows, W) float32
        as visibility()'s. A Hemisphere's rotations are indexed by the pixel's place in its 4 x 4
        block of the whole frame."""
        if row_count is None:
            row_count = self.height - row_begin
        self._check_buffer("offsets", offsets, row_count, 2, "f32")
        self._check_buffer("ids", ids, row_count, 0, "i32")
        g = self._generator(generator)
        out = self._visibility_outputs(visible, fraction, (row_count, self.width))
        _check(self._lib.rtaVisibilityFrameAsync(self.handle, _ptr(offsets), _ptr(ids), row_begin, row_count,
                                                 ctypes.byref(g), ctypes.byref(out), _stream(stream)))

    def generate_rays(self, positions, ids, generator, rays, stream=None):
        """The generator's rays themselves, for closest() / occluded(): positions and ids as
        visibility()'s -> rays (S, count, 8) float32, sample-major (plane s holds sample s of every
        element). A Mirror generator (S = 1) gives the primary rays' mirror bounces."""
        count = self._elements(positions, ids)
        g = self._generator(generator)
        self._check_rays_out(rays, (generator.count, count))
        _check(self._lib.rtaRaysPointsAsync(self.handle, _ptr(positions), _ptr(ids), count, ctypes.byref(g),
                                            _ptr(rays), _stream(stream)))

    def generate_rays_frame(self, offsets, ids, generator, rays, row_begin: int = 0, row_count: int | None = None,
                            stream=None):
        """generate_rays() for the prepared frame's rows: offsets and ids as visibility_frame()'s ->
        rays (S, rows, W, 8) float32."""
        if row_count is None:
            row_count = self.height - row_begin
        self._check_buffer("offsets", offsets, row_count, 2, "f32")
        self._check_buffer("ids", ids, row_count, 0, "i32")
        g = self._generator(generator)
        self._check_rays_out(rays, (generator.count, row_count, self.width))
        _check(self._lib.rtaRaysFrameAsync(self.handle, _ptr(offsets), _ptr(ids), row_begin, row_count, ctypes.byref(g),
                                           _ptr(rays), _stream(stream)))

    def spatial_order(self):
        """(order, build_ms): the record ids in spatial order (numpy uint32), built on the device
        at load (and again by a reordering set_camera() / set_vertices()), and the load-time build's
        device time."""
        import numpy as np

        out = np.empty(max(1, self.triangles), np.uint32)
        ms = ctypes.c_double()
        _check(self._lib.srtDeviceSceneOrder(self.handle, out.ctypes.data, out.size, ctypes.byref(ms)))
        return out[:self.triangles], ms.value

    def set_stage_timing(self, enable: bool = True):
        """Bind HIP events to the prepare, bin and trace kernels' dispatches (no extra packets)."""
        _check(self._lib.srtSetStageTiming(self.handle, 1 if enable else 0))

    def take_stage_times(self):
        """(timed trace calls, mean prepare ms, mean bin-stage ms, mean trace-kernel ms) since the
        last take; waits for the events."""
        n, p, b, t = ctypes.c_uint(), ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
        _check(self._lib.srtTakeStageTimes(self.handle, ctypes.byref(n), ctypes.byref(p), ctypes.byref(b),
                                           ctypes.byref(t)))
        return n.value, p.value, b.value, t.value

    def omni_shadow(self, light, offsets, ids, mask, face=None, rgba=None, bias: float = 0.0, dim: float = 0.0,
                    row_begin: int = 0, row_count: int | None = None, stream=None):
        """Omni-light shadow mask of the prepared frame's rows (include/srt_omni.h): `light` is a
        prepared OmniLight of the same triangles. offsets, ids, mask, rgba, bias, dim as shadow()'s;
        face (rows, W) uint8, optional: the cube face each pixel selected, 255 for a class-3 pixel.
        One launch: every pixel runs shadow()'s test in its own face's frame only."""
        if row_count is None:
            row_count = self.height - row_begin
        self._check_buffer("offsets", offsets, row_count, 2, "f32")
        self._check_buffer("ids", ids, row_count, 0, "i32")
        self._check_buffer("mask", mask, row_count, 0, "u8")
        if face is not None:
            self._check_buffer("face", face, row_count, 0, "u8")
        if rgba is not None:
            self._check_buffer("rgba", rgba, row_count, 4, "f32")
        _check(self._lib.rtoShadowAsync(self.handle, light.handle, _ptr(offsets), _ptr(ids), row_begin, row_count, bias,
                                        _ptr(mask), _ptr(face), _ptr(rgba), dim, _stream(stream)))

    def light(self, lights, offsets, ids, rgba, ambient=(0.0, 0.0, 0.0), classes=None, row_begin: int = 0,
              row_count: int | None = None, stream=None):
        """Direct lighting of the prepared frame's rows (include/srt_lighting.h): `lights` is a
        sequence of 0 to 8 lighting.SpotLight / lighting.PointLight over prepared scenes of the same
        triangles (at most 16 light frames: 1 per spot, 6 per point light). offsets, ids as
        shadow()'s; rgba (rows, W, 4) float32: albedo . (ambient + the lights that reach the pixel
        from the eye's side of its triangle), alpha = the id, the background and -1 without a
        surface; classes (len(lights), rows, W) uint8, optional: plane l is shadow()'s /
        omni_shadow()'s mask under light l alone at its bias. One launch whatever len(lights)."""
        from . import lighting

        if row_count is None:
            row_count = self.height - row_begin
        self._check_buffer("offsets", offsets, row_count, 2, "f32")
        self._check_buffer("ids", ids, row_count, 0, "i32")
        self._check_buffer("rgba", rgba, row_count, 4, "f32")
        arr, count = lighting.pack_device(lights)
        if classes is not None:
            if hasattr(classes, "shape") and tuple(classes.shape) != (count, row_count, self.width):
                raise ValueError(f"classes must be {(count, row_count, self.width)}, got {tuple(classes.shape)}")
            self._check_tensor("classes", classes, "u8")
        _check(self._lib.rtdLightAsync(self.handle, ctypes.addressof(arr) if arr is not None else None, count,
                                       lighting.ambient3(ambient), _ptr(offsets), _ptr(ids), row_begin, row_count,
                                       _ptr(rgba), _ptr(classes), _stream(stream)))

    def render_lit(self, lights, offsets, ids, rgba, ambient=(0.0, 0.0, 0.0), classes=None, variant: str = "cull",
                   stream=None):
        """The lit picture of the whole prepared frame: trace_ids() into ids ((H, W) int32; they stay
        available), then light() from them, both on `stream`."""
        self.trace_ids(offsets, ids, variant=variant, stream=stream)
        self.light(lights, offsets, ids, rgba, ambient=ambient, classes=classes, stream=stream)

    def light_hits(self, lights, rays, ids, t, rgba, ambient=(0.0, 0.0, 0.0), classes=None, base=None,
                   weight=(1.0, 1.0, 1.0), stream=None):
        """Lit ray hits (include/srt_hits.h): light() for the hits of caller-supplied rays -- a
        mirror bounce, probe rays, rays from another vantage point. rays (count, 8) float32 with
        closest()'s ids (count,) int32 and t (count,) float32 -> rgba (count, 4) float32: albedo .
        (ambient + the lights that reach the hit from the ray's side of its triangle), alpha = the
        id; the background and -1 for a miss; zeros and -1 for a zero ray (generate_rays()'s "no ray
        here"). classes (len(lights), count) uint8, optional. base (count, 4) float32 with weight
        (3 floats): rgba = (base.rgb + weight . rgb, base's alpha), a zero ray keeping base's
        element; base may be rgba itself. `lights` as light()'s; this scene needs no prepare(). One
        launch whatever len(lights). Device buffers, checked like closest()'s."""
        from . import lighting

        count = self._ray_count((("rays", rays, (8,), "f32"), ("ids", ids, (), "i32"), ("t", t, (), "f32"),
                                 ("rgba", rgba, (4,), "f32"), ("base", base, (4,), "f32")))
        arr, n_lights = lighting.pack_device(lights)
        if classes is not None:
            if hasattr(classes, "shape") and tuple(classes.shape) != (n_lights, count):
                raise ValueError(f"classes must be {(n_lights, count)}, got {tuple(classes.shape)}")
            self._check_tensor("classes", classes, "u8")
        blend = ctypes.byref(_blend(_ptr(base), weight)) if base is not None else None
        _check(self._lib.rthLightHitsAsync(self.handle, ctypes.addressof(arr) if arr is not None else None, n_lights,
                                           lighting.ambient3(ambient), _ptr(rays), _ptr(ids), _ptr(t), count, blend,
                                           _ptr(rgba), _ptr(classes), _stream(stream)))

    def render_reflection(self, lights, offsets, ids, rgba, reflectivity, ambient=(0.0, 0.0, 0.0),
                          tmin: float = 2.0 ** -10, scratch=None, variant: str = "cull", stream=None):
        """The lit picture of the whole prepared frame with one mirror bounce added, on `stream`:
        trace_ids() into ids ((H, W) int32), light() into rgba ((H, W, 4) float32), the mirror rays
        of the frame (generate_rays_frame(Mirror(tmin))), their closest() hits, and light_hits() of
        those onto rgba in place with weight `reflectivity` (3 floats). A pixel without a surface has
        no bounce and keeps the lit frame's background. scratch: a ReflectionScratch of the frame's
        size holding the bounce's rays, ids and t (None: a new one; pass one to allocate nothing in
        later calls). Returns the scratch."""
        if scratch is None:
            scratch = ReflectionScratch(self.width, self.height, self.device)
        if (scratch.width, scratch.height) != (self.width, self.height):
            raise ValueError(f"scratch is {scratch.width} x {scratch.height}, the frame {self.width} x {self.height}")
        flat = rgba.view(-1, 4)
        self.trace_ids(offsets, ids, variant=variant, stream=stream)
        self.light(lights, offsets, ids, rgba, ambient=ambient, stream=stream)
        self.generate_rays_frame(offsets, ids, Mirror(tmin), scratch.rays, stream=stream)
        self.closest(scratch.rays.view(-1, 8), scratch.ids, scratch.t, stream=stream)
        self.light_hits(lights, scratch.rays.view(-1, 8), scratch.ids, scratch.t, flat, ambient=ambient, base=flat,
                        weight=reflectivity, stream=stream)
        return scratch

    def _radiance_call(self, lights, ambient, generator, rgba, lead, modulate, base, weight):
        from . import lighting

        for name, buf in (("rgba", rgba), ("base", base)):
            if buf is None:
                continue
            if hasattr(buf, "shape") and tuple(buf.shape) != lead + (4,):
                raise ValueError(f"{name} must be {lead + (4,)}, got {tuple(buf.shape)}")
            self._check_tensor(name, buf, "f32")
        g = self._generator(generator)
        options, blend = _radiance_options(modulate, _ptr(base) if base is not None else None, weight)
        arr, n_lights = lighting.pack_device(lights)
        return (ctypes.addressof(arr) if arr is not None else None, n_lights, lighting.ambient3(ambient), g, options,
                (arr, blend))

    def radiance(self, lights, positions, ids, generator, rgba, ambient=(0.0, 0.0, 0.0), modulate: bool = False,
                 base=None, weight=(1.0, 1.0, 1.0), stream=None):
        """Sampled radiance (include/srt_radiance.h) at arbitrary image positions of the prepared
        frame: one bounce of indirect light. positions (count, 2) float32 and ids (count,) int32 --
        query()'s input and output --, a Hemisphere (S = 1 ... 64) or a Mirror of device tables, and
        `lights` as light()'s -> rgba (count, 4) float32: the mean of what light_hits() gives for the
        closest() hits of the generator's S rays (the background for a miss), in ascending sample
        order; alpha = the share of rays that hit a surface; zeros off a surface. modulate: times the
        element's own albedo. base (count, 4) float32 with weight (3 floats): rgba = (base.rgb +
        weight . mean, base's alpha), an element off a surface keeping base's; base may be rgba
        itself. One launch whatever len(lights) and S, no scratch: the bits of generate_rays() ->
        closest() -> light_hits() -> a float32 sum over the samples."""
        count = self._elements(positions, ids)
        arr, n_lights, amb, g, options, keep = self._radiance_call(lights, ambient, generator, rgba, (count,), modulate,
                                                                   base, weight)
        _check(self._lib.rtiRadiancePointsAsync(self.handle, arr, n_lights, amb, _ptr(positions), _ptr(ids), count,
                                                ctypes.byref(g), ctypes.byref(options), _ptr(rgba), _stream(stream)))
        del keep

    def radiance_frame(self, lights, offsets, ids, generator, rgba, ambient=(0.0, 0.0, 0.0), modulate: bool = False,
                       base=None, weight=(1.0, 1.0, 1.0), row_begin: int = 0, row_count: int | None = None,
                       stream=None):
        """radiance() for the prepared frame's rows from hit ids: offsets (rows, W, 2) float32 and ids
        (rows, W) int32, band-local -> rgba (rows, W, 4) float32; base (rows, W, 4). A Hemisphere's
        rotations are indexed by the pixel's place in its 4 x 4 block of the whole frame."""
        if row_count is None:
            row_count = self.height - row_begin
        self._check_buffer("offsets", offsets, row_count, 2, "f32")
        self._check_buffer("ids", ids, row_count, 0, "i32")
        arr, n_lights, amb, g, options, keep = self._radiance_call(lights, ambient, generator, rgba,
                                                                   (row_count, self.width), modulate, base, weight)
        _check(self._lib.rtiRadianceFrameAsync(self.handle, arr, n_lights, amb, _ptr(offsets), _ptr(ids), row_begin,
                                               row_count, ctypes.byref(g), ctypes.byref(options), _ptr(rgba),
                                               _stream(stream)))
        del keep

    def render_indirect(self, lights, offsets, ids, rgba, generator, ambient=(0.0, 0.0, 0.0), weight=(1.0, 1.0, 1.0),
                        variant: str = "cull", stream=None):
        """The lit picture of the whole prepared frame with one bounce of indirect light added, on
        `stream`: trace_ids() into ids ((H, W) int32), light() into rgba ((H, W, 4) float32), then
        radiance_frame(generator, modulate=True) onto rgba in place with `weight`. Three calls,
        nothing allocated. A pixel without a surface keeps the lit frame's background."""
        self.trace_ids(offsets, ids, variant=variant, stream=stream)
        self.light(lights, offsets, ids, rgba, ambient=ambient, stream=stream)
        self.radiance_frame(lights, offsets, ids, generator, rgba, ambient=ambient, modulate=True, base=rgba,
                            weight=weight, stream=stream)

    def light_surface(self, lights, offsets, ids, surface, rgba, ambient=(0.0, 0.0, 0.0), material=None, classes=None,
                      row_begin: int = 0, row_count: int | None = None, stream=None):
        """The textured, smooth-shaded, shadowed rows of the prepared frame (include/srt_material.h):
        light() on the surface a Surface of device tables describes (None: none) -- its smooth normal
        under the lights, its textured albedo -- with a lighting.Material (None: no highlight) adding
        a Blinn-Phong term. lights, offsets, ids, rgba, ambient, classes as light()'s; the classes
        are light()'s whatever the surface, and without surface and material so is rgba. One launch."""
        from . import lighting

        if row_count is None:
            row_count = self.height - row_begin
        self._check_buffer("offsets", offsets, row_count, 2, "f32")
        self._check_buffer("ids", ids, row_count, 0, "i32")
        self._check_buffer("rgba", rgba, row_count, 4, "f32")
        s = ctypes.byref(self._surface(surface, (), ())[0]) if surface is not None else None
        arr, count = lighting.pack_device(lights)
        if classes is not None:
            if hasattr(classes, "shape") and tuple(classes.shape) != (count, row_count, self.width):
                raise ValueError(f"classes must be {(count, row_count, self.width)}, got {tuple(classes.shape)}")
            self._check_tensor("classes", classes, "u8")
        _check(self._lib.rtpLightSurfaceAsync(self.handle, ctypes.addressof(arr) if arr is not None else None, count,
                                              lighting.ambient3(ambient), s, lighting.material_ref(material),
                                              _ptr(offsets), _ptr(ids), row_begin, row_count, _ptr(rgba), _ptr(classes),
                                              _stream(stream)))

    def render_lit_surface(self, lights, offsets, ids, surface, rgba, ambient=(0.0, 0.0, 0.0), material=None,
                           classes=None, variant: str = "cull", stream=None):
        """The lit surface of the whole prepared frame: trace_ids() into ids ((H, W) int32; they stay
        available), then light_surface() from them, both on `stream`."""
        self.trace_ids(offsets, ids, variant=variant, stream=stream)
        self.light_surface(lights, offsets, ids, surface, rgba, ambient=ambient, material=material, classes=classes,
                           stream=stream)

    def close(self):
        if self.handle:
            if self._owned:
                self._lib.srtDeviceSceneRelease(self.handle)
            self.handle = None

    def __del__(self):
        self.close()


class OmniLight:
    """A point light resident on one HIP device (include/srt_omni.h): six cube-face scenes of the
    file's triangles under the cameras omni_face_camera(origin, k), prepared at one face size."""

    def __init__(self, path: str, device: int = 0, origin=(0.0, 0.0, 0.0)):
        self._lib = _native.lib()
        self.handle = None
        self.handle = self._lib.rtoLightCreate(os.fsencode(path), device, _float3("origin", origin))
        if not self.handle:
            raise SrtError(_native.last_error())
        self.device = device
        self.path = path
        self.origin = tuple(float(v) for v in origin)
        self.face_size = 0
        self._faces = {}

    def prepare(self, face_size: int, stream=None):
        _check(self._lib.rtoLightPrepareAsync(self.handle, face_size, _stream(stream)))
        self.face_size = face_size
        for f in self._faces.values():
            f.width = f.height = face_size

    def set_origin(self, origin, reorder: bool = True, stream=None):
        """Move the light in place (rtmLightSetOriginAsync): the six faces take the cameras
        omni_face_camera(origin, k) on one stream; the face size stays. reorder as
        DeviceScene.set_camera()'s."""
        _check(self._lib.rtmLightSetOriginAsync(self.handle, _float3("origin", origin),
                                                RTM_REORDER if reorder else RTM_KEEP_ORDER, _stream(stream)))
        self.origin = tuple(float(v) for v in origin)

    def set_vertices(self, vertices, reorder: bool = True, stream=None):
        """Move the triangles of all six faces in place (rtmLightSetVerticesAsync); vertices and
        reorder as DeviceScene.set_vertices()'s."""
        self.face(0)._check_vertices(vertices)
        _check(self._lib.rtmLightSetVerticesAsync(self.handle, _ptr(vertices),
                                                  RTM_REORDER if reorder else RTM_KEEP_ORDER, _stream(stream)))

    def face(self, k: int):
        """Face k (0 .. 5) as a DeviceScene that does not own its handle: every DeviceScene call
        works on it (trace_ids() of the six gives a cube map); close() on it releases nothing, and
        it must not be used after the light's close()."""
        if k not in self._faces:
            handle = self._lib.rtoLightFace(self.handle, k)
            if not handle:
                raise SrtError(_native.last_error())
            self._faces[k] = DeviceScene._borrowed(handle, self.device, self.path, self.face_size)
        return self._faces[k]

    def close(self):
        if self.handle:
            for f in self._faces.values():
                f.handle = None
            self._faces = {}
            self._lib.rtoLightRelease(self.handle)
            self.handle = None

    def __del__(self):
        self.close()
