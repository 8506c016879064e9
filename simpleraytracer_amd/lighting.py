"""The lights of the direct-lighting calls (include/srt_lighting.h): what DeviceScene.light(),
DeviceScene.render_lit() and device.lighting_host() take -- and, with a device.Surface and a
Material, DeviceScene.light_surface(), render_lit_surface() and device.lit_surface_host()
(include/srt_material.h).

    key = SpotLight(DeviceScene(path, 0, camera=cam), color=(1.0, 0.9, 0.8), falloff=9.0, bias=2 ** -10)
    bulb = PointLight(OmniLight(path, 0, origin), color=(0.3, 0.3, 1.0), falloff=4.0)
    view.render_lit([key, bulb], offsets, ids, rgba, ambient=(0.05, 0.05, 0.05), stream=s)

A device light wraps a prepared scene of the same triangles -- a DeviceScene under the light's
camera (a spot light) or an OmniLight (a point light) -- and may appear in a call more than once.
It holds that scene by reference, so a moved light scene is a moved light: after
scene.set_camera() / OmniLight.set_origin() / set_vertices() (include/srt_motion.h) the same
SpotLight / PointLight object lights from the new pose, with nothing to rebuild here.
The host twins describe the same lights without a device: a camera and its frame, or an origin and
the cube faces' size.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Any, Sequence

from . import _native
from ._native import RTD_MAX_FRAMES, RTD_MAX_LIGHTS, RTP_MAX_SHININESS_LOG2  # noqa: F401


def _three(name: str, values) -> tuple:
    vals = tuple(float(v) for v in values)
    if len(vals) != 3:
        raise ValueError(f"{name} must be 3 floats, got {len(vals)}")
    return vals


@dataclass
class SpotLight:
    """A spot light on the device: `scene` is a prepared DeviceScene under the light's camera."""

    scene: Any
    color: Sequence[float] = (1.0, 1.0, 1.0)
    falloff: float = 0.0
    bias: float = 0.0

    def _fill(self, out: _native.RtdLight):
        out.spot, out.point = self.scene.handle, None


@dataclass
class PointLight:
    """A point light on the device: `light` is a prepared OmniLight."""

    light: Any
    color: Sequence[float] = (1.0, 1.0, 1.0)
    falloff: float = 0.0
    bias: float = 0.0

    def _fill(self, out: _native.RtdLight):
        out.spot, out.point = None, self.light.handle


@dataclass
class SpotLightHost:
    """A spot light for the host call: camera (eye, lookat, up, vfov_deg: 10 floats) at width x height."""

    camera: Sequence[float]
    width: int
    height: int
    color: Sequence[float] = (1.0, 1.0, 1.0)
    falloff: float = 0.0
    bias: float = 0.0

    def _fill(self, out: _native.RtdLightHost):
        cam = tuple(float(v) for v in self.camera)
        if len(cam) != 10:
            raise ValueError(f"camera must be 10 floats (eye, lookat, up, vfov_deg), got {len(cam)}")
        out.kind = 0
        out.camera10[:] = cam
        out.width, out.height = self.width, self.height


@dataclass
class PointLightHost:
    """A point light for the host call: origin (3 floats) with face_size x face_size cube faces."""

    origin: Sequence[float]
    face_size: int
    color: Sequence[float] = (1.0, 1.0, 1.0)
    falloff: float = 0.0
    bias: float = 0.0

    def _fill(self, out: _native.RtdLightHost):
        out.kind = 1
        out.origin[:] = _three("origin", self.origin)
        out.face_size = self.face_size


@dataclass
class Material:
    """The highlight of a lit surface (``rtp_material``, include/srt_material.h): a Blinn-Phong term
    of colour `specular` with the exponent 2 ** shininess_log2 (0 .. 12)."""

    specular: Sequence[float] = (0.0, 0.0, 0.0)
    shininess_log2: int = 0

    def _struct(self) -> _native.RtpMaterial:
        out = _native.RtpMaterial(ctypes.sizeof(_native.RtpMaterial))
        out.specular[:] = _three("specular", self.specular)
        out.shininess_log2 = int(self.shininess_log2)
        return out


def material_ref(material):
    """The `material` argument of the rtp calls: a pointer to its struct, or None."""
    if material is None:
        return None
    if not isinstance(material, Material):
        raise TypeError(f"material must be a Material, got {type(material).__name__}")
    return ctypes.byref(material._struct())


def _pack(lights, struct, kinds):
    """The C array of the lights (None for no lights) -- kept alive by the caller during the call."""
    lights = list(lights)
    if not lights:
        return None, 0
    arr = (struct * len(lights))()
    for k, light in enumerate(lights):
        if not isinstance(light, kinds):
            raise TypeError(f"lights[{k}] must be one of {', '.join(c.__name__ for c in kinds)}, got {type(light).__name__}")
        arr[k].struct_size = ctypes.sizeof(struct)
        light._fill(arr[k])
        arr[k].color[:] = _three(f"lights[{k}].color", light.color)
        arr[k].falloff = float(light.falloff)
        arr[k].bias = float(light.bias)
    return arr, len(lights)


def pack_device(lights):
    return _pack(lights, _native.RtdLight, (SpotLight, PointLight))


def pack_host(lights):
    return _pack(lights, _native.RtdLightHost, (SpotLightHost, PointLightHost))


def ambient3(ambient):
    return (ctypes.c_float * 3)(*_three("ambient", ambient))
