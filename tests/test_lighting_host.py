"""Direct lighting on the host (include/srt_lighting.h rtdLightHost): exact against the numpy float32
restatement of DESIGN.md section 2 "Lighting" over the oracle's records (tests/lighting_cases.py).
No device.

Argument errors of rtdLightAsync that need device scenes (an unprepared light, unequal triangle
counts, both handles set) are in test_gpu_lighting.py.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import lighting_cases as lc
import shadow_cases as sc
from oracle import srt_oracle as oracle
from simpleraytracer_amd import PointLightHost, SpotLightHost, SrtError, _native, device

W, H = lc.W, lc.H


def host(c, lights, ambient=lc.AMBIENT, offsets=None, ids=None, row_begin=0, row_count=None):
    offsets = c.offsets if offsets is None else offsets
    ids = c.ids if ids is None else ids
    return device.lighting_host(c.view, W, H, lc.host_lights(lights), ambient, offsets, ids, row_begin=row_begin,
                                row_count=row_count)


@pytest.mark.parametrize("name", list(lc.CASES))
def test_expected_data_are_not_vacuous(name):
    lc.check_expected(name)


@pytest.mark.parametrize("name", list(lc.CASES))
def test_classes_and_rgba_equal_the_restatement(name):
    c = lc.case(name)
    want = lc.expected(name)
    rgba, classes = host(c, c.lights)
    lc.assert_same_classes(classes, want.classes)
    lc.same_bits(f"{name} rgba", rgba, want.rgba)


def test_no_lights_and_white_ambient_give_the_albedo_plane():
    for name in ("T4", "roomB"):
        c = lc.case(name)
        rgba, classes = host(c, [], ambient=(1.0, 1.0, 1.0))
        _, _, _, albedo = device.attributes_host(c.view, W, H, device.pixel_positions(W, H, c.offsets), c.ids.reshape(-1))
        assert classes.shape == (0, H, W)
        lc.same_bits(f"{name} albedo", rgba, albedo.reshape(H, W, 4))
    assert (lc.case("T4").ids < 0).sum() > 1000  # hits and misses alike


def test_headlight_is_the_shaded_frame_within_the_shading_tolerance():
    for name in ("T4", "roomA"):
        c = lc.case(name)
        s = oracle.OracleScene(c.view)
        shade = s.shade(W, H, c.ids, c.offsets)
        s.close()
        rgba, classes = host(c, [lc.headlight(c.view_cam)], ambient=(0.0, 0.0, 0.0))
        surface = c.ids >= 0
        assert (classes[0][surface] == sc.LIT).all() and (classes[0][~surface] == sc.NO_SURFACE).all()
        err = float(np.abs(rgba[..., :3] - shade[..., :3]).max())
        print(f"{name}: headlight against shade, max abs error {err:.3e}")
        assert err <= 1e-5
        assert np.array_equal(rgba[..., 3], shade[..., 3])


def test_band_equals_the_slice_of_the_frame():
    c = lc.case("T4")
    want = lc.expected("T4")
    rgba, classes = host(c, c.lights, offsets=c.offsets[16:53], ids=c.ids[16:53], row_begin=16, row_count=37)
    lc.assert_same_classes(classes, want.classes[:, 16:53])
    lc.same_bits("band rgba", rgba, want.rgba[16:53])


def test_every_prefix_of_the_lights():
    c = lc.case("T4")
    for k in range(len(c.lights) + 1):
        rgba, classes = host(c, c.lights[:k])
        lc.assert_same_classes(classes, lc.expected_classes("T4", c.lights[:k]))
        lc.same_bits(f"first {k} lights", rgba, lc.restate_rgba("T4", c.lights[:k]))


def test_a_light_may_appear_twice():
    c = lc.case("T4")
    a = c.lights[0]
    b = lc.spot(a.cam, a.wl, a.hl, (0.1, 0.7, 0.2), a.falloff, a.bias)
    rgba, classes = host(c, [a, b])
    sc.assert_same_mask(classes[0], classes[1])
    lc.same_bits("the same spot twice", rgba, lc.restate_rgba("T4", [a, b]))
    once, _ = host(c, [a])
    assert not np.array_equal(rgba, once)


def test_sentinel_ids_are_the_background_and_class_3():
    c = lc.case("roomA")
    ids = np.array(c.ids)
    sentinels = np.array([-7, c.n, 2 ** 31 - 1], np.int32)
    ids[5, :3] = sentinels
    ids[40, 7:10] = sentinels
    changed = ids != c.ids
    assert changed.sum() == 6
    rgba, classes = host(c, c.lights, ids=ids)
    want = lc.expected("roomA")
    assert (classes[:, changed] == sc.NO_SURFACE).all()
    assert (rgba[changed] == np.float32(lc.BACKGROUND + (-1.0,))).all()
    lc.assert_same_classes(classes[:, ~changed][None], want.classes[:, ~changed][None])
    lc.same_bits("the other pixels", rgba[~changed], want.rgba[~changed])


def _light(kind=0, **kw):
    l = _native.RtdLightHost()
    l.struct_size = ctypes.sizeof(_native.RtdLightHost)
    l.kind = kind
    l.camera10[:] = sc.LIGHT_CAM
    l.width, l.height = sc.WL, sc.HL
    l.origin[:] = (0.25, 1.0, 4.0)
    l.face_size = 64
    l.color[:] = (1.0, 1.0, 1.0)
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(l, k)[:] = v
        else:
            setattr(l, k, v)
    return l


def test_argument_errors():
    L = _native.lib()
    c = lc.case("T4")
    off = np.ascontiguousarray(c.offsets)
    ids = np.ascontiguousarray(c.ids)
    rgba = np.empty((H, W, 4), np.float32)
    f3 = ctypes.c_float * 3
    nan, inf = float("nan"), float("inf")

    def call(lights=(), path=c.view.encode(), ambient=f3(0.0, 0.0, 0.0), off=off.ctypes.data, ids=ids.ctypes.data,
             rgba=rgba.ctypes.data, r0=0, rows=H, count=None):
        arr = (_native.RtdLightHost * max(1, len(lights)))(*lights)
        count = len(lights) if count is None else count
        return L.rtdLightHost(path, W, H, ctypes.addressof(arr) if lights else None, count, ambient, off, ids, r0, rows,
                              rgba, None)

    assert call([_light()]) == 0  # (classes are optional)
    lc.same_bits("one light", rgba, lc.restate_rgba("T4", [lc.spot(sc.LIGHT_CAM, sc.WL, sc.HL, (1.0, 1.0, 1.0))], (0, 0, 0)))
    spots9 = [_light() for _ in range(9)]
    for kw, text in (
            ({"path": None}, "scene_path is NULL"),
            ({"lights": [_light(), _light(struct_size=8)]}, "light 1: rtd_light_host.struct_size is 8, expected"),
            ({"lights": [_light(kind=2)]}, "light 0: kind must be 0 (spot) or 1 (point), got 2"),
            ({"lights": spots9}, "at most 8 lights per call, got 9"),
            ({"lights": [_light(1), _light(1), _light(), _light(), _light(), _light(), _light()]},
             "light 6 brings the call to 17 light frames, at most 16"),
            ({"lights": [_light(1), _light(1), _light(1)]}, "light 2 brings the call to 18 light frames"),
            ({"lights": [_light(color=(1.0, nan, 1.0))]}, "light 0: color value 1 is not finite"),
            ({"lights": [_light(), _light(color=(1.0, 1.0, inf))]}, "light 1: color value 2 is not finite"),
            ({"ambient": f3(0.0, 0.0, nan)}, "ambient value 2 is not finite"),
            ({"ambient": None}, "ambient is NULL"),
            ({"lights": [_light(falloff=-1.0)]}, "light 0: falloff must be finite and >= 0"),
            ({"lights": [_light(falloff=inf)]}, "light 0: falloff must be finite and >= 0"),
            ({"lights": [_light(), _light(1, bias=-0.5)]}, "light 1: bias must be finite and >= 0"),
            ({"lights": [_light(bias=nan)]}, "light 0: bias must be finite and >= 0"),
            ({"lights": [_light(width=0)]}, "light 0: frame dimensions must be non-zero"),
            ({"lights": [_light(1, face_size=0)]}, "light 0: face_size must be non-zero"),
            ({"lights": [_light(1, origin=(0.0, 1e6, 0.0))]}, "light 0: Bad light origin: value 1"),
            ({"lights": [_light(camera10=(0, 0, 0, 0, 0, 0, 0, 1, 0, 60))]}, "light 0: Bad camera: eye equals lookat"),
            ({"lights": [], "count": 1}, "lights is NULL"),
            ({"r0": 90, "rows": 7}, "row band outside the frame"),
            ({"off": None}, "offsets is NULL"), ({"ids": None}, "ids is NULL"), ({"rgba": None}, "rgba is NULL")):
        assert call(**kw) == -1, kw
        assert text in _native.last_error(), (kw, _native.last_error())
    assert call(rows=0, off=None, ids=None, rgba=None) == 0  # no rows: nothing is read
    assert call([]) == 0                                      # no lights, lights == NULL
    # sixteen frames are allowed
    assert call([_light(1), _light(1), _light(), _light(), _light(), _light()], rows=1) == 0
    # the device entry point: a NULL view is refused before anything else
    assert L.rtdLightAsync(None, None, 0, f3(0.0, 0.0, 0.0), None, None, 0, 0, None, None, None) == -1
    assert _native.last_error() == "Bad scene handle: view is NULL"
    # the wrapper's own checks
    with pytest.raises(ValueError):
        device.lighting_host(c.view, W, H, [], (0, 0, 0), c.offsets[:5], c.ids)
    with pytest.raises(ValueError):
        device.lighting_host(c.view, W, H, [], (0, 0), c.offsets, c.ids)
    with pytest.raises(ValueError):
        device.lighting_host(c.view, W, H, [SpotLightHost(sc.LIGHT_CAM[:9], 64, 64)], (0, 0, 0), c.offsets, c.ids)
    with pytest.raises(TypeError):
        device.lighting_host(c.view, W, H, [object()], (0, 0, 0), c.offsets, c.ids)
    with pytest.raises(SrtError, match="light 0: falloff must be finite"):
        device.lighting_host(c.view, W, H, [PointLightHost((0, 1, 4), 64, falloff=-2.0)], (0, 0, 0), c.offsets, c.ids)
