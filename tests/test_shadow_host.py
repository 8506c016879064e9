"""The shadow mask on the host (include/srt_light.h rtlShadowHost, rtlProjectionHost): exact against
the numpy float32 restatement of DESIGN.md section 2 "Shadow" over the oracle's records
(tests/shadow_cases.py). No device.

Argument errors of rtlShadowAsync that need two device scenes (unequal triangle counts, an
unprepared light) are in test_gpu_shadow.py: a device scene cannot be created without a device.
"""
from __future__ import annotations

import numpy as np
import pytest

import gbuffer_cases as gc
import shadow_cases as sc
from oracle import srt_oracle as oracle
from simpleraytracer_amd import SrtError, _native, device

W, H = sc.W, sc.H


def host(c, bias=0.0, dim=0.0, offsets=None, ids=None, row_begin=0, row_count=None):
    offsets = c.offsets if offsets is None else offsets
    ids = c.ids if ids is None else ids
    return device.shadow_host(c.view, W, H, c.light_cam, c.wl, c.hl, offsets, ids, bias=bias, dim=dim,
                              row_begin=row_begin, row_count=row_count)


@pytest.mark.parametrize("cam,wl,hl", [(sc.LIGHT_CAM, sc.WL, sc.HL), (sc.VIEW_CAM, 200, 72),
                                       ((-2.5, 0.75, 9.0, 0.3, -0.2, 1.0, 0.1, 1.0, 0.2, 33.5), 1920, 1080)])
def test_projection_rows_equal_the_restatement(tmp_path, cam, wl, hl):
    path = sc.write_with_camera(tmp_path / "cam.srt", sc.grid_floor_vertices(1), cam)
    s = oracle.OracleScene(path)
    want = sc.projection_rows(s.frame(wl, hl))
    s.close()
    sc.same_bits("projection rows", device.light_projection(cam, wl, hl), want)
    # the rows project the light's own view: the frame's centre direction lands on (1/2, 1/2) at depth 1
    px, py, pz = want.astype(np.float64)
    f = pz
    assert abs(px @ f / (pz @ f) - 0.5) < 1e-6 and abs(py @ f / (pz @ f) - 0.5) < 1e-6 and abs(pz @ f - 1) < 1e-6


@pytest.mark.parametrize("bias", sc.BIASES)
def test_scene_t_equals_the_expected_mask(bias):
    c = sc.case("T")
    want = sc.expected("T", bias)
    n = want.size
    assert all(k >= 0.02 * n for k in sc.counts(want)), f"degenerate scene: class counts {sc.counts(want)}"
    mask, _ = host(c, bias)
    sc.assert_same_mask(mask, want)


def test_bias_moves_a_pixel():
    """The two biases do not give the same expected mask, so the threshold is exercised."""
    a, b = sc.expected("T", sc.BIASES[0]), sc.expected("T", sc.BIASES[1])
    assert (a != b).any() and np.all((a != b) <= ((a == sc.SHADOWED) & (b == sc.LIT)))


@pytest.mark.parametrize("dim", [0.0, 0.25])
def test_rgba_is_the_shaded_pixel_times_the_class_scale(dim):
    c = sc.case("T")
    want = sc.expected("T", 0.0)
    # Shade's pixel on the host: dim = 1 multiplies every rgb by 1; its rgb is the one-sample resolve's
    # bit for bit and within the project's shading tolerance of the oracle's, its alpha the id.
    _, shade = host(c, 0.0, dim=1.0)
    one = device.resolve_host(c.view, W, H, [c.offsets], [c.ids])
    sc.same_bits("k = 1 rgb", shade[..., :3], one[..., :3])
    s = oracle.OracleScene(c.view)
    ref = s.shade(W, H, c.ids, c.offsets)
    s.close()
    assert np.array_equal(shade[..., 3], ref[..., 3])
    assert float(np.abs(shade[..., :3] - ref[..., :3]).max()) <= 1e-5
    mask, rgba = host(c, 0.0, dim=dim)
    sc.assert_same_mask(mask, want)
    sc.same_bits("rgba", rgba, sc.dimmed(shade, want, dim))
    assert (rgba[want == sc.NO_SURFACE] == np.float32([0.1, 0.2, 0.3, -1.0])).all()


def test_band_equals_the_slice_of_the_frame():
    c = sc.case("T")
    want = sc.expected("T", 0.0)
    _, whole = host(c, 0.0, dim=0.25)
    mask, rgba = host(c, 0.0, dim=0.25, offsets=c.offsets[16:53], ids=c.ids[16:53], row_begin=16, row_count=37)
    sc.assert_same_mask(mask, want[16:53])
    sc.same_bits("band rgba", rgba, whole[16:53])


def test_sentinel_ids_are_no_surface():
    c = sc.case("T")
    ids = np.array(c.ids)
    sentinels = gc.miss_ids(c.n)
    ids[5, :len(sentinels)] = sentinels
    ids[40, 7:7 + len(sentinels)] = sentinels
    mask, rgba = host(c, 0.0, dim=0.25, ids=ids)
    want = np.array(sc.expected("T", 0.0))
    changed = ids != c.ids
    assert changed.sum() >= len(sentinels)
    want[changed] = sc.NO_SURFACE
    sc.assert_same_mask(mask, want)
    assert (rgba[changed] == np.float32([0.1, 0.2, 0.3, -1.0])).all()


def test_light_at_the_eye_lights_every_hit():
    c = sc.case("eye")
    for bias in sc.BIASES:
        want = sc.expected("eye", bias)
        assert sc.counts(want)[sc.SHADOWED] == 0 and sc.counts(want)[sc.OUTSIDE] == 0
        assert sc.counts(want)[sc.LIT] == int((c.ids >= 0).sum()) > 1000
        mask, _ = host(c, bias)
        sc.assert_same_mask(mask, want)


def test_gridded_floor_has_no_shadow():
    c = sc.case("grid")
    for bias in sc.BIASES:
        want = sc.expected("grid", bias)
        assert sc.counts(want)[sc.SHADOWED] == 0 and sc.counts(want)[sc.LIT] > 1000
        mask, _ = host(c, bias)
        sc.assert_same_mask(mask, want)


def test_light_looking_away_is_outside():
    c = sc.case("away")
    want = sc.expected("away", 0.0)
    assert np.array_equal(want == sc.OUTSIDE, c.ids >= 0) and (c.ids >= 0).sum() > 1000
    mask, _ = host(c, 0.0)
    sc.assert_same_mask(mask, want)


def test_argument_errors():
    import ctypes

    L = _native.lib()
    c = sc.case("T")
    cam = (ctypes.c_float * 10)(*sc.LIGHT_CAM)
    off = np.ascontiguousarray(c.offsets)
    ids = np.ascontiguousarray(c.ids)
    mask = np.empty((H, W), np.uint8)
    path = c.view.encode()

    def call(path=path, cam=cam, off=off.ctypes.data, ids=ids.ctypes.data, mask=mask.ctypes.data, bias=0.0, dim=0.0,
             r0=0, rows=H):
        return L.rtlShadowHost(path, W, H, cam, sc.WL, sc.HL, off, ids, r0, rows, bias, mask, None, dim)

    assert call() == 0  # (rgba is optional)
    for kw, text in (({"path": None}, "scene_path is NULL"), ({"cam": None}, "light_camera10 is NULL"),
                     ({"off": None}, "offsets is NULL"), ({"ids": None}, "ids is NULL"), ({"mask": None}, "mask is NULL"),
                     ({"bias": -0.5}, "bias must be finite and >= 0"), ({"bias": float("nan")}, "bias must be finite"),
                     ({"bias": float("inf")}, "bias must be finite"), ({"dim": float("nan")}, "dim must be finite"),
                     ({"r0": 90, "rows": 7}, "row band outside the frame")):
        assert call(**kw) == -1
        assert text in _native.last_error(), (kw, _native.last_error())
    assert call(rows=0, off=None, ids=None, mask=None) == 0  # no rows: nothing is read
    # device entry points: NULL handles are refused before anything else
    assert L.rtlShadowAsync(None, None, None, None, 0, 0, 0.0, None, None, 0.0, None) == -1
    assert _native.last_error() == "Bad scene handle: view is NULL"
    assert not L.rtlSceneCreate(None, 0, None)
    assert _native.last_error() == "Bad path argument"
    # bad cameras, through each entry point that takes one
    rows = (ctypes.c_float * 9)()
    good = list(sc.LIGHT_CAM)
    for k, v, text in ((4, float("nan"), "value 4 is not finite"), (0, float("inf"), "value 0 is not finite"),
                       (9, 0.0, "vfov must be in (0, 180)"), (9, 180.0, "vfov must be in (0, 180)"),
                       (9, -20.0, "vfov must be in (0, 180)")):
        bad = list(good)
        bad[k] = v
        arr = (ctypes.c_float * 10)(*bad)
        assert L.rtlProjectionHost(arr, sc.WL, sc.HL, rows) == -1
        assert text in _native.last_error()
        assert call(cam=arr) == -1
        assert text in _native.last_error()
        assert not L.rtlSceneCreate(path, 0, arr)
        assert text in _native.last_error()
    same = (ctypes.c_float * 10)(1, 2, 3, 1, 2, 3, 0, 1, 0, 50)
    assert L.rtlProjectionHost(same, sc.WL, sc.HL, rows) == -1 and "eye equals lookat" in _native.last_error()
    par = (ctypes.c_float * 10)(0, 0, 0, 0, 2, 0, 0, -3, 0, 50)
    assert L.rtlProjectionHost(par, sc.WL, sc.HL, rows) == -1 and "up is parallel" in _native.last_error()
    assert L.rtlProjectionHost(cam, 0, sc.HL, rows) == -1 and "dimensions must be non-zero" in _native.last_error()
    assert L.rtlProjectionHost(None, sc.WL, sc.HL, rows) == -1
    with pytest.raises(ValueError):
        device.light_projection(sc.LIGHT_CAM[:9], sc.WL, sc.HL)
    with pytest.raises(SrtError, match="vfov"):
        device.light_projection(sc.LIGHT_CAM[:9] + (190.0,), sc.WL, sc.HL)
    with pytest.raises(ValueError):
        device.shadow_host(c.view, W, H, sc.LIGHT_CAM, sc.WL, sc.HL, c.offsets[:5], c.ids)
