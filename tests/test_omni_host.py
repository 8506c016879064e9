"""The omni-light shadow mask on the host (include/srt_omni.h rtoShadowHost, rtoFaceCameraHost,
rtoFaceOfHost): exact against the numpy float32 restatement of DESIGN.md section 2 "Omni shadow"
over the oracle's records (tests/omni_cases.py). No device.

Argument errors of rtoShadowAsync that need device scenes (an unprepared light, unequal triangle
counts) are in test_gpu_omni.py.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import gbuffer_cases as gc
import omni_cases as oc
from oracle import srt_oracle as oracle
from simpleraytracer_amd import SrtError, _native, device

W, H = oc.W, oc.H
CASES = [(v, f) for v in oc.VIEWS for f in oc.FACE_SIZES]


def host(c, face_size, bias=0.0, dim=0.0, offsets=None, ids=None, row_begin=0, row_count=None):
    offsets = c.offsets if offsets is None else offsets
    ids = c.ids if ids is None else ids
    return device.omni_shadow_host(c.view, W, H, c.origin, face_size, offsets, ids, bias=bias, dim=dim,
                                   row_begin=row_begin, row_count=row_count)


@pytest.mark.parametrize("view,face_size", CASES)
def test_expected_data_cover_every_face_class_and_seam(view, face_size):
    oc.check_expected(view, face_size)


@pytest.mark.parametrize("bias", oc.BIASES)
@pytest.mark.parametrize("view,face_size", CASES)
def test_mask_and_face_plane_equal_the_expected_ones(view, face_size, bias):
    c = oc.case(view)
    mask, face, _ = host(c, face_size, bias)
    oc.assert_same_face(face, oc.facts(view, face_size).face)
    oc.assert_same_mask(mask, oc.expected(view, face_size, bias))


@pytest.mark.parametrize("view,face_size", CASES)
def test_class_equals_the_spot_light_class_of_the_selected_face(view, face_size):
    """The consequence of the definition: per pixel, rtlShadowHost's class for the light camera of
    the selected face at F x F; none of the selected classes is 2."""
    c = oc.case(view)
    for bias in oc.BIASES:
        mask, face, _ = host(c, face_size, bias)
        select = np.full((H, W), 9, np.uint8)
        for k in range(6):
            spot, _ = device.shadow_host(c.view, W, H, device.omni_face_camera(c.origin, k), face_size, face_size,
                                         c.offsets, c.ids, bias=bias)
            select[face == k] = spot[face == k]
        assert not (select == oc.OUTSIDE).any()
        oc.assert_same_mask(mask, select)


@pytest.mark.parametrize("dim", [0.0, 0.25])
def test_rgba_is_the_shaded_pixel_times_the_class_scale(dim):
    for view in oc.VIEWS:
        c = oc.case(view)
        s = oracle.OracleScene(c.view)
        shade = s.shade(W, H, c.ids, c.offsets)
        s.close()
        want = oc.expected(view, 64, 0.0)
        mask, _, rgba = host(c, 64, 0.0, dim=dim)
        oc.assert_same_mask(mask, want)
        oc.same_bits("rgba", rgba, oc.dimmed(shade, want, dim))


def test_band_equals_the_slice_of_the_frame():
    c = oc.case("A")
    _, _, whole = host(c, 64, 0.0, dim=0.25)
    mask, face, rgba = host(c, 64, 0.0, dim=0.25, offsets=c.offsets[24:64], ids=c.ids[24:64], row_begin=24, row_count=40)
    oc.assert_same_mask(mask, oc.expected("A", 64, 0.0)[24:64])
    oc.assert_same_face(face, oc.facts("A", 64).face[24:64])
    oc.same_bits("band rgba", rgba, whole[24:64])


def test_sentinel_ids_are_no_surface_and_no_face():
    c = oc.case("A")
    ids = np.array(c.ids)
    sentinels = gc.miss_ids(c.n)
    assert {-1, c.n, np.iinfo(np.int32).min} <= set(int(s) for s in sentinels)
    ids[5, :len(sentinels)] = sentinels
    ids[40, 7:7 + len(sentinels)] = sentinels
    mask, face, rgba = host(c, 64, 0.0, dim=0.25, ids=ids)
    changed = ids != c.ids
    assert changed.sum() == 2 * len(sentinels)
    want = np.array(oc.expected("A", 64, 0.0))
    want[changed] = oc.NO_SURFACE
    want_face = np.array(oc.facts("A", 64).face)
    want_face[changed] = oc.NO_FACE
    oc.assert_same_mask(mask, want)
    oc.assert_same_face(face, want_face)
    assert (rgba[changed] == np.float32([0.1, 0.2, 0.3, -1.0])).all()


def test_face_cameras_equal_the_table():
    for origin in (oc.ORIGIN, (0.0, 0.0, 0.0), (-65536.0, 65536.0, 12345.678), (1e-3, -7.25, 65535.99)):
        for k in range(6):
            got = np.array(device.omni_face_camera(origin, k), np.float32)
            oc.same_bits(f"face {k} of {origin}", got, np.array(oc.face_camera(origin, k), np.float32))
    axis, up = oc.FACES[3]
    assert device.omni_face_camera((1.0, 2.0, 3.0), 3) == (1.0, 2.0, 3.0, 1.0, 1.0, 3.0, 0.0, 0.0, 1.0, 92.0)
    assert (axis, up) == ((0, -1, 0), (0, 0, 1))


def test_face_of():
    nan, inf = float("nan"), float("inf")
    for k, (axis, _) in enumerate(oc.FACES):
        assert device.omni_face_of(axis) == k
        assert device.omni_face_of([3.5 * a for a in axis]) == k
    # ties go to the lower axis, the sign is the winning component's
    for q, want in (((1, 1, 0), 0), ((1, -1, 1), 0), ((-1, 1, 1), 1), ((0, 2, 2), 2), ((0, -2, 2), 3), ((0, 2, -2), 2),
                    ((1, 1, 1), 0), ((-1, -1, -1), 1), ((1, 0, 1), 0), ((-2, 0, 2), 1), ((1, 2, 2), 2), ((1, -2, -2), 3),
                    ((2, 2, 3), 4), ((2, 2, -3), 5)):
        assert device.omni_face_of(q) == want == oc.face_of(q), q
    # +-0 picks the + face; a NaN component never wins a comparison
    for q, want in (((0.0, 0.0, 0.0), 0), ((-0.0, -0.0, -0.0), 0), ((-0.0, 0.0, 0.0), 0),
                    ((nan, 1.0, 2.0), 0), ((nan, -1.0, -2.0), 0), ((1.0, nan, 2.0), 4), ((1.0, nan, -2.0), 5),
                    ((-3.0, nan, 2.0), 1), ((1.0, 2.0, nan), 2), ((1.0, -2.0, nan), 3), ((nan, nan, nan), 0),
                    ((inf, 1.0, -inf), 0), ((1.0, -inf, inf), 3)):
        assert device.omni_face_of(q) == want == oc.face_of(q), q
    rng = np.random.default_rng(11)
    qs = rng.normal(size=(10_000, 3)).astype(np.float32)
    qs[::7] = np.round(qs[::7])          # exact ties
    qs[::11, 1] = qs[::11, 0]
    qs[::13, 2] = -qs[::13, 1]
    lib = _native.lib()
    arr = ctypes.c_float * 3
    got = np.array([lib.rtoFaceOfHost(arr(*q)) for q in qs])
    want = np.array([oc.face_of(q) for q in qs])
    assert np.array_equal(got, want)
    assert set(got) == set(range(6))


def test_argument_errors():
    L = _native.lib()
    c = oc.case("A")
    origin = (ctypes.c_float * 3)(*oc.ORIGIN)
    off = np.ascontiguousarray(c.offsets)
    ids = np.ascontiguousarray(c.ids)
    mask = np.empty((H, W), np.uint8)
    path = c.view.encode()

    def call(path=path, origin=origin, f=64, off=off.ctypes.data, ids=ids.ctypes.data, mask=mask.ctypes.data, bias=0.0,
             dim=0.0, r0=0, rows=H):
        return L.rtoShadowHost(path, W, H, origin, f, off, ids, r0, rows, bias, mask, None, None, dim)

    assert call() == 0  # (face and rgba are optional)
    oc.assert_same_mask(mask, oc.expected("A", 64, 0.0))
    f3 = ctypes.c_float * 3
    for kw, text in (({"path": None}, "scene_path is NULL"), ({"origin": None}, "origin is NULL"),
                     ({"origin": f3(0.0, float("nan"), 0.0)}, "Bad light origin: value 1"),
                     ({"origin": f3(float("inf"), 0.0, 0.0)}, "Bad light origin: value 0"),
                     ({"origin": f3(0.0, 0.0, -65537.0)}, "Bad light origin: value 2"),
                     ({"f": 0}, "face_size must be non-zero"),
                     ({"off": None}, "offsets is NULL"), ({"ids": None}, "ids is NULL"), ({"mask": None}, "mask is NULL"),
                     ({"bias": -0.5}, "bias must be finite and >= 0"), ({"bias": float("nan")}, "bias must be finite"),
                     ({"dim": float("nan")}, "dim must be finite"),
                     ({"r0": 90, "rows": 7}, "row band outside the frame")):
        assert call(**kw) == -1
        assert text in _native.last_error(), (kw, _native.last_error())
    assert call(origin=f3(65536.0, -65536.0, 0.0), rows=0) == 0  # 2^16 itself is allowed
    assert call(rows=0, off=None, ids=None, mask=None) == 0      # no rows: nothing is read
    # the face index and the origin, through the entry points that take them
    cam = (ctypes.c_float * 10)()
    for face in (-1, 6, 255):
        assert L.rtoFaceCameraHost(origin, face, cam) == -1 and "Bad face index" in _native.last_error()
        with pytest.raises(SrtError, match="faces are 0 to 5"):
            device.omni_face_camera(oc.ORIGIN, face)
    assert L.rtoFaceCameraHost(f3(1e6, 0.0, 0.0), 0, cam) == -1 and "Bad light origin" in _native.last_error()
    assert L.rtoFaceCameraHost(origin, 0, None) == -1
    assert L.rtoFaceOfHost(None) == -1
    # device entry points: NULL handles are refused before anything else
    assert L.rtoShadowAsync(None, None, None, None, 0, 0, 0.0, None, None, None, 0.0, None) == -1
    assert _native.last_error() == "Bad scene handle: view is NULL"
    assert not L.rtoLightCreate(None, 0, origin) and _native.last_error() == "Bad path argument"
    assert not L.rtoLightCreate(path, 0, f3(0.0, float("nan"), 0.0)) and "Bad light origin" in _native.last_error()
    assert L.rtoLightPrepareAsync(None, 64, None) == -1 and _native.last_error() == "Bad light handle"
    assert not L.rtoLightFace(None, 0) and _native.last_error() == "Bad light handle"
    L.rtoLightRelease(None)
    # the wrapper's own checks
    with pytest.raises(ValueError):
        device.omni_shadow_host(c.view, W, H, oc.ORIGIN, 64, c.offsets[:5], c.ids)
    with pytest.raises(ValueError):
        device.omni_shadow_host(c.view, W, H, oc.ORIGIN[:2], 64, c.offsets, c.ids)
