"""Lit surfaces on the host (include/srt_material.h rtpLightSurfaceHost): exact on the uint32 view
against the numpy float32 restatement of DESIGN.md section 2 "Lit surfaces" (tests/litsurface_cases.py),
and the two reductions to rtdLightHost. No device.
"""
from __future__ import annotations

import ctypes
import itertools
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import lighting_cases as lc
import litsurface_cases as pc
import shadow_cases as sc
import surface_cases as sv
from simpleraytracer_amd import Surface, _native, device

W, H = pc.W, pc.H
REPO = Path(__file__).resolve().parent.parent
RTP = {"rtpLightSurfaceAsync", "rtpLightSurfaceHost"}
CASES = ("T4", "roomA")


def host(c, surface=None, material=None, lights=None, ambient=pc.AMBIENT, ids=None, row_begin=0, row_count=None):
    ids = c.ids if ids is None else ids
    return device.lit_surface_host(c.view, W, H, lc.host_lights(c.lights if lights is None else lights), ambient,
                                   c.offsets[row_begin:None if row_count is None else row_begin + row_count],
                                   ids[row_begin:None if row_count is None else row_begin + row_count], surface,
                                   pc.host_material(material), row_begin=row_begin, row_count=row_count)


@pytest.mark.parametrize("name", CASES)
def test_expected_data_are_not_vacuous(name):
    pc.check_not_vacuous(name, pc.tables(name).normals, (pc.SPECULAR, 5))


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("material", [None] + [(pc.SPECULAR, k) for k in pc.SHININESS],
                         ids=["plain"] + [f"k{k}" for k in pc.SHININESS])
def test_textured_smooth_pixels_equal_the_restatement(name, material):
    """Normals + uvs + a 3 x 5 texture: repeat / clamp x bilinear / nearest, RTV_MODULATE on and off."""
    c = lc.case(name)
    tb = pc.tables(name)
    tex = sv.texture(*pc.TEXTURE, 11)
    want_classes = lc.expected(name).classes
    for wrap, filt, modulate in itertools.product(sv.WRAPS, sv.FILTERS, (False, True)):
        rgba, classes = host(c, Surface(tb.normals, tb.uvs, tex, wrap, filt, modulate), material)
        want = pc.restate(name, tb.normals, tb.uvs, tex, wrap, filt, modulate, material)
        pc.same_bits(f"{name} {wrap} {filt} modulate={modulate} rgba", rgba, want)
        lc.assert_same_classes(classes, want_classes)


@pytest.mark.parametrize("name", CASES)
def test_each_table_alone(name):
    """Normals only (the table albedo), a texture only (the flat weight), both with a material."""
    c = lc.case(name)
    tb = pc.tables(name)
    tex = sv.texture(*pc.TEXTURE, 11)
    rgba, _ = host(c, Surface(normals=tb.normals), (pc.SPECULAR, 5))
    pc.same_bits("normals only", rgba, pc.restate(name, normals=tb.normals, material=(pc.SPECULAR, 5)))
    rgba, _ = host(c, Surface(uvs=tb.uvs, texture=tex))
    pc.same_bits("texture only", rgba, pc.restate(name, uvs=tb.uvs, tex=tex))
    rgba, _ = host(c, Surface(uvs=tb.uvs))
    pc.same_bits("uvs without a texture change nothing", rgba, lc.expected(name).rgba)


@pytest.mark.parametrize("name", CASES)
def test_reductions_to_direct_lighting(name):
    """No surface and no material: rtdLightHost's pixel on the bits, with surface=None and with an
    empty Surface. Any surface: rtdLightHost's classes."""
    c = lc.case(name)
    tb = pc.tables(name)
    rgba0, classes0 = device.lighting_host(c.view, W, H, lc.host_lights(c.lights), pc.AMBIENT, c.offsets, c.ids)
    for surface in (None, Surface()):
        rgba, classes = host(c, surface)
        pc.same_bits("rgba", rgba, rgba0)
        lc.assert_same_classes(classes, classes0)
    pc.same_bits("against the restatement", rgba0, lc.expected(name).rgba)
    # a material alone uses the fallback normal (rtg's, fma arithmetic: not restated): the diffuse part is unchanged
    rgba, classes = host(c, None, (pc.SPECULAR, 5))
    lc.assert_same_classes(classes, classes0)
    black, _ = host(c, None, ((0.0, 0.0, 0.0), 5))
    pc.same_bits("a black highlight", black, rgba0)
    shines = (rgba[..., :3] != rgba0[..., :3]).any(-1)
    assert shines.sum() >= (W * H) // 100 and (rgba[..., :3] >= rgba0[..., :3]).all()
    assert np.array_equal(rgba[..., 3], rgba0[..., 3])
    rgba, classes = host(c, Surface(tb.normals, tb.uvs, sv.texture(*pc.TEXTURE, 11)), (pc.SPECULAR, 12))
    lc.assert_same_classes(classes, classes0)


def test_planted_uvs_are_hit():
    """0, 1, -1e-30, NaN and +-inf corners on triangles the frame hits (the pixels are compared in
    test_textured_smooth_pixels_equal_the_restatement)."""
    for name in CASES:
        c = lc.case(name)
        tb = pc.tables(name)
        assert len(tb.planted) == len(sv.PLANTED)
        for i in tb.planted:
            assert (c.ids == i).sum() >= 1
        uv = sv.interpolate(pc.edges(name), tb.uvs).reshape(H, W, 2)
        assert np.isnan(uv[np.isin(c.ids, tb.planted[3:])]).any()


def test_sentinel_ids_and_a_band():
    name = "roomA"
    c = lc.case(name)
    tb = pc.tables(name)
    surface = Surface(tb.normals, tb.uvs, sv.texture(*pc.TEXTURE, 11))
    material = (pc.SPECULAR, 5)
    want = pc.restate(name, tb.normals, tb.uvs, surface.texture, material=material)
    ids, changed = pc.sentinel_ids(name)
    rgba, classes = host(c, surface, material, ids=ids)
    assert changed.sum() == 4 and (classes[:, changed] == sc.NO_SURFACE).all()
    assert (rgba[changed] == np.float32(lc.BACKGROUND + (-1.0,))).all()
    pc.same_bits("the other pixels", rgba[~changed], want[~changed])
    band, band_classes = host(c, surface, material, row_begin=37, row_count=5)
    pc.same_bits("band", band, want[37:42])
    lc.assert_same_classes(band_classes, lc.expected(name).classes[:, 37:42])


def test_refusals():
    c = lc.case("T4")
    tb = pc.tables("T4")
    L = _native.lib()
    off = np.ascontiguousarray(c.offsets, np.float32)
    ids = np.ascontiguousarray(c.ids, np.int32)
    rgba = np.full((H, W, 4), 7.0, np.float32)
    amb = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    tex = np.ascontiguousarray(sv.texture(2, 2, 3))
    uvs = np.ascontiguousarray(tb.uvs)
    size_s, size_m = ctypes.sizeof(_native.RtvSurface), ctypes.sizeof(_native.RtpMaterial)

    def call(surface=None, material=None):
        return L.rtpLightSurfaceHost(c.view.encode(), W, H, None, 0, amb, ctypes.byref(surface) if surface else None,
                                     ctypes.byref(material) if material else None, off.ctypes.data, ids.ctypes.data, 0,
                                     H, rgba.ctypes.data, None)

    def material(size=size_m, specular=(0.5, 0.5, 0.5), k=3):
        return _native.RtpMaterial(size, (ctypes.c_float * 3)(*specular), k)

    assert call() == 0 and call(_native.RtvSurface(size_s, 0, 0, 0, 0, 0, 0), material()) == 0
    rgba[:] = 7.0
    for size in (0, 8, size_m + 8):
        assert call(material=material(size=size)) == -1
        assert f"rtp_material.struct_size is {size}, expected {size_m}" in _native.last_error()
    for k in (-1, 13):
        assert call(material=material(k=k)) == -1
        assert f"rtp_material.shininess_log2 must be 0 to 12, got {k}" in _native.last_error()
    for j, bad in enumerate((float("nan"), float("inf"), -float("inf"))):
        spec = [0.5, 0.5, 0.5]
        spec[j] = bad
        assert call(material=material(specular=spec)) == -1
        assert f"rtp_material.specular value {j} is not finite" in _native.last_error()
    for size in (0, 48, 64):
        assert call(_native.RtvSurface(size, 0, 0, 0, 0, 0, 0)) == -1
        assert "rtv_surface.struct_size" in _native.last_error()
    assert call(_native.RtvSurface(size_s, 0, 0, tex.ctypes.data, 2, 2, 0)) == -1
    assert "a texture needs uvs" in _native.last_error()
    for tw, th in ((0, 2), (2, 16385)):
        assert call(_native.RtvSurface(size_s, 0, uvs.ctypes.data, tex.ctypes.data, tw, th, 0)) == -1
        assert "rtv_surface.tex_" in _native.last_error()
    for flags in (8, 16, 0x80000000 | 1):
        assert call(_native.RtvSurface(size_s, 0, 0, 0, 0, 0, flags)) == -1
        assert "rtv_surface.flags" in _native.last_error()
    assert (rgba == 7.0).all()  # a refused call writes nothing
    # the lights' rules are rtdLightHost's
    with pytest.raises(device.SrtError, match="at most 8 lights per call, got 9"):
        host(c, Surface(normals=tb.normals), lights=[c.lights[0]] * 9)
    with pytest.raises(device.SrtError, match="ambient value 1 is not finite"):
        host(c, None, (pc.SPECULAR, 2), ambient=(0.0, float("nan"), 0.0))
    # the wrapper's own checks
    with pytest.raises(TypeError):
        device.lit_surface_host(c.view, W, H, [], pc.AMBIENT, c.offsets, c.ids, None, material=(pc.SPECULAR, 2))
    with pytest.raises(ValueError):
        host(c, None, ((1.0, 1.0), 2))
    with pytest.raises(ValueError):
        host(c, Surface(normals=tb.normals[:-1]))
    with pytest.raises(ValueError):
        device.lit_surface_host(c.view, W, H, [], pc.AMBIENT, c.offsets, c.ids, "surface")


def test_exports_and_the_pinned_families():
    out = subprocess.run(["nm", "-D", "--defined-only", str(_native.LIB_PATH)], capture_output=True, text=True,
                         check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert {s for s in exported if s.startswith("rtp")} == RTP
    header = (REPO / "include" / "srt_material.h").read_text()
    assert "ML_API" + "_ENTRY" not in header
    assert set(re.findall(r"RTP_API\s+int\s+(\w+)\s*\(", header)) == RTP
    assert len({s for s in exported if s.startswith(("ml", "srt"))}) == 52  # 14 ml* + 38 srt*: unchanged
    assert ctypes.sizeof(_native.RtpMaterial) == 24
    assert int(re.search(r"#define RTP_MAX_SHININESS_LOG2 (\d+)", header).group(1)) == _native.RTP_MAX_SHININESS_LOG2
