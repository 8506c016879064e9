"""Lit surfaces on the device (include/srt_material.h rtpLightSurfaceAsync; render.hip
LitSurfaceKernel): the textured, smooth-shaded, shadowed RGBA and the per-light class planes of a
view frame, one launch.

Every comparison is exact on the uint32 view: against rtpLightSurfaceHost, against the numpy float32
restatement of DESIGN.md section 2 "Lit surfaces" (tests/litsurface_cases.py) where a normals table
is given, and against rtdLightAsync for the two reductions. View frames are 160 x 96, spot frames
192 x 80, cube faces 64 x 64, as in test_gpu_lighting.py.
"""
from __future__ import annotations

import ctypes

import numpy as np
import pytest

import lighting_cases as lc
import litsurface_cases as pc
import shadow_cases as sc
import surface_cases as sv
from oracle import srt_oracle as oracle
from test_gpu_lighting import Rig, default_env

pytestmark = pytest.mark.gpu

W, H = pc.W, pc.H
MATERIAL = (pc.SPECULAR, 5)


class SurfaceRig(Rig):
    """test_gpu_lighting's rig with light_surface(): `surface` holds numpy tables, uploaded here."""

    def device_surface(self, surface):
        if surface is None:
            return None
        up = lambda a: None if a is None else self.torch.from_numpy(np.array(a, np.float32)).cuda()  # noqa: E731
        return self.srt.Surface(up(surface.normals), up(surface.uvs), up(surface.texture), surface.wrap, surface.filter,
                                surface.modulate)

    def light_surface(self, surface=None, material=None, lights=None, ambient=pc.AMBIENT, r0=0, rows=None, ids=None,
                      with_classes=True):
        lights = self.lights if lights is None else lights
        off, idt, rgba, classes = self.buffers(len(lights), r0, rows, ids)
        self.view.light_surface(lights, off, idt, self.device_surface(surface), rgba, ambient=ambient,
                                material=pc.host_material(material), classes=classes if with_classes else None,
                                row_begin=r0, row_count=rgba.shape[0], stream=self.stream)
        self.torch.cuda.synchronize()
        return rgba.cpu().numpy(), classes.cpu().numpy()


def host(c, surface=None, material=None, ids=None, lights=None):
    from simpleraytracer_amd import device

    return device.lit_surface_host(c.view, W, H, lc.host_lights(c.lights if lights is None else lights), pc.AMBIENT,
                                   c.offsets, c.ids if ids is None else ids, surface, pc.host_material(material))


def full_surface(name, size=pc.TEXTURE, **kw):
    tb = pc.tables(name)
    return pc.host_surface(tb.normals, tb.uvs, sv.texture(*size, 11), **kw)


@pytest.mark.parametrize("name", ["T4", "roomA"])
def test_device_equals_the_host_and_the_restatement(gpu, monkeypatch, name):
    """Fails without the feature. Normals + uvs + a texture of 1 x 1, 3 x 5 and 64 x 64 texels under
    a material; then clamp + nearest + modulate without one; then a material on the fallback normal
    (not restated in numpy: against the host)."""
    default_env(monkeypatch)
    c = lc.case(name)
    tb = pc.tables(name)
    want_classes = lc.expected(name).classes
    rig = SurfaceRig(c)
    for size in ((1, 1), pc.TEXTURE, (64, 64)):
        s = full_surface(name, size)
        rgba, classes = rig.light_surface(s, MATERIAL)
        hrgba, hclasses = host(c, s, MATERIAL)
        lc.assert_same_classes(classes, want_classes)
        lc.assert_same_classes(classes, hclasses)
        pc.same_bits(f"{size} rgba against the host's", rgba, hrgba)
        pc.same_bits(f"{size} rgba", rgba, pc.restate(name, tb.normals, tb.uvs, s.texture, material=MATERIAL))
    s = full_surface(name, wrap="clamp", filter="nearest", modulate=True)
    rgba, _ = rig.light_surface(s)
    pc.same_bits("clamp nearest modulate", rgba, pc.restate(name, tb.normals, tb.uvs, s.texture, "clamp", "nearest", True))
    s = pc.host_surface(uvs=tb.uvs, tex=sv.texture(*pc.TEXTURE, 11), wrap="clamp")
    rgba, classes = rig.light_surface(s, (pc.SPECULAR, 12))
    rig.close()
    hrgba, hclasses = host(c, s, (pc.SPECULAR, 12))
    pc.same_bits("a material on the fallback normal, against the host's", rgba, hrgba)
    lc.assert_same_classes(classes, hclasses)


@pytest.mark.parametrize("shininess_log2", [0, 1, 12])
def test_every_shininess_equals_the_restatement_and_the_host(gpu, monkeypatch, shininess_log2):
    """roomA under the normals table: no squaring, one, and twelve (s^4096: most highlights underflow)."""
    default_env(monkeypatch)
    name = "roomA"
    c = lc.case(name)
    tb = pc.tables(name)
    s = full_surface(name)
    material = (pc.SPECULAR, shininess_log2)
    rig = SurfaceRig(c)
    rgba, classes = rig.light_surface(s, material)
    rig.close()
    hrgba, hclasses = host(c, s, material)
    lc.assert_same_classes(classes, lc.expected(name).classes)
    lc.assert_same_classes(classes, hclasses)
    pc.same_bits("rgba against the host's", rgba, hrgba)
    pc.same_bits("rgba", rgba, pc.restate(name, tb.normals, tb.uvs, s.texture, material=material))


def test_sixteen_light_frames(gpu, monkeypatch):
    default_env(monkeypatch)
    c = lc.case("full")
    tb = pc.tables("full")
    s = full_surface("full")
    rig = SurfaceRig(c)
    rgba, classes = rig.light_surface(s, MATERIAL)
    rig.close()
    lc.assert_same_classes(classes, lc.expected("full").classes)
    pc.same_bits("rgba", rgba, pc.restate("full", tb.normals, tb.uvs, s.texture, material=MATERIAL))
    pc.same_bits("rgba against the host's", rgba, host(c, s, MATERIAL)[0])


@pytest.mark.parametrize("name", ["T4", "roomA"])
def test_reductions_and_class_planes(gpu, monkeypatch, name):
    """surface=None, material=None: light()'s pixel on the bits. Any surface: light()'s classes. The
    RGBA without class planes (lights that are not facing skip their scan) is the RGBA with them."""
    default_env(monkeypatch)
    c = lc.case(name)
    s = full_surface(name)
    rig = SurfaceRig(c)
    rgba0, classes0 = rig.light()
    plain, plain_classes = rig.light_surface(None, None)
    empty, _ = rig.light_surface(pc.host_surface(), None)
    rgba, classes = rig.light_surface(s, MATERIAL)
    bare, canary = rig.light_surface(s, MATERIAL, with_classes=False)
    rig.close()
    pc.same_bits("no surface, no material", plain, rgba0)
    pc.same_bits("an empty surface", empty, rgba0)
    pc.same_bits("against the restatement", plain, lc.expected(name).rgba)
    lc.assert_same_classes(plain_classes, classes0)
    lc.assert_same_classes(classes, classes0)
    pc.same_bits("rgba without class planes", bare, rgba)
    assert (canary == 9).all()  # classes=None: nothing is written to a buffer that was not passed
    assert (rgba[..., :3] != rgba0[..., :3]).any(-1).sum() >= (W * H) // 20


def test_band_sentinels_and_planted_uvs(gpu, monkeypatch):
    default_env(monkeypatch)
    name = "roomA"
    c = lc.case(name)
    tb = pc.tables(name)
    s = full_surface(name)
    want = pc.restate(name, tb.normals, tb.uvs, s.texture, material=MATERIAL)
    ids, changed = pc.sentinel_ids(name)
    rig = SurfaceRig(c)
    band, band_classes = rig.light_surface(s, MATERIAL, r0=37, rows=5)
    rgba, classes = rig.light_surface(s, MATERIAL, ids=ids)
    rig.close()
    pc.same_bits("band", band, want[37:42])
    lc.assert_same_classes(band_classes, lc.expected(name).classes[:, 37:42])
    assert changed.sum() == 4 and (classes[:, changed] == sc.NO_SURFACE).all()
    assert (rgba[changed] == np.float32(lc.BACKGROUND + (-1.0,))).all()
    pc.same_bits("the other pixels", rgba[~changed], want[~changed])
    # the planted uvs (0, 1, -1e-30, NaN, +-inf) lie on triangles the frame hits: compared above
    assert len(tb.planted) == len(sv.PLANTED) and all((c.ids == i).any() for i in tb.planted)


def test_odd_frame_exercises_the_tail_guard(gpu, monkeypatch):
    """150 x 91 of the room: 13650 pixels, not a multiple of the kernel's pixels per block. The ids are
    the oracle's; the device equals the host."""
    import torch

    import simpleraytracer_amd as srt
    from simpleraytracer_amd import device

    default_env(monkeypatch)
    w, h = 150, 91
    c = lc.case("roomA")
    tb = pc.tables("roomA")
    off = np.random.default_rng(5).random((h, w, 2), dtype=np.float32)
    o = oracle.OracleScene(c.view)
    ids = o.render(w, h, off)[..., 3].astype(np.int32)
    o.close()
    assert (ids >= 0).sum() > 1000 and (w * h) % 16 != 0
    s = full_surface("roomA")
    lights = c.lights[:2]  # the point light and the spot light inside the room
    stream = torch.cuda.current_stream()
    view = srt.DeviceScene(c.view, 0)
    view.prepare(w, h, stream)
    bulb = srt.OmniLight(c.view, 0, lights[0].origin)
    bulb.prepare(64, stream)
    spot = srt.DeviceScene(c.view, 0, camera=lights[1].cam)
    spot.prepare(lights[1].wl, lights[1].hl, stream)
    dl = [srt.PointLight(bulb, lights[0].color, lights[0].falloff, lights[0].bias),
          srt.SpotLight(spot, lights[1].color, lights[1].falloff, lights[1].bias)]
    up = lambda a: torch.from_numpy(np.array(a)).cuda()  # noqa: E731
    rgba = torch.full((h + 1, w, 4), float("nan"), dtype=torch.float32, device="cuda")  # one canary row
    classes = torch.full((2, h, w), 9, dtype=torch.uint8, device="cuda")
    view.light_surface(dl, up(off), up(ids), srt.Surface(up(tb.normals), up(tb.uvs), up(s.texture)), rgba[:h],
                       ambient=pc.AMBIENT, material=pc.host_material(MATERIAL), classes=classes, stream=stream)
    torch.cuda.synchronize()
    got, got_classes = rgba.cpu().numpy(), classes.cpu().numpy()
    for x in (bulb, spot, view):
        x.close()
    hrgba, hclasses = device.lit_surface_host(c.view, w, h, lc.host_lights(lights), pc.AMBIENT, off, ids, s,
                                              pc.host_material(MATERIAL))
    assert np.isnan(got[h]).all()  # nothing past the frame
    pc.same_bits("rgba against the host's", got[:h], hrgba)
    lc.assert_same_classes(got_classes, hclasses)


def test_render_lit_surface_traces_the_oracles_ids(gpu, monkeypatch):
    default_env(monkeypatch)
    name = "roomA"
    c = lc.case(name)
    tb = pc.tables(name)
    s = full_surface(name)
    rig = SurfaceRig(c)
    off, _, lit, classes = rig.buffers(len(rig.lights))
    traced = rig.torch.full((H, W), -7, dtype=rig.torch.int32, device="cuda")
    rig.view.render_lit_surface(rig.lights, off, traced, rig.device_surface(s), lit, ambient=pc.AMBIENT,
                                material=pc.host_material(MATERIAL), classes=classes, stream=rig.stream)
    rig.torch.cuda.synchronize()
    traced, lit, classes = traced.cpu().numpy(), lit.cpu().numpy(), classes.cpu().numpy()
    rig.close()
    assert np.array_equal(traced, c.ids)
    pc.same_bits("rgba", lit, pc.restate(name, tb.normals, tb.uvs, s.texture, material=MATERIAL))
    lc.assert_same_classes(classes, lc.expected(name).classes)


def test_recomputed_records_give_the_same_bits(gpu, monkeypatch):
    """SRT_TRACE_RECORDS=recompute: the kernel's other instantiation."""
    default_env(monkeypatch)
    monkeypatch.setenv("SRT_TRACE_RECORDS", "recompute")
    name = "roomA"
    c = lc.case(name)
    tb = pc.tables(name)
    s = full_surface(name)
    rig = SurfaceRig(c)
    rgba, classes = rig.light_surface(s, MATERIAL)
    rig.close()
    pc.same_bits("rgba", rgba, pc.restate(name, tb.normals, tb.uvs, s.texture, material=MATERIAL))
    lc.assert_same_classes(classes, lc.expected(name).classes)


def test_a_refused_call_leaves_the_output_untouched(gpu, monkeypatch):
    from simpleraytracer_amd import Material, SpotLight, SrtError, _native

    default_env(monkeypatch)
    c = lc.case("roomA")
    tb = pc.tables("roomA")
    rig = SurfaceRig(c)
    L = _native.lib()
    off, idt, out, cls = rig.buffers(len(rig.lights))
    s = rig.device_surface(full_surface("roomA"))
    point, spot_in, head = rig.lights
    nan = float("nan")
    for lights, kw, text in (
            ([spot_in] * 9, {}, "at most 8 lights per call, got 9"),
            ([spot_in, SpotLight(spot_in.scene, (1.0, nan, 1.0))], {}, "light 1: color value 1 is not finite"),
            ([spot_in], {"ambient": (0.0, nan, 0.0)}, "ambient value 1 is not finite"),
            ([spot_in], {"material": Material((0.5, 0.5, 0.5), 13)}, "rtp_material.shininess_log2 must be 0 to 12, got 13"),
            ([spot_in], {"material": Material((0.5, 0.5, 0.5), -1)}, "rtp_material.shininess_log2 must be 0 to 12, got -1"),
            ([spot_in], {"material": Material((0.5, nan, 0.5), 3)}, "rtp_material.specular value 1 is not finite")):
        with pytest.raises(SrtError, match=text):
            rig.view.light_surface(lights, off, idt, s, out, classes=None, **kw)
    # the structs themselves: sizes, a texture without uvs, texture sizes, unknown flags
    amb = (ctypes.c_float * 3)(0.0, 0.0, 0.0)
    size_s, size_m = ctypes.sizeof(_native.RtvSurface), ctypes.sizeof(_native.RtpMaterial)

    def call(surface=None, material=None, view=rig.view.handle):
        return L.rtpLightSurfaceAsync(view, None, 0, amb, ctypes.byref(surface) if surface else None,
                                      ctypes.byref(material) if material else None, off.data_ptr(), idt.data_ptr(), 0, H,
                                      out.data_ptr(), None, None)

    tex, uvs = s.texture.data_ptr(), s.uvs.data_ptr()
    for surface, material, text in (
            (_native.RtvSurface(48, 0, 0, 0, 0, 0, 0), None, "rtv_surface.struct_size is 48"),
            (_native.RtvSurface(size_s, 0, 0, tex, 5, 3, 0), None, "a texture needs uvs"),
            (_native.RtvSurface(size_s, 0, uvs, tex, 0, 3, 0), None, "rtv_surface.tex_width"),
            (_native.RtvSurface(size_s, 0, uvs, tex, 5, 16385, 0), None, "rtv_surface.tex_height"),
            (_native.RtvSurface(size_s, 0, 0, 0, 0, 0, 8), None, "rtv_surface.flags"),
            (None, _native.RtpMaterial(8, (ctypes.c_float * 3)(0.5, 0.5, 0.5), 3), "rtp_material.struct_size is 8")):
        assert call(surface, material) == -1 and text in _native.last_error()
    assert call(view=None) == -1 and "view is NULL" in _native.last_error()
    rig.torch.cuda.synchronize()
    assert rig.torch.isnan(out).all() and (cls == 9).all()  # nothing was enqueued
    # the wrapper's own checks
    with pytest.raises(ValueError):
        rig.view.light_surface(rig.lights, off, idt, "surface", out)
    with pytest.raises(TypeError):
        rig.view.light_surface(rig.lights, off, idt, s, out, material=MATERIAL)
    with pytest.raises(ValueError):
        rig.view.light_surface(rig.lights, off, idt, rig.srt.Surface(normals=s.normals[:-1]), out)
    # the valid call still works after the refused ones
    rgba, classes = rig.light_surface(full_surface("roomA"), MATERIAL)
    rig.close()
    pc.same_bits("rgba", rgba, pc.restate("roomA", tb.normals, tb.uvs, sv.texture(*pc.TEXTURE, 11), material=MATERIAL))
    lc.assert_same_classes(classes, lc.expected("roomA").classes)
