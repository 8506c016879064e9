"""Lit ray hits on the device (include/srt_hits.h rthLightHitsAsync; render.hip LightHitsKernel): what
the hits of caller-supplied rays look like under the lights, one launch, and render_reflection()'s
five steps.

Every comparison is exact: against rthLightHitsHost, against rtdLightAsync for the eye rays of a
frame, and against the numpy float32 restatement of DESIGN.md section 2 "Hits" for the mirror
bounce (tests/hits_cases.py). View frames are 160 x 96, the lights lighting_cases'.
"""
from __future__ import annotations

import ctypes
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import hits_cases as hc
import lighting_cases as lc
import omni_cases as oc
import shadow_cases as sc

pytestmark = pytest.mark.gpu

W, H = hc.W, hc.H
f32 = np.float32
SENTINEL = 7.25  # what an output buffer holds where nothing may be written


def default_env(monkeypatch):
    for name in ("SRT_SETUP", "SRT_CULL_BIN", "SRT_CULL_BIN_CAP", "SRT_TRACE_RECORDS"):
        monkeypatch.delenv(name, raising=False)


class Rig:
    """A case's scene (NOT prepared unless asked: the hits need no frame) and its lights over the
    same file on cuda:0, the lights prepared; hits() returns numpy arrays."""

    def __init__(self, name, lights=None, prepare=False, path=None):
        import torch

        import simpleraytracer_amd as srt

        self.torch, self.srt, self.c = torch, srt, lc.case(name)
        self.path = self.c.view if path is None else path
        self.stream = torch.cuda.current_stream()
        self.view = srt.DeviceScene(self.path, 0)
        if prepare:
            self.view.prepare(W, H, self.stream)
        self.owned = []
        self.lights = [self.make(l) for l in (self.c.lights if lights is None else lights)]

    def make(self, l):
        srt = self.srt
        if l.kind == "point":
            light = srt.OmniLight(self.path, 0, l.origin)
            light.prepare(l.face_size, self.stream)
            self.owned.append(light)
            return srt.PointLight(light, l.color, l.falloff, l.bias)
        scene = srt.DeviceScene(self.path, 0, camera=l.cam)
        scene.prepare(l.wl, l.hl, self.stream)
        self.owned.append(scene)
        return srt.SpotLight(scene, l.color, l.falloff, l.bias)

    def upload(self, el):
        torch = self.torch
        out = tuple(torch.from_numpy(np.array(a)).cuda() for a in (el.rays, el.ids, el.t))
        torch.cuda.synchronize()
        return out

    def hits(self, el, lights=None, ambient=lc.AMBIENT, with_classes=True, base=None, weight=(1.0, 1.0, 1.0), extra=3):
        """(rgba, classes) of the elements. The rgba buffer holds `extra` more elements than the call
        is given, which must keep the sentinel; with a `base` (a numpy array) the buffer holds it and
        the call blends in place. Without class planes the returned planes are the untouched canary."""
        torch = self.torch
        lights = self.lights if lights is None else lights
        rays, ids, t = self.upload(el)
        count = ids.shape[0]
        rgba = torch.full((count + extra, 4), SENTINEL, dtype=torch.float32, device="cuda")
        planes = torch.full((len(lights), count), 9, dtype=torch.uint8, device="cuda")
        if base is not None:
            rgba[:count] = torch.from_numpy(np.array(base)).cuda()
        torch.cuda.synchronize()
        self.view.light_hits(lights, rays, ids, t, rgba[:count], ambient=ambient, classes=planes if with_classes else None,
                             base=rgba[:count] if base is not None else None, weight=weight, stream=self.stream)
        torch.cuda.synchronize()
        assert (rgba[count:].cpu().numpy() == f32(SENTINEL)).all(), "the call wrote behind its last element"
        return rgba[:count].cpu().numpy(), planes.cpu().numpy()

    def close(self):
        for o in self.owned:
            o.close()
        self.view.close()


@functools.lru_cache(maxsize=None)
def host_answer(name: str, kind: str):
    c = lc.case(name)
    el = hc.eye(name) if kind == "eye" else hc.bounce(name)
    rgba, classes = hc.host(name, c.lights, el)
    rgba.setflags(write=False)
    classes.setflags(write=False)
    return rgba, classes


@pytest.mark.parametrize("records", ["stored", "recompute"])
@pytest.mark.parametrize("name,kind", [("T4", "eye"), ("roomA", "eye"), ("full", "eye"), ("roomA", "bounce")])
def test_device_equals_the_host(gpu, monkeypatch, name, kind, records):
    """Fails without the feature. Eye rays (coherent) and a mirror bounce (scattered over the light
    frames), on stored and on recomputed records; the scene is not prepared."""
    default_env(monkeypatch)
    monkeypatch.setenv("SRT_TRACE_RECORDS", records)
    el = hc.eye(name) if kind == "eye" else hc.bounce(name)
    want_rgba, want_classes = host_answer(name, kind)
    rig = Rig(name)
    rgba, classes = rig.hits(el)
    bare, canary = rig.hits(el, with_classes=False)
    rig.close()
    hc.assert_same_classes(classes, want_classes)
    lc.same_bits("rgba", rgba, want_rgba)
    lc.same_bits("rgba without class planes", bare, rgba)
    assert (canary == 9).all()  # classes=None: nothing is written to a buffer that was not passed
    if kind == "bounce":
        want = hc.expected_bounce(name)
        hc.assert_same_classes(classes, want.classes)
        lc.same_bits("rgba against the restatement", rgba, want.rgba)


@pytest.mark.parametrize("name", ["T4", "roomA"])
def test_eye_rays_equal_light_on_the_same_frame(gpu, monkeypatch, name):
    """scene.light_hits of (eye ray, traced id, G-buffer depth) is scene.light of the frame, bit for
    bit, class planes included; the depth is the device's own gbuffer()."""
    import torch

    default_env(monkeypatch)
    c = lc.case(name)
    rig = Rig(name, prepare=True)
    off = torch.from_numpy(np.array(c.offsets)).cuda()
    idt = torch.from_numpy(np.array(c.ids)).cuda()
    lit = torch.full((H, W, 4), SENTINEL, dtype=torch.float32, device="cuda")
    lit_classes = torch.full((len(rig.lights), H, W), 9, dtype=torch.uint8, device="cuda")
    depth = torch.full((H, W), SENTINEL, dtype=torch.float32, device="cuda")
    rig.view.light(rig.lights, off, idt, lit, ambient=lc.AMBIENT, classes=lit_classes, stream=rig.stream)
    rig.view.gbuffer(off, idt, depth=depth, stream=rig.stream)
    torch.cuda.synchronize()
    el = hc.eye(name)
    lc.same_bits("the device's depth plane", depth.cpu().numpy().reshape(-1), el.t)
    rgba, classes = rig.hits(el)
    bare, _ = rig.hits(el, with_classes=False)
    rig.close()
    hc.assert_same_classes(classes, lit_classes.cpu().numpy().reshape(len(rig.lights), -1))
    lc.same_bits("rgba", rgba, lit.cpu().numpy().reshape(-1, 4))
    lc.same_bits("rgba without class planes", bare, rgba)


def test_element_counts_at_the_launch_shape_boundaries(gpu, monkeypatch):
    """16 elements per block, 16 lanes per element: 1, 15, 16, 17, 255, 256, 257 elements cut from the
    bounce each give the same slice of the full answer and leave the buffer behind them alone."""
    default_env(monkeypatch)
    el = hc.bounce("roomA")
    want = hc.expected_bounce("roomA")
    rig = Rig("roomA")
    start = 4000  # (mid-frame: surfaces of every class)
    for count in (1, 15, 16, 17, 255, 256, 257):
        part = SimpleNamespace(rays=el.rays[start:start + count], ids=el.ids[start:start + count],
                               t=el.t[start:start + count])
        rgba, classes = rig.hits(part, extra=40)
        hc.assert_same_classes(classes, want.classes[:, start:start + count])
        lc.same_bits(f"{count} elements", rgba, want.rgba[start:start + count])
    rig.close()
    assert len(set(want.classes[2, start:start + 257])) == 3  # the slice holds shadowed, lit and outside elements


def test_light_counts(gpu, monkeypatch):
    """No light (the albedo . ambient plane), one spot, one point, 2 point + 4 spot = 16 frames, and one
    light given twice."""
    from oracle import srt_oracle as oracle

    default_env(monkeypatch)
    el = hc.bounce("roomA")
    full = lc.case("full").lights
    point, spot = full[0], full[1]
    twice = [spot, lc.spot(spot.cam, spot.wl, spot.hl, (0.1, 0.7, 0.2), spot.falloff, spot.bias)]
    rig = Rig("roomA", full)
    by_spec = dict(zip(map(id, full), rig.lights))
    second = rig.srt.SpotLight(by_spec[id(spot)].scene, twice[1].color, twice[1].falloff, twice[1].bias)
    got = {}
    for what, specs, lights in (("none", [], []), ("a spot", [spot], [by_spec[id(spot)]]),
                                ("a point", [point], [by_spec[id(point)]]), ("sixteen frames", full, rig.lights),
                                ("twice", twice, [by_spec[id(spot)], second])):
        got[what] = (specs, *rig.hits(el, lights=lights, ambient=(0.5, 0.25, 1.0) if what == "none" else lc.AMBIENT))
    rig.close()
    for what, (specs, rgba, classes) in got.items():
        if what == "none":
            continue
        want_rgba, want_classes = hc.host("roomA", specs, el)
        hc.assert_same_classes(classes, want_classes)
        lc.same_bits(what, rgba, want_rgba)
    sc.assert_same_mask(got["twice"][2][0], got["twice"][2][1])
    assert not np.array_equal(got["twice"][1], got["a spot"][1])
    # no light: albedo . ambient, alpha the id (every element of the closed room has a surface)
    s = oracle.OracleScene(lc.case("roomA").view)
    albedo = s.albedo.astype(f32)
    s.close()
    _, rgba, classes = got["none"]
    assert classes.shape == (0, el.ids.size) and (el.ids >= 0).all()
    lc.same_bits("no lights", rgba[:, :3], (albedo[el.ids] * f32((0.5, 0.25, 1.0))[None, :]).astype(f32))
    assert np.array_equal(rgba[:, 3], el.ids.astype(f32))


def test_every_kind_of_element_and_the_blend_in_place(gpu, monkeypatch):
    default_env(monkeypatch)
    c = lc.case("roomA")
    edges = hc.edge_elements("roomA")
    want = hc.expected_edges("roomA", edges)
    rig = Rig("roomA")
    rgba, classes = rig.hits(edges.el)
    base = np.random.default_rng(3).random((17, 4), dtype=f32)
    base[2] = (-0.0, np.nan, -np.inf, -0.0)  # an absent element: these bits stay
    base[14].view(np.uint32)[:] = (0x7FC12345, 0xFFC00001, 0x80000000, 0x7F800001)
    blended, _ = rig.hits(edges.el, base=base, weight=(0.5, 0.25, 2.0))
    zero, _ = rig.hits(edges.el, base=base, weight=(0.0, 0.0, 0.0))
    rig.close()
    for k, what in enumerate(edges.what):
        lc.same_bits(what, rgba[k], want.rgba[k])
        assert (classes[:, k] == want.classes[:, k]).all(), (what, classes[:, k], want.classes[:, k])
    assert edges.kind[2] == edges.kind[14] == "absent"
    lc.same_bits("blended in place", blended, hc.blend(want.rgba, want.absent, base, (0.5, 0.25, 2.0)))
    lc.same_bits("a zero weight", zero, hc.blend(want.rgba, want.absent, base, (0.0, 0.0, 0.0)))
    lc.same_bits("absent elements keep the base's bits", blended[want.absent], base[want.absent])
    # the T4 bounce: thousands of absent elements and misses in one call, on a base, against the host
    t4 = lc.case("T4")
    el = hc.bounce("T4")
    big = np.random.default_rng(5).random((el.ids.size, 4), dtype=f32)
    rig = Rig("T4")
    got, _ = rig.hits(el, base=big, weight=(0.5, 0.25, 2.0))
    rig.close()
    lc.same_bits("T4 bounce on a base", got, hc.host("T4", t4.lights, el, base=big, weight=(0.5, 0.25, 2.0))[0])
    assert hc.kinds(el).absent.sum() > 1000 and len(c.lights) == 3


def test_moved_lights_and_triangles(gpu, monkeypatch):
    """After light.set_camera / OmniLight.set_origin, and after set_vertices on the scene and on the
    lights, the answer is the host's at the new pose (a fresh scene's); set_camera on the shaded scene
    changes nothing: none of its frame is read."""
    import torch

    default_env(monkeypatch)
    c = lc.case("roomA")
    el = hc.bounce("roomA")
    p, s, head = c.lights
    rig = Rig("roomA")
    before, _ = rig.hits(el)
    rig.view.set_camera(oc.VIEWS["B"], stream=rig.stream)
    same, _ = rig.hits(el)
    lc.same_bits("after set_camera on the shaded scene", same, before)
    # the lights move
    moved = [lc.point(lc.ORIGIN2, p.face_size, p.color, p.falloff, p.bias),
             lc.spot(lc.SPOT_IN2, s.wl, s.hl, s.color, s.falloff, s.bias), head]
    rig.owned[0].set_origin(lc.ORIGIN2, stream=rig.stream)
    rig.owned[1].set_camera(lc.SPOT_IN2, stream=rig.stream)
    after, after_classes = rig.hits(el)
    want_rgba, want_classes = hc.host("roomA", moved, el)
    hc.assert_same_classes(after_classes, want_classes)
    lc.same_bits("after the lights moved", after, want_rgba)
    assert not np.array_equal(after, before)
    # the triangles move (a shear: every normal and every light frame changes)
    shape = np.shape(oc.room_vertices())
    v = np.array(oc.room_vertices(), f32).reshape(-1, 3, 3)
    v[..., 0] = v[..., 0] + f32(0.125) * v[..., 1]
    path = sc.write_with_camera(sc._dir() / "hits_sheared.srt", v.reshape(shape), oc.VIEWS["A"])
    dv = torch.from_numpy(np.ascontiguousarray(v.reshape(-1, 9))).cuda()
    torch.cuda.synchronize()
    for scene in [rig.view] + rig.owned:
        scene.set_vertices(dv, stream=rig.stream)
    sheared, sheared_classes = rig.hits(el)
    rig.close()
    from simpleraytracer_amd import device

    want_rgba, want_classes = device.light_hits_host(path, lc.host_lights(moved), lc.AMBIENT, el.rays, el.ids, el.t,
                                                     classes=True)
    hc.assert_same_classes(sheared_classes, want_classes)
    lc.same_bits("after the triangles moved", sheared, want_rgba)
    assert not np.array_equal(sheared, after)
    fresh = Rig("roomA", moved, path=path)
    again, again_classes = fresh.hits(el)
    fresh.close()
    hc.assert_same_classes(again_classes, sheared_classes)
    lc.same_bits("a fresh scene at the new pose", again, sheared)


def _reflection_by_hand(rig, off, reflectivity, stream):
    """render_reflection's five steps, one call each -> (ids, rgba, bounce ids, bounce t)."""
    torch = rig.torch
    ids = torch.full((H, W), -7, dtype=torch.int32, device="cuda")
    rgba = torch.full((H, W, 4), SENTINEL, dtype=torch.float32, device="cuda")
    rays = torch.full((1, H, W, 8), SENTINEL, dtype=torch.float32, device="cuda")
    hit = torch.full((H * W,), -7, dtype=torch.int32, device="cuda")
    t = torch.full((H * W,), SENTINEL, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rig.view.trace_ids(off, ids, stream=stream)
    rig.view.light(rig.lights, off, ids, rgba, ambient=lc.AMBIENT, stream=stream)
    rig.view.generate_rays_frame(off, ids, rig.srt.Mirror(), rays, stream=stream)
    rig.view.closest(rays.view(-1, 8), hit, t, stream=stream)
    rig.view.light_hits(rig.lights, rays.view(-1, 8), hit, t, rgba.view(-1, 4), ambient=lc.AMBIENT, base=rgba.view(-1, 4),
                        weight=reflectivity, stream=stream)
    torch.cuda.synchronize()
    return ids, rgba, hit, t


@pytest.mark.parametrize("name", ["T4", "roomA"])
def test_render_reflection(gpu, monkeypatch, name):
    """render_reflection equals its five steps by hand, which equal the host chain lighting_host ->
    rays_host(Mirror) -> closest_host -> light_hits_host(base); a second call with the same scratch
    allocates nothing; and on another stream it needs no host synchronise between the steps."""
    import torch

    from simpleraytracer_amd import device
    from simpleraytracer_amd.device import ReflectionScratch

    default_env(monkeypatch)
    c = lc.case(name)
    reflectivity = (0.5, 0.25, 0.75)
    rig = Rig(name, prepare=True)
    off = torch.from_numpy(np.array(c.offsets)).cuda()
    ids_h, rgba_h, hit_h, t_h = _reflection_by_hand(rig, off, reflectivity, rig.stream)
    ids = torch.full((H, W), -7, dtype=torch.int32, device="cuda")
    rgba = torch.full((H, W, 4), SENTINEL, dtype=torch.float32, device="cuda")
    scratch = ReflectionScratch(W, H, 0)
    torch.cuda.synchronize()
    out = rig.view.render_reflection(rig.lights, off, ids, rgba, reflectivity, ambient=lc.AMBIENT, scratch=scratch,
                                     stream=rig.stream)
    torch.cuda.synchronize()
    assert out is scratch
    first = rgba.cpu().numpy()
    held = torch.cuda.memory_allocated()
    rig.view.render_reflection(rig.lights, off, ids, rgba, reflectivity, ambient=lc.AMBIENT, scratch=scratch,
                               stream=rig.stream)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == held
    lc.same_bits("the second call", rgba.cpu().numpy(), first)
    assert np.array_equal(ids.cpu().numpy(), c.ids) and np.array_equal(ids_h.cpu().numpy(), c.ids)
    lc.same_bits("against the five steps by hand", first, rgba_h.cpu().numpy())
    assert np.array_equal(scratch.ids.cpu().numpy(), hit_h.cpu().numpy())
    lc.same_bits("the bounce's t", scratch.t.cpu().numpy(), t_h.cpu().numpy())
    # another stream: everything prepared and built on `one`, the composition on `two`, no synchronise between
    one, two = torch.cuda.Stream(), torch.cuda.Stream()
    rgba2 = torch.full((H, W, 4), SENTINEL, dtype=torch.float32, device="cuda")
    ids2 = torch.full((H, W), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rig.view.prepare(W, H, one)
    for o, l in zip(rig.owned, c.lights):
        o.prepare(*((l.face_size,) if l.kind == "point" else (l.wl, l.hl)), one)
    rig.view.render_reflection(rig.lights, off, ids2, rgba2, reflectivity, ambient=lc.AMBIENT, scratch=scratch, stream=two)
    two.synchronize()
    streamed = rgba2.cpu().numpy()
    torch.cuda.synchronize()
    rig.close()
    lc.same_bits("on another stream", streamed, first)
    # the host chain
    pos = device.pixel_positions(W, H, c.offsets)
    lit, _ = device.lighting_host(c.view, W, H, lc.host_lights(c.lights), lc.AMBIENT, c.offsets, c.ids)
    el = hc.bounce(name)
    assert np.array_equal(hit_h.cpu().numpy(), el.ids)  # (the device's mirror rays and their hits are the host's)
    want = device.light_hits_host(c.view, lc.host_lights(c.lights), lc.AMBIENT, el.rays, el.ids, el.t,
                                  base=lit.reshape(-1, 4), weight=reflectivity)
    lc.same_bits("against the host chain", first.reshape(-1, 4), want)
    surface = (c.ids >= 0).reshape(-1)
    lc.same_bits("pixels without a surface keep the lit frame's background", first.reshape(-1, 4)[~surface],
                 lit.reshape(-1, 4)[~surface])
    assert pos.shape == (H * W, 2) and not np.array_equal(first.reshape(-1, 4)[surface], lit.reshape(-1, 4)[surface])


def test_refusals_leave_the_output_alone(gpu, monkeypatch):
    import torch

    import simpleraytracer_amd as srt
    from simpleraytracer_amd import PointLight, SpotLight, SrtError, _native

    default_env(monkeypatch)
    c = lc.case("roomA")
    el = hc.bounce("roomA")
    rig = Rig("roomA")
    rays, ids, t = rig.upload(el)
    count = ids.shape[0]
    out = torch.full((count + 1, 4), SENTINEL, dtype=torch.float32, device="cuda")
    cls = torch.full((3, count), 9, dtype=torch.uint8, device="cuda")
    long_rays = torch.zeros((count + 1, 8), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    point, spot_in, head = rig.lights
    nan = float("nan")
    fresh = srt.DeviceScene(c.view, 0, camera=lc.SPOT_IN)
    fresh_omni = srt.OmniLight(c.view, 0, oc.ORIGIN)
    other = srt.DeviceScene(sc.case("grid").view, 0)
    other.prepare(W, H, rig.stream)
    big = srt.DeviceScene(c.view, 0, camera=lc.SPOT_IN)
    big.prepare(3072, 3072, rig.stream)
    big_light = SpotLight(big, spot_in.color, spot_in.falloff, spot_in.bias)
    for lights, kw, text in (
            ([spot_in, SpotLight(fresh)], {}, "light 1 has not been prepared"),
            ([PointLight(fresh_omni)], {}, "light 0 has not been prepared"),
            ([spot_in, head, SpotLight(other)], {}, r"light 2: the view scene has 216 triangles, the light's scene 288"),
            ([spot_in, big_light], {}, "light 1: its 3072 x 3072 frame reads recomputed records, the light frames before "
                                       "it stored ones: a light frame too large for a shared cull setup"),
            ([spot_in] * 9, {}, "at most 8 lights per call, got 9"),
            ([point, point, spot_in, spot_in, spot_in, spot_in, head], {}, "light 6 brings the call to 17 light frames"),
            ([spot_in, SpotLight(spot_in.scene, (1.0, nan, 1.0))], {}, "light 1: color value 1 is not finite"),
            ([PointLight(point.light, falloff=-1.0)], {}, "light 0: falloff must be finite and >= 0"),
            ([spot_in, SpotLight(spot_in.scene, bias=nan)], {}, "light 1: bias must be finite and >= 0"),
            ([spot_in], {"ambient": (0.0, nan, 0.0)}, "ambient value 1 is not finite"),
            ([spot_in], {"base": out[:count], "weight": (1.0, float("inf"), 1.0)}, "weight value 1 is not finite")):
        with pytest.raises(SrtError, match=text):
            rig.view.light_hits(lights, rays, ids, t, out[:count], classes=cls[:len(lights)] if len(lights) <= 3 else None,
                                **kw)
    # misaligned rays and rgba (raw pointers: 4 bytes past a 16-byte boundary)
    L = _native.lib()
    amb = (ctypes.c_float * 3)(0.0, 0.0, 0.0)

    def call(r=rays.data_ptr(), i=ids.data_ptr(), tt=t.data_ptr(), o=out.data_ptr(), n=count, blend=None):
        return L.rthLightHitsAsync(rig.view.handle, None, 0, amb, r, i, tt, n, blend, o, None, None)

    assert call(r=long_rays.data_ptr() + 4) == -1 and "d_rays is not 16-byte aligned" in _native.last_error()
    assert call(o=out.data_ptr() + 4) == -1 and "d_rgba is not 16-byte aligned" in _native.last_error()
    for kw, text in (({"r": None}, "d_rays is NULL"), ({"i": None}, "d_ids is NULL"), ({"tt": None}, "d_t is NULL"),
                     ({"o": None}, "d_rgba is NULL"), ({"n": 2 ** 31}, "at most 2147483647 elements per call")):
        assert call(**kw) == -1 and text in _native.last_error(), (kw, _native.last_error())
    bad = _native.RthBlend(8, out.data_ptr(), (1.0, 1.0, 1.0))
    assert call(blend=ctypes.byref(bad)) == -1
    assert f"rth_blend.struct_size is 8, expected {ctypes.sizeof(_native.RthBlend)}" in _native.last_error()
    assert call(r=None, i=None, tt=None, o=None, n=0) == 0  # no elements: nothing is enqueued
    # the wrapper's buffer checks
    with pytest.raises(ValueError):
        rig.view.light_hits(rig.lights, rays, ids[:5], t, out[:count])
    with pytest.raises(ValueError):
        rig.view.light_hits(rig.lights, rays, ids, t, out[:count], classes=cls[:2])
    with pytest.raises(ValueError):
        rig.view.light_hits(rig.lights, rays, ids.to(torch.float32), t, out[:count])
    with pytest.raises(TypeError):
        rig.view.light_hits([spot_in.scene], rays, ids, t, out[:count])
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == f32(SENTINEL)).all() and (cls.cpu().numpy() == 9).all()  # every refused call wrote nothing
    for o in (fresh, fresh_omni, other, big):
        o.close()
    # the valid call still works after the refused ones
    rig.view.light_hits(rig.lights, rays, ids, t, out[:count], ambient=lc.AMBIENT, classes=cls, stream=rig.stream)
    torch.cuda.synchronize()
    got, got_classes = out.cpu().numpy(), cls.cpu().numpy()
    rig.close()
    want = hc.expected_bounce("roomA")
    hc.assert_same_classes(got_classes, want.classes)
    lc.same_bits("rgba", got[:count], want.rgba)
    assert (got[count] == f32(SENTINEL)).all()
