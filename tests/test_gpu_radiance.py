"""Sampled radiance on the device (include/srt_radiance.h rtiRadiance*Async; render.hip
RadianceKernel): one bounce of indirect light in one launch.

Every comparison is exact: against rtiRadianceHost, against the device composition
generate_rays_frame -> closest -> light_hits -> a float32 sum in ascending sample order, and between
the tree and SRT_RAYS=brute (tests/radiance_cases.py). Every test fails without the feature: the
entry points are missing.
"""
from __future__ import annotations

import ctypes
import os
import re
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import lighting_cases as lc
import omni_cases as oc
import radiance_cases as rd
import shadow_cases as sc
import visibility_cases as vc

pytestmark = pytest.mark.gpu

f32 = np.float32
SENTINEL = 7.25  # what an output buffer holds where nothing may be written
REPO = Path(__file__).resolve().parent.parent


def default_env(monkeypatch):
    for name in ("SRT_SETUP", "SRT_CULL_BIN", "SRT_CULL_BIN_CAP", "SRT_TRACE_RECORDS", "SRT_RAYS"):
        monkeypatch.delenv(name, raising=False)


class Rig:
    """A scene file prepared at w x h on cuda:0 and light specs (lighting_cases' spot / point) as
    prepared lights over the same file; the calls return numpy arrays."""

    def __init__(self, path, w, h, lights, prepare=True):
        import torch

        import simpleraytracer_amd as srt

        self.torch, self.srt, self.path, self.w, self.h = torch, srt, path, w, h
        self.stream = torch.cuda.current_stream()
        self.view = srt.DeviceScene(path, 0)
        if prepare:
            self.view.prepare(w, h, self.stream)
        self.owned = []
        self.lights = [self.make(l) for l in lights]

    def make(self, l, path=None):
        srt = self.srt
        path = self.path if path is None else path
        if l.kind == "point":
            light = srt.OmniLight(path, 0, l.origin)
            light.prepare(l.face_size, self.stream)
            self.owned.append(light)
            return srt.PointLight(light, l.color, l.falloff, l.bias)
        scene = srt.DeviceScene(path, 0, camera=l.cam)
        scene.prepare(l.wl, l.hl, self.stream)
        self.owned.append(scene)
        return srt.SpotLight(scene, l.color, l.falloff, l.bias)

    def up(self, a, dtype=None):
        t = self.torch.from_numpy(np.array(a, dtype=dtype)).cuda()
        self.torch.cuda.synchronize()
        return t

    def out(self, lead, base=None, extra=3):
        """A buffer of `lead` + (4,) behind which `extra` elements must keep the sentinel; with a base
        (numpy) the buffer holds it: the in-place form."""
        torch = self.torch
        count = int(np.prod(lead))
        flat = torch.full((count + extra, 4), SENTINEL, dtype=torch.float32, device="cuda")
        if base is not None:
            flat[:count] = torch.from_numpy(np.array(base, f32).reshape(count, 4)).cuda()
        torch.cuda.synchronize()
        return flat, flat[:count].view(*lead, 4)

    def done(self, flat, count):
        self.torch.cuda.synchronize()
        assert (flat[count:].cpu().numpy() == f32(SENTINEL)).all(), "the call wrote behind its last element"
        return flat[:count].cpu().numpy()

    def frame(self, off, ids, gen, row_begin=0, rows=None, lights=None, ambient=rd.AMBIENT, modulate=False, base=None,
              weight=(1.0, 1.0, 1.0), in_place=False):
        """radiance_frame of the band; off (rows, W, 2) and ids (rows W,) or (rows, W) numpy, band-local."""
        rows = self.h - row_begin if rows is None else rows
        lights = self.lights if lights is None else lights
        d_off, d_ids = self.up(np.asarray(off, f32).reshape(rows, self.w, 2)), self.up(np.asarray(ids).reshape(rows, self.w), np.int32)
        flat, rgba = self.out((rows, self.w), base if in_place else None)
        d_base = rgba if in_place else (self.up(np.asarray(base, f32).reshape(rows, self.w, 4)) if base is not None else None)
        self.view.radiance_frame(lights, d_off, d_ids, vc.to_device(gen), rgba, ambient=ambient, modulate=modulate,
                                 base=d_base, weight=weight, row_begin=row_begin, row_count=rows, stream=self.stream)
        return self.done(flat, rows * self.w)

    def points(self, pos, ids, gen, lights=None, ambient=rd.AMBIENT, **store):
        lights = self.lights if lights is None else lights
        count = len(ids)
        d_pos, d_ids = self.up(pos, f32), self.up(ids, np.int32)
        flat, rgba = self.out((count,), extra=40)
        self.view.radiance(lights, d_pos, d_ids, vc.to_device(gen), rgba, ambient=ambient, stream=self.stream, **store)
        return self.done(flat, count)

    def composition(self, off, ids, gen, lights=None, ambient=rd.AMBIENT):
        """The calls the fused one replaces, whole frame: the (S, count, 4) colours and the element's
        `on` from the exported rays."""
        torch = self.torch
        lights = self.lights if lights is None else lights
        S, count = gen.count, self.w * self.h
        d_off, d_ids = self.up(np.asarray(off, f32).reshape(self.h, self.w, 2)), self.up(np.asarray(ids).reshape(self.h, self.w), np.int32)
        rays = torch.empty((S, self.h, self.w, 8), dtype=torch.float32, device="cuda")
        hid = torch.empty(S * count, dtype=torch.int32, device="cuda")
        t = torch.empty(S * count, dtype=torch.float32, device="cuda")
        c = torch.empty((S * count, 4), dtype=torch.float32, device="cuda")
        self.view.generate_rays_frame(d_off, d_ids, vc.to_device(gen), rays, stream=self.stream)
        self.view.closest(rays.view(-1, 8), hid, t, stream=self.stream)
        self.view.light_hits(lights, rays.view(-1, 8), hid, t, c, ambient=ambient, stream=self.stream)
        torch.cuda.synchronize()
        c, rays = c.cpu().view(S, count, 4), rays.cpu().view(S, count, 8)
        total = torch.zeros((count, 3), dtype=torch.float32)
        for s in range(S):
            total = total + c[s, :, :3]
            assert total.dtype == torch.float32
        hits = (c[..., 3] >= 0).sum(dim=0).to(torch.float32)
        on = (rays[0] != 0).any(dim=1)
        out = torch.zeros((count, 4), dtype=torch.float32)
        out[on, :3] = (total / torch.tensor(S, dtype=torch.float32))[on]
        out[on, 3] = (hits / torch.tensor(S, dtype=torch.float32))[on]
        return out.numpy()

    def stats(self, capfd):
        lines = re.findall(r"srt rays: scene \S+ builds (\d+) allocations (\d+)", capfd.readouterr().err)
        assert lines, "no ray counters on stderr: is SRT_SETUP_LOG honoured?"
        return tuple(int(v) for v in lines[-1])

    def close(self):
        for o in self.owned:
            o.close()
        self.view.close()


def rig_of(c, lights=None, **kw):
    return Rig(c.path, c.w, c.h, c.lights if lights is None else lights, **kw)


CORNELL7 = ("cornell", 70, 33, 7, True, 4.0)  # 70 x 33: no multiple of the wave, the block or the 8-wide tile


def test_main_case_equals_the_host_and_the_composition(gpu, monkeypatch):
    default_env(monkeypatch)
    c = rd.main_case()
    want = rd.host_frame("frame", *rd.MAIN)
    rig = rig_of(c)
    got = rig.frame(c.offsets, c.ids, c.gen)
    again = rig.frame(c.offsets, c.ids, c.gen)
    composed = rig.composition(c.offsets, c.ids, c.gen)
    rig.close()
    rd.same_bits("the frame call", got, want)
    rd.same_bits("a second call", again, got)
    rd.same_bits("the device composition", composed, got)
    assert (got[:, 3] == 1).sum() >= 32 and ((got[:, 3] > 0) & (got[:, 3] < 1)).sum() >= 32


def test_odd_frame_two_bands_and_the_composition(gpu, monkeypatch):
    """70 x 33 with rotations; the bands [0, 5) and [5, 33): row_begin = 5 is no multiple of 4, so the
    rotation index must come from the absolute row."""
    default_env(monkeypatch)
    c = rd.small_case(*CORNELL7)
    want = rd.host_frame("small", *CORNELL7)
    rig = rig_of(c)
    whole = rig.frame(c.offsets, c.ids, c.gen)
    w = c.w
    top = rig.frame(c.offsets[0:5], c.ids[:5 * w], c.gen, row_begin=0, rows=5)
    rest = rig.frame(c.offsets[5:], c.ids[5 * w:], c.gen, row_begin=5, rows=c.h - 5)
    composed = rig.composition(c.offsets, c.ids, c.gen)
    rig.close()
    rd.same_bits("the whole frame", whole, want)
    rd.same_bits("rows [0, 5)", top, want[:5 * w])
    rd.same_bits("rows [5, 33)", rest, want[5 * w:])
    rd.same_bits("the device composition", composed, whole)
    wrong = rd.host(c.path, c.w, c.h, c.lights, rd.AMBIENT, c.pos[5 * w:], c.ids[5 * w:], c.gen, vc.frame_turns(w, c.h - 5))
    assert not np.array_equal(wrong, want[5 * w:]), "band-local rotation indices give the same answer: the case is blind"


@pytest.mark.parametrize("samples,rot", [(1, False), (3, True), (64, False)])
def test_sample_counts(gpu, monkeypatch, samples, rot):
    """S = 1; S = 3: a last round that is not full; S = 64: more rounds than slots per round."""
    default_env(monkeypatch)
    args = ("cornell", 48, 32, samples, rot, 4.0)
    c = rd.small_case(*args)
    rig = rig_of(c)
    got = rig.frame(c.offsets, c.ids, c.gen)
    mod = rig.frame(c.offsets, c.ids, c.gen, modulate=True)
    rig.close()
    rd.same_bits(f"S = {samples}", got, rd.host_frame("small", *args))
    rd.same_bits(f"S = {samples}, modulate", mod, rd.host(c.path, c.w, c.h, c.lights, rd.AMBIENT, c.pos, c.ids, c.gen, c.turns,
                                                         modulate=True))


def test_points_calls_at_the_block_boundaries(gpu, monkeypatch):
    default_env(monkeypatch)
    c = rd.small_case("cornell", 48, 32, 4, True, 4.0)
    rig = rig_of(c)
    start = 300
    got = {n: rig.points(c.pos[start:start + n], c.ids[start:start + n], c.gen) for n in (1, 255, 256, 257)}
    rig.close()
    for n, rgba in got.items():
        sel = slice(start, start + n)
        rd.same_bits(f"{n} elements", rgba, rd.host(c.path, c.w, c.h, c.lights, rd.AMBIENT, c.pos[sel], c.ids[sel], c.gen))
    assert (got[257][:, 3] > 0).sum() > 100


def test_brute_force_in_a_fresh_process_equals_the_tree(gpu, monkeypatch, tmp_path):
    default_env(monkeypatch)
    args = ("cornell", 48, 32, 4, True, 4.0)
    c = rd.small_case(*args)
    rig = rig_of(c)
    tree = rig.frame(c.offsets, c.ids, c.gen, modulate=True)
    rig.close()
    out = tmp_path / "brute.npy"
    code = ("import sys, numpy as np\n"
            f"sys.path[:0] = [{str(REPO)!r}, {str(REPO / 'tests')!r}]\n"
            "import radiance_cases as rd, test_gpu_radiance as tg\n"
            f"c = rd.small_case(*{args!r})\n"
            "rig = tg.rig_of(c)\n"
            f"np.save({str(out)!r}, rig.frame(c.offsets, c.ids, c.gen, modulate=True))\n"
            "rig.close()\n")
    env = dict(os.environ, SRT_RAYS="brute")
    done = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert done.returncode == 0, done.stderr[-2000:]
    rd.same_bits("SRT_RAYS=brute", np.load(out), tree)
    rd.same_bits("the host", tree, rd.host(c.path, c.w, c.h, c.lights, rd.AMBIENT, c.pos, c.ids, c.gen, c.turns, modulate=True))


def test_blocks_without_and_with_one_surface_element(gpu, monkeypatch):
    """A band of sky: no block has an element on a surface, nothing is walked, zeros (or the base) are
    stored. A points call of 256 elements of which exactly one is on a surface."""
    default_env(monkeypatch)
    c = rd.main_case()
    w = c.w
    ids2 = c.ids.reshape(c.h, w)
    sky = np.flatnonzero((ids2 < 0).all(axis=1))
    assert sky.size >= 3 and (np.diff(sky[:3]) == 1).all(), "the main case has no band of sky"
    r0 = int(sky[0])
    rig = rig_of(c)
    zeros = rig.frame(c.offsets[r0:r0 + 3], ids2[r0:r0 + 3], c.gen, row_begin=r0, rows=3)
    base = rd.base_of(3 * w)
    kept = rig.frame(c.offsets[r0:r0 + 3], ids2[r0:r0 + 3], c.gen, row_begin=r0, rows=3, base=base, weight=(2.0, 2.0, 2.0))
    want = rd.host_frame("frame", *rd.MAIN)
    one = int(np.flatnonzero(want[:, 3] > 0)[7])
    pos = np.array(c.pos[:256])
    ids = np.full(256, -1, np.int32)
    pos[100], ids[100] = c.pos[one], c.ids[one]
    single = rig.points(pos, ids, c.gen)
    rig.close()
    assert (zeros.view(np.uint32) == 0).all()
    rd.same_bits("a band of sky keeps the base", kept, base)
    rd.same_bits("one surface element", single[100], want[one])
    assert (np.delete(single, 100, axis=0).view(np.uint32) == 0).all()


@pytest.mark.parametrize("n", [8, 9, 64, 65, 512, 513])
def test_triangle_counts_where_the_tree_gains_a_level(gpu, monkeypatch, n):
    default_env(monkeypatch)
    c = rd.count_case(n)
    want = rd.host(c.path, c.w, c.h, c.lights, rd.AMBIENT, c.pos, c.ids, c.gen)
    rig = rig_of(c)
    got = rig.points(c.pos, c.ids, c.gen)
    rig.close()
    rd.same_bits(f"n = {n}", got, want)
    print(f"n = {n}: {c.hitting} of 28 surface elements have a ray that hits")
    assert (want[:c.hitting, 3] > 0).all() and (want[28:30] == 0).all()
    assert c.hitting >= 1 or n < 64, "no ray of the case hits a triangle: the walk is not exercised"


def test_light_counts(gpu, monkeypatch):
    """No light, one spot light, one point light (six frames) and the 16 frames of `full`."""
    default_env(monkeypatch)
    c = rd.frame_case("full", 2, True)
    point, spot = c.lights[0], c.lights[1]
    rig = rig_of(c)
    by_spec = dict(zip(map(id, c.lights), rig.lights))
    got = {}
    for what, specs in (("none", []), ("a spot", [spot]), ("a point", [point]), ("sixteen frames", c.lights)):
        ambient = (0.5, 0.25, 1.0) if what == "none" else rd.AMBIENT
        got[what] = (specs, ambient, rig.frame(c.offsets, c.ids, c.gen, lights=[by_spec[id(s)] for s in specs], ambient=ambient))
    rig.close()
    for what, (specs, ambient, rgba) in got.items():
        rd.same_bits(what, rgba, rd.host(c.path, c.w, c.h, specs, ambient, c.pos, c.ids, c.gen, c.turns))
    assert not np.array_equal(got["a spot"][2], got["a point"][2])


def test_moved_camera_and_triangles(gpu, monkeypatch):
    """After set_camera and after set_vertices (the ray tree is rebuilt) the answer is a fresh scene's
    at the new pose: the traced ids and the radiance of the whole frame."""
    import torch

    default_env(monkeypatch)
    a, b = lc.case("roomA"), lc.case("roomB")
    gen = vc.hemisphere(4, rd.INF, True)
    off = np.array(a.offsets)

    def picture(rig):
        d_off = rig.up(off)
        ids = torch.empty((lc.H, lc.W), dtype=torch.int32, device="cuda")
        rig.view.trace_ids(d_off, ids, stream=rig.stream)
        torch.cuda.synchronize()
        host_ids = ids.cpu().numpy()
        return host_ids, rig.frame(off, host_ids, gen, modulate=True)

    rig = Rig(a.view, lc.W, lc.H, a.lights)
    ids0, before = picture(rig)
    rig.view.set_camera(oc.VIEWS["B"], stream=rig.stream)
    ids1, moved = picture(rig)
    shape = np.shape(oc.room_vertices())
    v = np.array(oc.room_vertices(), f32).reshape(-1, 3, 3)
    v[..., 0] = v[..., 0] + f32(0.125) * v[..., 1]
    path = sc.write_with_camera(sc._dir() / "radiance_sheared.srt", v.reshape(shape), oc.VIEWS["B"])
    dv = rig.up(np.ascontiguousarray(v.reshape(-1, 9)))
    for scene in [rig.view] + rig.owned:
        scene.set_vertices(dv, stream=rig.stream)
    ids2, sheared = picture(rig)
    rig.close()
    fresh = Rig(b.view, lc.W, lc.H, a.lights)
    fids1, want_moved = picture(fresh)
    fresh.close()
    fresh = Rig(path, lc.W, lc.H, a.lights)
    fids2, want_sheared = picture(fresh)
    fresh.close()
    assert np.array_equal(ids1, fids1) and np.array_equal(ids2, fids2) and not np.array_equal(ids0, ids1)
    rd.same_bits("after set_camera", moved, want_moved)
    rd.same_bits("after set_vertices", sheared, want_sheared)
    assert not np.array_equal(moved, before) and not np.array_equal(sheared, moved)


def test_blend_in_place_equals_out_of_place(gpu, monkeypatch):
    default_env(monkeypatch)
    c = rd.main_case()
    base = rd.base_of(len(c.ids))
    weight = (0.5, 0.25, 2.0)
    rig = rig_of(c)
    apart = rig.frame(c.offsets, c.ids, c.gen, modulate=True, base=base, weight=weight)
    within = rig.frame(c.offsets, c.ids, c.gen, modulate=True, base=base, weight=weight, in_place=True)
    rig.close()
    rd.same_bits("in place", within, apart)
    rd.same_bits("the host", apart, rd.host(c.path, c.w, c.h, c.lights, rd.AMBIENT, c.pos, c.ids, c.gen, c.turns, modulate=True,
                                            base=base, weight=weight))


def test_render_indirect_and_the_mirror_as_render_reflection(gpu, monkeypatch):
    """render_indirect is trace_ids, light and radiance_frame(modulate, in place) by hand;
    radiance_frame(Mirror(), base, weight) gives render_reflection's bits."""
    import torch

    default_env(monkeypatch)
    c = rd.frame_case("roomA", 4, True)
    weight = (0.5, 0.4, 0.3)
    rig = rig_of(c)
    d_off = rig.up(np.array(c.offsets))
    gen = vc.to_device(c.gen)

    def buffers():
        return (torch.full((c.h, c.w), -7, dtype=torch.int32, device="cuda"),
                torch.full((c.h, c.w, 4), SENTINEL, dtype=torch.float32, device="cuda"))

    ids_a, rgba_a = buffers()
    rig.view.render_indirect(rig.lights, d_off, ids_a, rgba_a, gen, ambient=rd.AMBIENT, weight=weight, stream=rig.stream)
    ids_b, rgba_b = buffers()
    rig.view.trace_ids(d_off, ids_b, stream=rig.stream)
    rig.view.light(rig.lights, d_off, ids_b, rgba_b, ambient=rd.AMBIENT, stream=rig.stream)
    torch.cuda.synchronize()
    lit = rgba_b.cpu().numpy()
    rig.view.radiance_frame(rig.lights, d_off, ids_b, gen, rgba_b, ambient=rd.AMBIENT, modulate=True, base=rgba_b,
                            weight=weight, stream=rig.stream)
    ids_c, rgba_c = buffers()
    scratch = rig.view.render_reflection(rig.lights, d_off, ids_c, rgba_c, weight, ambient=rd.AMBIENT, stream=rig.stream)
    ids_d, rgba_d = buffers()
    rig.view.trace_ids(d_off, ids_d, stream=rig.stream)
    rig.view.light(rig.lights, d_off, ids_d, rgba_d, ambient=rd.AMBIENT, stream=rig.stream)
    rig.view.radiance_frame(rig.lights, d_off, ids_d, rig.srt.Mirror(), rgba_d, ambient=rd.AMBIENT, base=rgba_d, weight=weight,
                            stream=rig.stream)
    torch.cuda.synchronize()
    del scratch
    rig.close()
    assert np.array_equal(ids_a.cpu().numpy(), ids_b.cpu().numpy())
    rd.same_bits("render_indirect", rgba_a.cpu().numpy(), rgba_b.cpu().numpy())
    rd.same_bits("the mirror", rgba_d.cpu().numpy(), rgba_c.cpu().numpy())
    want = rd.host(c.path, c.w, c.h, c.lights, rd.AMBIENT, c.pos, ids_b.cpu().numpy().reshape(-1), c.gen, c.turns, modulate=True,
                   base=lit.reshape(-1, 4), weight=weight)
    rd.same_bits("render_indirect against the host", rgba_a.cpu().numpy(), want)
    assert not np.array_equal(rgba_a.cpu().numpy(), lit)


def test_a_second_call_allocates_nothing(gpu, monkeypatch, capfd):
    import torch

    default_env(monkeypatch)
    monkeypatch.setenv("SRT_SETUP_LOG", "1")
    c = rd.small_case("cornell", 48, 32, 4, True, 4.0)
    rig = rig_of(c)
    d_off, d_ids = rig.up(np.array(c.offsets)), rig.up(c.ids.reshape(c.h, c.w), np.int32)
    gen = vc.to_device(c.gen)
    out = [torch.full((c.h, c.w, 4), SENTINEL, dtype=torch.float32, device="cuda") for _ in range(2)]
    rig.view.radiance_frame(rig.lights, d_off, d_ids, gen, out[0], ambient=rd.AMBIENT, stream=rig.stream)
    torch.cuda.synchronize()
    first = rig.stats(capfd)
    held = torch.cuda.memory_allocated()
    free0 = torch.cuda.mem_get_info()[0]
    rig.view.radiance_frame(rig.lights, d_off, d_ids, gen, out[1], ambient=rd.AMBIENT, stream=rig.stream)
    torch.cuda.synchronize()
    assert torch.cuda.memory_allocated() == held
    assert torch.cuda.mem_get_info()[0] >= free0, "the second call took device memory"
    assert rig.stats(capfd) == first == (1, 1), "one build and one allocation of the ray tree, in the first call"
    rig.close()
    rd.same_bits("a second call", out[1].cpu().numpy(), out[0].cpu().numpy())


def test_refusals_leave_the_output_untouched(gpu, monkeypatch):
    import torch

    from simpleraytracer_amd import SrtError, _native, device, lighting

    default_env(monkeypatch)
    c = rd.small_case("cornell", 48, 32, 4, True, 4.0)
    rig = rig_of(c)
    d_off, d_ids = rig.up(np.array(c.offsets)), rig.up(c.ids.reshape(c.h, c.w), np.int32)
    rgba = torch.full((c.h, c.w, 4), SENTINEL, dtype=torch.float32, device="cuda")
    base = torch.zeros((c.h, c.w, 4), dtype=torch.float32, device="cuda")
    gen = vc.to_device(c.gen)
    nan = float("nan")
    other = rig.srt.DeviceScene(vc.scene_path("q"), 0, camera=rd.CORNELL_LIGHTS[0].cam)
    other.prepare(64, 48, rig.stream)
    unprepared = rig.srt.DeviceScene(c.path, 0)

    def call(view=rig.view, lights=rig.lights, g=gen, **kw):
        view.radiance_frame(lights, d_off, d_ids, g, rgba, ambient=rd.AMBIENT, stream=rig.stream, **kw)

    def hemi(count):
        return device.Hemisphere(torch.zeros((count, 3), dtype=torch.float32, device="cuda"), vc.TMIN, 1.0)

    for kw, text in (
            ({"g": vc.to_device(vc.area_light(4))}, "rta_generator.kind is RTA_AREA"),
            ({"g": hemi(0)}, "rta_generator.samples must be 1 to 64, got 0"),
            ({"g": hemi(65)}, "rta_generator.samples must be 1 to 64, got 65"),
            ({"base": base, "weight": (1.0, 1.0, nan)}, "weight value 2 is not finite"),
            ({"lights": rig.lights + [rig.srt.SpotLight(other)]}, "light 2: the view scene has")):
        with pytest.raises(SrtError, match=re.escape(text)):
            call(**kw)
    # what the wrapper cannot express: through the C entry point
    L = _native.lib()
    arr, n_lights = lighting.pack_device(rig.lights)
    g = rig.view._generator(gen)
    mirror2 = _native.RtaGenerator(ctypes.sizeof(_native.RtaGenerator), _native.RTA_MIRROR, 2, None, None, (0, 0, 0), (0, 0, 0),
                                   (0, 0, 0), vc.TMIN, 1.0)
    blend8 = _native.RthBlend(8, base.data_ptr(), (1.0, 1.0, 1.0))

    def raw(gen_struct=g, options=None, view=rig.view):
        return L.rtiRadianceFrameAsync(view.handle, ctypes.addressof(arr), n_lights, lighting.ambient3(rd.AMBIENT),
                                       d_off.data_ptr(), d_ids.data_ptr(), 0, c.h, ctypes.byref(gen_struct),
                                       ctypes.byref(options) if options is not None else None, rgba.data_ptr(),
                                       rig.stream.cuda_stream)

    size = ctypes.sizeof(_native.RtiOptions)
    for kw, text in (
            ({"gen_struct": mirror2}, "rta_generator.samples must be 1 for RTA_MIRROR, got 2"),
            ({"view": unprepared}, "Radiance: Prepare() has not been called"),
            ({"options": _native.RtiOptions(8, 0, None)}, f"rti_options.struct_size is 8, expected {size}"),
            ({"options": _native.RtiOptions(size, 0, ctypes.pointer(blend8))}, "rth_blend.struct_size is 8, expected")):
        assert raw(**kw) == -1, kw
        assert text in _native.last_error(), (kw, _native.last_error())
    torch.cuda.synchronize()
    assert (rgba.cpu().numpy() == f32(SENTINEL)).all(), "a refused call wrote its output"
    # zero rows enqueue nothing and read nothing
    rig.view.radiance_frame(rig.lights, d_off[:0], d_ids[:0], gen, rgba[:0], row_begin=3, row_count=0, stream=rig.stream)
    torch.cuda.synchronize()
    assert (rgba.cpu().numpy() == f32(SENTINEL)).all()
    assert raw() == 0, _native.last_error()
    torch.cuda.synchronize()
    rd.same_bits("after the refusals", rgba.cpu().numpy().reshape(-1, 4), rd.host_frame("small", "cornell", 48, 32, 4, True, 4.0))
    other.close()
    unprepared.close()
    rig.close()
