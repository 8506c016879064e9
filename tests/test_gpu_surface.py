"""Vertex attributes on the device (include/srt_surface.h rtvSurfaceFrameAsync / rtvSurfacePointsAsync /
rtvInterpolate*Async; outputs.hip SurfaceKernel, InterpolateKernel): smooth normals, UVs, textured
albedo and the shaded pixel from hit ids and the caller's corner tables.

Expected values come from the oracle and numpy (tests/surface_cases.py: the float32 restatement),
never from the library; every comparison is on the uint32 view. The host path (rtvSurfaceHost) must
give the same bits, and without normals and texture the planes are the G-buffer's and the traced
RGBA frame's.

Frames are 200 x 150 unless a test says otherwise; scene Q and the position families are
tests/query_cases.py's.
"""
from __future__ import annotations

import re

import numpy as np
import pytest

import gbuffer_cases as gc
import query_cases as qc
import surface_cases as sv

pytestmark = pytest.mark.gpu

W, H = qc.W, qc.H
W2, H2 = 333, 170
PAD = 64             # elements past every output plane
SENTINEL = -77777.0  # no plane takes this value: |n| <= 1, uv and albedo small, alpha >= -1
PLANES = (("normal", (4,)), ("albedo", (4,)), ("rgba", (4,)), ("uv", (2,)))
ALL = tuple(name for name, _ in PLANES)
TABLE_SEED = 27


@pytest.fixture(scope="module")
def scene_q(tmp_path_factory):
    return qc.write_scene_q(tmp_path_factory.mktemp("surface") / "q.srt")


class Rig:
    """One scene on cuda:0 and its stream. surface_frame() / surface() / interpolate*() allocate
    every plane asked for PAD elements longer, prefilled with SENTINEL, check that the tail is
    untouched and the body fully written, and return the bodies as numpy arrays."""

    def __init__(self, path, w=None, h=None, camera=None):
        import torch

        import simpleraytracer_amd as srt

        self.torch = torch
        self.srt = srt
        self.scene = srt.DeviceScene(path, 0, camera=camera)
        self.stream = torch.cuda.current_stream()
        if w is not None:
            self.prepare(w, h)

    def prepare(self, w, h):
        self.w, self.h = w, h
        self.scene.prepare(w, h, self.stream)

    def dev(self, a, dtype=np.float32):
        return self.torch.from_numpy(np.array(a, dtype)).cuda()  # (a copy: the shared cases are read-only)

    def surface_of(self, normals=None, uvs=None, tex=None, **kw):
        """A Surface of device copies of numpy tables."""
        up = lambda a: None if a is None else self.dev(a)  # noqa: E731
        return self.srt.Surface(up(normals), up(uvs), up(tex), **kw)

    def trace(self, offsets, ids=False):
        torch = self.torch
        off = self.dev(offsets)
        if ids:
            out = torch.full((self.h, self.w), -7, dtype=torch.int32, device="cuda")
            self.scene.trace_ids(off, out, stream=self.stream)
        else:
            out = torch.full((self.h, self.w, 4), float("nan"), dtype=torch.float32, device="cuda")
            self.scene.trace(off, out, stream=self.stream)
        torch.cuda.synchronize()
        return out.cpu().numpy()

    def query(self, pos):
        torch = self.torch
        ids = torch.full((len(pos),), -7, dtype=torch.int32, device="cuda")
        t = torch.full((len(pos),), float("nan"), dtype=torch.float32, device="cuda")
        self.scene.query(self.dev(pos), ids, t, stream=self.stream)
        torch.cuda.synchronize()
        return ids.cpu().numpy()

    def _planes(self, lead, which, planes=PLANES):
        torch = self.torch
        count = int(np.prod(lead))
        raw, views = {}, {}
        for name, tail in planes:
            if name in which:
                ch = int(np.prod(tail))
                raw[name] = torch.full(((count + PAD) * ch,), SENTINEL, dtype=torch.float32, device="cuda")
                views[name] = raw[name][:count * ch].view(lead + tail)
        return raw, views

    def _collect(self, raw, views):
        self.torch.cuda.synchronize()
        out = {}
        for name, v in views.items():
            body = v.cpu().numpy()
            tail = raw[name][body.size:].cpu().numpy()
            assert tail.size >= PAD and np.all(tail == np.float32(SENTINEL)), f"{name}: written past its end"
            assert not np.any(body == np.float32(SENTINEL)), f"{name}: not fully written"
            out[name] = body
        return out

    def surface_frame(self, offsets, ids, surface, r0=0, rows=None, which=ALL, stream=None):
        rows = self.h - r0 if rows is None else rows
        off, idv = self.dev(offsets[r0:r0 + rows]), self.dev(ids[r0:r0 + rows], np.int32)
        raw, views = self._planes((rows, self.w), which)
        self.torch.cuda.synchronize()
        self.scene.surface_frame(off, idv, surface, row_begin=r0, row_count=rows,
                                 stream=self.stream if stream is None else stream, **views)
        return self._collect(raw, views)

    def surface(self, pos, ids, surface, which=ALL):
        raw, views = self._planes((len(pos),), which)
        p, i = self.dev(pos), self.dev(ids, np.int32)
        self.torch.cuda.synchronize()
        self.scene.surface(p, i, surface, stream=self.stream, **views)
        return self._collect(raw, views)

    def interpolate_frame(self, offsets, ids, table, r0=0, rows=None):
        rows = self.h - r0 if rows is None else rows
        off, idv = self.dev(offsets[r0:r0 + rows]), self.dev(ids[r0:r0 + rows], np.int32)
        raw, views = self._planes((rows, self.w), ("out",), (("out", (table.shape[2],)),))
        self.torch.cuda.synchronize()
        self.scene.interpolate_frame(off, idv, self.dev(table), views["out"], row_begin=r0, row_count=rows,
                                     stream=self.stream)
        return self._collect(raw, views)["out"]

    def interpolate(self, pos, ids, table):
        raw, views = self._planes((len(pos),), ("out",), (("out", (table.shape[2],)),))
        p, i = self.dev(pos), self.dev(ids, np.int32)
        self.torch.cuda.synchronize()
        self.scene.interpolate(p, i, self.dev(table), views["out"], stream=self.stream)
        return self._collect(raw, views)["out"]

    def stats(self, capfd):
        lines = re.findall(r"srt setup: scene \S+ builds (\d+) shared_frames (\d+) per_frame_frames (\d+)",
                           capfd.readouterr().err)
        assert lines, "no setup counters on stderr: is SRT_SETUP_LOG honoured?"
        return tuple(int(v) for v in lines[-1])

    def close(self):
        self.scene.close()


def default_env(monkeypatch):
    for name in ("SRT_SETUP", "SRT_CULL_BIN", "SRT_CULL_BIN_CAP", "SRT_TRACE_RECORDS", "SRT_SETUP_LOG"):
        monkeypatch.delenv(name, raising=False)


def same(a, b):
    """Every plane of two results bit-equal."""
    assert a.keys() == b.keys()
    for name in a:
        assert a[name].shape == b[name].shape, name
        assert np.array_equal(a[name].view(np.uint32), b[name].view(np.uint32)), f"{name} differs"


def host_planes(path, w, h, pos, ids, normals=None, uvs=None, tex=None, **kw):
    import simpleraytracer_amd.device as device

    got = device.surface_host(path, w, h, pos, ids, device.Surface(normals, uvs, tex, **kw))
    return dict(zip(ALL, got))


def flat(planes):
    return {k: v.reshape((-1, v.shape[-1])) for k, v in planes.items()}


@pytest.fixture(scope="module")
def frame_q(gpu, scene_q):
    """Scene Q's whole frame with random offsets (seed 3): the trace's ids and RGBA, the G-buffer's
    normal and albedo, the random tables and a 5 x 3 texture, and the surface planes under them
    (repeat, bilinear, modulate): computed once, read-only."""
    off = qc.random_offsets(W, H, 3)
    ev = sv.cached_edges(scene_q, W, H, "pixels")
    tb = sv.tables(ev.n, TABLE_SEED, ev.ids)
    tex = sv.texture(3, 5, 5)
    rig = Rig(scene_q, W, H)
    ids = rig.trace(off, ids=True)
    rgba = rig.trace(off)
    torch = rig.torch
    gn = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    ga = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    rig.scene.gbuffer(rig.dev(off), rig.dev(ids, np.int32), normal=gn, albedo=ga, stream=rig.stream)
    torch.cuda.synchronize()
    planes = rig.surface_frame(off, ids, rig.surface_of(tb.normals, tb.uvs, tex, modulate=True))
    rig.close()
    out = dict(off=off, ids=ids, rgba=rgba, g_normal=gn.cpu().numpy(), g_albedo=ga.cpu().numpy(), ev=ev, tb=tb, tex=tex,
               planes=planes)
    for a in (off, ids, rgba, out["g_normal"], out["g_albedo"], *planes.values()):
        a.setflags(write=False)
    return out


def test_whole_frame(scene_q, frame_q, monkeypatch):
    """Bit-equal to the restatement and to rtvSurfaceHost; every wrap / filter / modulate combination."""
    default_env(monkeypatch)
    f = frame_q
    ev, tb, tex = f["ev"], f["tb"], f["tex"]
    assert np.array_equal(f["ids"].reshape(-1), ev.ids)
    qc.assert_mix(ev.ids)
    g = flat(f["planes"])
    assert f["planes"]["normal"].shape == (H, W, 4) and f["planes"]["uv"].shape == (H, W, 2)
    sv.check_surface(sv.expected(ev, tb.normals, tb.uvs, tex, modulate=True), **g)
    same(g, host_planes(scene_q, W, H, ev.pos, ev.ids, tb.normals, tb.uvs, tex, modulate=True))
    rig = Rig(scene_q, W, H)
    for size in ((1, 1), (64, 64)):
        t2 = sv.texture(*size, seed=5)
        for wrap in sv.WRAPS:
            for filt in sv.FILTERS:
                got = flat(rig.surface_frame(f["off"], f["ids"], rig.surface_of(tb.normals, tb.uvs, t2, wrap=wrap, filter=filt)))
                sv.check_surface(sv.expected(ev, tb.normals, tb.uvs, t2, wrap, filt), **got)
    for c in (1, 2, 3, 4):
        table = np.ascontiguousarray(tb.generic[:, :, :c])
        got = rig.interpolate_frame(f["off"], f["ids"], table)
        assert got.shape == (H, W, c)
        sv.same_bits(f"interpolation, C = {c}", got.reshape(-1, c), sv.interpolate(ev, table))
    rig.close()


def test_band(scene_q, frame_q, monkeypatch):
    """Rows 40..117: not tile-aligned; band-local buffers; every plane the slice of the whole frame's."""
    default_env(monkeypatch)
    f = frame_q
    rig = Rig(scene_q, W, H)
    band = rig.surface_frame(f["off"], f["ids"], rig.surface_of(f["tb"].normals, f["tb"].uvs, f["tex"], modulate=True),
                             r0=40, rows=78)
    table = f["tb"].generic
    whole = rig.interpolate_frame(f["off"], f["ids"], table)
    part = rig.interpolate_frame(f["off"], f["ids"], table, r0=40, rows=78)
    rig.close()
    same(band, {k: v[40:118] for k, v in f["planes"].items()})
    assert np.array_equal(part.view(np.uint32), whole[40:118].view(np.uint32))


def test_points(scene_q, frame_q, monkeypatch):
    """The mixed positions with the query's ids against the restatement and the host; the frame's
    pixels as points give the frame's planes."""
    import simpleraytracer_amd.device as device

    default_env(monkeypatch)
    f = frame_q
    tb, tex = f["tb"], f["tex"]
    ev = sv.cached_edges(scene_q, W, H, "mixed")
    qc.assert_mix(ev.ids)
    rig = Rig(scene_q, W, H)
    q_ids = rig.query(ev.pos)
    s = rig.surface_of(tb.normals, tb.uvs, tex, modulate=True)
    a = rig.surface(ev.pos, q_ids, s)
    b = rig.surface(device.pixel_positions(W, H, f["off"]), f["ids"].reshape(-1), s)
    i = rig.interpolate(ev.pos, q_ids, tb.generic)
    rig.close()
    assert np.array_equal(q_ids, ev.ids)
    sv.check_surface(sv.expected(ev, tb.normals, tb.uvs, tex, modulate=True), **a)
    same(a, host_planes(scene_q, W, H, ev.pos, ev.ids, tb.normals, tb.uvs, tex, modulate=True))
    same(b, flat(f["planes"]))
    sv.same_bits("interpolation", i, sv.interpolate(ev, tb.generic))


@pytest.mark.parametrize("count", [1, 63, 65, 257])
def test_bounds_counts(scene_q, frame_q, monkeypatch, count):
    import simpleraytracer_amd.device as device

    default_env(monkeypatch)
    f = frame_q
    first = 75 * W + 60  # mid-frame: hits and misses among the first 257
    pixels = device.pixel_positions(W, H, f["off"])[first:first + count]
    sub = f["ids"].reshape(-1)[first:first + count]
    rig = Rig(scene_q, W, H)
    a = rig.surface(pixels, sub, rig.surface_of(f["tb"].normals, f["tb"].uvs, f["tex"], modulate=True))
    i = rig.interpolate(pixels, sub, f["tb"].generic)  # (the rig checks the padded tail and the body)
    rig.close()
    same(a, {k: v[first:first + count] for k, v in flat(f["planes"]).items()})
    sv.same_bits("interpolation", i, sv.interpolate(f["ev"], f["tb"].generic)[first:first + count])


@pytest.mark.parametrize("w,h", [(1, 1), (65, 17)])
def test_bounds_frames(scene_q, frame_q, monkeypatch, w, h):
    import simpleraytracer_amd.device as device

    default_env(monkeypatch)
    tb, tex = frame_q["tb"], frame_q["tex"]
    off = qc.random_offsets(w, h, 4)
    rig = Rig(scene_q, w, h)
    ids = rig.trace(off, ids=True)
    g = flat(rig.surface_frame(off, ids, rig.surface_of(tb.normals, tb.uvs, tex)))
    i = rig.interpolate_frame(off, ids, tb.generic)
    rig.close()
    assert w == 1 or ((ids >= 0).any() and (ids < 0).any())
    ev = sv.edge_values(scene_q, w, h, device.pixel_positions(w, h, off), ids.reshape(-1))
    sv.check_surface(sv.expected(ev, tb.normals, tb.uvs, tex), **g)
    sv.same_bits("interpolation", i.reshape(-1, 4), sv.interpolate(ev, tb.generic))


def test_optional_outputs(scene_q, frame_q, monkeypatch):
    """Each output plane alone gives the bits of all together; no plane at all succeeds."""
    default_env(monkeypatch)
    f = frame_q
    tb, tex = f["tb"], f["tex"]
    ev = sv.cached_edges(scene_q, W, H, "mixed")
    rig = Rig(scene_q, W, H)
    s = rig.surface_of(tb.normals, tb.uvs, tex, modulate=True)
    every = rig.surface(ev.pos, ev.ids, s)
    for name in ALL:
        same(rig.surface_frame(f["off"], f["ids"], s, which=(name,)), {name: f["planes"][name]})
        same(rig.surface(ev.pos, ev.ids, s, which=(name,)), {name: every[name]})
    assert rig.surface_frame(f["off"], f["ids"], s, which=()) == {} and rig.surface(ev.pos, ev.ids, s, which=()) == {}
    rig.close()


def test_optional_inputs(scene_q, frame_q, monkeypatch):
    """Each of normals, uvs and texture absent: rtg's normal and albedo planes, srtTraceAsync's RGBA
    of the same offsets, uv (0, 0); the planes that still have their input keep their bits."""
    default_env(monkeypatch)
    f = frame_q
    tb, tex, ev = f["tb"], f["tex"], f["ev"]
    full = f["planes"]
    rig = Rig(scene_q, W, H)
    bare = rig.surface_frame(f["off"], f["ids"], rig.surface_of())
    same(bare, {"normal": f["g_normal"], "albedo": f["g_albedo"], "rgba": f["rgba"],
                "uv": np.zeros((H, W, 2), np.float32)})
    for which in ALL:  # ... and each plane alone
        same(rig.surface_frame(f["off"], f["ids"], rig.surface_of(), which=(which,)), {which: bare[which]})
    no_normals = rig.surface_frame(f["off"], f["ids"], rig.surface_of(None, tb.uvs, tex, modulate=True))
    same({k: no_normals[k] for k in ("normal", "albedo", "uv")},
         {"normal": f["g_normal"], "albedo": full["albedo"], "uv": full["uv"]})
    sv.same_bits("rgba", no_normals["rgba"], gc.composed_rgba(f["g_normal"], full["albedo"]))
    no_texture = rig.surface_frame(f["off"], f["ids"], rig.surface_of(tb.normals, tb.uvs))
    same({k: no_texture[k] for k in ("normal", "albedo", "uv")},
         {"normal": full["normal"], "albedo": f["g_albedo"], "uv": full["uv"]})
    sv.same_bits("rgba", no_texture["rgba"], gc.composed_rgba(full["normal"], f["g_albedo"]))
    no_uvs = rig.surface_frame(f["off"], f["ids"], rig.surface_of(tb.normals))
    same(no_uvs, {**no_texture, "uv": np.zeros((H, W, 2), np.float32)})
    rig.close()
    same(flat(bare), host_planes(scene_q, W, H, ev.pos, ev.ids))


def test_invalid_ids(scene_q, frame_q, monkeypatch):
    """Ids outside the scene scattered among valid ones: the miss values, the neighbours unaffected;
    every table row of triangle 0 set to NaN changes nothing for them."""
    default_env(monkeypatch)
    f = frame_q
    tb, tex, ev = f["tb"], f["tex"], f["ev"]
    bad = gc.miss_ids(ev.n)
    mixed = f["ids"].copy()
    flat_ids = mixed.reshape(-1)
    at = np.random.default_rng(8).choice(flat_ids.size, 50, replace=False)
    flat_ids[at] = np.resize(bad, at.size)
    keep = np.ones(flat_ids.size, bool)
    keep[at] = False
    keep &= flat_ids != 0
    poisoned = [np.array(a) for a in (tb.normals, tb.uvs, tb.generic)]
    for a in poisoned:
        a[0] = np.nan
    rig = Rig(scene_q, W, H)
    results = [(rig.surface_frame(f["off"], mixed, rig.surface_of(n, u, tex, modulate=True)),
                rig.interpolate_frame(f["off"], mixed, g))
               for n, u, g in ((tb.normals, tb.uvs, tb.generic), poisoned)]
    rig.close()
    want_i = sv.interpolate(ev, tb.generic)
    for planes, interp in results:
        g = flat(planes)
        for name, want in zip(ALL, sv.miss_planes(at.size, ev.background)):
            sv.same_bits(f"miss {name}", g[name][at], want)
        sv.same_bits("miss interpolation", interp.reshape(-1, 4)[at], np.zeros((at.size, 4), np.float32))
        for name, want in flat(f["planes"]).items():
            assert np.array_equal(g[name][keep].view(np.uint32), want[keep].view(np.uint32)), name
        assert np.array_equal(interp.reshape(-1, 4)[keep].view(np.uint32), want_i[keep].view(np.uint32))


def test_no_setup(scene_q, frame_q, monkeypatch, capfd):
    """The surface calls build and read no cull setup: none after them on a fresh frame."""
    default_env(monkeypatch)
    monkeypatch.setenv("SRT_SETUP_LOG", "1")
    f = frame_q
    tb, tex = f["tb"], f["tex"]
    ev = sv.cached_edges(scene_q, W, H, "mixed")
    rig = Rig(scene_q, W, H)
    s = rig.surface_of(tb.normals, tb.uvs, tex, modulate=True)
    before = rig.surface(ev.pos, ev.ids, s)
    builds_surface = rig.stats(capfd)[0]
    rig.interpolate(ev.pos, ev.ids, tb.generic)
    builds_interpolate = rig.stats(capfd)[0]
    rig.trace(f["off"])
    builds_traced = rig.stats(capfd)[0]
    after = rig.surface(ev.pos, ev.ids, s)
    builds_after = rig.stats(capfd)[0]
    rig.close()
    assert (builds_surface, builds_interpolate, builds_traced, builds_after) == (0, 0, 1, 1)
    sv.check_surface(sv.expected(ev, tb.normals, tb.uvs, tex, modulate=True), **before)
    same(before, after)


def test_reprepare_on_a_second_stream(scene_q, frame_q, monkeypatch):
    """prepare(333, 170), a trace on the first stream, the surface call on a second right after, no
    host sync in between: the values follow the new frame."""
    import torch

    import simpleraytracer_amd.device as device

    default_env(monkeypatch)
    f = frame_q
    tb, tex = f["tb"], f["tex"]
    off2 = qc.random_offsets(W2, H2, 6)
    pixels = device.pixel_positions(W2, H2, off2)
    want_ids, _ = device.query_host(scene_q, W2, H2, pixels)
    sel = np.random.default_rng(1).choice(W2 * H2, 3000, replace=False)  # the oracle's share of the frame
    ev = sv.edge_values(scene_q, W2, H2, pixels[sel], want_ids[sel])
    rig = Rig(scene_q, W, H)
    s = rig.surface_of(tb.normals, tb.uvs, tex, modulate=True)
    rig.surface_frame(f["off"], f["ids"], s)
    rig.prepare(W2, H2)
    other = torch.cuda.Stream()
    off_d = rig.dev(off2)
    ids_d = torch.full((H2, W2), -7, dtype=torch.int32, device="cuda")
    raw, views = rig._planes((H2, W2), ALL)
    torch.cuda.synchronize()
    rig.scene.trace_ids(off_d, ids_d, stream=rig.stream)
    rig.scene.surface_frame(off_d, ids_d, s, stream=other, **views)  # reads the ids the trace is still writing
    g = flat(rig._collect(raw, views))
    ids = ids_d.cpu().numpy()
    rig.close()
    assert np.array_equal(ids.reshape(-1), want_ids)
    sv.check_surface(sv.expected(ev, tb.normals, tb.uvs, tex, modulate=True), **{k: v[sel] for k, v in g.items()})
    same(g, host_planes(scene_q, W2, H2, pixels, want_ids, tb.normals, tb.uvs, tex, modulate=True))


def test_moved_camera(scene_q, frame_q, monkeypatch):
    """After scene.set_camera the outputs are bit-equal to a fresh scene's at that camera."""
    import simpleraytracer_amd.device as device

    default_env(monkeypatch)
    f = frame_q
    tb, tex = f["tb"], f["tex"]
    cam = np.array(device.read_scene(scene_q)["camera"])
    cam[0:3] += np.float32([0.4, -0.3, -0.5])
    cam[9] = 50.0
    results = []
    for moved in (True, False):
        rig = Rig(scene_q, camera=None if moved else cam)
        rig.prepare(W, H)
        if moved:
            rig.surface_frame(f["off"], f["ids"], rig.surface_of(tb.normals, tb.uvs, tex))
            rig.scene.set_camera(cam, stream=rig.stream)
        ids = rig.trace(f["off"], ids=True)
        results.append((ids, rig.surface_frame(f["off"], ids, rig.surface_of(tb.normals, tb.uvs, tex, modulate=True)),
                        rig.interpolate_frame(f["off"], ids, tb.generic)))
        rig.close()
    (ids_a, a, ia), (ids_b, b, ib) = results
    assert np.array_equal(ids_a, ids_b) and (ids_a >= 0).any() and not np.array_equal(ids_a, f["ids"])
    same(a, b)
    assert np.array_equal(ia.view(np.uint32), ib.view(np.uint32))


def test_long_scene(scenes, monkeypatch):
    """soup-100k at 1920 x 1080: band rows 536..539 with the trace's ids, 4 096 random points with the
    query's, a 64 x 64 texture: bit-equal to the host path."""
    import simpleraytracer_amd.device as device

    default_env(monkeypatch)
    w, h = 1920, 1080
    path = scenes["soup100k"]
    n = device.scene_triangles(path)
    tb = sv.tables(n, 31)
    tex = sv.texture(64, 64, 9)
    off = np.full((h, w, 2), 0.5, np.float32)
    points = np.random.default_rng(17).random((4096, 2), dtype=np.float32)
    rig = Rig(path, w, h)
    s = rig.surface_of(tb.normals, tb.uvs, tex, modulate=True)
    ids = rig.trace(off, ids=True)
    band = rig.surface_frame(off, ids, s, r0=536, rows=4)
    band_i = rig.interpolate_frame(off, ids, tb.generic, r0=536, rows=4)
    q_ids = rig.query(points)
    pts = rig.surface(points, q_ids, s)
    rig.close()
    for got_ids in (ids[536:540], q_ids):
        assert (got_ids >= 0).mean() >= 0.10 and (got_ids < 0).mean() >= 0.10
    pixels = device.pixel_positions(w, h, 0.5).reshape(h, w, 2)[536:540].reshape(-1, 2)
    band_ids = ids[536:540].reshape(-1)
    same(flat(band), host_planes(path, w, h, pixels, band_ids, tb.normals, tb.uvs, tex, modulate=True))
    same(pts, host_planes(path, w, h, points, q_ids, tb.normals, tb.uvs, tex, modulate=True))
    want_i = device.interpolate_host(path, w, h, pixels, band_ids, tb.generic)
    assert np.array_equal(band_i.reshape(-1, 4).view(np.uint32), want_i.view(np.uint32))


def test_errors(scene_q, frame_q, monkeypatch):
    import ctypes

    import torch

    from simpleraytracer_amd import SrtError, Surface, _native

    default_env(monkeypatch)
    L = _native.lib()
    f32 = dict(dtype=torch.float32, device="cuda")
    tb = frame_q["tb"]
    rig = Rig(scene_q)
    n = rig.scene.triangles
    pos = torch.full((4, 2), 0.5, **f32)
    pid = torch.zeros((4,), dtype=torch.int32, device="cuda")
    plane = torch.zeros((4, 4), **f32)
    uvs = rig.dev(tb.uvs)
    table = rig.dev(tb.generic)
    tex = torch.zeros((2, 2, 4), **f32)
    # a scene that was never prepared
    with pytest.raises(SrtError, match=r"Surface: Prepare\(\) has not been called"):
        rig.scene.surface(pos, pid, Surface(), rgba=plane)
    with pytest.raises(SrtError, match=r"Interpolate: Prepare\(\) has not been called"):
        rig.scene.interpolate(pos, pid, table, plane)
    rig.prepare(W, H)
    off = torch.full((H, W, 2), 0.5, **f32)
    ids = torch.zeros((H, W), dtype=torch.int32, device="cuda")
    fplane = torch.zeros((H, W, 4), **f32)
    size_s, size_o = ctypes.sizeof(_native.RtvSurface), ctypes.sizeof(_native.RtvOutputs)
    s = _native.RtvSurface(size_s, 0, 0, 0, 0, 0, 0)
    out = _native.RtvOutputs(size_o, 0, 0, plane.data_ptr(), 0)
    fout = _native.RtvOutputs(size_o, 0, 0, fplane.data_ptr(), 0)
    h = rig.scene.handle
    P, I, O, D = pos.data_ptr(), pid.data_ptr(), off.data_ptr(), ids.data_ptr()

    def points(scene=h, p=P, i=I, count=4, surface=s, outputs=out):
        return L.rtvSurfacePointsAsync(scene, p, i, count, ctypes.byref(surface) if surface else None,
                                       ctypes.byref(outputs) if outputs else None, None)

    def frame(scene=h, o=O, i=D, r0=0, rows=H, surface=s, outputs=fout):
        return L.rtvSurfaceFrameAsync(scene, o, i, r0, rows, ctypes.byref(surface) if surface else None,
                                      ctypes.byref(outputs) if outputs else None, None)

    # NULL scene, NULL structs, wrong struct_size, unknown flags
    assert points(scene=None) == -1 and _native.last_error() == "Bad scene handle"
    assert frame(scene=None) == -1
    assert points(surface=None) == -1 and "surface" in _native.last_error()
    assert points(outputs=None) == -1 and "outputs" in _native.last_error()
    for size in (0, 48, 64):
        assert points(surface=_native.RtvSurface(size, 0, 0, 0, 0, 0, 0)) == -1
        assert "rtv_surface.struct_size" in _native.last_error()
        assert frame(surface=_native.RtvSurface(size, 0, 0, 0, 0, 0, 0)) == -1
    for size in (0, 32, 48):
        assert points(outputs=_native.RtvOutputs(size, 0, 0, plane.data_ptr(), 0)) == -1
        assert "rtv_outputs.struct_size" in _native.last_error()
        assert frame(outputs=_native.RtvOutputs(size, 0, 0, fplane.data_ptr(), 0)) == -1
    assert points(surface=_native.RtvSurface(size_s, 0, 0, 0, 0, 0, 8)) == -1 and "rtv_surface.flags" in _native.last_error()
    # a texture without uvs, a texture size outside the limits
    assert points(surface=_native.RtvSurface(size_s, 0, 0, tex.data_ptr(), 2, 2, 0)) == -1
    assert "rtv_surface.uvs" in _native.last_error()
    for tw, th, field in ((0, 2, "tex_width"), (16385, 2, "tex_width"), (2, 0, "tex_height"), (2, 16385, "tex_height")):
        assert frame(surface=_native.RtvSurface(size_s, 0, uvs.data_ptr(), tex.data_ptr(), tw, th, 0)) == -1
        assert f"rtv_surface.{field}" in _native.last_error()
    # NULL inputs with a nonzero count; nothing to do with a zero count or no plane
    assert points(p=None) == -1 and "d_positions" in _native.last_error()
    assert points(i=None) == -1 and "d_ids" in _native.last_error()
    assert frame(o=None) == -1 and "d_offsets" in _native.last_error()
    assert frame(i=None) == -1 and "d_ids" in _native.last_error()
    none = _native.RtvOutputs(size_o, 0, 0, 0, 0)
    assert points(p=None, i=None, count=0) == 0 and frame(o=None, i=None, rows=0) == 0
    assert points(p=None, i=None, outputs=none) == 0 and frame(o=None, i=None, outputs=none) == 0
    # a band past the frame
    assert frame(r0=1) == -1 and "outside the frame" in _native.last_error()
    assert frame(r0=H + 1, rows=0) == -1
    with pytest.raises(SrtError, match="outside the frame"):
        rig.scene.surface_frame(off[:10], ids[:10], Surface(), rgba=fplane[:10], row_begin=H - 5, row_count=10)
    # the interpolation: channels, NULL inputs, the band
    T, R = table.data_ptr(), fplane.data_ptr()
    for channels in (0, 5):
        assert L.rtvInterpolatePointsAsync(h, P, I, 4, T, channels, plane.data_ptr(), None) == -1
        assert "channels" in _native.last_error()
        assert L.rtvInterpolateFrameAsync(h, O, D, 0, H, T, channels, R, None) == -1
    assert L.rtvInterpolatePointsAsync(None, P, I, 4, T, 4, plane.data_ptr(), None) == -1
    assert L.rtvInterpolatePointsAsync(h, None, I, 4, T, 4, plane.data_ptr(), None) == -1 and "d_positions" in _native.last_error()
    assert L.rtvInterpolatePointsAsync(h, P, None, 4, T, 4, plane.data_ptr(), None) == -1 and "d_ids" in _native.last_error()
    assert L.rtvInterpolatePointsAsync(h, P, I, 4, None, 4, plane.data_ptr(), None) == -1 and "d_table" in _native.last_error()
    assert L.rtvInterpolatePointsAsync(h, P, I, 4, T, 4, None, None) == -1 and "d_out" in _native.last_error()
    assert L.rtvInterpolateFrameAsync(h, None, D, 0, H, T, 4, R, None) == -1 and "d_offsets" in _native.last_error()
    assert L.rtvInterpolatePointsAsync(h, None, None, 0, None, 4, None, None) == 0
    assert L.rtvInterpolateFrameAsync(h, None, None, 0, 0, None, 4, None, None) == 0
    assert L.rtvInterpolateFrameAsync(h, O, D, 1, H, T, 4, R, None) == -1 and "outside the frame" in _native.last_error()
    # the wrapper's shape / dtype / device checks
    with pytest.raises(ValueError):
        rig.scene.surface(pos, pid, "surface", rgba=plane)
    with pytest.raises(ValueError):
        rig.scene.surface(torch.zeros((4, 3), **f32), pid, Surface(), rgba=plane)
    with pytest.raises(ValueError):
        rig.scene.surface(pos, torch.zeros((5,), dtype=torch.int32, device="cuda"), Surface(), rgba=plane)
    with pytest.raises(ValueError):
        rig.scene.surface(pos, pid.to(torch.int64), Surface(), rgba=plane)
    with pytest.raises(ValueError):
        rig.scene.surface(pos, pid, Surface(), rgba=torch.zeros((5, 4), **f32))
    with pytest.raises(ValueError):
        rig.scene.surface(pos, pid, Surface(), uv=torch.zeros((4, 3), **f32))
    with pytest.raises(ValueError):
        rig.scene.surface(pos, pid, Surface(), normal=torch.zeros((4, 4), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        rig.scene.surface(pos.cpu(), pid, Surface(), rgba=plane)
    with pytest.raises(ValueError):
        rig.scene.surface(pos, pid, Surface(normals=torch.zeros((n - 1, 3, 3), **f32)), rgba=plane)
    with pytest.raises(ValueError):
        rig.scene.surface(pos, pid, Surface(uvs=uvs.cpu()), rgba=plane)
    with pytest.raises(ValueError):
        rig.scene.surface(pos, pid, Surface(uvs=uvs, texture=torch.zeros((2, 2, 3), **f32)), rgba=plane)
    with pytest.raises(ValueError):
        rig.scene.surface_frame(off[:, :-1], ids, Surface(), rgba=fplane)
    with pytest.raises(ValueError):
        rig.scene.surface_frame(off, ids, Surface(), albedo=fplane.cpu())
    with pytest.raises(ValueError):
        rig.scene.interpolate(pos, pid, table, torch.zeros((4, 5), **f32))
    with pytest.raises(ValueError):
        rig.scene.interpolate(pos, pid, table, torch.zeros((4, 3), **f32))
    with pytest.raises(ValueError):
        rig.scene.interpolate_frame(off, ids, table, torch.zeros((H, W + 1, 4), **f32))
    # a valid call still works afterwards
    ev = sv.cached_edges(scene_q, W, H, "mixed")
    got = rig.surface(ev.pos, ev.ids, rig.surface_of(tb.normals, tb.uvs, frame_q["tex"]), which=("rgba",))
    rig.close()
    sv.same_bits("rgba", got["rgba"], sv.expected(ev, tb.normals, tb.uvs, frame_q["tex"]).rgba)
